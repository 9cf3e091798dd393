"""What the impulse calls enqueue (hare_amd/csrc/hist.cpp: hare_hist_impulses_device, hare_hist_impulses; bounce.cpp: hare_source_paths),
pinned without a GPU as tests/test_decode_trace.py pins the decode calls: a fresh child `python` runs the unmodified library against
tests/stubs/fake_hip.cpp with allocations, frees and synchronisations logged too (fake_hip_log_enable(2)) and prints one row per call; the
parent reads the rows.

The device call is ONE launch of hare_hist_impulses on the caller's stream and no other runtime call.  The host call stages its buffers in
one device block: one allocation, `out` copied up only with add == 1 or a stride gap, histogram and taps (and weights) up, one launch, out
down, one synchronisation, one free.  Grid, block and dynamic LDS are impulses_plan's (restated in tests/impulse_cases.py from the kernel's
constants).  hare_source_paths zeroes the histogram, launches the direct sound's, the first order's and the second order's kernels in that
order on one stream, downloads, and synchronises once.  Against a code object without the kernel both impulse calls answer HARE_E_STATE."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.impulse_cases import TILE, plan
from tests.test_host_trace import ROOT, build_stub

K, NB, B, C, T = 2, 700, 3, 9, 65
TOTAL = NB + T - 1
# name: (n0, n_out, out_stride, add, weight)
SHAPES = {"whole": (0, TOTAL, TOTAL, 0, False), "one tile": (5, TILE, TILE, 0, True), "a tile and a sample": (5, TILE + 1, TILE + 1, 1, False),
          "one sample in a stride": (TOTAL - 1, 1, 4, 0, False)}


# ---------------------------------------------------------------------------------------------------------------- the child
def child():
    import hare_amd as H
    from hare_amd import capi

    lib = capi.lib
    stub = ctypes.CDLL(os.environ["HARE_HIP_RUNTIME"])
    stub.fake_hip_log.restype = ctypes.c_char_p
    stub.fake_hip_name_host_range.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t]
    stub.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    stub.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    box = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(box.verts, box.nverts)], 8)
    g.set_receivers(np.array([[3.0, 2.0, 1.5], [6.0, 4.0, 2.0]]), np.array([0.25, 0.5]))
    g.set_source((2.0, 1.0, 1.0))
    A = dict(hist=np.zeros((K, NB, B, C), np.uint64), taps=np.ones((B, T)), weight=np.ones((NB, B), np.uint32), out=np.zeros((K, C, TOTAL)),
             phist=np.zeros((2, 64, 1), np.uint64), pdet=np.zeros((2, 2), np.uint64))
    for name, a in A.items():
        stub.fake_hip_name_host_range(name.encode(), a.ctypes.data, a.nbytes)
    P = {k: a.ctypes.data for k, a in A.items()}
    g.get_option("hip_malloc_calls")                # the scene's device side exists before the first traced call
    assert lib.hare_hist_impulses(g._h, 1, 1, 1, 1, P["hist"], None, 0, 1, P["taps"], 0, 1, 1, 0, P["out"]) in (0, capi.HARE_E_STATE)
    flags = capi.RECEIVE_DIRECT | capi.RECEIVE_IMAGE | capi.RECEIVE_IMAGE2
    assert lib.hare_source_paths(g._h, g._kind, 0, 4097, flags, 64, 0.5, 40, P["phist"], P["pdet"]) == 0, capi.last_error()      # buffers grown, tables up
    stream = ctypes.c_void_p()
    assert stub.hipStreamCreate(ctypes.byref(stream)) == 0
    stub.fake_hip_log_enable(2)
    stub.fake_hip_log_clear()
    stub.hipStreamSynchronize(stream)               # how the log names the caller's stream
    print(json.dumps(dict(case="stream", log=stub.fake_hip_log().decode().splitlines())), flush=True)
    for name, (n0, n_out, stride, add, weight) in SHAPES.items():
        for device in (True, False):
            stub.fake_hip_log_clear()
            live = stub.fake_hip_live_allocations()
            if device:          # any addresses: the stand-in runs no kernel
                rc = lib.hare_hist_impulses_device(g._h, K, NB, B, C, 0x10000000, 0x18000000 if weight else None, 24, T, 0x20000000, n0, n_out, stride, add,
                                                   0x30000000, stream)
            else:
                rc = lib.hare_hist_impulses(g._h, K, NB, B, C, P["hist"], P["weight"] if weight else None, 24, T, P["taps"], n0, n_out, stride, add, P["out"])
            print(json.dumps(dict(case=name, device=device, rc=rc, error=capi.last_error() if rc else "",
                                  log=stub.fake_hip_log().decode().splitlines(), leaked=stub.fake_hip_live_allocations() - live)), flush=True)
    for name, fl in (("paths all", flags), ("paths direct", capi.RECEIVE_DIRECT), ("paths image", capi.RECEIVE_IMAGE)):
        stub.fake_hip_log_clear()
        live = stub.fake_hip_live_allocations()
        rc = lib.hare_source_paths(g._h, g._kind, 0, 4097, fl, 64, 0.5, 40, P["phist"], P["pdet"])
        print(json.dumps(dict(case=name, device=False, rc=rc, error=capi.last_error() if rc else "",
                              log=stub.fake_hip_log().decode().splitlines(), leaked=stub.fake_hip_live_allocations() - live)), flush=True)
    stub.fake_hip_log_enable(1)
    g.close()
    stub.fake_hip_name_host_range(None, None, 0)
    assert stub.fake_hip_live_allocations() == 0


# ---------------------------------------------------------------------------------------------------------------- the parent
def run_child(stub, missing=None):
    env = dict(os.environ, HARE_HIP_RUNTIME=stub, HARE_BUILD="host", FAKE_HIP_CUS="256")
    for k in ("HARE_DEV", "HARE_TUNE", "HARE_LIB", "FAKE_HIP_MISSING", "FAKE_HIP_BUFFERS"):
        env.pop(k, None)
    if missing:
        env["FAKE_HIP_MISSING"] = missing
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + [p for p in sys.path if p])
    c = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True)
    assert c.returncode == 0, c.stdout[-2000:] + c.stderr[-4000:]
    rows = [json.loads(line) for line in c.stdout.splitlines()]
    assert rows[0]["case"] == "stream" and len(rows[0]["log"]) == 1 and rows[0]["log"][0].startswith("sync s")
    stream = rows[0]["log"][0].split()[1]
    assert stream not in ("s0", "s?")
    return stream, {(r["case"], r["device"]): r for r in rows[1:]}


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return build_stub(tmp_path_factory.mktemp("fake_hip"))


@pytest.fixture(scope="module")
def traced(stub):
    return run_child(stub)


def launch_words(n_out, stream):
    grid, block, lds = plan(K, B, C, T, n_out)
    return ["launch", "hare_hist_impulses", "grid=%d" % grid, "block=%d" % block, "lds=%d" % lds, stream]


def test_the_launch_geometry_of_three_shapes():
    assert plan(K, B, C, T, TOTAL) == (2 * 3, 256, 8 * 3 * 65 + 256 * (8 * 11 + 4) + 16)
    assert plan(K, B, C, T, TILE)[0] == 2 and plan(K, B, C, T, TILE + 1)[0] == 4 and plan(K, B, C, T, 1)[0] == 2


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_device_call_is_one_launch_on_the_callers_stream(traced, name):
    stream, rows = traced
    r = rows[(name, True)]
    assert r["rc"] == 0 and r["leaked"] == 0, r
    assert [l.split() for l in r["log"]] == [launch_words(SHAPES[name][1], stream)], r["log"]


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_host_call_stages_one_block_and_uploads_out_only_where_it_must(traced, name):
    _, rows = traced
    n0, n_out, stride, add, weight = SHAPES[name]
    r = rows[(name, False)]
    assert r["rc"] == 0 and r["leaked"] == 0, r
    log = [l.split() for l in r["log"]]
    up = ["out"] * (add == 1 or stride > n_out) + ["hist", "taps"] + ["weight"] * weight
    assert [w[0] for w in log] == ["malloc"] + ["memcpy"] * len(up) + ["launch", "memcpy", "sync", "free"], r["log"]
    blk, size = log[0][1], int(log[0][2].split("=")[1])
    assert log[-1] == ["free", blk] and log[-2] == ["sync", "s0"]
    assert log[1 + len(up)] == launch_words(n_out, "s0"), log[1 + len(up)]
    sizes = dict(hist=K * NB * B * C * 8, taps=B * T * 8, weight=NB * B * 4, out=K * C * stride * 8)
    spans = {}
    for w, host in zip(log[1:], up):
        assert w[2:] == ["<-", host + "+0", "bytes=%d" % sizes[host], "kind=1", "s0"] and w[1].startswith(blk + "+"), w
        spans[host] = int(w[1].split("+")[1])
    w = log[-3]
    assert w[1:3] == ["out+0", "<-"] and w[4:] == ["bytes=%d" % sizes["out"], "kind=2", "s0"] and w[3].startswith(blk + "+"), w
    assert spans.setdefault("out", int(w[3].split("+")[1])) == int(w[3].split("+")[1])
    order = sorted(spans, key=spans.get)
    for a in order:
        assert spans[a] % 16 == 0 and spans[a] + sizes[a] <= size
    for a, b in zip(order, order[1:]):
        assert spans[a] + sizes[a] <= spans[b], spans


def test_source_paths_enqueues_the_three_deposits_in_order_and_synchronises_once(traced):
    _, rows = traced
    first = {"direct": "hare_direct_emit", "image": "hare_image_mirror", "image2": "hare_image2_mirror"}
    last = {"direct": "hare_direct_deposit", "image": "hare_image_deposit", "image2": "hare_image2_deposit"}
    for name, orders in (("paths all", ("direct", "image", "image2")), ("paths direct", ("direct",)), ("paths image", ("image",))):
        r = rows[(name, False)]
        assert r["rc"] == 0 and r["leaked"] == 0, r
        log = [l.split() for l in r["log"]]
        words = [w[0] for w in log]
        assert words.count("sync") == 1 and words[-1] == "sync" and "malloc" not in words and "free" not in words, r["log"]
        streams = {t for w in log if w[0] in ("launch", "memcpy", "memset", "sync") for t in w[1:] if t[0] == "s" and (t[1:].isdigit() or t == "s?")}
        assert len(streams) == 1 and streams != {"s0"}, streams                      # the leased context's stream, all of it
        assert words[0] == "memset"
        kernels = [w[1] for w in log if w[0] == "launch"]
        at = [kernels.index(first[o]) for o in orders]
        assert at == sorted(at) and at[0] == 0
        ends = [max(i for i, k in enumerate(kernels) if k.startswith(last[o])) for o in orders]
        assert all(e < a for e, a in zip(ends, at[1:])) and ends[-1] == len(kernels) - 1          # an order is enqueued whole before the next
        for o in first:
            assert (first[o] in kernels) == (o in orders)
        down = [w for w in log if w[0] == "memcpy" and "kind=2" in w]
        assert [w[1] for w in down[:2]] == ["phist+0", "pdet+0"] and len(down) == 2 + ("image" in orders) + ("image2" in orders)
        assert words.index("memcpy") > max(i for i, w in enumerate(words) if w == "launch")          # nothing comes down before the last deposit


def test_a_missing_kernel_is_a_state_error(stub):
    from hare_amd import capi
    _, rows = run_child(stub, missing="hare_hist_impulses")
    for (name, device), r in rows.items():
        if name.startswith("paths"):
            assert r["rc"] == 0, r
            continue
        assert r["rc"] == capi.HARE_E_STATE and "hare_hist_impulses missing from code object" in r["error"], r
        words = [l.split()[0] for l in r["log"]]
        assert "launch" not in words and r["leaked"] == 0, r
        assert words == [] if device else (words.count("malloc") == 1 and words.count("free") == 1), r


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        child()
    else:
        sys.exit(__doc__)
