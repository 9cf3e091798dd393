"""What the two decode calls enqueue (hare_amd/csrc/hist.cpp: hare_decode_device, hare_decode), pinned without a GPU as
tests/test_convolve_trace.py pins the convolve calls: a fresh child `python` runs the unmodified library against tests/stubs/fake_hip.cpp
with allocations, frees and synchronisations logged too (fake_hip_log_enable(2)) and prints one row per call; the parent reads the rows.

The device call is ONE launch of hare_decode on the caller's stream and no other runtime call.  The host call stages its three buffers in
one device block: one allocation, in and h copied up, one launch, y copied down, one synchronisation, one free.  Grid, block and dynamic
LDS are decode_plan's (restated in tests/decode_cases.py from the kernel's constants): a workgroup of 256 per (k, o) and tile of 2 048
outputs, whatever C.  Against a code object without the kernel both calls answer HARE_E_STATE, the host call's block freed."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.decode_cases import TILE, plan
from tests.test_host_trace import ROOT, build_stub

K, C, N, O, T = 2, 9, 3000, 3, 1200
SHAPES = {"whole": (0, N + T - 1), "one tile": (5, TILE), "a tile and a sample": (5, TILE + 1), "one sample": (N + T - 2, 1)}


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
    rng = np.random.default_rng(5)
    A = dict(x=rng.standard_normal((K, C, N)), h=rng.standard_normal((O, C, T)), y=np.zeros((K, O, N + T - 1)))
    for name, a in A.items():
        stub.fake_hip_name_host_range(name.encode(), a.ctypes.data, a.nbytes)
    P = {k: a.ctypes.data for k, a in A.items()}
    g.get_option("hip_malloc_calls")                # the scene's device side exists before the first traced call
    assert lib.hare_decode(g._h, 1, 1, 1, P["x"], 1, 1, P["h"], 0, 1, P["y"]) in (0, capi.HARE_E_STATE)
    stream = ctypes.c_void_p()
    assert stub.hipStreamCreate(ctypes.byref(stream)) == 0
    stub.fake_hip_log_enable(2)
    stub.fake_hip_log_clear()
    stub.hipStreamSynchronize(stream)               # how the log names the caller's stream
    print(json.dumps(dict(case="stream", log=stub.fake_hip_log().decode().splitlines())), flush=True)
    for name, (n0, n_out) in SHAPES.items():
        for device in (True, False):
            stub.fake_hip_log_clear()
            live = stub.fake_hip_live_allocations()
            if device:          # any addresses: the stand-in runs no kernel
                rc = lib.hare_decode_device(g._h, K, C, N, 0x10000000, O, T, 0x20000000, n0, n_out, 0x30000000, stream)
            else:
                rc = lib.hare_decode(g._h, K, C, N, P["x"], O, T, P["h"], n0, n_out, P["y"])
            print(json.dumps(dict(case=name, device=device, rc=rc, error=capi.last_error() if rc else "",
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
    grid, block, lds = plan(K, O, n_out)
    return ["launch", "hare_decode", "grid=%d" % grid, "block=%d" % block, "lds=%d" % lds, stream]


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_device_call_is_one_launch_on_the_callers_stream(traced, name):
    stream, rows = traced
    r = rows[(name, True)]
    assert r["rc"] == 0 and r["leaked"] == 0, r
    assert [l.split() for l in r["log"]] == [launch_words(SHAPES[name][1], stream)], r["log"]


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_host_call_stages_one_block(traced, name):
    _, rows = traced
    n_out = SHAPES[name][1]
    r = rows[(name, False)]
    assert r["rc"] == 0 and r["leaked"] == 0, r
    log = [l.split() for l in r["log"]]
    assert [w[0] for w in log] == ["malloc", "memcpy", "memcpy", "launch", "memcpy", "sync", "free"], r["log"]
    blk, size = log[0][1], int(log[0][2].split("=")[1])
    assert log[-1] == ["free", blk] and log[-2] == ["sync", "s0"]
    assert log[3] == launch_words(n_out, "s0"), log[3]
    sizes = dict(x=K * C * N * 8, h=O * C * T * 8, y=K * O * n_out * 8)
    spans = {}
    for w, host in ((log[1], "x"), (log[2], "h")):
        assert w[2:] == ["<-", host + "+0", "bytes=%d" % sizes[host], "kind=1", "s0"] and w[1].startswith(blk + "+"), w
        spans[host] = int(w[1].split("+")[1])
    w = log[4]
    assert w[1:3] == ["y+0", "<-"] and w[4:] == ["bytes=%d" % sizes["y"], "kind=2", "s0"] and w[3].startswith(blk + "+"), w
    spans["y"] = int(w[3].split("+")[1])
    order = sorted(spans, key=spans.get)
    for a in order:
        assert spans[a] % 16 == 0 and spans[a] + sizes[a] <= size
    for a, b in zip(order, order[1:]):
        assert spans[a] + sizes[a] <= spans[b], spans
    assert sum(sizes.values()) <= size <= sum(sizes.values()) + 16 * 3


def test_a_missing_kernel_is_a_state_error(stub):
    from hare_amd import capi
    _, rows = run_child(stub, missing="hare_decode")
    assert len(rows) == 2 * len(SHAPES)
    for (name, device), r in rows.items():
        assert r["rc"] == capi.HARE_E_STATE and "hare_decode missing from code object" in r["error"], r
        words = [l.split()[0] for l in r["log"]]
        assert "launch" not in words and r["leaked"] == 0, r
        assert words == [] if device else (words.count("malloc") == 1 and words.count("free") == 1), r


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        child()
    else:
        sys.exit(__doc__)
