"""What the two calls of the directional projection enqueue (hare_amd/csrc/hist.cpp: hare_hist_project_channels, _device), pinned without
a GPU in the manner of tests/test_hist_trace.py: a fresh child `python` runs the unmodified library against tests/stubs/fake_hip.cpp with
allocations, frees and synchronisations logged, and prints one row per call; the parent reads the rows.

The host call stages its buffers in ONE device block: one allocation, the inputs copied up (histogram, coefficients, weights when given),
one launch of hare_hist_project_channels with a workgroup of 256 per receiver and no dynamic LDS, the output -- K x B x J x channels x 16
bytes -- copied down, one synchronisation, one free.  The device call is that one launch and nothing else.  (The stand-in does not decode
this kernel's arguments; where the parts lie is read from the copies.)  Shape: K = 2, n_bins = 8, B = 2, four channels, J = 3."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_host_trace import ROOT, build_stub

K, NB, B, C, J = 2, 8, 2, 4, 3
HIST, WEIGHT, COEF, PROJ = K * NB * B * C * 8, NB * B * 4, J * NB * 4, K * B * J * C * 16
KERNEL = "hare_hist_project_channels"
CASES = ("host", "host, weight", "device", "device, weight")


# ---------------------------------------------------------------------------------------------------------------- the child
def child():
    import hare_amd as H
    from hare_amd import capi

    L = capi.lib
    stub = ctypes.CDLL(os.environ["HARE_HIP_RUNTIME"])
    stub.fake_hip_log.restype = ctypes.c_char_p
    stub.fake_hip_name_host_range.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t]
    box = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(box.verts, box.nverts)], 8)
    rng = np.random.default_rng(5)
    A = dict(hist=rng.integers(0, 1 << 40, (K, NB, B, C), np.uint64), weight=rng.integers(0, 1 << 32, (NB, B), np.uint32),
             coef=rng.integers(-5, 6, (J, NB), np.int32), proj=np.zeros((K, B, J, C, 2), np.uint64))
    for name, a in A.items():
        stub.fake_hip_name_host_range(name.encode(), a.ctypes.data, a.nbytes)
    P = {k: a.ctypes.data for k, a in A.items()}
    g.get_option("hip_malloc_calls")                # the scene's device side exists before the first traced call
    assert L.hare_hist_project_channels(g._h, K, NB, B, C, P["hist"], None, J, P["coef"], P["proj"]) in (0, capi.HARE_E_STATE)
    stub.fake_hip_log_enable(2)
    for name in CASES:
        w = P["weight"] if name.endswith("weight") else None
        stub.fake_hip_log_clear()
        live = stub.fake_hip_live_allocations()
        if name.startswith("host"):
            rc = L.hare_hist_project_channels(g._h, K, NB, B, C, P["hist"], w, J, P["coef"], P["proj"])
        else:                                       # any non-null addresses: the stand-in launches nothing
            rc = L.hare_hist_project_channels_device(g._h, K, NB, B, C, P["hist"], w, J, P["coef"], P["proj"], None)
        print(json.dumps(dict(case=name, rc=rc, error=capi.last_error() if rc else "", log=stub.fake_hip_log().decode().splitlines(),
                              leaked=stub.fake_hip_live_allocations() - live)), flush=True)
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
    return {r["case"]: r for r in (json.loads(line) for line in c.stdout.splitlines())}


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return build_stub(tmp_path_factory.mktemp("fake_hip"))


@pytest.fixture(scope="module")
def traced(stub):
    return run_child(stub)


@pytest.mark.parametrize("name", CASES[2:])
def test_the_device_call_is_one_launch_and_nothing_else(traced, name):
    r = traced[name]
    assert r["rc"] == 0 and r["leaked"] == 0, r
    assert len(r["log"]) == 1, r["log"]
    assert r["log"][0].split()[:6] == ["launch", KERNEL, "grid=%d" % K, "block=256", "lds=0", "s0"], r["log"]


@pytest.mark.parametrize("name", CASES[:2])
def test_the_host_call_is_one_staging(traced, name):
    r = traced[name]
    assert r["rc"] == 0 and r["leaked"] == 0, r
    up = [("hist", HIST), ("coef", COEF)] + ([("weight", WEIGHT)] if name.endswith("weight") else [])
    log = [l.split() for l in r["log"]]
    assert [w[0] for w in log] == ["malloc"] + ["memcpy"] * len(up) + ["launch", "memcpy", "sync", "free"], r["log"]
    blk, size = log[0][1], int(log[0][2].split("=")[1])
    assert log[-1] == ["free", blk] and log[-2] == ["sync", "s0"]
    assert log[1 + len(up)][:6] == ["launch", KERNEL, "grid=%d" % K, "block=256", "lds=0", "s0"], log[1 + len(up)]
    spans = []
    for (host, n), w in zip(up, log[1:]):
        assert w[2:] == ["<-", host + "+0", "bytes=%d" % n, "kind=1", "s0"] and w[1].split("+")[0] == blk, w
        spans.append((int(w[1].split("+")[1]), n))
    down = log[2 + len(up)]
    assert down[1:3] == ["proj+0", "<-"] and down[4:] == ["bytes=%d" % PROJ, "kind=2", "s0"] and down[3].split("+")[0] == blk, down
    spans.append((int(down[3].split("+")[1]), PROJ))
    spans.sort()
    for off, n in spans:
        assert off % 16 == 0 and off + n <= size, (spans, size)
    for (o0, n0), (o1, _) in zip(spans, spans[1:]):
        assert o0 + n0 <= o1, spans
    total = sum(n for _, n in spans)
    assert total <= size <= total + (0 if name.endswith("weight") else WEIGHT) + 16 * 4, (size, spans)


def test_a_missing_kernel_is_a_state_error_and_frees_the_block(stub):
    from hare_amd import capi
    rows = run_child(stub, missing=KERNEL)
    assert set(rows) == set(CASES)
    for name, r in rows.items():
        assert r["rc"] == capi.HARE_E_STATE and "hare_hist_project_channels missing from code object" in r["error"], r
        words = [l.split()[0] for l in r["log"]]
        assert "launch" not in words and r["leaked"] == 0, r
        assert (words.count("malloc"), words.count("free")) == ((1, 1) if name.startswith("host") else (0, 0)), r


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        child()
    else:
        sys.exit(__doc__)
