"""What the host-buffer calls on a histogram enqueue (hare_amd/csrc/hist.cpp: hare_hist_reduce, hare_hist_project, hare_hist_render), pinned
without a GPU as tests/test_host_trace.py pins the batch calls: a fresh child `python` runs the unmodified library against
tests/stubs/fake_hip.cpp, which here also logs allocations, frees and synchronisations (fake_hip_log_enable(2)), and prints one row per
call; the parent reads the rows.

A call stages its buffers in ONE device block: one allocation, the inputs copied up in a fixed order, one launch on addresses inside the
block, the outputs copied down, one synchronisation, one free.  The expectations below restate include/hare_hip.h and the launch shapes
of hist.cpp -- a workgroup of 256 per receiver for the two integer kernels; for the rendering K x tiles workgroups of 512 and the dynamic
LDS of render_plan, worked out by hand for the one shape used.  The block's size is bounded, not pinned: the sum of the parts and at most
16 bytes of padding per part (room for weights that were not given is allowed, not required).

Shape: K = 2, n_bins = 8, B = 2, one channel; each call once with and once without `weight`; the reduction also with no windows and with
no levels; and every call once against a code object that lacks its kernel (HARE_E_STATE, the block freed)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_host_trace import ROOT, build_stub

K, NB, B = 2, 8, 2
N_WIN, N_LEV, J, M, T = 3, 2, 3, 4, 3
HIST, WEIGHT = K * NB * B * 8, NB * B * 4
# render_plan at B = 2, C = 1, M = 4, T = 3, n_bins = 8: tile_bins = min(2048 / 4, 2048 / 2, 8) = 8, one tile of S = 32 samples,
# sign words ((32 + 3 + 8 + 62) >> 6) + 2 = 3, LDS 8 * (B T + B S + 8 B C + 8 B + 3) = 8 * 105
RENDER_LDS = 840


def cases():
    """name -> (kernel, grid, block, lds, up [(host name, device field, bytes)], down [(host name, device field, bytes)])"""
    out = {}
    for weight in (True, False):
        w = [("weight", "weight", WEIGHT)] if weight else []
        tag = ", weight" if weight else ""
        for n_win, n_lev in ((N_WIN, N_LEV), (0, N_LEV), (N_WIN, 0)) if weight else ((N_WIN, N_LEV),):
            down = [("sums", "sums", K * B * n_win * 32)] * (n_win > 0) + [("cross", "cross", K * B * n_lev * 4)] * (n_lev > 0)
            out["reduce %d %d%s" % (n_win, n_lev, tag)] = ("hare_hist_reduce", K, 256, 0, [("hist", "hist", HIST)] + w, down)
        out["project" + tag] = ("hare_hist_project", K, 256, 0, [("hist", "hist", HIST), ("coef", "coef", J * NB * 4)] + w,
                                [("proj", "proj", K * B * J * 16)])
        out["render" + tag] = ("hare_hist_render", K, 512, RENDER_LDS, [("hist", "hist", HIST), ("taps", "taps", B * T * 8)] + w,
                               [("out", "out", K * NB * M * 8)])
    return out


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
    A = dict(hist=rng.integers(0, 1 << 40, (K, NB, B), np.uint64), weight=rng.integers(0, 1 << 32, (NB, B), np.uint32),
             win=np.array([[0, 8], [2, 5], [3, 3]], np.int32), levels=np.array([1 << 31, 1 << 22], np.uint32),
             sums=np.zeros((K, B, N_WIN, 4), np.uint64), cross=np.zeros((K, B, N_LEV), np.int32),
             coef=rng.integers(-5, 6, (J, NB), np.int32), proj=np.zeros((K, B, J, 2), np.uint64),
             taps=rng.standard_normal((B, T)), out=np.zeros((K, 1, NB * M)))
    for name, a in A.items():
        stub.fake_hip_name_host_range(name.encode(), a.ctypes.data, a.nbytes)
    P = {k: a.ctypes.data for k, a in A.items()}
    g.get_option("hip_malloc_calls")                # the scene's device side exists before the first traced call
    assert L.hare_hist_project(g._h, K, NB, B, 1, P["hist"], None, J, P["coef"], P["proj"]) in (0, capi.HARE_E_STATE)
    stub.fake_hip_log_enable(2)
    for name in cases():
        w = P["weight"] if name.endswith("weight") else None
        stub.fake_hip_log_clear()
        live = stub.fake_hip_live_allocations()
        if name.startswith("reduce"):
            n_win, n_lev = (int(x) for x in name.split(",")[0].split()[1:])
            rc = L.hare_hist_reduce(g._h, K, NB, B, 1, P["hist"], w, n_win, P["win"], n_lev, P["levels"], P["sums"], P["cross"])
        elif name.startswith("project"):
            rc = L.hare_hist_project(g._h, K, NB, B, 1, P["hist"], w, J, P["coef"], P["proj"])
        else:
            rc = L.hare_hist_render(g._h, K, NB, B, 1, P["hist"], w, 40, M, T, P["taps"], 7, P["out"])
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


def device(word, block):
    """`a3+96` -> 96, of the block `a3`"""
    name, off = word.split("+")
    assert name == block, (word, block)
    return int(off)


@pytest.mark.parametrize("name", list(cases()))
def test_a_call_stages_one_block(traced, name):
    kernel, grid, block, lds, up, down = cases()[name]
    r = traced[name]
    assert r["rc"] == 0 and r["leaked"] == 0, r
    log = [l.split() for l in r["log"]]
    # the sequence: one allocation, the copies up, one launch, the copies down, one synchronisation, one free
    assert [w[0] for w in log] == ["malloc"] + ["memcpy"] * len(up) + ["launch"] + ["memcpy"] * len(down) + ["sync", "free"], r["log"]
    blk, size = log[0][1], int(log[0][2].split("=")[1])
    assert log[-1] == ["free", blk] and log[-2] == ["sync", "s0"]
    launch = log[1 + len(up)]
    assert launch[1:5] == [kernel, "grid=%d" % grid, "block=%d" % block, "lds=%d" % lds] and launch[5] == "s0", launch
    args = dict(re.findall(r" (\w+)=(\S+)", r["log"][1 + len(up)].split("{", 1)[1]))
    # every part: where the kernel finds it, its bytes; the copies go to and from exactly these
    parts = {}
    for (host, field, n), w in zip(up, log[1:]):
        assert w[1:] == ["%s+%d" % (blk, device(args[field], blk)), "<-", host + "+0", "bytes=%d" % n, "kind=1", "s0"], (w, field)
        parts[field] = (device(args[field], blk), n)
    for (host, field, n), w in zip(down, log[2 + len(up):]):
        assert w[1:] == [host + "+0", "<-", "%s+%d" % (blk, device(args[field], blk)), "bytes=%d" % n, "kind=2", "s0"], (w, field)
        parts[field] = (device(args[field], blk), n)
    buffers = {"hist", "weight", "sums", "cross", "coef", "proj", "taps", "out"}
    # no other address, but for an output of no bytes (no windows, no levels): null, or a place in the block
    empty = ({"sums"} if name.startswith("reduce 0 ") else set()) | ({"cross"} if " 0," in name else set())
    assert set(parts) <= {f for f in args if f in buffers} <= set(parts) | empty, (args, parts)
    assert all(device(args[f], blk) <= size for f in empty if f in args), (args, size)
    spans = sorted(parts.values())
    for off, n in spans:
        assert off % 16 == 0 and off + n <= size, (parts, size)
    for (o0, n0), (o1, _) in zip(spans, spans[1:]):
        assert o0 + n0 <= o1, parts
    total = sum(n for _, n in spans)
    # four parts at most, at most 16 bytes of padding each; weights left out may keep their place
    assert total <= size <= total + (0 if "weight" in parts else WEIGHT) + 16 * 4, (size, parts)


def test_a_missing_kernel_is_a_state_error_and_frees_the_block(stub):
    from hare_amd import capi
    rows = run_child(stub, missing="hare_hist_reduce,hare_hist_project,hare_hist_render")
    assert set(rows) == set(cases())
    for name, r in rows.items():
        assert r["rc"] == capi.HARE_E_STATE and "missing from code object" in r["error"], r
        words = [l.split()[0] for l in r["log"]]
        assert words.count("malloc") == 1 and words.count("free") == 1 and "launch" not in words and r["leaked"] == 0, r


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        child()
    else:
        sys.exit(__doc__)
