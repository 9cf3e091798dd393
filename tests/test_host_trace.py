"""What the host-buffer calls enqueue (hare_amd/csrc/api.cpp, bounce.cpp: the chunks of hare_shoot_batch / hare_occluded_batch, the shards of
the _sharded calls, the staging contexts they lease), pinned without a GPU as tests/test_launch_trace.py pins the launcher: a fresh child
`python` runs the unmodified library against tests/stubs/fake_hip.cpp and prints one row per call; the parent compares the rows with
tests/golden/launch/host_trace.json.

That file is this module's own record of the commit BEFORE the host calls were folded into one fan-out, one context lease and one shard
driver: `python tests/test_host_trace.py --record FILE` with that commit's package first on the path; it is never written from the code under
test, and no row of it is edited by hand.  The stub and this module run unchanged on both commits.

The caller's buffers are real numpy arrays here (the library reads them): the child names each to the stub (fake_hip_name_host_range), so a
copy prints as `rays+96 -> a7+96`.  Chunks and shards run on threads, so the order of the log's lines is not defined: a row holds the lines
PER STREAM (a chunk and a shard each have their own), in order.  Every scene is warmed by one sequential single-scene call of the full n
before the traced call, which therefore creates no stream and allocates nothing: each row asserts that "hip_malloc_calls" and
"hip_free_calls" did not move.  What the launcher's slot ring contributes is left out of the lines (NORMALIZE below): a launch takes the
next slot of its scene from an atomic counter, so which slot a chunk's thread gets -- ShootIO::work, the slot's event waited for and
recorded -- is decided by the race of the threads, on both commits alike.

Scenes: the 972-triangle shoebox as Voxel_Grid at D = 8 and as Octree at the bench's (8, 16).  SHAPES below is asserted against the rows, so
a thinned case list cannot lose a kind of case."""
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "launch", "host_trace.json")
STUB_SRC = os.path.join(HERE, "stubs", "fake_hip.cpp")
WRITEBACK, SLIM = 1, 16
N_MAX = 37
BOUNCES, BINS = 2, 4
NORMALIZE = ((re.compile(r" (work|oct_tail|oct_spill)=\S+"), ""),)      # and the `wait` / `record` lines, dropped whole

# case kind -> a predicate one row must satisfy
SHAPES = {
    "shoot, no chunk option": lambda r: r["call"] == "shoot" and r["chunks"] == 0 and r["rc"] == 0,
    "shoot, eleven empty chunks": lambda r: r["call"] == "shoot" and r["chunks"] == 16 and r["n"] == 5 and len(r["streams"]) == 5,
    "shoot, chunks of 2 and 3": lambda r: r["call"] == "shoot" and r["chunks"] == 16 and r["n"] == 37 and len(r["streams"]) == 16,
    "shoot, three chunks": lambda r: r["call"] == "shoot" and r["chunks"] == 3 and r["n"] == 37 and len(r["streams"]) == 3,
    "shoot, n = 0": lambda r: r["call"] == "shoot" and r["n"] == 0 and r["rc"] == 0 and not r["streams"],
    "shoot with exclusions": lambda r: r["call"] == "shoot excl" and any("e1+" in l for s in r["streams"].values() for l in s),
    "occluded, flags only": lambda r: r["call"] == "occluded" and r["n"] == 37,
    "occluded with events": lambda r: r["call"] == "occluded events" and r["n"] == 37,
    "occluded with exclusions": lambda r: r["call"] == "occluded excl",
    "slim events, 16-byte records": lambda r: r["call"] == "shoot slim" and r["scene"] == "voxel8" and any("hare_events_pack_slim" in l for s in r["streams"].values() for l in s),
    "slim events, 32-byte records": lambda r: r["call"] == "shoot slim" and r["scene"] == "octree",
    "origin write-back": lambda r: r["call"] == "shoot writeback" and r["rc"] == 0,
    "slim events with write-back refused": lambda r: r["call"] == "shoot slim writeback" and r["rc"] != 0,
    "shoot sharded, 1 scene": lambda r: r["call"] == "shoot_sharded" and r["scenes"] == 1 and r["n"] == 37,
    "shoot sharded, 3 scenes": lambda r: r["call"] == "shoot_sharded" and r["scenes"] == 3 and r["n"] == 37 and len(r["streams"]) == 3,
    "shoot sharded, empty shards": lambda r: r["call"] == "shoot_sharded" and r["scenes"] == 3 and r["n"] == 2 and len(r["streams"]) == 2,
    "shoot sharded, slim records": lambda r: r["call"] == "shoot_sharded slim" and r["scenes"] == 3,
    "occluded sharded": lambda r: r["call"] == "occluded_sharded" and r["scenes"] == 3 and r["n"] == 37,
    "occluded sharded with events": lambda r: r["call"] == "occluded_sharded events" and r["scenes"] == 3,
    "bounce sharded": lambda r: r["call"] == "bounce_sharded" and r["scenes"] == 3 and r["n"] == 37 and r["rc"] == 0,
    "receive sharded": lambda r: r["call"] == "receive_sharded" and r["scenes"] == 3 and r["n"] == 37 and r["rc"] == 0,
    "receive sharded, 1 scene": lambda r: r["call"] == "receive_sharded" and r["scenes"] == 1 and r["n"] == 5 and r["rc"] == 0,
    "receive source sharded": lambda r: r["call"] == "receive_source_sharded" and r["scenes"] == 3 and r["n"] == 37 and r["rc"] == 0,
    "sharded, n = 0": lambda r: r["call"].endswith("_sharded") and r["scenes"] == 3 and r["n"] == 0 and r["rc"] == 0,
    "refused: no scenes": lambda r: r["call"].startswith("refuse 0 scenes") and "need 1..64 scenes" in r.get("error", ""),
    "refused: 65 scenes": lambda r: r["call"].startswith("refuse 65 scenes") and "need 1..64 scenes" in r.get("error", ""),
    "refused: null scene": lambda r: r["call"].startswith("refuse null scene") and "null scene" in r.get("error", ""),
    "refused: null rays": lambda r: r["call"].startswith("refuse null rays") and r["rc"] != 0,
    "refused: receivers differ": lambda r: r["call"].startswith("refuse receivers differ") and "differ in receivers" in r.get("error", ""),
}
SHARDED = ("shoot_sharded", "occluded_sharded", "bounce_sharded", "receive_sharded", "receive_source_sharded")


def build_stub(out_dir):
    so = os.path.join(str(out_dir), "libfake_hip.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "hare_amd", "csrc"), STUB_SRC, "-o", so])
    return so


# ---------------------------------------------------------------------------------------------------------------- the child
def child():
    import hare_amd as H
    from hare_amd import capi

    assert "torch" not in sys.modules
    L = capi.lib
    stub = ctypes.CDLL(os.environ["HARE_HIP_RUNTIME"])
    stub.fake_hip_log.restype = ctypes.c_char_p
    stub.fake_hip_name_host_range.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t]
    assert H.device_count() == 1 and L.hare_hip_runtime_path().decode() == os.environ["HARE_HIP_RUNTIME"]
    box = H.scenes.shoebox()
    tri = lambda: [H.Topology(box.verts, box.nverts)]
    makers = {"voxel8": lambda: H.Voxel_Grid(tri(), 8), "octree": lambda: H.Octree(tri(), 8, 16)}

    # the caller's buffers, made once: every call sees the same addresses under the same names
    B = dict(rays=H.scenes.random_rays(N_MAX, box.size).astype(np.float64), e1=np.full(N_MAX, -1, np.int32), e2=np.full(N_MAX, -1, np.int32),
             out=np.zeros(N_MAX, capi.XEVENT_DTYPE), tmax=np.full(N_MAX, 3.0), occ=np.zeros(N_MAX, np.int32), last=np.zeros(N_MAX, capi.XEVENT_DTYPE),
             state=np.zeros((2, N_MAX)), hist=np.zeros((1, BINS, 1), np.uint64), det=np.zeros((1, 2), np.uint64))
    for name, a in B.items():
        stub.fake_hip_name_host_range(name.encode(), a.ctypes.data, a.nbytes)
    P = {k: a.ctypes.data for k, a in B.items()}
    ctr = capi.Counters()
    pctr = ctypes.addressof(ctr)

    def handles(gs):
        return (ctypes.c_void_p * len(gs))(*[g._h if g is not None else None for g in gs])

    def per_stream(lines):
        streams = {}
        for l in lines:
            if l.startswith(("wait ", "record ")):
                continue
            for pat, to in NORMALIZE:
                l = pat.sub(to, l)
            st = [w for w in l.split() if re.fullmatch(r"s\d+", w)]
            assert len(st) == 1, l
            streams.setdefault(st[0], []).append(l)
        return streams

    def emit(g, scene, call, n, fn, n_scenes=1, chunks=0, warm=()):
        for w in warm:                       # sequential, each scene by itself, the full n
            w()
        before = [g.get_option(k) for k in ("hip_malloc_calls", "hip_free_calls")]
        stub.fake_hip_log_clear()
        rc = fn()
        row = dict(scene=scene, call=call, n=n, scenes=n_scenes, chunks=chunks, rc=rc)
        if rc:
            row["error"] = capi.last_error()
        row["streams"] = per_stream(stub.fake_hip_log().decode().splitlines())
        row["hip_calls"] = [g.get_option(k) - b for k, b in zip(("hip_malloc_calls", "hip_free_calls"), before)]
        print(json.dumps(row), flush=True)

    def shoot(g, n, flags=0, excl=False):
        return lambda: L.hare_shoot_batch(g._h, g._kind, 0, n, P["rays"], P["e1"] if excl else None, P["e2"] if excl else None, flags, P["out"], pctr)

    def occluded(g, n, events=False, excl=False):
        return lambda: L.hare_occluded_batch(g._h, g._kind, 0, n, P["rays"], P["e1"] if excl else None, P["e2"] if excl else None, P["tmax"], 0, P["occ"],
                                             P["out"] if events else None, pctr)

    def sharded(call, gs, n, rays=True, flags=0, events=False):
        h, G, kind = handles(gs), len(gs), next((g._kind for g in gs if g is not None), 0)
        r = P["rays"] if rays else None
        if call == "shoot_sharded":
            return lambda: L.hare_shoot_batch_sharded(h, G, kind, 0, n, r, None, None, flags, P["out"], pctr)
        if call == "occluded_sharded":
            return lambda: L.hare_occluded_batch_sharded(h, G, kind, 0, n, r, None, None, P["tmax"], 0, P["occ"], P["out"] if events else None, pctr)
        if call == "bounce_sharded":
            return lambda: L.hare_bounce_batch_sharded(h, G, kind, 0, n, r, None, None, BOUNCES, 0, None, P["last"], pctr, None)
        if call == "receive_sharded":
            return lambda: L.hare_receive_batch_sharded(h, G, kind, 0, n, r, None, None, BOUNCES, 0, BINS, 1.0, 40, None, P["state"], P["hist"], P["det"], pctr)
        assert call == "receive_source_sharded"
        return lambda: L.hare_receive_source_sharded(h, G, kind, 0, n, 0, BOUNCES, 0, BINS, 1.0, 40, P["state"], P["hist"], P["det"], pctr)

    # ---- hare_shoot_batch and hare_occluded_batch: the chunks
    for name in ("voxel8", "octree"):
        g = makers[name]()
        for chunks in (0, 3, 16):
            g.set_option("batch_chunks", chunks)
            for n in (0, 1, 5, N_MAX):
                for call, fn in (("shoot", shoot(g, n)), ("shoot excl", shoot(g, n, excl=True)), ("occluded", occluded(g, n)),
                                 ("occluded events", occluded(g, n, events=True)), ("occluded excl", occluded(g, n, excl=True))):
                    emit(g, name, call, n, fn, chunks=chunks, warm=(fn,))
            for call, flags in (("shoot slim", SLIM), ("shoot writeback", WRITEBACK), ("shoot slim writeback", SLIM | WRITEBACK)):
                for n in (5, N_MAX):
                    fn = shoot(g, n, flags)
                    emit(g, name, call, n, fn, chunks=chunks, warm=(fn,))
        g.close()

    # ---- the sharded calls: 1 and 3 scenes
    def receiving(g, radius=0.5):
        g.set_receivers([[5.0, 3.5, 2.0]], [radius])
        g.set_source([2.0, 2.0, 1.5])
        return g

    for name in ("voxel8", "octree"):
        gs = [receiving(makers[name]()) for _ in range(3)]
        for call in SHARDED if name == "voxel8" else SHARDED[:2]:
            for G in (1, 3):
                for n in (0, 1, 2, 5, N_MAX):
                    warm = [sharded(call, [g], N_MAX) for g in gs[:G]]
                    emit(gs[0], name, call, n, sharded(call, gs[:G], n), n_scenes=G, warm=warm)
        warm = [sharded("shoot_sharded", [g], N_MAX, flags=SLIM) for g in gs]
        emit(gs[0], name, "shoot_sharded slim", N_MAX, sharded("shoot_sharded", gs, N_MAX, flags=SLIM), n_scenes=3, warm=warm)
        warm = [sharded("occluded_sharded", [g], N_MAX, events=True) for g in gs]
        emit(gs[0], name, "occluded_sharded events", N_MAX, sharded("occluded_sharded", gs, N_MAX, events=True), n_scenes=3, warm=warm)
        # ---- refusals: code and message
        if name == "voxel8":
            many = gs * 22
            for call in SHARDED:
                emit(gs[0], name, "refuse 0 scenes " + call, 5, sharded(call, [], 5), n_scenes=0)
                emit(gs[0], name, "refuse 65 scenes " + call, 5, sharded(call, many[:65], 5), n_scenes=65)
                emit(gs[0], name, "refuse null scene " + call, 5, sharded(call, [gs[0], None, gs[2]], 5), n_scenes=3)
                if call != "receive_source_sharded":
                    emit(gs[0], name, "refuse null rays " + call, 5, sharded(call, gs, 5, rays=False), n_scenes=3)
            receiving(gs[2], radius=0.25)
            for call in SHARDED[3:]:
                emit(gs[0], name, "refuse receivers differ " + call, 5, sharded(call, gs, 5), n_scenes=3)
        for g in gs:
            g.close()
    stub.fake_hip_name_host_range(None, None, 0)
    assert stub.fake_hip_live_allocations() == 0


# ---------------------------------------------------------------------------------------------------------------- the parent
def run_child(stub):
    env = dict(os.environ, HARE_HIP_RUNTIME=stub, HARE_BUILD="host", FAKE_HIP_CUS="256")
    for k in ("HARE_DEV", "HARE_TUNE", "HARE_LIB", "FAKE_HIP_MISSING", "FAKE_HIP_BUFFERS", "HARE_BATCH_CHUNKS"):
        env.pop(k, None)
    env["PYTHONPATH"] = os.pathsep.join([p for p in sys.path if p])          # the package this process would import
    c = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True)
    assert c.returncode == 0, c.stdout[-2000:] + c.stderr[-4000:]
    return [json.loads(line) for line in c.stdout.splitlines()]


def brief(line):
    """one log line as the file holds it: a launch as `kernel grid x block / lds n`, a copy as `dst<-src:bytes`, a memset as `dst=0:bytes`"""
    w = line.split()
    f = dict(x.split("=", 1) for x in w if "=" in x)
    if w[0] == "launch":
        return "%s %sx%s/%s n%s" % (w[1], f["grid"], f["block"], f["lds"], f.get("n", "-"))
    if w[0] == "memcpy":
        return "%s<-%s:%s" % (w[1], w[3], f["bytes"])
    return "%s=%s:%s" % (w[1], f["value"], f["bytes"])


def compact(rows):
    """The rows as the file holds them, one JSON list per line: scene, call, n, scenes, the "batch_chunks" option, the return code (or [code,
    message]), per stream (sorted by its number) the brief lines, and the first 12 hex digits of the SHA-256 of the streams' full lines."""
    out = []
    for r in rows:
        order = sorted(r["streams"], key=lambda s: int(s[1:]))
        full = "\n".join(s + "\n" + "\n".join(r["streams"][s]) for s in order)
        out.append([r["scene"], r["call"], r["n"], r["scenes"], r["chunks"], [r["rc"], r["error"]] if r["rc"] else 0,
                    [[s] + [brief(l) for l in r["streams"][s]] for s in order], hashlib.sha256(full.encode()).hexdigest()[:12]])
    return out


@pytest.fixture(scope="module")
def traced(tmp_path_factory):
    return run_child(build_stub(tmp_path_factory.mktemp("fake_hip")))


def test_the_host_calls_enqueue_what_was_recorded(traced):
    want = [json.loads(l) for l in open(FIXTURE)]
    mine = compact(traced)
    assert [r[:5] for r in want] == [r[:5] for r in mine]                           # the fixture holds these cases, in this order
    for w, m, row in zip(want, mine, traced):
        assert w == m, "\nrecorded: %s\nnow:      %s\nin full:  %s" % (json.dumps(w), json.dumps(m), json.dumps(row))


def test_a_warmed_call_allocates_nothing(traced):
    for r in traced:
        assert r["hip_calls"] == [0, 0], r


def test_every_case_kind_has_a_row(traced):
    for name, pred in SHAPES.items():
        assert any(pred(r) for r in traced), name


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        child()
    elif len(sys.argv) == 3 and sys.argv[1] in ("--record", "--dump"):
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            recorded = run_child(build_stub(tmp))
        with open(sys.argv[2], "w") as f:
            for row in (compact(recorded) if sys.argv[1] == "--record" else recorded):
                f.write(json.dumps(row, separators=(",", ":")) + "\n")
        print(len(recorded), "rows;", "missing kinds:", [k for k, p in SHAPES.items() if not any(p(r) for r in recorded)])
    else:
        sys.exit(__doc__)
