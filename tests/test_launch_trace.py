"""What the shoot launcher launches (hare_amd/csrc/launch.cpp: the kernel choice, the launch geometry, the scratch requests), pinned without a
GPU: hiprt.cpp binds the HIP runtime HARE_HIP_RUNTIME names, so a fresh child `python` that imports only numpy and hare_amd -- never torch,
which would map libamdhip64 -- runs the whole unmodified library against tests/stubs/fake_hip.cpp, a stand-in that executes nothing and logs
every launch (kernel, grid, block, LDS, both argument structs decoded), memset, copy, event wait and event record.  The child walks a fixed
case list and prints one row per call: the two hare_shoot_kernel_name answers (plain and with HARE_SHOOT_BOUNCE_LOOP), the return code (and the
message of a refusal), the log of the call, "octree_scratch_bytes" and "voxel_order_bytes", and what the call added to "hip_malloc_calls" /
"hip_free_calls" / "hip_sync_calls".  The parent compares the rows with tests/golden/launch/trace.json.

That file is this module's own record of the commit BEFORE the launcher was folded into one launch plan: `python tests/test_launch_trace.py
--record FILE` with that commit's package first on the path; it is never written from the code under test, and no row of it is edited by hand.
The stub and this module run unchanged on both commits.  Caller buffers are addresses only (as in tests/test_deposit_refusals.py).

The file holds one short row per call (compact() below): the names, the code, each launch as kernel, grid, block, LDS and the fields the
launch plan sets, and a digest of the call's full log, which pins every other decoded field and pointer.

Scenes: the 972-triangle shoebox and a box of six quadrilaterals; Voxel_Grid at D = 8 and at D = 81, the smallest D whose occupancy bitmap is
coarse (81^3 bits pass the 64 KiB the kernels stage; scene.h: occ_layout); Octree at the bench's (8, 16), six interior levels, and at (7, 2), seven (K2g's stack
spills from four); KDTree.  hare_octree_build caps maxDepth at 24 and K2d's LDS at 24 levels is 126 976 bytes: no tree that can be built takes
it past the 160 KiB of a workgroup, so the fall-back to K2p for want of LDS has no row.  Every other launch shape has one: SHAPES below is
asserted against the rows, so a thinned case list cannot silently lose one (the audit and the profiling build run on a scene with the `dev`
option, which the stub reaches like any other).  Two further children run on a code object that lacks kernels (MISSING below): the
fall-backs of the kernel choice, and a reservation that does not depend on what the code object holds."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "launch", "trace.json")
STUB_SRC = os.path.join(HERE, "stubs", "fake_hip.cpp")
CUS = (256, 8)
# further children on 256 CUs whose code object lacks these kernels: the pool / occlusion / fused members and K2d with K2g-tail; one K1p member
MISSING = ("hare_voxel_pool_tri,hare_voxel_occl_tri,hare_voxel_bounce_tri,hare_octree_dense,hare_octree_group_tail", "hare_voxel_persist_quad_g")
BUFFERS = ("rays", "out", "e1", "e2", "ctr", "tmax", "occ", "work", "all", "last", "ctrc")
ADDR = {name: 0x1000_0000_0000 + (k << 40) for k, name in enumerate(BUFFERS)}       # far apart, 16-byte boundaries; never memory
COUNT_WORK, SIMPLE, RETIRED, BOUNCE_LOOP, COUNT_OWN = 2, 4, 8, 32, 64
ORDER_MIN = 1572864          # kOrderMinRays (hare_device.h)

# launch shape -> a pattern one row's log must match (launch lines joined by " > ")
SHAPES = {
    "voxel simple": r"^hare_voxel_shoot_(tri|quad)$", "voxel count": r"^hare_voxel_shoot_count$", "voxel audit": r"^hare_cull_audit$",
    "voxel prof": r"^hare_voxel_persist_prof$", "voxel pool": r"^hare_voxel_pool_\w+$", "voxel pool + order pass": r"^hare_cost_order > hare_voxel_pool_\w+$",
    "voxel persist": r"^hare_voxel_persist_(tri|quad)(_g)?$", "voxel occl": r"^hare_voxel_occl_\w+$",
    "octree simple": r"^hare_octree_shoot$", "octree pool": r"^hare_octree_pool$", "octree group": r"^hare_octree_group$",
    "octree persist + K2t": r"^hare_octree_persist > hare_octree_tail$", "octree persist + K2g-tail": r"^hare_octree_persist > hare_octree_group_tail$",
    "octree dense": r"^hare_octree_dense$", "octree occl": r"^hare_octree_occl$", "octree occl_any": r"^hare_octree_occl_any$",
    "kd simple": r"^hare_kdtree_shoot$", "kd dense": r"^hare_kdtree_dense$", "kd occl": r"^hare_kdtree_occl$",
    "fused bounce loop": r"hare_voxel_bounce_\w+$", "per-cast loop with the block list": r"hare_reflect > hare_live_blocks > hare_voxel_pool",
    "per-cast loop without the block list": r"hare_voxel_pool_\w+ > hare_reflect > hare_voxel_pool_\w+( > hare_reflect > hare_voxel_pool_\w+)*$",
}


def build_stub(out_dir):
    so = os.path.join(str(out_dir), "libfake_hip.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "hare_amd", "csrc"), STUB_SRC, "-o", so])
    return so


# ---------------------------------------------------------------------------------------------------------------- the child
def quad_box():
    c = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [0, 0, 2], [2, 0, 2], [2, 2, 2], [0, 2, 2]], np.float64)
    f = [[0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 5, 4], [3, 2, 6, 7], [0, 3, 7, 4], [1, 2, 6, 5]]
    return c[np.array(f)], np.full(6, 4, np.int32)


def n_list(cus, kind):
    fill = cus * 12 * 128                # rays in flight when every pool of the chip is full
    full = [1, 63, 64, 65, 1000, 4097, 4159, 65537, 320 * cus - 1, 320 * cus, 1280 * cus - 1, 1280 * cus, 2 * fill - 1, 2 * fill,
            ORDER_MIN - 1, ORDER_MIN, 6291456, 12582912, 0x7FFFFF00]
    return sorted(set(full))


def child(cus):
    import hare_amd as H
    from hare_amd import capi

    assert "torch" not in sys.modules
    stub = ctypes.CDLL(os.environ["HARE_HIP_RUNTIME"])
    stub.fake_hip_log.restype = ctypes.c_char_p
    assert H.device_count() == 1 and capi.lib.hare_hip_runtime_path().decode() == os.environ["HARE_HIP_RUNTIME"]
    box = H.scenes.shoebox()
    tri = lambda: [H.Topology(box.verts, box.nverts)]
    quad = lambda: [H.Topology(*quad_box())]
    A = ADDR
    fill = cus * 12 * 128

    def emit(g, scene, opts, call, n, fn):
        names = [g.kernel_name(n), g.kernel_name(n, flags=BOUNCE_LOOP)]
        before = [g.get_option(k) for k in ("hip_malloc_calls", "hip_free_calls", "hip_sync_calls")]
        stub.fake_hip_log_clear()
        rc = fn()
        row = dict(cus=cus, scene=scene, opts=opts, call=call, n=n, names=names, rc=rc)
        if rc:
            row["error"] = capi.last_error()
        row["log"] = stub.fake_hip_log().decode().splitlines()
        row["scratch"] = g.get_option("octree_scratch_bytes")
        row["order"] = g.get_option("voxel_order_bytes")
        row["hip_calls"] = [g.get_option(k) - b for k, b in zip(("hip_malloc_calls", "hip_free_calls", "hip_sync_calls"), before)]
        print(json.dumps(row), flush=True)

    def shoot(g, n, flags=0, excl=False, ctr=False):
        return lambda: capi.lib.hare_shoot_device(g._h, g._kind, 0, n, A["rays"], A["e1"] if excl else None, A["e2"] if excl else None, flags, A["out"],
                                                  A["ctr"] if ctr else None, None)

    def occluded(g, n, tmax, events):
        return lambda: capi.lib.hare_occluded_device(g._h, g._kind, 0, n, A["rays"], None, None, A["tmax"] if tmax else None, 0, A["out"] if events else None,
                                                     A["occ"], None, None)

    def bounce(g, n, casts, every, flags=0):
        return lambda: capi.lib.hare_bounce_device(g._h, g._kind, 0, n, A["rays"], None, None, casts, flags, A["work"], A["all"] if every else None,
                                                   None if every else A["last"], A["ctr"], A["ctrc"] if every else None, None)

    def scene(name, make, opts=(), env=None):
        for k, v in (env or {}).items():
            os.environ[k] = v
        g = make()
        for k in env or {}:
            del os.environ[k]
        for k, v in opts:
            g.set_option(k, v)
        label = ",".join("%s=%s" % kv for kv in list((env or {}).items()) + list(opts))
        return g, name, label

    def standard_calls(g, name, label, sizes):
        """every n with flags 0; the other flags, the exclusion arrays and the occlusion calls at a few"""
        for n in sizes:
            emit(g, name, label, "shoot", n, shoot(g, n))
        few = [n for n in (1000, 2 * fill, ORDER_MIN) if n in sizes]
        for n in few:
            for fname, f in (("count_work", COUNT_WORK), ("simple", SIMPLE), ("count_own", COUNT_OWN), ("retired", RETIRED)):
                emit(g, name, label, "shoot " + fname, n, shoot(g, n, f, ctr=True))
            emit(g, name, label, "shoot excl", n, shoot(g, n, excl=True))
        for n in [n for n in (1000, 320 * cus, 0x7FFFFF00) if n in sizes]:
            emit(g, name, label, "occluded t_max", n, occluded(g, n, True, False))
            emit(g, name, label, "occluded any", n, occluded(g, n, False, False))
            emit(g, name, label, "occluded events", n, occluded(g, n, True, True))

    sizes = n_list(cus, None)
    few_sizes = [1000, 320 * cus, 2 * fill]
    makers = {
        "voxel8": lambda: H.Voxel_Grid(tri(), 8), "voxel81": lambda: H.Voxel_Grid(tri(), 81), "voxel8q": lambda: H.Voxel_Grid(quad(), 8),
        "voxel81q": lambda: H.Voxel_Grid(quad(), 81), "octree": lambda: H.Octree(tri(), 8, 16), "octree_deep": lambda: H.Octree(tri(), 7, 2),
        "octree_q": lambda: H.Octree(quad(), 8, 16), "kdtree": lambda: H.KDTree(tri(), 16, 8), "kdtree_q": lambda: H.KDTree(quad(), 16, 8),
    }
    # ---- a code object that lacks kernels (FAKE_HIP_MISSING, a process of its own: the module is loaded once): the fall-backs
    if os.environ.get("FAKE_HIP_MISSING"):
        lacks = "lacks " + os.environ["FAKE_HIP_MISSING"]
        for name, opts in (("voxel8", (("bounce_fused", 1),)), ("octree", ()), ("octree", (("octree_kernel", 1),))):
            g, nm, label = scene(name, makers[name], opts)
            label = lacks + ("," + label if label else "")
            for n in few_sizes:
                emit(g, nm, label, "shoot", n, shoot(g, n))
            emit(g, nm, label, "shoot count_own", 2 * fill, shoot(g, 2 * fill, COUNT_OWN, ctr=True))
            emit(g, nm, label, "occluded t_max", 1000, occluded(g, 1000, True, False))
            emit(g, nm, label, "bounce 2 last", 4159, bounce(g, 4159, 2, False))
            g.close()
        return
    # ---- the library's rule, every size
    for name in ("voxel8", "voxel81", "octree", "octree_deep", "kdtree"):
        g, nm, label = scene(name, makers[name])
        standard_calls(g, nm, label, sizes)
        g.close()
    for name in ("voxel8q", "voxel81q", "octree_q", "kdtree_q"):
        g, nm, label = scene(name, makers[name])
        standard_calls(g, nm, label, [n for n in few_sizes])
        g.close()
    # ---- the bounce loop (a launch per cast logs three lines a cast: the long loops run once per path)
    fused, unpacked = ("bounce_fused", 1), ("bounce_pack", 0)
    for name, opt_sets in (("voxel8", ((), (fused,), (unpacked,), (fused, unpacked))), ("voxel81q", ((), (fused,)))):
        for opts in opt_sets:
            g, nm, label = scene(name, makers[name], opts)
            for n in (1000, 4159):                      # below and above the 4 096 rays the block list starts at
                for casts in (1, 2, 3, 16):
                    if casts == 16 and not (fused in opts and name == "voxel8"):
                        continue
                    for every in (False, True):
                        emit(g, nm, label, "bounce %d %s" % (casts, "all" if every else "last"), n, bounce(g, n, casts, every))
            if name == "voxel8" and unpacked not in opts:
                emit(g, nm, label, "bounce 17 last", 1000, bounce(g, 1000, 17, False))
            emit(g, nm, label, "bounce 2 last simple", 4159, bounce(g, 4159, 2, False, SIMPLE))
            g.close()
    for name in ("octree", "kdtree"):
        g, nm, label = scene(name, makers[name])
        emit(g, nm, label, "bounce 2 last", 4159, bounce(g, 4159, 2, False))
        g.close()
    # ---- the options, one at a time off their defaults
    voxel_opts = [("voxel_kernel", 1), ("voxel_kernel", 2), ("ticket_rays", 4), ("ticket_rays", 48), ("k1p_static_rays", 40), ("coop_tail", 0), ("wide_drain", 0),
                  ("voxel_walk", 0), ("voxel_overlap", 1), ("voxel_skip", 1), ("voxel_tight", 0), ("voxel_order", 0), ("voxel_order", 2)]
    for opt in voxel_opts:
        for name in ("voxel8", "voxel81") if opt[0] in ("voxel_kernel", "voxel_overlap", "voxel_skip") else ("voxel8",):
            g, nm, label = scene(name, makers[name], (opt,))
            for n in few_sizes + ([ORDER_MIN] if opt[0] == "voxel_order" else []):
                emit(g, nm, label, "shoot", n, shoot(g, n))
            emit(g, nm, label, "shoot count_own", 1000, shoot(g, 1000, COUNT_OWN, ctr=True))
            emit(g, nm, label, "shoot excl", 2 * fill, shoot(g, 2 * fill, excl=True))
            g.close()
    g, nm, label = scene("voxel8", makers["voxel8"], (("voxel_kernel", 1), ("k1p_static_rays", 40)))
    for n in few_sizes:
        emit(g, nm, label, "shoot", n, shoot(g, n))
    g.close()
    octree_opts = [[("octree_kernel", k)] for k in (1, 2, 3, 4)] + [[("octree_tail", 0)], [("octree_tail", 1)], [("k2p_tail_max", 8)], [("k2p_tail_patience", 5)]]
    octree_opts += [[("octree_kernel", 1), o] for o in (("octree_tail", 0), ("octree_tail", 1), ("k2p_tail_max", 8), ("k2p_tail_patience", 5), ("ticket_rays", 48),
                                                        ("k2p_static_rays", 40), ("coop_tail", 0))]
    octree_opts += [[("ticket_rays", 48)], [("k2p_static_rays", 40)], [("octree_tight", 0)]]
    for opts in octree_opts:
        for name in ("octree", "octree_deep") if opts[0][0] == "octree_kernel" else ("octree",):
            g, nm, label = scene(name, makers[name], tuple(opts))
            for n in few_sizes:
                emit(g, nm, label, "shoot", n, shoot(g, n))
            emit(g, nm, label, "shoot count_own", 2 * fill, shoot(g, 2 * fill, COUNT_OWN, ctr=True))
            emit(g, nm, label, "occluded any", 1000, occluded(g, 1000, False, False))
            g.close()
    for opt in (("kdtree_kernel", 1), ("kdtree_kernel", 2), ("ticket_rays", 48), ("k2p_static_rays", 40), ("octree_tight", 0)):
        g, nm, label = scene("kdtree", makers["kdtree"], (opt,))
        for n in few_sizes:
            emit(g, nm, label, "shoot", n, shoot(g, n))
        emit(g, nm, label, "occluded t_max", 1000, occluded(g, 1000, True, False))
        g.close()
    # ---- a `dev` scene: the developer flag bits pass, HARE_TUNE is read
    for env in ({"HARE_DEV": "1"}, {"HARE_DEV": "1", "HARE_TUNE": "6,24,96,3,12"}):
        for name in ("voxel8", "voxel81", "octree", "kdtree") if len(env) == 1 else ("voxel8", "octree", "kdtree"):
            g, nm, label = scene(name, makers[name], env=env)
            for n in (1000, 2 * fill):
                emit(g, nm, label, "shoot", n, shoot(g, n, ctr=True))
                for bit in (0x1000, 0x2000, 0x4000, 0x8000):
                    emit(g, nm, label, "shoot 0x%x" % bit, n, shoot(g, n, bit, ctr=True))
            emit(g, nm, label, "shoot 0x4000 no counters", 1000, shoot(g, 1000, 0x4000))
            emit(g, nm, label, "occluded t_max", 1000, occluded(g, 1000, True, False))
            if name.startswith("voxel"):
                g.set_option("voxel_kernel", 1)
                for n in (1000, 2 * fill):
                    emit(g, nm, label + ",voxel_kernel=1", "shoot", n, shoot(g, n, ctr=True))
                    emit(g, nm, label + ",voxel_kernel=1", "shoot 0x4000", n, shoot(g, n, 0x4000, ctr=True))
            g.close()
    assert stub.fake_hip_live_allocations() == 0


# ---------------------------------------------------------------------------------------------------------------- the parent
def run_children(stub):
    """the full rows of every child"""
    rows, children = [], []
    for cus, missing in [(c, None) for c in CUS] + [(256, m) for m in MISSING]:          # side by side: each is a process of its own
        env = dict(os.environ, HARE_HIP_RUNTIME=stub, HARE_BUILD="host", FAKE_HIP_CUS=str(cus),
                   FAKE_HIP_BUFFERS=",".join("%s=%x" % (k, v) for k, v in ADDR.items()))
        for k in ("HARE_DEV", "HARE_TUNE", "HARE_LIB", "FAKE_HIP_MISSING"):
            env.pop(k, None)
        if missing:
            env["FAKE_HIP_MISSING"] = missing
        env["PYTHONPATH"] = os.pathsep.join([p for p in sys.path if p])          # the package this process would import
        children.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", str(cus)], env=env, stdout=subprocess.PIPE,
                                         stderr=subprocess.PIPE, text=True))
    for c in children:
        out, err = c.communicate()
        assert c.returncode == 0, out[-2000:] + err[-4000:]
        rows += [json.loads(line) for line in out.splitlines()]
    return rows


PLAN_FIELDS = (("ticket_rays", "t"), ("static_rays", "s"), ("walk_steps", "w"), ("refill_min_idle", "r"), ("oct_tail_max", "tm"), ("oct_tail_patience", "tp"),
               ("oct_tail_stride", "ts"), ("oct_spill_cap", "sp"), ("bounce_casts", "bc"))


def brief(line):
    """one log line as the file holds it: a launch as `kernel grid x block lds` and what the plan put into ShootIO; the other calls by their size"""
    w = line.split()
    if w[0] != "launch":
        return w[0] + "".join(":" + x[6:] for x in w if x.startswith("bytes="))
    f = dict(x.split("=", 1) for x in w[2:] if "=" in x)
    return "%s %sx%s/%s" % (w[1], f["grid"], f["block"], f["lds"]) + "".join(" %s%s" % (short, f[name]) for name, short in PLAN_FIELDS if name in f)


def compact(rows):
    """The rows as the file holds them, one JSON list per line.  A row of three names the group (cus, scene, options) of the rows behind it.  A
    case row: call, n, the kernel names (one when both answers agree), the return code (or [code, message]), the brief log, octree_scratch_bytes,
    voxel_order_bytes, the runtime calls made (when any), and the first 12 hex digits of the SHA-256 of the FULL log -- every decoded field,
    every pointer -- which is what pins the rest.  `--dump FILE` writes the full rows of the package on the path, to diff two commits with."""
    import hashlib
    out, group = [], None
    for r in rows:
        if (r["cus"], r["scene"], r["opts"]) != group:
            group = (r["cus"], r["scene"], r["opts"])
            out.append(list(group))
        names = r["names"][0] if r["names"][0] == r["names"][1] else r["names"]
        calls = r["hip_calls"] if any(r["hip_calls"]) else 0
        out.append([r["call"], r["n"], names, [r["rc"], r["error"]] if r["rc"] else 0, [brief(l) for l in r["log"]], r["scratch"], r["order"], calls,
                    hashlib.sha256("\n".join(r["log"]).encode()).hexdigest()[:12]])
    return out


def shape_of(row):
    return " > ".join(l.split()[1] for l in row["log"] if l.startswith("launch "))


@pytest.fixture(scope="module")
def traced(tmp_path_factory):
    return run_children(build_stub(tmp_path_factory.mktemp("fake_hip")))


def test_the_launches_are_the_recorded_ones(traced):
    want = [json.loads(l) for l in open(FIXTURE)]
    mine = compact(traced)
    assert [r[:2] for r in want] == [r[:2] for r in mine]                           # the fixture holds these cases, in this order
    full = iter(traced)
    for w, m in zip(want, mine):
        row = next(full) if len(m) > 3 else None
        assert w == m, "\nrecorded: %s\nnow:      %s\nin full:  %s" % (json.dumps(w), json.dumps(m), json.dumps(row))


def test_every_launch_shape_has_a_row(traced):
    shapes = [shape_of(r) for r in traced]
    for name, pattern in SHAPES.items():
        assert any(re.search(pattern, s) for s in shapes), name


def test_a_shoot_allocates_nothing_but_the_octree_pool_ring(traced):
    """hare_shoot_device is stream-ordered: no hipMalloc, hipFree or host-side wait -- K2q's private scratch ring apart, which allocates on first use"""
    for r in traced:
        if r["call"].startswith(("shoot", "occluded")) and "hare_octree_pool" not in shape_of(r):
            assert r["hip_calls"] == [0, 0, 0], r


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    elif len(sys.argv) == 3 and sys.argv[1] in ("--record", "--dump"):
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            recorded = run_children(build_stub(tmp))
        with open(sys.argv[2], "w") as f:
            for row in (compact(recorded) if sys.argv[1] == "--record" else recorded):
                f.write(json.dumps(row, separators=(",", ":")) + "\n")
        found = [shape_of(r) for r in recorded]
        print(len(recorded), "rows;", "missing shapes:", [k for k, p in SHAPES.items() if not any(re.search(p, s) for s in found)])
    else:
        sys.exit(__doc__)
