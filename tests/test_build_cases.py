"""The partition builders' device cases cannot pass vacuously, and their reference is pinned (no GPU).  With tests.build_cases.reference
-- the oracle -- alone: every edge case reaches what it claims (the list lengths occur in the oracle's lists, the node counts in its
export, the `ct` is what it returns); the cover the device tests rely on is there; the host builder (scene option "build_host") equals
the oracle on every case and every sweep seed.  tests/golden/build_reference_digests.json holds tests.build_cases.digest of every edge
case and sweep seed, so that an edit of a generator shows as a diff.  A digest that changes on purpose is a change of the cases:
regenerate the file and say so."""
import numpy as np
import pytest

from tests import build_cases as bc
from tests.test_gpu_build_sweep import N

EDGES = {c.name: c for c in bc.edge_cases()}


def ref(name):
    return bc.reference(EDGES[name], keep=True)


def lengths_of(r):
    """Per topology the list length of every cell."""
    return [np.diff(s.astype(np.int64)) for s, _ in r["lists"]]


def tree_counts(case, r):
    """(leaf counts, list lengths of the nodes that split, every node's list length) of an exported tree.  A node that split has handed its
    list on (item_count 0).  The root's list is every polygon; a deeper node's was the union of its children's, counted here as their sum:
    exact where no polygon falls in two children, as in the cluster scenes, an upper bound elsewhere."""
    _, fc, _, cn, _ = r["nodes"]
    total = cn.astype(np.int64).copy()
    for n in range(len(fc) - 1, -1, -1):                                 # children are numbered after their parent
        if fc[n] >= 0:
            total[n] = total[fc[n]:fc[n] + 8].sum()
    total[0] = case.topos[0][0].shape[0]
    return cn[fc < 0], total[fc >= 0], total


def test_the_file_holds_exactly_the_cases():
    assert set(bc.pinned_digests()) == {"edge/" + n for n in EDGES} | {f"sweep/{s}" for s in range(N)}


@pytest.mark.parametrize("name", list(EDGES))
def test_edge_case_gives_the_pinned_result(name):
    assert bc.digest(ref(name)) == bc.pinned_digests()["edge/" + name], EDGES[name].describe()


@pytest.mark.parametrize("name", list(EDGES))
def test_host_builder_equals_the_oracle(name):
    case = EDGES[name]
    part = bc.build(case, host=True)
    assert part.info().built_on_device == 0
    bad = bc.compare(case, part, ref(name))
    assert bad is None, (case.describe(), bad)


@pytest.mark.parametrize("name", list(EDGES))
def test_edge_case_reaches_what_it_claims(name):
    case, r = EDGES[name], ref(name)
    reach = case.reaches
    if case.kind == "voxel":
        n = lengths_of(r)
        every = np.concatenate(n)
        assert r["ct"] == (reach["ct"] if "ct" in reach else case.builder[1] if case.builder[0] == "fixed" else r["ct"])
        for want in reach.get("lengths", ()):
            assert (every == want).any(), (name, want)
        if "P" in reach:
            assert case.P == reach["P"]
        if "lengths" in reach:                                           # no list is a contiguous index range: the atomic fill's order cannot be right by luck
            s, i = r["lists"][-1]
            c = int(np.argmax(n[-1]))
            assert not np.array_equal(np.diff(i[s[c]:s[c + 1]]), np.ones(n[-1][c] - 1, np.int32))
        if reach.get("quads"):
            nv = case.topos[0][1]
            assert 0.2 < (nv == 4).mean() < 0.3
        if "long_in" in reach:
            assert len(n) == 2 and n[0].max() < 4095 and {4095, 8192, 8193, 8194} <= set(n[1].tolist())
        if "scan_levels" in reach:
            counters = r["ct"] ** 3 + 1
            levels, m = 1, counters
            while m > bc.SCAN_BLOCK:
                m = (m + bc.SCAN_BLOCK - 1) // bc.SCAN_BLOCK
                levels += 1
            assert levels == reach["scan_levels"]
            assert n[0][:bc.SCAN_BLOCK].any() and n[0][-(counters % bc.SCAN_BLOCK or bc.SCAN_BLOCK) + 1:].any()      # first and last block of counters
            assert n[0][-1] > 0                                          # the far corner's triangle, in the grid's last cell
        if reach.get("on_planes"):
            v = case.topos[0][0]
            pts = v[:, :3].reshape(-1, 3)
            planes, low, high = bc.grid_planes(pts.min(axis=0), pts.max(axis=0), r["ct"])
            for a in range(3):
                assert np.isin(pts[:, a], planes[a]).sum() >= 10 and np.isin(pts[:, a], low[a]).any() and np.isin(pts[:, a], high[a]).any()
            mn, mx = r["oracle"].box(1, 1, 1)                            # the planes are the oracle's: cell (1, 1, 1)'s padded low faces
            assert np.array_equal(mn, low[:, 0])
            tri = v[:, :3]
            area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
            assert (area == 0).any() and (tri[:, 1] == tri[:, 2]).all(axis=1).any()
        if "mean8" in reach:
            at8 = bc.reference(bc.BuildCase("at-8", case.topos, ("adaptive", 3, 0)))
            every8 = np.concatenate(lengths_of(at8))
            assert at8["ct"] == 8 and every8.sum() == reach["mean8"] * np.count_nonzero(every8)
            if len(case.topos) == 2:                                     # neither topology alone has that mean
                assert all(x.sum() != reach["mean8"] * np.count_nonzero(x) for x in lengths_of(at8))
    else:
        leaves, split, total = tree_counts(case, r)
        for want in reach.get("leaf_counts", ()):
            assert (leaves == want).any(), (name, want)
        for want in reach.get("split_counts", ()) + reach.get("parent_counts", ()):
            assert (split == want).any(), (name, want, split)
        if "parent_min" in reach:
            assert split.max() >= reach["parent_min"]
        if "n_nodes" in reach:
            assert len(total) == reach["n_nodes"]
        if "parent_counts" in reach:
            assert r["nodes"][1][0] == 1 and case.P == reach["parent_counts"][0]


def test_the_mean_cases_differ_in_ct_by_one_unit_of_avg_polys():
    for tag in ("one", "two"):
        equal, above = ref(f"adaptive-mean-{tag}-equal"), ref(f"adaptive-mean-{tag}-above")
        assert EDGES[f"adaptive-mean-{tag}-above"].builder[2] == EDGES[f"adaptive-mean-{tag}-equal"].builder[2] + 1
        assert above["ct"] == 8 and equal["ct"] > 8


def test_the_cover_of_the_device_tests():
    """What tests/test_gpu_build_edges.py relies on, counted on the oracle."""
    fixed = [c for c in EDGES.values() if c.builder[0] == "fixed"]
    one_grid = lengths_of(ref("lengths-D4"))[0]
    assert (one_grid <= bc.SMALL_MAX).any() and ((one_grid > bc.SMALL_MAX) & (one_grid <= bc.BIG_LIST)).any() and (one_grid > bc.BIG_LIST).any()
    every = np.concatenate([x for c in fixed for x in lengths_of(ref(c.name))])
    for want in (bc.SMALL_MAX, bc.SMALL_MAX + 1, 4096, 4097, bc.BIG_LIST, bc.BIG_LIST + 1):
        assert (every == want).any(), want
    domains = {c.builder[1] for c in fixed}
    assert {12, 13, 80, 81, 160, 161, 162} <= domains
    assert 12 ** 3 + 1 <= bc.SCAN_BLOCK < 13 ** 3 + 1 and 161 ** 3 + 1 <= bc.SCAN_BLOCK ** 2 < 162 ** 3 + 1
    adaptive = {c.builder[1:] for c in EDGES.values() if c.builder[0] == "adaptive"}
    assert {(md, avg) for md in (1, 2, 3, 5) for avg in (0, 1, 10 ** 6)} <= adaptive
    assert {len(c.topos) for c in EDGES.values() if c.builder[0] == "adaptive"} == {1, 2}
    parents, survivors = set(), set()
    for c in EDGES.values():
        if c.kind == "octree":
            leaves, split, total = tree_counts(c, ref(c.name))
            parents |= set(split.tolist())
            survivors |= set(total.tolist())
    assert {bc.SEG - 1, bc.SEG, bc.SEG + 1, 2 * bc.SEG, 2 * bc.SEG + 1} <= parents and {255, 256, 257} <= survivors
    depths = {c.builder[1] for c in EDGES.values() if c.kind == "octree"}
    assert {0, 1} <= depths and any(len(c.topos) > 1 for c in EDGES.values() if c.kind == "octree")


@pytest.fixture(scope="module")
def sweep():
    return [(c, bc.reference(c)) for c in (bc.sweep_case(seed) for seed in range(N))]


def test_every_sweep_seed_gives_the_pinned_result_and_the_host_builder_equals_it(sweep):
    for seed, (case, r) in enumerate(sweep):
        assert 40 <= case.topos[0][0].shape[0] <= 3000 and len(case.topos) in (1, 2), case.describe()
        assert bc.digest(r) == bc.pinned_digests()[f"sweep/{seed}"], case.describe()
        bad = bc.compare(case, bc.build(case, host=True), r)
        assert bad is None, (case.describe(), bad)


def test_the_sweep_covers_the_builders(sweep):
    cases = [c for c, _ in sweep]
    for kind in ("fixed", "adaptive", "octree"):
        assert sum(c.builder[0] == kind for c in cases) >= 4, kind
    assert {len(c.topos) for c in cases} == {1, 2}
    assert {c.builder[1] for c in cases if c.builder[0] == "fixed"} <= set(bc.SWEEP_DOMAINS)
    assert all(c.builder[1] <= 5 for c in cases if c.builder[0] == "adaptive") and all(c.builder[1] <= 7 for c in cases if c.kind == "octree")
    device_trees = [r for c, r in sweep if c.kind == "octree" and len(c.topos) == 1 and len(r["nodes"][1]) > 1]
    assert len(device_trees) >= 3 and max(len(r["nodes"][4]) for r in device_trees) > 10_000
    assert any(np.concatenate(lengths_of(r)).max() > bc.SMALL_MAX for c, r in sweep if c.builder[0] == "fixed")
