"""The receive loop's termination rules (include/hare_hip.h, "receivers", "Termination") without a GPU: the flag's value, the two scene
options' ranges and read-back, the sharded call's refusal of scenes that differ in them before any device work -- and, with the numpy
restatement alone (tests/receive_ref.py), what the device tests rest on: with both rules off it returns what the loop returned before
it knew the rules (the pinned digests of tests/golden/receive_reference_digests.json); the time limit leaves the histogram and
detections[:, 0] as they are; the cases of tests/test_gpu_receive_cut.py are not vacuous (every
rule under test retires at least 10 % of the rays before the last cast, at least 10 % still run the last cast, a roulette has survivors
and casualties); and the roulette keeps every band's expected histogram total."""
import dataclasses

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from oracle import pyoracle as po
from tests.receive_cases import digest, oracle_of, pinned_digests, reference as any_reference
from tests.receive_cut_ref import cut_case, cut_cases, sweep_cut_case
from tests.receive_harness import same_bits
from tests.receive_ref import receive_loop

CASES = cut_cases()


def reference(cc):
    return any_reference(cc, keep=True)          # the fixed cases and their variants: shared, unchanged


def grid():
    m = H.scenes.shoebox()
    T = H.Topology(m.verts, m.nverts)
    return H.Voxel_Grid([T], 8), T


def test_the_flag_is_bit_512_in_the_header_and_the_mirror():
    hdr = open(capi.os.path.join(capi.os.path.dirname(capi._HERE), "include", "hare_hip.h")).read()
    assert "#define HARE_RECEIVE_TIME_LIMIT 512u" in hdr
    assert capi.RECEIVE_TIME_LIMIT == 512
    assert capi.RECEIVE_TIME_LIMIT & (capi.RECEIVE_DIFFUSE_RAIN | capi.RECEIVE_DIRECTIONAL | 0x7F) == 0


def test_the_options_have_their_ranges_defaults_and_read_back():
    g, _ = grid()
    assert g.get_option("receive_floor_bits") == 0 and g.get_option("receive_roulette") == 0
    for f in (1, 20, 1000, 0):
        g.set_option("receive_floor_bits", f)
        assert g.get_option("receive_floor_bits") == f
    for r in (1, 0):
        g.set_option("receive_roulette", r)
        assert g.get_option("receive_roulette") == r
    g.set_option("receive_floor_bits", 7)
    for name, bad in (("receive_floor_bits", -1), ("receive_floor_bits", 1001), ("receive_floor_bits", 1 << 40), ("receive_roulette", 2),
                      ("receive_roulette", -1)):
        with pytest.raises(H.HareError) as ei:
            g.set_option(name, bad)
        assert ei.value.code == capi.HARE_E_INVALID
    assert g.get_option("receive_floor_bits") == 7 and g.get_option("receive_roulette") == 0      # a refused call changes nothing


def test_the_sharded_call_refuses_scenes_that_differ_in_the_options_before_any_device_work():
    rays = H.scenes.burst_rays(128, H.scenes.shoebox().size)

    def pair():
        out = []
        for _ in range(2):
            g, _ = grid()
            out.append(g.set_receivers([[1.0, 1.0, 1.0]], [0.5]))
        return out

    for name, v0, v1 in (("receive_floor_bits", 20, 0), ("receive_floor_bits", 20, 21), ("receive_roulette", 1, 0)):
        a, b = pair()
        a.set_option(name, v0)
        b.set_option(name, v1)
        with pytest.raises(H.HareError) as ei:
            H.Voxel_Grid.Receive_batch_sharded([a, b], rays, 4, 100, 0.1)
        assert ei.value.code == capi.HARE_E_INVALID, name                  # not HARE_E_NODEVICE: nothing has touched a device yet
        assert "receive_floor_bits" in str(ei.value)
    # the roulette draws from "scatter_seed", with or without a scattering table
    a, b = pair()
    for g, seed in ((a, 1), (b, 2)):
        g.set_option("receive_floor_bits", 20).set_option("receive_roulette", 1).set_option("scatter_seed", seed)
    with pytest.raises(H.HareError) as ei:
        H.Voxel_Grid.Receive_batch_sharded([a, b], rays, 4, 100, 0.1)
    assert ei.value.code == capi.HARE_E_INVALID


@pytest.mark.parametrize("cc", [CASES[1], CASES[12], CASES[16], CASES[17]], ids=lambda cc: cc.name)
def test_with_both_rules_off_the_restatement_is_the_receive_loop(cc):
    """The digest was taken from the loop without the rules, before the one with them replaced it."""
    off = reference(cc.without(time_limit=False, floor_bits=0, roulette=False))
    assert digest(off) == pinned_digests()["rules-off/" + cc.name], cc.name
    assert off["per_cast"]["time"].sum() == 0 and off["per_cast"]["floor"].sum() == 0 and off["per_cast"]["boosted"].sum() == 0


@pytest.mark.parametrize("cc", [c for c in CASES if c.time_limit], ids=lambda cc: cc.name)
def test_the_time_limit_leaves_the_histogram_and_the_binned_detections_alone(cc):
    on, off = reference(cc), reference(cc.without(time_limit=False))
    assert same_bits(on["hist"], off["hist"]) is None
    assert same_bits(on["det"][:, 0], off["det"][:, 0]) is None
    assert on["hist"].any()
    assert on["det"][:, 1].sum() < off["det"][:, 1].sum()                   # the unbinned detections of the retired rays are gone


@pytest.mark.parametrize("cc", CASES, ids=lambda cc: cc.name)
def test_the_cases_are_not_vacuous(cc):
    pc, n = reference(cc)["per_cast"], cc.n
    print(cc.describe(), {k: v.tolist() for k, v in pc.items()})
    assert cc.time_limit or cc.floor_bits
    assert pc["time"][-1] == 0 and pc["floor"][-1] == 0 and pc["boosted"][-1] == 0           # the last cast decides nothing
    if cc.time_limit:
        assert pc["time"].sum() >= 0.1 * n
    else:
        assert pc["time"].sum() == 0
    if cc.floor_bits:
        assert pc["floor"].sum() >= 0.1 * n
    else:
        assert pc["floor"].sum() == 0 and pc["boosted"].sum() == 0
    if cc.roulette:
        assert pc["boosted"].sum() >= 0.1 * n                               # survivors beside the casualties counted above
    elif cc.floor_bits:
        assert pc["boosted"].sum() == 0
    assert pc["live"][-1] >= 0.1 * n
    if cc.scene[0] == "room-open":                                          # rays retire by missing too
        retired = n - pc["live"][-1]
        assert retired - pc["time"].sum() - pc["floor"].sum() >= 0.02 * n


def test_the_cases_cover_what_they_claim():
    def has(**kw):
        return any(all(getattr(c, k) == v for k, v in kw.items()) for c in CASES)
    for n in (63, 257, 4097, 4159):
        assert any(c.n == n for c in CASES)
    for kind in ("voxel", "octree", "kdtree"):
        assert any(c.partition[0] == kind for c in CASES)
    assert any(c.B == 1 for c in CASES) and any(c.B == 3 for c in CASES)
    for mode in ("specular", "scatter", "rain"):
        assert has(mode=mode)
    assert has(time_limit=True, floor_bits=0) and has(time_limit=False, roulette=False) and has(time_limit=False, roulette=True)
    assert has(time_limit=True, roulette=True)
    assert has(mode="specular", roulette=True)                              # the roulette without a scattering table
    assert has(directional=True) and has(pack=0) and has(pack=1) and has(aggregate=0) and has(aggregate=1) and has(device=True)
    assert any(c.state_in is not None and np.isnan(c.state_in[0]).any() and np.isinf(c.state_in[0]).any() for c in CASES)
    # both sides of the live-block list's threshold, on the partition that has the list, with it and without
    assert any(c.partition[0] == "voxel" and c.n >= 4096 and c.pack == 1 for c in CASES)
    assert any(c.partition[0] == "voxel" and c.n >= 4096 and c.pack == 0 for c in CASES)
    assert any(c.partition[0] == "voxel" and c.n < 4096 for c in CASES)


def test_a_sweep_seed_draws_every_rule_somewhere():
    drawn = [sweep_cut_case(s) for s in range(40)]
    assert any(c.time_limit for c in drawn) and any(not c.time_limit for c in drawn)
    assert any(c.floor_bits and c.roulette for c in drawn) and any(c.floor_bits and not c.roulette for c in drawn)
    assert any(c.floor_bits == 0 for c in drawn) and any(c.floor_bits == 1000 for c in drawn)


def test_the_roulette_keeps_every_bands_expected_histogram_total():
    """A shoebox with one alpha everywhere, 16 scatter seeds, the roulette against no floor at all: the seeds' mean histogram total per
    band agrees within three standard errors of the mean, the standard error being that of the 16 totals without a floor.  F = 2^-2 and
    alpha = 0.3: every ray passes under the floor at its fourth hit, so three quarters of the 24 casts are played by survivors.  (The
    plain floor at the same F loses a fifth of the total -- asserted too: the bound is not so wide that it would pass anything.)"""
    base = cut_case("unbiased", "roulette", 4096, B=3, mode="scatter")
    P = base.alpha.shape[0]
    alpha = np.full((P, 3), 0.3) * np.array([1.0, 0.9, 1.1])
    case = dataclasses.replace(base, alpha=alpha, sigma=np.full((P, 3), 0.5), bounces=24, n_bins=400, bin_len=0.5, frac_bits=30)
    To, o = oracle_of(case)

    def totals(seed, **rules):
        hist = receive_loop(po, To, o, case.rays, case.bounces, case.centers, case.radii, case.n_bins, case.bin_len, case.frac_bits, alpha=case.alpha,
                            sigma=case.sigma, seed=seed, **rules)[0]
        return hist.astype(np.float64).sum(axis=(0, 1)) * 2.0 ** -case.frac_bits                # [B]

    none = np.array([totals(s) for s in range(16)])
    roul = np.array([totals(s, floor_bits=2, roulette=True) for s in range(16)])
    plain = np.array([totals(s, floor_bits=2) for s in range(16)])
    sem = none.std(axis=0, ddof=1) / np.sqrt(16.0)
    print("no floor", none.mean(axis=0), "roulette", roul.mean(axis=0), "plain floor", plain.mean(axis=0), "standard error", sem)
    assert (np.abs(roul.mean(axis=0) - none.mean(axis=0)) <= 3.0 * sem).all(), (roul.mean(axis=0), none.mean(axis=0), sem)
    assert (none.mean(axis=0) - plain.mean(axis=0) > 3.0 * sem).all()
