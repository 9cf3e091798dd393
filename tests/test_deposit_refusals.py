"""What hare_direct_device, hare_image_device and hare_image2_device refuse before they touch a device (include/hare_hip.h, "receivers"):
each bad argument in turn, and pairs of bad arguments for the order in which the checks fire, against the code and the message recorded in
tests/golden/deposits/refusals.json.  That file is this module's own record of the commit BEFORE the three calls' checks were folded into
one (receive.cpp: deposit_call_check): `python tests/test_deposit_refusals.py --record FILE` with that commit's package first on the path;
it is never written from the code under test.  Every row is refused with HARE_E_INVALID ahead of the device, so the buffers are
addresses only, never memory, and the module needs no GPU.  A misaligned work array for hare_direct_device is no row: that call aligns the
array itself and goes on to the device."""
import json
import os
import sys

import numpy as np
import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deposits", "refusals.json")
WORK, HIST, DET = 0x7000_0000_0000, 0x7100_0000_0000, 0x7200_0000_0000          # far apart, 16-byte boundaries
CALLS = ("hare_direct_device", "hare_image_device", "hare_image2_device")
LISTS = {"hare_direct_device": (), "hare_image_device": ("max_pairs",), "hare_image2_device": ("max_cands", "max_paths")}


def cases():
    """(call, case, overrides of the good arguments) in a fixed order"""
    out = []
    for call in CALLS:
        rows = [("null scene", dict(scene=None)),
                ("weight 0", dict(n_weight=0)),
                ("weight 2^53 + 1", dict(n_weight=2 ** 53 + 1)),
                ("bad kind", dict(kind=99)),
                ("bad top_index", dict(top=7)),
                ("n_bins 0", dict(n_bins=0)),
                ("wrong band count", dict(bands=3))]
        for name in LISTS[call]:
            rows += [(name + " 0", {name: 0}), (name + " 2^26 + 1", {name: 2 ** 26 + 1})]
        rows += [("null work array", dict(work=0)), ("null histogram", dict(hist=0)), ("null detections", dict(det=0))]
        if LISTS[call]:
            rows += [("work array off a 16-byte boundary", dict(work=WORK + 8))]
        rows += [("histogram inside the work array", dict(hist=WORK + 16)),
                 ("detections inside the work array", dict(det=WORK + 32)),
                 ("detections inside the histogram", dict(det=HIST + 8)),
                 # two faults: the one that is reported
                 ("weight 0 and a null histogram", dict(n_weight=0, hist=0)),
                 ("bad top_index and overlapping buffers", dict(top=-1, det=HIST)),
                 ("wrong band count and a null work array", dict(bands=3, work=0)),
                 ("null detections and overlapping buffers", dict(det=0, hist=WORK))]
        for name in LISTS[call]:
            rows += [("bad top_index and " + name + " 0", {"top": 7, name: 0}),
                     ("wrong band count and " + name + " 0", {"bands": 3, name: 0}),
                     (name + " 0 and a null work array", {name: 0, "work": 0}),
                     (name + " 0 and a work array off a 16-byte boundary", {name: 0, "work": WORK + 8})]
        out += [(call, case, over) for case, over in rows]
    return out


def refusal(call, over):
    """(code, message) of one call: a shoebox with eight receivers and a source of `bands` bands (the topology has one)"""
    import hare_amd as H
    from hare_amd import capi

    a = dict(scene=True, kind=None, top=0, n_weight=1000, n_bins=16, bands=1, max_pairs=64, max_cands=64, max_paths=64, work=WORK, hist=HIST, det=DET)
    a.update(over)
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.set_receivers(np.array([[0.3 + 0.1 * k, 0.4, 0.5] for k in range(8)]), np.full(8, 0.05))
    g.set_source((0.5, 0.5, 0.5), power=np.ones(a["bands"]))
    lists = [a[name] for name in LISTS[call]]
    args = [g._h if a["scene"] else None, g._kind if a["kind"] is None else a["kind"], a["top"], a["n_weight"], 0, a["n_bins"], 0.01, 20]
    rc = getattr(capi.lib, call)(*args, *lists, a["work"], a["hist"], a["det"], None)
    return rc, capi.last_error()


def record():
    return [dict(call=call, case=case, code=rc, message=msg) for call, case, over in cases() for rc, msg in [refusal(call, over)]]


@pytest.mark.parametrize("call", CALLS)
def test_the_refusals_are_the_recorded_ones(call):
    from hare_amd import capi

    want = [r for r in json.load(open(FIXTURE)) if r["call"] == call]
    mine = [(c, case, over) for c, case, over in cases() if c == call]
    assert [r["case"] for r in want] == [case for _, case, _ in mine]              # the fixture holds these cases, in this order
    for r, (_, case, over) in zip(want, mine):
        assert r["code"] == capi.HARE_E_INVALID, r                                    # a row that went on to the device was not to be recorded
        rc, msg = refusal(call, over)
        assert (rc, msg) == (r["code"], r["message"]), (call, case, rc, msg, r)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit(__doc__)
    rows = record()
    json.dump(rows, open(sys.argv[2], "w"), indent=1)
    print(len(rows), "rows;", sum(r["code"] != -1 for r in rows), "with a code other than -1")
