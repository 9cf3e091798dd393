"""What hare_scene_set_edges, hare_diffract_device and hare_diffract_paths refuse before they touch a device (include/hare_hip.h,
"receivers", "Edge diffraction (first order)"), each refusal in turn and pairs of faults for the order in which the checks fire;
HARE_E_NODEVICE on a host without a GPU; the edge count read back; and hare_amd.edges on the CPU.  The buffers of the device call are
addresses only, never memory: every row is refused ahead of the device."""
import ctypes as C

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi, edges
from tests import diffract_cases as dc

WORK, HIST, DET = 0x7000_0000_0000, 0x7100_0000_0000, 0x7200_0000_0000          # far apart, 16-byte boundaries
INVALID = capi.HARE_E_INVALID


def scene(bands=1, with_edges=True, table_bands=None):
    v, n, _, ends, faces = dc.screen_scene()
    g = H.Voxel_Grid([H.Topology(v, n)], 8)
    g.set_receivers(np.array([[6.0 + 0.2 * k, 3.5, 1.0] for k in range(8)]), np.full(8, 0.1))
    g.set_source(dc.SRC, power=np.ones(bands))
    if with_edges:
        g.set_edges(ends, faces, np.ones(table_bands or bands))
    return g, ends, faces


def set_edges(g, E, ends, faces, B, lam, top=0):
    e = None if ends is None else np.ascontiguousarray(ends, np.float64)
    f = None if faces is None else np.ascontiguousarray(faces, np.int32)
    w = None if lam is None else np.ascontiguousarray(lam, np.float64)
    return capi.lib.hare_scene_set_edges(g._h, top, E, capi.ptr(e), capi.ptr(f), B, capi.ptr(w)), capi.last_error()


def test_the_setter_refuses_in_the_stated_order_and_a_refused_call_changes_nothing():
    g, ends, faces = scene()
    assert g.get_option("edges") == 3 and g.get_option("edges:0") == 3
    one = np.ones(1)
    bad_end, same, bad_face = ends.copy(), ends.copy(), faces.copy()
    bad_end[1, 0, 2] = np.inf
    same[2, 1] = same[2, 0]
    bad_face[0, 1] = 13                                                              # P = 13: the faces are -1 .. 12
    rows = [("bad top_index", dict(top=3), "top_index"),
            ("E < 0", dict(E=-1), "E out of range"),
            ("E > 2^20", dict(E=2 ** 20 + 1), "E out of range"),
            ("E = 0 with arrays", dict(E=0), "E out of range"),
            ("null ends", dict(ends=None), "null ends"),
            ("a non-finite end", dict(ends=bad_end), "edge 1 has a non-finite end"),
            ("a == b", dict(ends=same), "edge 2 has no length"),
            ("a face beyond P - 1", dict(faces=bad_face), "faces[1]"),
            ("a face below -1", dict(faces=np.full_like(faces, -2)), "faces[0]"),
            ("B = 0", dict(B=0), "bands out of range"),
            ("B = 9", dict(B=9, lam=np.ones(9)), "bands out of range"),
            ("a NaN inv_lambda", dict(lam=np.array([np.nan])), "inv_lambda[0]"),
            ("a negative inv_lambda", dict(lam=np.array([-1.0])), "inv_lambda[0]"),
            ("an infinite inv_lambda", dict(lam=np.array([np.inf])), "inv_lambda[0]"),
            # two faults: the one that is reported
            ("E out of range and a bad face", dict(E=-1, faces=bad_face), "E out of range"),
            ("a non-finite end and a == b", dict(ends=np.concatenate([same[2:], bad_end[1:2]]), E=2, faces=faces[:2]), "edge 0 has no length"),
            ("a == b and a bad face", dict(ends=same, faces=bad_face), "edge 2 has no length"),
            ("a bad face and B = 0", dict(faces=bad_face, B=0), "faces[1]"),
            ("B = 0 and a NaN inv_lambda", dict(B=0, lam=np.array([np.nan])), "bands out of range")]
    for case, over, text in rows:
        a = dict(E=3, ends=ends, faces=faces, B=1, lam=one, top=0)
        a.update(over)
        rc, msg = set_edges(g, a["E"], a["ends"], a["faces"], a["B"], a["lam"], a["top"])
        assert rc == INVALID and text in msg, (case, rc, msg)
        assert g.get_option("edges") == 3, case
    # the row "a non-finite end and a == b": ends are checked edge by edge, finiteness first within an edge
    assert set_edges(g, 1, ends[:1], faces[:1], 1, one)[0] == capi.HARE_OK and g.get_option("edges") == 1
    g.set_edges(None, None, None)
    assert g.get_option("edges") == 0
    with pytest.raises(H.HareError):
        g.get_option("edges:5")


def call(g, name, over=()):
    a = dict(scene=True, kind=None, top=0, n_weight=1000, flags=0, n_bins=16, bin_len=0.25, frac_bits=20, max_detour=float("inf"), max_pairs=64,
             work=WORK, hist=HIST, det=DET)
    a.update(over)
    head = [g._h if a["scene"] else None, g._kind if a["kind"] is None else a["kind"], a["top"], a["n_weight"], a["flags"], a["n_bins"], a["bin_len"],
            a["frac_bits"], a["max_detour"], a["max_pairs"]]
    if name == "hare_diffract_device":
        rc = capi.lib.hare_diffract_device(*head, a["work"], a["hist"], a["det"], None)
    else:
        rc = capi.lib.hare_diffract_paths(*head, a["hist"], a["det"], a.get("found"))
    return rc, capi.last_error()


ROWS = [("null scene", dict(scene=None), "null scene"),
        ("an order flag without the directional one", dict(flags=capi.RECEIVE_ORDER2), "HARE_RECEIVE_ORDER2"),
        ("weight 0", dict(n_weight=0), "n_weight"),
        ("bad kind", dict(kind=99), "bad kind"),
        ("bad top_index", dict(top=7), "bad top_index"),
        ("n_bins 0", dict(n_bins=0), "n_bins"),
        ("bin_len 0", dict(bin_len=0.0), "bin_len"),
        ("frac_bits 63", dict(frac_bits=63), "frac_bits"),
        ("max_pairs 0", dict(max_pairs=0), "max_pairs"),
        ("max_pairs 2^26 + 1", dict(max_pairs=2 ** 26 + 1), "max_pairs"),
        ("max_detour NaN", dict(max_detour=float("nan")), "max_detour"),
        ("max_detour < 0", dict(max_detour=-1.0), "max_detour"),
        ("null histogram", dict(hist=0), "null"),
        ("null detections", dict(det=0), "null"),
        ("detections inside the histogram", dict(det=HIST + 8), "overlap"),
        # two faults: the one that is reported
        ("weight 0 and max_pairs 0", dict(n_weight=0, max_pairs=0), "n_weight"),
        ("bad top_index and max_detour NaN", dict(top=7, max_detour=float("nan")), "bad top_index"),
        ("max_pairs 0 and max_detour NaN", dict(max_pairs=0, max_detour=float("nan")), "max_pairs"),
        ("max_detour NaN and a null histogram", dict(max_detour=float("nan"), hist=0), "max_detour")]
DEVICE_ROWS = [("null work array", dict(work=0), "null"),
               ("work array off a 16-byte boundary", dict(work=WORK + 8), "16-byte"),
               ("histogram inside the work array", dict(hist=WORK + 16), "overlap"),
               ("max_detour < 0 and a null work array", dict(max_detour=-1.0, work=0), "max_detour")]


@pytest.mark.parametrize("name", ("hare_diffract_device", "hare_diffract_paths"))
def test_the_calls_refuse_in_the_stated_order(name):
    g, _, _ = scene()
    hist, det = np.zeros(8 * 16, np.uint64), np.zeros(16, np.uint64)
    host = dict(hist=hist.ctypes.data, det=det.ctypes.data) if name == "hare_diffract_paths" else {}
    for case, over, text in ROWS + (DEVICE_ROWS if name == "hare_diffract_device" else []):
        if name == "hare_diffract_paths" and "det" in over and over["det"] == HIST + 8:
            over = dict(over, det=hist.ctypes.data + 8)
        rc, msg = call(g, name, dict(host, **over))
        assert rc == INVALID and text in msg and (name in msg or "null scene" in msg), (name, case, rc, msg)
    assert not hist.any() and not det.any()


@pytest.mark.parametrize("name", ("hare_diffract_device", "hare_diffract_paths"))
def test_a_source_whose_bands_are_not_the_tables_is_refused(name):
    g, _, _ = scene(bands=1, table_bands=3)                                         # the topology has one band, as the source; the edge table three
    hist, det = np.zeros(8 * 16, np.uint64), np.zeros(16, np.uint64)
    host = dict(hist=hist.ctypes.data, det=det.ctypes.data) if name == "hare_diffract_paths" else {}
    rc, msg = call(g, name, host)
    assert rc == INVALID and "the edge table 3" in msg
    rc, msg = call(g, name, dict(host, max_detour=-1.0))                            # the detour is checked ahead of it
    assert rc == INVALID and "max_detour" in msg
    rc, msg = call(g, name, dict(host, hist=0))                                     # and the buffers behind it
    assert rc == INVALID and "the edge table 3" in msg
    g2, _, _ = scene(bands=3)                                                       # the topology's one band is checked first, as in hare_image_device
    rc, msg = call(g2, name, host)
    assert rc == INVALID and "the topology 1" in msg


@pytest.mark.parametrize("name", ("hare_diffract_device", "hare_diffract_paths"))
def test_behind_the_checks_come_the_device_and_then_the_state(name, gpu_available):
    hist, det = np.zeros(8 * 16, np.uint64), np.zeros(16, np.uint64)
    host = dict(hist=hist.ctypes.data, det=det.ctypes.data) if name == "hare_diffract_paths" else {}
    g2, _, _ = scene(with_edges=False)                                              # "no edges" is HARE_E_STATE, behind the device: nothing is enqueued
    rc, msg = call(g2, name, host)
    assert (rc == capi.HARE_E_STATE and "no edges set" in msg) if gpu_available else rc == capi.HARE_E_NODEVICE, (rc, msg)
    if not gpu_available:
        g, _, _ = scene()
        assert call(g, name, host)[0] == capi.HARE_E_NODEVICE


def test_the_work_bytes_are_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hare_hip.h")).read()
    m = re.search(r"#define HARE_DIFFRACT_WORK_BYTES\(K, max_pairs\) \((\d+) \+ (\d+) \* \(int64_t\)\(K\) \+ (\d+) \* \(int64_t\)\(max_pairs\)\)", text)
    assert m and H.Voxel_Grid.diffract_work_bytes(7, 11) == int(m.group(1)) + int(m.group(2)) * 7 + int(m.group(3)) * 11


# ---- hare_amd.edges
def test_a_closed_shoebox_seen_from_inside_has_no_diffracting_edge():
    for nface in (1, 3):
        m = H.scenes.shoebox(nface=nface)
        ends, faces = edges.find_edges(H.Topology(m.verts, m.nverts), 10.0)
        assert ends.shape == (0, 2, 3) and faces.shape == (0, 2)


def test_a_box_obstacle_in_the_shoebox_yields_its_twelve_edges_with_two_faces_each():
    v, n, _, want_ends, want_faces = dc.wedge_scene()
    ends, faces = edges.find_edges((v, n), 10.0)
    assert ends.shape == (12, 2, 3) and (faces >= 12).all() and (faces[:, 0] != faces[:, 1]).all()
    key = lambda e, f: (tuple(sorted(map(tuple, e.tolist()))), tuple(sorted(f.tolist())))
    assert sorted(key(e, f) for e, f in zip(ends, faces)) == sorted(key(e, f) for e, f in zip(want_ends, want_faces))
    assert edges.find_edges((v, n), 95.0)[0].shape[0] == 0                          # right angles open by 90 degrees


def test_a_screen_yields_its_free_edges():
    v, n, _, want_ends, _ = dc.screen_scene()
    ends, faces = edges.find_edges((v, n))
    assert ends.shape[0] == 4 and (faces[:, 0] == 12).all() and (faces[:, 1] == -1).all()      # the three of the case and the one on the floor
    have = {tuple(sorted(map(tuple, e.tolist()))) for e in ends}
    assert all(tuple(sorted(map(tuple, e.tolist()))) in have for e in want_ends)


def test_band_inv_lambda():
    assert (edges.band_inv_lambda([0.0, 343.0, 686.0], 343.0) == np.array([0.0, 1.0, 2.0])).all()
    with pytest.raises(ValueError):
        edges.band_inv_lambda([-1.0])
