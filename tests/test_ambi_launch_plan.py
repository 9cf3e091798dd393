"""Which kernels the receive plan picks for the order flags, read without a GPU as tests/test_launch_trace.py reads the shoot launcher:
a fresh child `python` runs the unmodified library against tests/stubs/fake_hip.cpp (HARE_HIP_RUNTIME), which executes nothing and logs
every launch.  The child calls hare_receive_device on five scenes -- no table, a scattering table, rain, a receiver map, a map with a
table -- and the three source-path calls, each with no channel flag, HARE_RECEIVE_DIRECTIONAL, and the flag with HARE_RECEIVE_ORDER2 and
_ORDER3, and prints the kernels launched.  The new names (_dir2, _dir3) must be chosen for the new flags and the old names otherwise."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_launch_trace import ADDR, build_stub

FLAGS = {"": 0, "_dir": 256, "_dir2": 256 | 131072, "_dir3": 256 | 1048576}
SCENES = {"plain": "hare_receive_reflect", "scatter": "hare_receive_scatter", "rain": "hare_receive_scatter_rain", "map": "hare_receive_reflect_map",
          "map-scatter": "hare_receive_scatter_map"}
RAIN = 128


def child():
    import ctypes

    import hare_amd as H
    from hare_amd import capi
    assert "torch" not in sys.modules
    stub = ctypes.CDLL(os.environ["HARE_HIP_RUNTIME"])
    stub.fake_hip_log.restype = ctypes.c_char_p
    box = H.scenes.shoebox(nface=1)
    A, n = ADDR, 4097
    rng = np.random.default_rng(1)

    def launched(fn):
        stub.fake_hip_log_clear()
        rc = fn()
        assert rc == 0, capi.last_error()
        return [l.split()[1] for l in stub.fake_hip_log().decode().splitlines() if l.startswith("launch ")]
    for scene in SCENES:
        g = H.Voxel_Grid([H.Topology(box.verts, box.nverts)], 4)
        centers, radii = rng.uniform(1.0, 3.0, (5, 3)), np.full(5, 0.5)
        (g.set_receiver_map if scene.startswith("map") else g.set_receivers)(centers, radii)
        g.set_absorption(np.full((12, 3), 0.1))
        if scene in ("scatter", "rain", "map-scatter"):
            g.set_scattering(np.full((12, 3), 0.5))
        g.set_source([3.0, 3.0, 1.5], power=[1.0, 1.0, 1.0])
        for suffix, flags in FLAGS.items():
            f = flags | (RAIN if scene == "rain" else 0)
            names = launched(lambda: capi.lib.hare_receive_device(g._h, g._kind, 0, n, A["rays"], None, None, 3, f, 16, 0.5, 30, A["out"], A["work"],
                                                                  A["last"], A["all"], A["tmax"], A["ctr"], None))
            print(json.dumps(dict(scene=scene, suffix=suffix, call="receive", names=names)), flush=True)
            if scene != "plain":
                continue
            for call, fn in (("direct", lambda: capi.lib.hare_direct_device(g._h, g._kind, 0, n, flags, 16, 0.5, 30, A["work"], A["all"], A["tmax"], None)),
                             ("image", lambda: capi.lib.hare_image_device(g._h, g._kind, 0, n, flags, 16, 0.5, 30, 64, A["work"], A["all"], A["tmax"], None)),
                             ("image2", lambda: capi.lib.hare_image2_device(g._h, g._kind, 0, n, flags, 16, 0.5, 30, 64, 64, A["work"], A["all"], A["tmax"],
                                                                            None))):
                print(json.dumps(dict(scene=scene, suffix=suffix, call=call, names=launched(fn))), flush=True)
        g.close()


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    stub = build_stub(tmp_path_factory.mktemp("fake_hip_ambi"))
    env = dict(os.environ, HARE_HIP_RUNTIME=stub, HARE_BUILD="host", FAKE_HIP_CUS="256",
               FAKE_HIP_BUFFERS=",".join("%s=%x" % (k, v) for k, v in ADDR.items()))
    for k in ("HARE_DEV", "HARE_TUNE", "HARE_LIB", "FAKE_HIP_MISSING"):
        env.pop(k, None)
    env["PYTHONPATH"] = os.pathsep.join([p for p in sys.path if p])
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return [json.loads(l) for l in p.stdout.splitlines()]


def test_the_receive_plan_picks_the_kernel_of_the_order(rows):
    seen = 0
    for r in rows:
        if r["call"] != "receive":
            continue
        want = SCENES[r["scene"]] + r["suffix"]
        receive = [k for k in r["names"] if k.startswith("hare_receive_")]
        assert receive and set(receive) == {want}, (r["scene"], r["suffix"], receive)
        rain = {k for k in r["names"] if k.startswith("hare_rain_step")}
        assert rain == ({"hare_rain_step" + r["suffix"]} if r["scene"] == "rain" else set()), (r["scene"], r["suffix"], rain)
        seen += 1
    assert seen == len(SCENES) * len(FLAGS)


def test_the_source_paths_pick_the_deposit_of_the_order(rows):
    seen = 0
    for r in rows:
        if r["call"] == "receive":
            continue
        deposit = [k for k in r["names"] if "_deposit" in k]
        assert deposit == ["hare_%s_deposit%s" % (r["call"], r["suffix"])], (r["call"], r["suffix"], r["names"])
        seen += 1
    assert seen == 3 * len(FLAGS)


if __name__ == "__main__" and "--child" in sys.argv:
    child()
