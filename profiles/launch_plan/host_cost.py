"""Host cost of one hare_shoot_device call at n = 1 000 under the recording runtime of tests/stubs/fake_hip.cpp (logging off): the median of
5 000 calls, five repeats, per partition kind.  Run once per build, alternating:  HARE_HIP_RUNTIME=<libfake_hip.so> HARE_BUILD=host
PYTHONPATH=<tree> python host_cost.py <label>"""
import ctypes, os, sys, time
import numpy as np
import hare_amd as H
from hare_amd import capi

stub = ctypes.CDLL(os.environ["HARE_HIP_RUNTIME"])
stub.fake_hip_log_enable(0)
box = H.scenes.shoebox()
T = lambda: [H.Topology(box.verts, box.nverts)]
for name, g in (("voxel", H.Voxel_Grid(T(), 8)), ("octree", H.Octree(T(), 8, 16)), ("kdtree", H.KDTree(T(), 16, 8))):
    call = lambda: capi.lib.hare_shoot_device(g._h, g._kind, 0, 1000, 0x100000000000, None, None, 0, 0x110000000000, None, None)
    meds = []
    for rep in range(5):
        t = np.empty(5000)
        for k in range(5000):
            a = time.perf_counter_ns(); call(); t[k] = time.perf_counter_ns() - a
        meds.append(float(np.median(t)))
    print(sys.argv[1], name, "median ns per call, five repeats:", [round(m) for m in meds])
