#!/usr/bin/env python3
"""Generate golden G16 (``g16_model_prep.npz``) by running the REFERENCE's model-preparation code on the clouds of ``synth.make_model_prep_inputs``.

Runs by hand, and only where the reference checkout is present (see make_golden.py); only its outputs are stored, arrays all of them.  Per case:
  "fps"      the index vector at K = 256 of ``farthest_point_sampling_init_center``: the reference's farthest_point_sampling.cpp is built with the
             host compiler into a temporary directory outside the repository, loaded with ctypes, called as core/csrc/fps/fps_utils.py:10-21 calls
             it (fp32 contiguous points, int32 indices), and the directory is removed: nothing compiled is kept
  "diameter" ``misc.calc_pts_diameter``
  "bbox"     ``misc.get_bbox3d_and_center`` (float32 [9,3])
  "extents"  the arithmetic of core/gdrn_modeling/data_loader.py:266-273 (float32 [3])
  "mean"     ``np.average`` per axis, as core/utils/data_utils.py:205-207 takes it
and the wall time of the reference's FPS (K = 256) and of ``calc_pts_diameter`` on this host is printed.  With ``--workload`` nothing is written:
the two are timed on the clouds of ``synth.make_model_prep_workload()``, what tools/model_prep_time.py times on the device (about 20 minutes:
the diameter of the 259 854-vertex object is 3.4e10 pairs in a Python loop).

Usage:  python tests/golden/make_golden_g16.py [--workload]
"""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, install_shims  # noqa: E402

K = 256


def load_reference_fps(tmp):
    src = os.path.join(REF, "core", "csrc", "fps", "src", "farthest_point_sampling.cpp")
    so = os.path.join(tmp, "libfps_ref.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.farthest_point_sampling_init_center.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.farthest_point_sampling_init_center.restype = None

    def fps(pts, sn):   # fps_utils.farthest_point_sampling(pts, sn, init_center=True), returning the indices
        pts = np.ascontiguousarray(pts, np.float32)
        idxs = np.ascontiguousarray(np.zeros([sn], np.int32))
        lib.farthest_point_sampling_init_center(pts.ctypes.data, idxs.ctypes.data, pts.shape[0], sn)
        return idxs

    return fps


def time_workload(fps, misc, synth):
    clouds = synth.make_model_prep_workload()
    t_fps = t_diam = 0.0
    for c, pts in enumerate(clouds):
        t0 = time.perf_counter()
        fps(pts, K)
        t1 = time.perf_counter()
        d = misc.calc_pts_diameter(pts)
        t2 = time.perf_counter()
        t_fps, t_diam = t_fps + (t1 - t0), t_diam + (t2 - t1)
        print(f"object {c}: n = {len(pts)}, reference FPS (K = {K}) {1e3 * (t1 - t0):.1f} ms, calc_pts_diameter {t2 - t1:.1f} s, diameter {d:.17g}", flush=True)
    print(f"workload: {len(clouds)} objects, {sum(len(p) for p in clouds)} vertices: reference FPS (K = {K}, one call; the tools make nine per object) "
          f"{t_fps:.2f} s, calc_pts_diameter {t_diam:.0f} s")


def main():
    install_shims()
    from lib.pysixd import misc

    from gdrnet_amd import synth

    tmp = tempfile.mkdtemp(prefix="g16_fps_")
    if "--workload" in sys.argv:
        try:
            time_workload(load_reference_fps(tmp), misc, synth)
        finally:
            shutil.rmtree(tmp)
        return
    g = {"seed": np.array(synth.MODEL_PREP_SEED), "K": np.array(K)}
    try:
        fps = load_reference_fps(tmp)
        for case in synth.MODEL_PREP_CASES:
            pts = synth.make_model_prep_inputs(case)
            t0 = time.perf_counter()
            g[f"{case}/fps"] = fps(pts, K)
            t1 = time.perf_counter()
            for k in (1, 8, 64):   # the prefix property, on the reference itself
                assert np.array_equal(fps(pts, k), g[f"{case}/fps"][:k]), (case, k)
            t2 = time.perf_counter()
            g[f"{case}/diameter"] = np.array(misc.calc_pts_diameter(pts), dtype=np.float64)
            t3 = time.perf_counter()
            g[f"{case}/bbox"] = misc.get_bbox3d_and_center(pts)
            xmin, xmax = np.amin(pts[:, 0]), np.amax(pts[:, 0])
            ymin, ymax = np.amin(pts[:, 1]), np.amax(pts[:, 1])
            zmin, zmax = np.amin(pts[:, 2]), np.amax(pts[:, 2])
            g[f"{case}/extents"] = np.array([xmax - xmin, ymax - ymin, zmax - zmin], dtype="float32")
            g[f"{case}/mean"] = np.array([np.average(pts[:, 0]), np.average(pts[:, 1]), np.average(pts[:, 2])])
            print(f"{case}: n = {len(pts)}, reference FPS (K = {K}) {1e3 * (t1 - t0):.2f} ms, calc_pts_diameter {1e3 * (t3 - t2):.1f} ms, "
                  f"diameter {float(g[f'{case}/diameter']):.17g}, first indices {g[f'{case}/fps'][:6].tolist()}", flush=True)
    finally:
        shutil.rmtree(tmp)
    out = os.path.join(HERE, "g16_model_prep.npz")
    np.savez_compressed(out, **g)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
