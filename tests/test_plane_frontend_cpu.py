"""CPU tests of the fused plane front end (ovp_plane_fit_refine): the entry is declared and bound, and the chained reference the
GPU tests use (tests/plane_frontend_ref.py: oracle.plane_fitting -> oracle.optimize_plane per plane, poses handed in) is shown to
exercise every branch of update/UpdaterMSCKF.cpp:262-401 on the generated scene and to recover the planes that generated it."""
import os
import re

import numpy as np

from ov_plane_amd.synth import make_plane_frontend_scene
from tests import plane_frontend_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The default planes of the generator at C = 20 (stereo tracks of 40 views): [free with outliers, in-state with SLAM constants,
# scattered points, three features, pixel noise at the Cauchy scale, free with camera-1 and short tracks].  Seeds chosen with the
# oracle alone; it is bit-reproducible, so the figures below only move with libm.
SEEDS = (1, 2, 4)
# max |cp - cp_true| of the successful free planes over SEEDS, measured: 0.0066 (seed 1, plane 0).  The generator displaces the
# triangulated points by 2 cm (1 sigma) along the viewing ray and the measurements by 0.25 px at f = 458 px over a 1.5 m window,
# so a plane of 10-16 points 3.5-4 m away is recovered to the centimetre.  Bound = 2 x the measured spread.
CP_BOUND = 2 * 0.0066


def _chain(oracle, seed):
    sc = make_plane_frontend_scene(C=20, seed=seed)
    return sc, R.chain(sc, R.pose_table(sc), oracle.plane_fitting, oracle.optimize_plane)


def test_entry_is_declared_and_bound():
    from ov_plane_amd import capi

    hdr = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    m = re.search(r"int ovp_plane_fit_refine\(([^;]*)\);", hdr)
    assert m, "ovp_plane_fit_refine is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert "const ovp_general_batch *batch" in args and "const float *uv_norm" in args
    assert hdr.index("int ovp_plane_optimize(") < hdr.index("int ovp_plane_fit_refine(") < hdr.index("---- diagnostics")
    assert "ovp_plane_fit_refine" in capi.EXPORTS and hasattr(capi.Context, "plane_fit_refine")
    src = open(os.path.join(ROOT, "ov_plane_amd", "capi.py")).read()
    b = re.search(r"L\.ovp_plane_fit_refine\.argtypes = \[([^\]]*)\]", src)
    assert b and len([a for a in b.group(1).split(",") if a.strip()]) == len(args)
    # the structs of the binding follow the header field for field
    for name, cls in (("ovp_planefront_in", capi.PlaneFrontIn), ("ovp_planefront_out", capi.PlaneFrontOut)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            names = re.findall(r"\*?\s*(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())
            fields += names
        assert fields == [f[0] for f in cls._fields_], (name, fields)


def test_generator_is_reproducible():
    a, b = make_plane_frontend_scene(C=9, seed=3), make_plane_frontend_scene(C=9, seed=3)
    for k in ("p_FinG", "uv_norm", "clone_q", "clone_p", "cp", "clone_idx", "cam_idx", "n_meas"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert a.uv_norm.dtype == np.float32 and a.n_meas.max() == 18 and set(np.unique(a.cam_idx)) == {0, 1}
    # the poses the measurements were generated with are the ones the tables give
    T = R.pose_table(a)
    assert np.abs(T[:, :, :9].reshape(9, 2, 3, 3) - a.R_GtoC).max() < 1e-14 and np.abs(T[:, :, 9:] - a.p_CinG).max() < 1e-14


def test_reference_is_not_vacuous(oracle):
    """Every branch of the loop occurs on the committed scene (seed 1)."""
    sc, o = _chain(oracle, SEEDS[0])
    assert sc.kinds == ["free", "fixed", "scatter", "free", "noisy", "free"] and sc.n_meas.max() == 40
    n = lambda k: int(sc.feat_start[k + 1] - sc.feat_start[k])
    free_ok = [k for k in range(sc.n_planes) if not sc.fix_plane[k] and o["fit_ok"][k] and o["ok"][k]]
    assert free_ok == [0, 5]                                                        # free planes that fit and refine
    assert sc.fix_plane[1] and o["ok"][1] and o["iterations"][1] > 0                # an in-state plane that is refined
    assert not o["fit_ok"][2] and n(2) >= sc.min_inlier_num                         # RANSAC fails
    assert n(3) < 4 and not o["fit_ok"][3] and not o["ok"][3]                       # fewer than 4 features
    assert o["fit_ok"][4] and not o["ok"][4] and o["iterations"][4] == 12           # no convergence
    k5 = slice(int(sc.feat_start[5]), int(sc.feat_start[6]))
    assert (o["kept"][k5] & (sc.n_meas[k5] > 32)).sum() >= 1 and (o["kept"][k5] & sc.sees_cam1[k5]).sum() >= 1
    # outliers are dropped by the RANSAC; SLAM constants keep their position
    k0 = slice(int(sc.feat_start[0]), int(sc.feat_start[1]))
    assert not o["inlier"][k0][-2:].any() and o["inlier"][k0].sum() >= 10
    slam = np.where(sc.n_meas == 0)[0]
    assert len(slam) == 2 and o["kept"][slam].all() and (o["p_FinG"][slam] == sc.p_FinG[slam]).all()
    # what is not kept keeps the input; what is kept moved
    assert (o["p_FinG"][~o["kept"]] == sc.p_FinG[~o["kept"]]).all()
    moved = o["kept"] & (sc.n_meas > 0)
    assert (np.abs(o["p_FinG"][moved] - sc.p_FinG[moved]).max(axis=1) > 0).all()


def test_reference_recovers_the_generating_planes(oracle):
    worst = 0.0
    for seed in SEEDS:
        sc, o = _chain(oracle, seed)
        good = [k for k in range(sc.n_planes) if not sc.fix_plane[k] and o["ok"][k]]
        assert len(good) >= 2, seed
        for k in good:
            e = float(np.abs(o["cp"][k] - sc.cp_true[k]).max())
            print("seed", seed, "plane", k, "|cp - cp_true|", e)
            worst = max(worst, e)
    assert worst < CP_BOUND


def test_host_mirror_switch_is_exported_and_bound():
    import ctypes
    import inspect

    from ov_plane_amd import hostlib
    from ov_plane_amd.build import build_host

    lib = ctypes.CDLL(build_host())
    assert hostlib.carries_option("fused_plane_fit", lib)
    assert inspect.signature(hostlib.run_msckf_update).parameters["fused_plane_fit"].default is False
    assert inspect.signature(hostlib.run_updater).parameters["fused_plane_fit"].default is False
    hdr = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "host", "ov_plane_host.h")).read()
    assert "bool gpu_fused_plane_fit = false;" in hdr
