"""GPU tests of ovp_plane_init_general: init_vio_plane's core in one device pass over the on-plane features of the uploaded batch
and of a general batch (any camera, tracks of up to 64 views).

References: oracle.plane_init (camera 0, tracks the batch carries) and the sequential numpy reference
tests/plane_init_general_ref.py (any camera; held to the oracle in tests/test_plane_init_general_cpu.py).  Bounds: those of
tests/test_gpu_parity.py::test_plane_initialisation_matches_oracle - |d state| and |d cp| < 1e-6, covariance 1e-4
correlation-normalised, decisions / new ids / rows of the gate / consumed features equal."""
import numpy as np
import pytest

from tests import general_planes_ref as R
from tests import plane_init_general_ref as I
from ov_plane_amd.synth import make_scene, make_stereo_plane_scene

pytestmark = pytest.mark.gpu
TOL_DX = 1e-6   # tests/test_gpu_parity.py
TOL_P = 1e-4
ENTRY_KEYS = ("dx", "chi2", "dof", "ok", "new_ids", "cp", "used")   # what both initialisation entries return

CAM0 = {
    "c8_ragged": dict(C=8, F=80, seed=16, n_planes=2, feats_per_plane=25, planes_in_state_frac=0.0, chi2_mult=1.0, ragged=True),
    "c11": dict(C=11, F=140, seed=15, n_planes=3, feats_per_plane=30, planes_in_state_frac=0.0, chi2_mult=1.0),
    # a state above 288 columns (N = 300): the loop runs on the marginal of the involved columns, the rest by push-through
    "n300": dict(C=30, F=150, seed=17, n_planes=2, feats_per_plane=35, planes_in_state_frac=0.0, chi2_mult=1.0, n_slam=30),
}
_cache = {}


def _cam0(oracle, name):
    if name not in _cache:
        sc = make_scene(**CAM0[name])
        _cache[name] = (sc, oracle.plane_init(sc, const_init_multi=5.0, const_init_chi2=1e9))
    return _cache[name]


def _against_oracle(sc, out, ref):
    assert (out["ok"] == ref["plane_ok"]).all() and out["ok"].all()
    assert (out["new_ids"] == ref["new_id"]).all() and (out["dof"] == ref["plane_dof"]).all()
    assert (out["used_all"] == ref["used"]).all()
    e, ecp, ep = I.state_err(out["state"], ref), float(np.abs(out["cp_end"] - ref["cp"]).max()), None
    assert out["P"].shape == ref["P"].shape
    ep = R.relP(out["P"], ref["P"])
    print("state err", e, "cp err", ecp, "relP", ep, "chi2", out["chi2"])
    assert e < TOL_DX and ecp < TOL_DX and ep < TOL_P
    _device_tables(out["ctx"], sc.C, ref)


def _device_tables(ctx, C, ref):
    """The tables the device holds after the call (what the next call linearises at) against the reference's final state."""
    from ov_plane_amd.synth import quat_2_rot
    Rd, pd, cal = ctx.debug_read("clone_R", (C, 3, 3)), ctx.debug_read("clone_p", (C, 3)), ctx.debug_read("cal", (20,))
    e = max(np.abs(pd - ref["clone_p"]).max(), max(np.abs(Rd[i] - quat_2_rot(ref["clone_q"][i])).max() for i in range(C)),
            np.abs(cal[:9].reshape(3, 3) - quat_2_rot(ref["calib_q"])).max(), np.abs(cal[9:12] - ref["calib_p"]).max(),
            np.abs(cal[12:20] - ref["intr"]).max())
    print("device tables err", e)
    assert e < TOL_DX


@pytest.mark.parametrize("name", ["c8_ragged", "c11", "n300"])
def test_empty_general_batch_against_the_oracle(hiplib, oracle, name):
    sc, ref = _cam0(oracle, name)
    if name == "n300":
        assert sc.N > 288
    out = I.run_init_general(hiplib, sc)
    assert len(out["gen"]) == 0
    _against_oracle(sc, out, ref)
    out["ctx"].close()


# plane_chi2 of the same scene through the batch alone and with every second on-plane feature moved to the general batch differs
# by 1.14e-6 on statistics of 52 .. 61 (c8_ragged) and 1.76e-7 on 74 .. 77 (c11), recorded in
# profiles/plane_init_general_timing.json; the bound is 4 x the larger, as tests/test_general_planes_gpu.py sets CHI2_SPLIT_OBSERVED's
CHI2_SPLIT_OBSERVED_INIT = 1.14e-6


@pytest.mark.parametrize("name", ["c8_ragged", "c11"])
def test_batch_and_general_features_are_one_system(hiplib, oracle, name):
    sc, ref = _cam0(oracle, name)
    a = I.run_init_general(hiplib, sc)
    on = np.where(sc.plane_id > 0)[0]
    b = I.run_init_general(hiplib, sc, move=on[::2])
    assert len(b["gen"]) == len(on[::2]) and b["gen_used"].all()
    _against_oracle(sc, b, ref)
    d_chi2 = float(np.abs(a["chi2"] - b["chi2"]).max())
    print("chi2 batch", a["chi2"], "split", b["chi2"], "max |d chi2|", d_chi2)
    assert np.abs(a["dx"] - b["dx"]).max() < TOL_DX and R.relP(b["P"], a["P"]) < TOL_P
    assert d_chi2 <= 4.0 * CHI2_SPLIT_OBSERVED_INIT, d_chi2
    a["ctx"].close()
    b["ctx"].close()


def _against_numpy(out, npr):
    assert (out["ok"] == npr["plane_ok"]).all() and out["ok"].all()
    assert (out["new_ids"] == npr["new_id"]).all() and (out["dof"] == npr["plane_dof"]).all()
    assert (out["used_all"] == npr["used"]).all()
    e, ecp = I.state_err(out["state"], npr["state"]), float(np.abs(out["cp_end"] - npr["cp"]).max())
    assert out["P"].shape == npr["P"].shape
    ep = R.relP(out["P"], npr["P"])
    print("state err", e, "cp err", ecp, "relP", ep)
    assert e < TOL_DX and ecp < TOL_DX and ep < TOL_P


def test_long_tracks(hiplib):
    """C = 34: the smallest clone window with on-plane tracks above the batch's 32 views; two planes outside the state, long and
    short tracks on each.  Against the numpy reference."""
    sc = make_scene(C=34, F=4 + 2 * 8, seed=3, ragged=True, min_meas=28, n_planes=2, feats_per_plane=8, planes_in_state_frac=0.0,
                    chi2_mult=1.0)
    for pl in (1, 2):
        on = sc.plane_id == pl
        assert ((sc.n_meas > 32) & on).sum() >= 3 and ((sc.n_meas <= 32) & on).sum() >= 3, (pl, sc.n_meas[on])
    npr = I.plane_init_ref(sc, 5.0, 1e9)
    out = I.run_init_general(hiplib, sc)
    assert len(out["gen"]) >= 6 and (sc.n_meas[out["gen"]] > 32).all()
    _against_numpy(out, npr)
    out["ctx"].close()


def test_second_camera(hiplib):
    """Stereo plane scene: plane 2's rows are built at the calibration of camera 1 that plane 1 left; a reference that freezes
    camera 1 is told apart; the tables of ovp_cameras_upload after the call are the reference's."""
    sc = make_stereo_plane_scene(C=8, n_planes=2, feats_per_plane=10, planes_in_state_frac=0.0)
    npr = I.plane_init_ref(sc, 5.0, 1e9)
    frozen = I.plane_init_ref(sc, 5.0, 1e9, freeze_cam1=True)
    assert npr["plane_ok"].all()
    assert np.abs(frozen["dx"][1][:sc.N] - npr["dx"][1][:sc.N]).max() > 100 * TOL_DX
    out = I.run_init_general(hiplib, sc)
    on_gen = sc.plane_id[out["gen"]]
    assert (on_gen == 1).sum() >= 2 and (on_gen == 2).sum() >= 2
    print("dx[1] vs reference", np.abs(out["dx"][1][:sc.N] - npr["dx"][1][:sc.N]).max(), "vs frozen",
          np.abs(out["dx"][1][:sc.N] - frozen["dx"][1][:sc.N]).max())
    _against_numpy(out, npr)
    assert np.abs(out["dx"][1][:sc.N] - npr["dx"][1][:sc.N]).max() < TOL_DX
    assert np.abs(out["dx"][1][:sc.N] - frozen["dx"][1][:sc.N]).max() > 100 * TOL_DX
    _, cams = out["ctx"].camera_tables_download(2)
    from ov_plane_amd.synth import quat_2_rot
    assert np.abs(cams[1][:9].reshape(3, 3) - quat_2_rot(npr["state"]["cam1"]["calib_q"])).max() < TOL_DX
    assert np.abs(cams[1][9:12] - npr["state"]["cam1"]["calib_p"]).max() < TOL_DX
    assert np.abs(cams[1][12:20] - npr["state"]["cam1"]["intr"]).max() < TOL_DX
    assert np.abs(cams[0][12:20] - npr["state"]["intr"]).max() < TOL_DX
    out["ctx"].close()


def test_singular_prior(hiplib, oracle):
    """An exact stochastic clone in the prior (the construction of tests/test_general_planes_gpu.py::_exact_clone_scene, every plane
    outside the state): chol(P) fails, the loop runs once more on the pivot-dropping factor, the call returns 0."""
    sc = make_scene(C=9, F=150, seed=43, n_planes=3, feats_per_plane=25, planes_in_state_frac=0.0, chi2_mult=99999.0)
    a, b = sc.ids["clones"][-2], sc.ids["clones"][-1]
    idx = np.arange(sc.N)
    idx[b:b + 6] = np.arange(a, a + 6)
    sc["P"] = sc.P[np.ix_(idx, idx)]
    for k in ("clone_q", "clone_p", "clone_q_fej", "clone_p_fej"):
        sc[k][-1] = sc[k][-2]
    assert np.linalg.eigvalsh(sc.P).min() < 1e-12 * np.linalg.eigvalsh(sc.P).max()
    ref = oracle.plane_init(sc, const_init_multi=5.0, const_init_chi2=1e9)
    out = I.run_init_general(hiplib, sc)
    assert out["rc"] == 0
    _against_oracle(sc, out, ref)
    out["ctx"].close()


def test_limits_leave_everything_untouched(hiplib, oracle):
    sc, ref = _cam0(oracle, "c8_ragged")
    o = hiplib.opts_from_scene(sc)
    NP = sc.cp.shape[0]

    def fresh(n_max):
        ctx = hiplib.Context(n_max, sc.C, sc.F)
        ctx.cov_upload(sc.P)
        ctx.state_upload(sc)
        ctx.cameras_upload(sc)
        ctx.batch_upload_scene(sc)
        return ctx

    f = int(np.where(sc.plane_id > 0)[0][0])
    M = 70
    uv, ci = np.zeros((1, M, 2), dtype=np.float32), np.zeros((1, M), dtype=np.int32)
    cam1 = np.zeros((1, M), dtype=np.int32)
    cam1[0, 0] = 1
    gen = dict(uv=uv, clone_idx=ci, p_FinG=sc.p_FinG[[f]], plane_of_gen=[int(sc.plane_id[f])], raise_on_error=False)
    for n_max, kw, code in [(sc.N + 3 * NP, dict(gen, n_meas=[65], cam_idx=0 * cam1), hiplib.OVP_E_CAPACITY),
                            (sc.N + 3 * NP - 1, dict(raise_on_error=False), hiplib.OVP_E_CAPACITY),
                            (sc.N + 3 * NP, dict(gen, n_meas=[5], cam_idx=cam1), hiplib.OVP_E_ARG)]:
        ctx = fresh(n_max)
        P0 = ctx.cov_download()
        r = ctx.plane_init_general(o, sc.plane_id, sc.cp, 5.0, 1e9, **kw)
        assert r["rc"] == code, (kw.get("n_meas"), r["rc"])
        assert ctx.cov_size() == sc.N and np.array_equal(ctx.cov_download(), P0)
        if n_max >= sc.N + 3 * NP:  # a valid call on the same context: a fresh context's result
            a = ctx.plane_init_general(o, sc.plane_id, sc.cp, 5.0, 1e9)
            a["P"] = ctx.cov_download()
            ctx2 = fresh(n_max)
            b = ctx2.plane_init_general(o, sc.plane_id, sc.cp, 5.0, 1e9)
            b["P"] = ctx2.cov_download()
            for k in ("dx", "chi2", "P", "ok", "cp", "new_ids", "used"):
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
            ctx2.close()
        ctx.close()


def test_repeatable_and_nothing_stale_behind(hiplib, oracle):
    """Two runs are bit-identical; behind either entry (ovp_plane_init is ovp_plane_init_general without a general batch) the
    initialisation, the plane loop and the point update that follow on the same context, and the covariance, have the same bits
    (kept factor, consumed-feature mask, sub-state tables)."""
    sc = make_stereo_plane_scene(C=8, n_planes=2, feats_per_plane=10, planes_in_state_frac=0.0)
    a, b = I.run_init_general(hiplib, sc), I.run_init_general(hiplib, sc)
    for k in ("dx", "chi2", "P", "ok", "cp", "new_ids", "gen_used", "used"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    a["ctx"].close()
    b["ctx"].close()
    sc, _ = _cam0(oracle, "c11")
    o = hiplib.opts_from_scene(sc)
    o.chi2_multiplier = 1e9
    res = []
    for entry in ("plane_init", "plane_init_general"):
        ctx = hiplib.Context(sc.N + 9, sc.C, sc.F)
        ctx.cov_upload(sc.P)
        ctx.state_upload(sc)
        ctx.batch_upload_scene(sc)
        r = getattr(ctx, entry)(o, np.where(sc.plane_id == 3, 0, sc.plane_id), sc.cp[:2], 5.0, 1e9)
        assert r["ok"].all() and ctx.cov_size() == sc.N + 6
        # the third plane's features against the two planes now in the state (none of them: an out-of-state plane), then the points
        pl = ctx.plane_update(o, np.where(sc.plane_id == 3, 1, 0), sc.cp[2:3], sc.cp[2:3], np.array([-1], dtype=np.int32))
        o.skip_plane_used = 1
        pt = ctx.msckf_update(o)
        o.skip_plane_used = 0
        res.append(dict(init=r, pl=pl, pt=pt, P=ctx.cov_download()))
        ctx.close()
    x, y = res
    assert x["pl"]["ok"].all()
    for part, keys in (("init", ENTRY_KEYS), ("pl", ("dx", "ok", "chi2", "dof", "used")), ("pt", ("dx", "accepted"))):
        for k in keys:
            assert np.array_equal(np.asarray(x[part][k]), np.asarray(y[part][k])), (part, k)
    assert np.array_equal(x["P"], y["P"])


def _gate_scene():
    """Three planes of 15 features outside the state, quiet measurements; the middle plane's closest point is displaced onto a
    direction perpendicular to its own (same distance)."""
    sc = make_scene(C=8, F=60, seed=21, n_planes=3, feats_per_plane=15, planes_in_state_frac=0.0, chi2_mult=1.0, px_noise=0.3,
                    err_scale=0.3)
    cp = sc.cp.copy()
    v = np.cross(cp[1], [1.0, 0.0, 0.0])
    cp[1] = np.linalg.norm(cp[1]) * v / np.linalg.norm(v)
    sc["cp"] = cp
    return sc


# plane_chi2 of the first-generation ovp_plane_init on _gate_scene() with const_init_chi2 = 1, from one run of the build in front of its
# retirement (profiles/plane_init_retire.json, "first_generation_gate_scene"): its marginal route, which reported no statistic - a
# NaN - for the plane it rejected this far out, and its whole-state route
FIRST_GEN_CHI2_MARGINAL = np.array([5.472808756418842, float("nan"), 6.530977312510375])
FIRST_GEN_CHI2_WHOLE_STATE = np.array([5.119923296342709, 485.40062386503536, 6.1842578744927215])


def test_gate_rejects_the_middle_plane(hiplib, oracle):
    """const_init_chi2 = 1: decisions against the oracle through both entries, the statistic against the first-generation
    ovp_plane_init's (recorded above), no column for the rejected plane, and the third plane as in a call without the middle one.
    The first generation's own two routes (marginal + push-through, whole state) differed by D_ROUTES = 0.353 on this scene (5.4728
    against 5.1199 on the first plane); the bound on |plane_chi2 - first generation's| is 10 x max(D_ROUTES, CHI2_SPLIT_OBSERVED_INIT)
    with CHI2_SPLIT_OBSERVED_INIT = 1.14e-6.  Measured: 4.8e-5 on the accepted planes against the marginal route, 0.37 on the rejected
    one against the whole-state route (485.77 against 485.40)."""
    from oracle import np_ref
    sc = _gate_scene()
    ref = oracle.plane_init(sc, const_init_multi=5.0, const_init_chi2=1.0)
    thr = np.array([np_ref.chi2_095(int(d)) for d in ref["plane_dof"]])
    assert list(ref["plane_ok"]) == [True, False, True]
    assert (ref["plane_chi2"][[0, 2]] < 0.5 * thr[[0, 2]]).all() and ref["plane_chi2"][1] > 2.0 * thr[1]
    o = hiplib.opts_from_scene(sc)
    ctx = hiplib.Context(sc.N + 9, sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.batch_upload_scene(sc)
    p = ctx.plane_init(o, sc.plane_id, sc.cp, 5.0, 1.0)
    ctx.close()
    assert np.isfinite(p["chi2"]).all()          # a rejected plane's statistic too
    g = I.run_init_general(hiplib, sc, chi2=1.0)
    old = [FIRST_GEN_CHI2_MARGINAL, FIRST_GEN_CHI2_WHOLE_STATE]
    # (the rejected plane is compared with the whole-state route's statistic: the marginal route had none)
    fin = np.isfinite(old[0])
    assert fin[[0, 2]].all() and np.isfinite(old[1]).all()
    d_routes = float(np.abs(old[0] - old[1])[fin].max())
    d_new = float(np.abs(g["chi2"] - np.where(fin, old[0], old[1])).max())
    print("chi2 oracle", ref["plane_chi2"], "first generation", old[0], old[1], "ovp_plane_init", p["chi2"], "general", g["chi2"])
    print("D_ROUTES", d_routes, "|general - first generation|", d_new)
    assert (g["ok"] == ref["plane_ok"]).all() and (p["ok"] == ref["plane_ok"]).all()
    assert (g["new_ids"] == ref["new_id"]).all() and list(g["new_ids"]) == [sc.N, -1, sc.N + 3]
    assert (g["dof"] == ref["plane_dof"]).all() and (g["used_all"] == ref["used"]).all()
    assert g["ctx"].cov_size() == sc.N + 6 and g["P"].shape == ref["P"].shape     # the rejected plane leaves no column
    assert not g["dx"][1].any()
    assert I.state_err(g["state"], ref) < TOL_DX and np.abs(g["cp_end"][[0, 2]] - ref["cp"][[0, 2]]).max() < TOL_DX
    assert R.relP(g["P"], ref["P"]) < TOL_P
    _device_tables(g["ctx"], sc.C, ref)
    h = I.run_init_general(hiplib, sc, chi2=1.0, planes=[0, 2])                   # the same call without the middle plane
    assert list(h["ok"]) == [True, False, True] and h["dof"][1] == 0
    assert np.abs(h["dx"][2] - g["dx"][2]).max() < TOL_DX and np.abs(h["cp_end"] - g["cp_end"]).max() < TOL_DX
    assert R.relP(h["P"], g["P"]) < TOL_P
    assert d_new <= 10.0 * max(d_routes, CHI2_SPLIT_OBSERVED_INIT), (d_new, d_routes)
    g["ctx"].close()
    h["ctx"].close()


@pytest.mark.parametrize("name", ["c8_ragged", "n300", "gate"])
def test_the_two_entries_are_one(hiplib, name):
    """ovp_plane_init and ovp_plane_init_general without a general batch on fresh contexts: the same bits.  C = 8; N > 288 (the
    marginal with push-through); a rejection in the middle (const_init_chi2 = 1)."""
    sc, chi2 = (_gate_scene(), 1.0) if name == "gate" else (make_scene(**CAM0[name]), 1e9)
    o = hiplib.opts_from_scene(sc)
    res = []
    for entry in ("plane_init", "plane_init_general"):
        ctx = hiplib.Context(sc.N + 3 * sc.cp.shape[0], sc.C, sc.F)
        ctx.cov_upload(sc.P)
        ctx.state_upload(sc)
        ctx.batch_upload_scene(sc)
        r = getattr(ctx, entry)(o, sc.plane_id, sc.cp, 5.0, chi2)
        r["P"] = ctx.cov_download()
        res.append(r)
        ctx.close()
    a, b = res
    assert list(a["ok"]) == ([True, False, True] if name == "gate" else [True, True])
    for k in ENTRY_KEYS + ("P",):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_refusals_through_plane_init(hiplib):
    """ovp_plane_init refuses what ovp_plane_init_general refuses, before anything is written: one column short of room for every
    candidate plane (test_limits_leave_everything_untouched's row), then a valid call on the same context gives a fresh context's
    bits; null arguments and a negative plane count are OVP_E_ARG."""
    import ctypes as C
    sc = make_scene(**CAM0["c8_ragged"])
    o = hiplib.opts_from_scene(sc)
    NP = sc.cp.shape[0]

    def fresh(n_max):
        ctx = hiplib.Context(n_max, sc.C, sc.F)
        ctx.cov_upload(sc.P)
        ctx.state_upload(sc)
        ctx.batch_upload_scene(sc)
        return ctx

    ctx = fresh(sc.N + 3 * NP - 1)
    P0 = ctx.cov_download()
    r = ctx.plane_init(o, sc.plane_id, sc.cp, 5.0, 1e9, raise_on_error=False)
    assert r["rc"] == hiplib.OVP_E_CAPACITY and not r["ok"].any()
    assert ctx.cov_size() == sc.N and np.array_equal(ctx.cov_download(), P0)
    pid = np.where(sc.plane_id == 2, 0, sc.plane_id)     # one candidate plane fits
    a = ctx.plane_init(o, pid, sc.cp, 5.0, 1e9)
    a["P"] = ctx.cov_download()
    ctx2 = fresh(sc.N + 3 * NP - 1)
    b = ctx2.plane_init(o, pid, sc.cp, 5.0, 1e9)
    b["P"] = ctx2.cov_download()
    assert list(a["ok"]) == [True, False] and ctx.cov_size() == sc.N + 3
    for k in ENTRY_KEYS + ("P",):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    ctx.close()
    # argument errors, straight at the C entry: nothing is read behind a null pointer, nothing is written
    pof = np.ascontiguousarray(sc.plane_id, dtype=np.int32)
    cp = np.ascontiguousarray(sc.cp, dtype=np.float64)
    sid = -np.ones(NP, dtype=np.int32)
    P0 = ctx2.cov_download()

    def call(h, opts, pb):
        return hiplib.lib().ovp_plane_init(h, opts, pb, C.c_double(5.0), C.c_double(1e9), None, C.c_int(0), None, None, None, None,
                                           None, None)

    good = hiplib.PlaneBatch(NP, pof.ctypes.data, cp.ctypes.data, cp.ctypes.data, sid.ctypes.data)
    for h, opts, pb in [(None, C.byref(o), C.byref(good)), (ctx2._h, None, C.byref(good)), (ctx2._h, C.byref(o), None),
                        (ctx2._h, C.byref(o), C.byref(hiplib.PlaneBatch(-1, pof.ctypes.data, cp.ctypes.data, cp.ctypes.data,
                                                                        sid.ctypes.data))),
                        (ctx2._h, C.byref(o), C.byref(hiplib.PlaneBatch(NP, pof.ctypes.data, None, None, sid.ctypes.data)))]:
        assert call(h, opts, pb) == hiplib.OVP_E_ARG
    assert ctx2.cov_size() == sc.N + 3 and np.array_equal(ctx2.cov_download(), P0)
    ctx2.close()


def test_no_plane_qualifies_above_288_columns(hiplib, oracle):
    """N = 300 (marginal route), every plane with fewer than three features: nothing is appended and the covariance keeps its
    bits, on a fresh context and behind a call that appended two planes."""
    sc, ref = _cam0(oracle, "n300")
    o = hiplib.opts_from_scene(sc)
    few = sc.plane_id.copy()
    for pl in (1, 2):
        few[np.where(sc.plane_id == pl)[0][2:]] = 0
    ctx = hiplib.Context(sc.N + 6, sc.C, sc.F)
    for first in (False, True):
        if first:
            ctx.cov_upload(sc.P)
            ctx.state_upload(sc)
            ctx.batch_upload_scene(sc)
            assert ctx.plane_init_general(o, sc.plane_id, sc.cp, 5.0, 1e9)["ok"].all() and ctx.cov_size() == sc.N + 6
        ctx.cov_upload(sc.P)
        ctx.state_upload(sc)
        ctx.batch_upload_scene(sc)
        P0 = ctx.cov_download()
        r = ctx.plane_init_general(o, few, sc.cp, 5.0, 1e9)
        assert r["rc"] == 0 and not r["ok"].any() and (r["new_ids"] == -1).all() and not r["used"].any()
        assert ctx.cov_size() == sc.N and np.array_equal(ctx.cov_download(), P0)
    ctx.close()


def test_more_than_287_involved_columns_are_refused(hiplib):
    sc = make_scene(C=46, F=20, seed=4, n_planes=2, feats_per_plane=6, planes_in_state_frac=0.0, chi2_mult=1.0)
    assert 6 * sc.C + 14 > 287
    ctx = hiplib.Context(sc.N + 6, sc.C, sc.F)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.batch_upload(sc.uv[:, :32], sc.clone_idx[:, :32], np.minimum(sc.n_meas, 32), sc.p_FinG)  # (the batch carries 32 views)
    P0 = ctx.cov_download()
    r = ctx.plane_init_general(hiplib.opts_from_scene(sc), sc.plane_id, sc.cp, 5.0, 1e9, raise_on_error=False)
    assert r["rc"] == hiplib.OVP_E_CAPACITY and ctx.cov_size() == sc.N and np.array_equal(ctx.cov_download(), P0)
    ctx.close()


def _mirror(sc, **kw):
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib

    return hostlib.run_updater(sc, "plane_init", 5.0, 1.0, **kw)


MIRROR_KEYS = ("P", "n", "clone_p", "clone_q", "intr", "calib_q", "calib_p", "new_p", "new_id", "kept", "deleted")
FIT = dict(min_feat=5, max_cond=200.0, variant=0)


def _existing_mirror_scenes():
    """Every plane_init scene of the existing mirror tests, with its arguments: tests/test_gpu_parity.py
    test_host_cpp_mirror_updater_plane_init and test_host_cpp_mirror_plane_init_fits_planes_first, and the latter's scene with
    gpu_fused_plane_fit off and on (tests/test_plane_frontend_gpu.py::test_host_init_vio_plane_fused_equals_per_plane_route)."""
    pre = make_scene(C=11, F=90, seed=33, n_planes=2, feats_per_plane=30, planes_in_state_frac=0.0, chi2_mult=1.0)
    fit = make_scene(C=10, F=16, seed=34, n_planes=2, feats_per_plane=8, planes_in_state_frac=0.0, chi2_mult=1.0, px_noise=0.25,
                     err_scale=0.05)
    return [("prefitted", pre, {}), ("fit", fit, dict(fit_planes=FIT)), ("fit_fused", fit, dict(fit_planes=FIT, fused_plane_fit=True))]


def test_host_mirror_on_the_camera0_scene(hiplib, oracle):
    """UpdaterPlane::init_vio_plane with StateOptions::gpu_general_plane_init on the scene of
    tests/test_gpu_parity.py::test_host_cpp_mirror_updater_plane_init: the oracle's result."""
    sc = _existing_mirror_scenes()[0][1]
    ref = oracle.plane_init(sc, const_init_multi=5.0, const_init_chi2=1.0)
    out = _mirror(sc, general_plane_init=True)
    assert ref["plane_ok"].all() and out["n"] == ref["n"] and (out["new_id"][:2] == ref["new_id"]).all()
    assert np.abs(out["new_p"][:2] - ref["cp"]).max() < TOL_DX
    assert (out["kept"] == ~ref["used"]).all() and (out["deleted"] == ref["used"]).all()
    assert np.abs(out["clone_p"] - ref["clone_p"]).max() < TOL_DX and np.abs(out["clone_q"] - ref["clone_q"]).max() < TOL_DX
    assert np.abs(out["intr"] - ref["intr"]).max() < TOL_DX and R.relP(out["P"], ref["P"]) < TOL_P


@pytest.mark.parametrize("case", [0, 1, 2], ids=["prefitted", "fit", "fit_fused"])
def test_host_mirror_option_off_keeps_its_bits(hiplib, case):
    """With the option off, every existing plane_init mirror scene - both settings of gpu_fused_plane_fit on the fit scene - gives
    the same bits before and behind a run with the option on in the same process, and the fit scene's two fused settings still agree
    bit for bit with each other (tests/test_plane_frontend_gpu.py).  On these camera-0 scenes no feature is a general one, so the
    option-on run must also agree with the option-off run to TOL_DX / TOL_P: both make the same call with an empty general batch."""
    name, sc, kw = _existing_mirror_scenes()[case]
    before = _mirror(sc, **kw)
    on = _mirror(sc, general_plane_init=True, **kw)
    after = _mirror(sc, **kw)
    for k in MIRROR_KEYS:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), (name, k)
    assert (before["new_id"][:2] >= 0).all() and before["deleted"].any()
    assert on["n"] == before["n"] and (on["new_id"] == before["new_id"]).all() and (on["deleted"] == before["deleted"]).all()
    assert np.abs(on["new_p"] - before["new_p"]).max() < TOL_DX and np.abs(on["clone_p"] - before["clone_p"]).max() < TOL_DX
    assert R.relP(on["P"], before["P"]) < TOL_P
    if case == 2:
        other = _mirror(sc, fit_planes=FIT)
        for k in ("new_id", "new_p", "deleted", "clone_q", "clone_p", "P"):
            assert np.array_equal(np.asarray(other[k]), np.asarray(after[k])), k


@pytest.mark.parametrize("fused", [False, True], ids=["host_fit", "fused_fit"])
def test_host_mirror_fit_path_with_general_features(hiplib, oracle, fused):
    """init_vio_plane with nothing pre-computed and the option on, on a stereo scene whose five two-camera tracks (16 views against
    the others' 8) sort to the END of the candidates: they are triangulated over both cameras; with the fused fit they take part in
    the fit and initialise their planes with the batch's features, without it they stay out of both (the host fit knows camera 0
    only) and plane 1, with five camera-0 tracks, is not fitted.  Against the composition of the reference pieces."""
    sc = I.fit_scene()
    sc2, ref, mono = I.fit_reference(sc, oracle, fused)
    assert list(ref["plane_ok"]) == ([True, True] if fused else [False, True])
    assert int((ref["used"] & ~mono).sum()) == (5 if fused else 0) and ref["used"].sum() == (16 if fused else 6)
    out = _mirror(sc, general_plane_init=True, fit_planes=FIT, fused_plane_fit=fused)
    st = ref["state"]
    e = max(np.abs(out["clone_p"] - st["clone_p"]).max(), np.abs(out["clone_q"] - st["clone_q"]).max(),
            np.abs(out["intr"] - st["intr"]).max(), np.abs(out["cam1"][7:15] - st["cam1"]["intr"]).max())
    acc = ref["plane_ok"]
    print("state err", e, "cp err", np.abs(out["new_p"][:2][acc] - ref["cp"][acc]).max(), "relP", R.relP(out["P"], ref["P"]))
    assert out["n"] == ref["n"] and (out["new_id"][:2] == ref["new_id"]).all()
    assert (out["deleted"] == ref["used"]).all()
    assert np.abs(out["new_p"][:2][acc] - ref["cp"][acc]).max() < TOL_DX and e < TOL_DX
    assert R.relP(out["P"], ref["P"]) < TOL_P


def test_host_mirror_consumes_the_second_cameras_features(hiplib):
    sc = make_stereo_plane_scene(C=8, n_planes=2, feats_per_plane=10, planes_in_state_frac=0.0)
    npr = I.plane_init_ref(sc, 5.0, 1.0)
    assert npr["plane_ok"].all()
    out = _mirror(sc, general_plane_init=True)
    _, gen = R.split_features(sc)
    on_gen = gen[sc.plane_id[gen] > 0]
    assert len(on_gen) >= 4 and out["deleted"][on_gen].all() and (out["deleted"] == npr["used"]).all()
    assert out["n"] == npr["n"] and (out["new_id"][:2] == npr["new_id"]).all()
    assert np.abs(out["new_p"][:2] - npr["cp"]).max() < TOL_DX
    st = npr["state"]
    assert np.abs(out["clone_p"] - st["clone_p"]).max() < TOL_DX and np.abs(out["clone_q"] - st["clone_q"]).max() < TOL_DX
    assert np.abs(out["intr"] - st["intr"]).max() < TOL_DX
    assert np.abs(out["cam1"][7:15] - st["cam1"]["intr"]).max() < TOL_DX and np.abs(out["cam1"][4:7] - st["cam1"]["calib_p"]).max() < TOL_DX
    assert R.relP(out["P"], npr["P"]) < TOL_P
