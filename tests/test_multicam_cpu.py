"""The K-camera scenes of tests/multicam.py and the references that read them (np_ref.feature_jacobian_full with sc.cams, oracle/ld_ref.py on
top of it), pinned on the CPU before the device is measured against them (tests/test_multicam_gpu.py)."""
import os

import numpy as np
import pytest

from oracle import ld_ref, np_ref
from ov_plane_amd.synth import make_stereo_scene, make_stereo_slam_scene, quat_boxplus
from tests import multicam as mc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def cases():
    return {name: mc.make_case(name) for name in mc.CASES}


def test_three_camera_rows_by_finite_differences():
    """Rows of a feature seen by cameras {0, 2, 3}, camera 2 equidistant, cameras 0 and 3 radtan: every column block - the three
    cameras' extrinsics and intrinsics, the clones (each measured three times), the feature - against central differences of the
    residual (method and tolerance of test_oracle_pins.test_two_camera_rows_by_finite_differences), and the column bookkeeping:
    a camera's measurements touch that camera's columns only, camera 1's columns do not appear."""
    a = np.arange(5, dtype=np.int32)
    sc = mc.make_multicam_scene(C=5, F=4, K=4, seed=7, fisheye=(False, False, True, False), do_fej=False,
                                force={0: [(0, a), (2, a), (3, a)]})
    sc.clone_q_fej, sc.clone_p_fej = sc.clone_q.copy(), sc.clone_p.copy()
    f = 0
    assert int(sc.n_meas[f]) == 15 and mc.cameras_of(sc, f) == [0, 2, 3]
    H_f, H_x, res0, order = np_ref.feature_jacobian_full(sc, f)
    ids = sc.ids
    assert [o[0] for o in order[:6]] == [ids["calib"], ids["intr"], ids["calib2"], ids["intr2"], ids["calib3"], ids["intr3"]]
    assert ids["calib2"] == sc.N - 28 and ids["calib3"] == sc.N - 14
    assert H_x.shape == (30, 42 + 6 * 5)
    for blk, (r0, r1) in enumerate([(0, 10), (10, 20), (20, 30)]):  # rows of camera 0 / 2 / 3 against the other cameras' columns
        other = np.ones(42, dtype=bool)
        other[14 * blk:14 * blk + 14] = False
        assert np.abs(H_x[r0:r1, :42][:, other]).max() == 0.0 and np.abs(H_x[r0:r1, 14 * blk:14 * blk + 14]).min(axis=0).max() > 0.0
    # the lens model is the camera's own: camera 2's rows change when it is read as radtan, the others' do not
    flat = mc.Scene(sc)
    flat["cams"] = [dict(t, fisheye=False) for t in sc.cams]
    H_x_flat = np_ref.feature_jacobian_full(flat, f)[1]
    assert np.array_equal(H_x_flat[:10], H_x[:10]) and np.array_equal(H_x_flat[20:], H_x[20:])
    assert np.abs(H_x_flat[10:20] - H_x[10:20]).max() > 1.0
    eps = 1e-6
    cam_of_id = {}
    for c, t in enumerate(sc.cams):
        cam_of_id[t["calib_id"]] = (c, "calib")
        cam_of_id[t["intr_id"]] = (c, "intr")

    def resid(cams=None, clone_q=None, clone_p=None):
        st = dict(clone_q=sc.clone_q if clone_q is None else clone_q, clone_p=sc.clone_p if clone_p is None else clone_p,
                  calib_q=sc.calib_q, calib_p=sc.calib_p, intr=sc.intr, cams=sc.cams if cams is None else cams)
        st["clone_q_fej"], st["clone_p_fej"] = st["clone_q"], st["clone_p"]
        return np_ref.feature_jacobian_full(sc, f, state=st)[2]

    col = 0
    for sid, sz in order:
        for k in range(sz):
            d = np.zeros(sz)
            d[k] = eps
            rr = []
            for sgn in (+1.0, -1.0):
                dd = sgn * d
                if sid in cam_of_id:
                    c, what = cam_of_id[sid]
                    cams = [dict(t) for t in sc.cams]
                    if what == "calib":
                        cams[c]["calib_q"] = quat_boxplus(sc.cams[c]["calib_q"], dd[:3])
                        cams[c]["calib_p"] = sc.cams[c]["calib_p"] + dd[3:]
                    else:
                        cams[c]["intr"] = sc.cams[c]["intr"] + dd
                    rr.append(resid(cams=cams))
                else:
                    ci = int(np.where(ids["clones"] == sid)[0][0])
                    cq, cp = sc.clone_q.copy(), sc.clone_p.copy()
                    cq[ci] = quat_boxplus(sc.clone_q[ci], dd[:3])
                    cp[ci] = sc.clone_p[ci] + dd[3:]
                    rr.append(resid(clone_q=cq, clone_p=cp))
            num = -(rr[0] - rr[1]) / (2 * eps)
            assert np.abs(num - H_x[:, col]).max() / max(1.0, np.abs(H_x[:, col]).max()) < 1e-6, (sid, k)
            col += 1
    assert col == H_x.shape[1]
    for k in range(3):
        p = sc.p_FinG[f].copy()
        p[k] += eps
        r1 = np_ref.feature_jacobian_full(sc, f, p_FinG=p)[2]
        p[k] -= 2 * eps
        r2 = np_ref.feature_jacobian_full(sc, f, p_FinG=p)[2]
        assert np.abs(-(r1 - r2) / (2 * eps) - H_f[:, k]).max() / max(1.0, np.abs(H_f[:, k]).max()) < 1e-6


def test_a_scene_with_cams_mirrors_the_two_camera_scene():
    """add_cameras on a stereo scene: entries 0 and 1 of sc.cams are the scene's own tables, so the rows of every feature are the
    rows of the two-camera scene, bit for bit, and the slot rotation [c0, c2, c3, c1] with camera 1 relabelled 3 gives them again."""
    s2 = make_stereo_scene(C=5, F=6, seed=7)
    s4 = mc.add_cameras(s2, 4)
    sB = mc.slots_rotated(s4)
    assert s4.N == s2.N + 28 and [t["calib_id"] for t in s4.cams] == [s2.ids["calib"], s2.ids["calib1"], s2.N, s2.N + 14]
    assert np.array_equal(s4.P[:s2.N, :s2.N], s2.P)
    for f in range(s2.F):
        a, b, c = (np_ref.feature_jacobian_full(s, f) for s in (s2, s4, sB))
        for x, y, z in zip(a[:3], b[:3], c[:3]):
            assert np.array_equal(x, y) and np.array_equal(x, z)
        assert a[3] == b[3] == c[3]


def test_projector_pair_equals_the_householder_pair_on_the_edge_features(cases):
    """ld_ref.feature_pair (projector identity, no basis) against ld_ref.nullspace_rows (the truth's Householder basis) on the edge
    features of every case - 64, 63 and 33 views, two views in one clone, a radtan and an equidistant camera in one feature, three
    and four calibration blocks - at the bounds of test_ld_ref_cpu.test_projector_pair_equals_the_householder_and_the_givens_pair."""
    n = 0
    for name, sc in cases.items():
        fish = [bool(t["fisheye"]) for t in sc.cams]
        for f in range(sc.F):
            cams, m = mc.cameras_of(sc, f), int(sc.n_meas[f])
            if not (m in (2, 33, 63, 64) or len(cams) >= 3 or len({fish[c] for c in cams}) == 2 or cams == [2]):
                continue
            H_f, H_x, res, _ = np_ref.feature_jacobian_full(sc, f)
            A, b, rr = ld_ref.feature_pair(H_f, H_x, res)
            Hp, rp = ld_ref.nullspace_rows(H_f, H_x, res)
            assert Hp.shape[0] == 2 * m - 3
            s = max(float(np.abs(A).max()), 1.0)
            assert np.abs(Hp.T @ Hp - A).max() <= 3e-14 * s, (name, f)
            assert np.abs(Hp.T @ rp - b).max() <= 1e-18 * s * max(1.0, float(np.sqrt(rr))), (name, f)
            assert abs(rp @ rp - rr) <= 1e-17 * max(1.0, float(rr)), (name, f)
            n += 1
    assert n >= 60


def test_generator_properties(cases):
    """Every edge feature the cases promise is there, every camera is used, the extended covariance is symmetric positive definite
    and correlates the new columns with the clones, the added tables are nothing like the others, and two calls give the same bytes."""
    for name, sc in cases.items():
        mc.check_case(name, sc)
        K = len(sc.cams)
        assert sc.P.shape == (sc.N, sc.N) and np.array_equal(sc.P, sc.P.T)
        assert np.linalg.eigvalsh(sc.P).min() > 0
        new = np.arange(sc.cams[1]["calib_id"], sc.N)
        assert len(new) == 14 * (K - 1) and sc.N == 30 + 6 * sc.C + 14 * (K - 1)
        clone_cols = np.concatenate([np.arange(c, c + 6) for c in sc.ids["clones"]])
        d = np.sqrt(np.diag(sc.P))
        corr = (sc.P / np.outer(d, d))[np.ix_(new, clone_cols)]
        assert np.abs(corr).max() > 0.02 and (np.abs(corr).max(axis=1) > 0).all()
        for a in range(K):
            for b in range(a + 1, K):
                assert abs(sc.cams[a]["intr"][0] - sc.cams[b]["intr"][0]) > 15.0
                assert np.linalg.norm(sc.cams[a]["calib_p"] - sc.cams[b]["calib_p"]) > 0.05
                assert sc.cams[a]["calib_id"] != sc.cams[b]["calib_id"]
        again = mc.make_case(name)
        for key in ("P", "uv", "uv_norm", "clone_idx", "cam_idx", "n_meas", "p_FinG", "clone_q", "clone_p"):
            assert np.asarray(sc[key]).tobytes() == np.asarray(again[key]).tobytes(), (name, key)
        for ta, tb in zip(sc.cams, again.cams):
            for key in ("calib_q", "calib_p", "intr"):
                assert ta[key].tobytes() == tb[key].tobytes()


def test_add_cameras_extends_slam_and_plane_scenes():
    """The scenes section 4 of the device tests extends: landmarks and planes keep their columns, the new columns go behind them."""
    sc = make_stereo_slam_scene(C=6, n_slam=8, seed=2, n_planes=2)
    s4 = mc.add_cameras(sc, 4)
    assert s4.N == sc.N + 28 and np.array_equal(s4.lm_id, sc.lm_id) and np.array_equal(s4.plane_state_id, sc.plane_state_id)
    assert s4.cams[2]["calib_id"] == sc.N and s4.cams[3]["intr_id"] == sc.N + 20
    assert np.array_equal(s4.P[:sc.N, :sc.N], sc.P) and np.linalg.eigvalsh(s4.P).min() > 0
    assert np.array_equal(s4.cam_idx, sc.cam_idx)


def test_add_cameras_extends_the_plane_front_end_scene():
    """synth.make_plane_frontend_scene has tables and columns but neither covariance nor truth (ovp_plane_fit_refine reads none):
    the added tables take the columns behind the state, the numpy pose table has one column per camera, each another camera by
    centimetres, and the rotated order moves camera 1's column to slot 3."""
    from ov_plane_amd.synth import make_plane_frontend_scene
    from tests import plane_frontend_ref as PF

    sc = make_plane_frontend_scene(C=8, seed=1)
    s4 = mc.add_cameras(sc, 4)
    sB = mc.slots_rotated(s4)
    assert "P" not in s4 and s4.N == sc.N + 28
    assert [t["calib_id"] for t in s4.cams] == [sc.ids["calib"], sc.ids["calib1"], sc.N, sc.N + 14]
    T2, T4, TB = PF.pose_table(sc), PF.pose_table(s4), PF.pose_table(sB)
    assert T4.shape == (8, 4, 12) and np.array_equal(T4[:, :2], T2) and np.array_equal(TB[:, [0, 3, 1, 2]], T4)
    assert min(np.abs(T4[:, i, 9:] - T4[:, j, 9:]).max() for i in range(4) for j in range(i)) > 0.05
    assert (sB.cam_idx == 3).sum() == (sc.cam_idx == 1).sum() > 0


def test_a_state_override_must_carry_the_camera_list(cases):
    """On a scene with `cams` a `state` without the list would leave the cameras at the scene's calibration: refused, not ignored."""
    sc = cases["K3"]
    st = {k: sc[k] for k in ("clone_q", "clone_p", "clone_q_fej", "clone_p_fej", "calib_q", "calib_p", "intr")}
    with pytest.raises(ValueError):
        np_ref.feature_jacobian_full(sc, 0, state=st)
    a = np_ref.feature_jacobian_full(sc, 0)
    b = np_ref.feature_jacobian_full(sc, 0, state=dict(st, cams=sc.cams))
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


@pytest.mark.parametrize("name", list(mc.CASES))
def test_the_reference_alone_meets_the_caps_of_the_case(cases, name):
    """np_ref.msckf_point_update_dense on the case: at least half of the features accepted, at least three rejected where the case
    is about rejection - what the device tests assert again on the device's decisions.  No feature sits on the gate: the closest
    is more than 1e-3 of the threshold away, nine decades above the chi2 error the device is held to."""
    sc = cases[name]
    tab = np.load(os.path.join(GOLD, "chi2_095_table.npy"))
    ref = np_ref.msckf_point_update_dense(sc, tab)
    mc.check_decisions(name, ref["accepted"], sc)
    thr = np.array([sc.opts["chi2_mult"] * tab[2 * int(m) - 3] for m in sc.n_meas])
    assert np.abs(ref["chi2"] / thr - 1.0).min() > 1e-3
    truth = ld_ref.point_pair(sc)
    assert (truth["dof"] == 2 * sc.n_meas - 3).all()
    assert ld_ref.err_chi2(ref["chi2"], truth["chi2"]) < 1e-13
