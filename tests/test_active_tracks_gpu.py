"""GPU tests of the active-tracks stage (k_active_tracks.hip) against the numpy restatement of the reference's function
(tests/active_tracks_ref.py): positions and uvd at 1e-9 relative per vector, flags and counts identical, every feature compared.
tests/test_active_tracks_cpu.py asserts on the restatement that no gated quantity of these scenes sits within 1e-6 of its
threshold, so no feature is left out of a comparison here."""
import numpy as np
import pytest

import active_tracks_ref as ref

pytestmark = pytest.mark.gpu
RTOL = 1e-9


def _close(a, b, what=""):
    """1e-9 relative, vector by vector"""
    a, b = np.asarray(a, float).reshape(-1, 3), np.asarray(b, float).reshape(-1, 3)
    assert a.shape == b.shape
    if a.size == 0:
        return
    scale = np.linalg.norm(b, axis=1)
    err = np.linalg.norm(a - b, axis=1)
    rel = np.where(err == 0.0, 0.0, err / np.where(scale > 0, scale, 1e-300))
    if what:
        print("%s max relative difference %.3e over %d vectors" % (what, rel.max(), len(a)))
    assert rel.max() <= RTOL, (what, rel.max())


@pytest.fixture()
def ctx(hiplib):
    c = hiplib.Context(64, 4, 8)
    yield c
    c.close()


def _args(fr, gates):
    """a frame of the restatement as the arguments of ActiveTracks.update: what a caller computes from the state"""
    cams = fr["cams"]
    n_cams = max([c[0] for c in cams] + [0]) + 1
    poses = [ref.cam_pose(fr, c) for c in range(n_cams)]
    slam = fr["slam"]
    m = len(slam)
    anchor = None
    if any(s["relative"] for s in slam):
        aR, ap, cR, cp = np.zeros((m, 3, 3)), np.zeros((m, 3)), np.zeros((m, 3, 3)), np.zeros((m, 3))
        for j, s in enumerate(slam):
            if s["relative"]:
                aR[j], ap[j] = s["anchor_R_GtoI"], s["anchor_p_IinG"]
                cR[j], cp[j] = fr["calib"][s["anchor_cam"]]
        anchor = (aR, ap, cR, cp)
    return dict(cam_idx=np.concatenate([np.full(len(c[1]), c[0]) for c in cams]), ids=np.concatenate([c[1] for c in cams]),
                uv=np.concatenate([c[2] for c in cams]), uv_norm=np.concatenate([c[3] for c in cams]),
                R_GtoC=np.array([p[0] for p in poses]), p_CinG=np.array([p[1] for p in poses]),
                R_ItoC0=fr["calib"][0][0], p_IinC0=fr["calib"][0][1], R_GtoI=fr["R_GtoI"], p_IinG=fr["p_IinG"],
                width=fr["wh"][0], height=fr["wh"][1], slam_ids=[s["id"] for s in slam],
                slam_xyz=np.array([s["xyz"] for s in slam]).reshape(-1, 3), slam_relative=[s["relative"] for s in slam],
                slam_anchor=anchor, **gates)


def _run(hiplib, ctx, frames, gates, expect=None, per_frame=None):
    """the scene through the device; with `expect` (the restatement's per-frame results) every frame is compared in full.
    Returns the raw output bytes of every frame."""
    at = hiplib.ActiveTracks(ctx)
    raw = []
    for k, fr in enumerate(frames):
        out = at.update(**_args(fr, gates))
        raw.append((out["ids"].tobytes(), out["flags"].tobytes(), out["p_FinG"].tobytes(), out["uvd_all"].tobytes()))
        if expect is not None:
            e = expect[k]
            assert sorted(out["posinG"]) == sorted(e["posinG"]), k           # flags identical: who has a position ...
            assert sorted(out["uvd"]) == sorted(e["uvd"]), k                 # ... and who has a uvd
            order = sorted(e["posinG"])
            _close([out["posinG"][f] for f in order], [e["posinG"][f] for f in order], "frame %d positions" % k)
            order = sorted(e["uvd"])
            _close([out["uvd"][f] for f in order], [e["uvd"][f] for f in order], "frame %d uvd" % k)
            tracked = [int(f) for c in fr["cams"] for f in c[1]]
            first = list(dict.fromkeys(tracked))
            assert out["n_feats"] == len(first) and list(out["ids"]) == first + [s["id"] for s in fr["slam"]]
            assert at.size() == len(e["count"])
            for f in first:                                                   # debug(id): the slot of every tracked feature
                d = at.debug(f)
                if f in e["count"]:
                    assert d is not None and d["count"] == e["count"][f], (k, f)
                    _close(d["A"], e["A"][f])
                    _close(d["b"], e["b"][f])
                else:
                    assert d is None, (k, f)                                  # (a landmark: its slot is gone)
        if per_frame:
            per_frame(k, at, out)
    at.close()
    return raw


def test_gates_and_history(hiplib, ctx):
    frames = ref.gate_scene()
    res, r = ref.run_reference(frames, **ref.GATES)
    counts = []

    def check(k, at, out):
        counts.append({f: (at.debug(f) or {}).get("count") for f in (1, 2, 3, 4, 5, 6)})

    _run(hiplib, ctx, frames, ref.GATES, res, check)
    assert [c[1] for c in counts] == [None, None, None, 1, 2, 3]       # too few observations
    assert [c[5] for c in counts] == [1, 2, 3, None, 1, 2]             # missed frame 3: starts again
    assert [c[6] for c in counts] == [1, 2, 3, 4, None, None]          # a landmark from frame 4 on
    assert all(c[f] == k + 1 for k, c in enumerate(counts) for f in (2, 3, 4))
    assert not any(f in x["posinG"] for x in res for f in (1, 2, 3, 4))  # (what the device was held to above)


def test_more_than_one_workgroup(hiplib, ctx):
    frames = ref.big_scene()
    res, r = ref.run_reference(frames)
    assert len(res[-1]["posinG"]) == 300
    _run(hiplib, ctx, frames, {}, res)


def test_two_cameras(hiplib, ctx):
    frames = ref.stereo_scene()
    res, r = ref.run_reference(frames)
    _run(hiplib, ctx, frames, {}, res)
    # the quirks, visible in what was just compared: a feature of both cameras counts one observation per frame and is solved
    # twice per frame from the fourth on; camera 1's features have a position and no uvd
    assert [x["count"][16] for x in res] == [1, 2, 3, 4, 5]
    assert len([1 for f, c, z in r.gate_log if f == 16]) == 4 and len([1 for f, c, z in r.gate_log if f == 0]) == 2
    assert all(f in res[-1]["posinG"] and f not in res[-1]["uvd"] for f in range(8, 16))


def test_two_cameras_in_the_other_order(hiplib, ctx):
    """sensor_ids = [1, 0]: the term a two-camera feature keeps is now camera 0's, and camera 0 gates its last solve"""
    frames = ref.stereo_scene()
    for fr in frames:
        fr["cams"] = fr["cams"][::-1]
    res, r = ref.run_reference(frames)
    _run(hiplib, ctx, frames, {}, res)
    straight, _ = ref.run_reference(ref.stereo_scene())
    assert not np.array_equal(res[-1]["A"][16], straight[-1]["A"][16])


def test_landmarks_and_projection(hiplib, ctx):
    frames = ref.landmark_scene()
    res, r = ref.run_reference(frames)
    _run(hiplib, ctx, frames, {}, res)
    assert sum(len(c[1]) for c in frames[-1]["cams"]) == 0 and len(res[-1]["posinG"]) == 12  # the n = 0 call, landmarks only


def test_capacity_and_bit_identical_runs(hiplib, ctx):
    frames = ref.gate_scene()
    first = _run(hiplib, ctx, frames, ref.GATES)
    assert _run(hiplib, ctx, frames, ref.GATES) == first          # two runs of scene 1: the same bits
    other = hiplib.Context(64, 4, 8)                              # ... and on a fresh context
    assert _run(hiplib, other, frames, ref.GATES) == first
    other.close()
    n = hiplib.OVP_AT_MAX_POINTS + 1
    at = hiplib.ActiveTracks(ctx)
    got = []
    for k, fr in enumerate(frames):
        if k == 4:  # 1025 features of one camera: refused, and nothing was touched
            a = _args(fr, ref.GATES)
            a.update(cam_idx=np.zeros(n), ids=np.arange(n), uv=np.zeros((n, 2)), uv_norm=np.zeros((n, 2)))
            with pytest.raises(hiplib.OvpError) as e:
                at.update(**a)
            assert e.value.code == hiplib.OVP_E_CAPACITY
            a = _args(fr, ref.GATES)
            a.update(slam_ids=np.arange(5000, 5000 + hiplib.OVP_AT_MAX_LANDMARKS + 1),
                     slam_xyz=np.ones((hiplib.OVP_AT_MAX_LANDMARKS + 1, 3)), slam_relative=None, slam_anchor=None)
            with pytest.raises(hiplib.OvpError) as e:
                at.update(**a)
            assert e.value.code == hiplib.OVP_E_CAPACITY
        out = at.update(**_args(fr, ref.GATES))
        got.append((out["ids"].tobytes(), out["flags"].tobytes(), out["p_FinG"].tobytes(), out["uvd_all"].tobytes()))
    assert got == first
    # the largest frame the entry takes: 1024 features of one camera
    big = ref.big_scene(n=1024, n_frames=1)[0]
    out = at.update(**_args(big, {}))
    assert out["n_feats"] == 1024 and at.size() == 1024 and not out["posinG"]
    at.reset()
    assert at.size() == 0
    at.close()


def test_memory_goes_with_the_context(hiplib):
    def live():
        b = np.zeros(2, dtype=np.int64)
        assert hiplib.lib().ovp_debug_read(c.handle, b"live_bytes", b.ctypes.data, 16) == 16
        return b.copy()

    c = hiplib.Context(64, 4, 8)
    before = live()
    hiplib.ActiveTracks(c)
    assert (live() > before).all()
    c2 = hiplib.Context(64, 4, 8)
    c.close()           # the object was never destroyed by hand
    c = c2
    assert (live() == before).all()
    c.close()


def test_session_active_tracks(hiplib):
    """StateOptions::gpu_active_tracks on the short session scene of the plane-detection test: the filter is bit-equal with the
    option on and off, the maps fill once tracks are four frames old, every uvd depth is the camera-0 depth of the returned
    position at the frame's returned pose, the detector and the stage share one hand-over, and a step without points for its
    timestamp has empty maps and an unchanged filter."""
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import closed_loop
    from ov_plane_amd.sim import Simulator, synthetic_trajectory

    def sim():  # (a simulator draws its noise as it goes: every run gets a fresh one)
        return Simulator(synthetic_trajectory(duration=20.0), num_pts=60, num_pts_plane=120)

    kw = dict(n_frames=12, C=8, planes=2)
    off = closed_loop.run_session(sim(), **kw)
    on = closed_loop.run_session(sim(), active_tracks=True, **kw)
    assert off["traj"].tobytes() == on["traj"].tobytes() and off["posecov"].tobytes() == on["posecov"].tobytes()
    assert np.array_equal(off["counts"], on["counts"])
    print("positions / uvd per frame", on["active_per_frame"].tolist(), "median depth error", on["active_depth_err"])
    assert (on["active_per_frame"][4:] > 0).all()                 # non-empty from the fifth frame on
    assert np.isfinite(on["active_depth_err"][4:]).all()
    n = 0
    for fr in on["active_frames"]:
        assert fr["valid"] and set(fr["uvd"]) <= set(fr["posinG"])
        ps = fr["pose"]                                            # the pose the stage used: camera 0's extrinsics, the newest clone
        for f, d in fr["uvd"].items():
            depth = (ps["R_ItoC"] @ (ps["R_GtoI"] @ (fr["posinG"][f] - ps["p_IinG"])) + ps["p_IinC"])[2]
            assert abs(d[2] - depth) <= RTOL * abs(depth), (f, d[2], depth)
            assert 0 <= d[0] < 752 and 0 <= d[1] < 480 and depth >= 0.1
            n += 1
    assert n > 100
    # with the detector also on, both work from one hand-over
    both = closed_loop.run_session(sim(), active_tracks=True, detect_planes=True, **kw)
    det = closed_loop.run_session(sim(), detect_planes=True, **kw)
    assert both["traj"].tobytes() == det["traj"].tobytes() and np.array_equal(both["detected_per_frame"], det["detected_per_frame"])
    assert (both["active_per_frame"][4:] > 0).all()
    # a step with no points for its timestamp: empty maps that say so, and an unchanged filter
    gap = closed_loop.run_session(sim(), active_tracks=True, active_tracks_skip=(6,), **kw)
    assert off["traj"].tobytes() == gap["traj"].tobytes() and off["posecov"].tobytes() == gap["posecov"].tobytes()
    g = gap["active_frames"]
    assert not g[6]["valid"] and not g[6]["posinG"] and not g[6]["uvd"] and g[5]["valid"] and g[7]["valid"]
    # the stage did not run at that step, so the table was not touched: the histories go on at the next one
    assert gap["active_per_frame"][6].tolist() == [0, 0] and gap["active_per_frame"][5, 0] > 0 and gap["active_per_frame"][7, 0] > 0
