"""CPU tests of the active-tracks stage's surroundings: the new symbols against the header, the binding and the built libraries;
the numpy restatement (tests/active_tracks_ref.py) against cases computed by hand; and the condition on the inputs of the GPU file:
on every scene it uses, no gated quantity of the restatement lies within MARGIN of its threshold, so no feature may be left out of
a comparison there."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import active_tracks_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_in_header_binding_and_library(hiplib):
    L = hiplib.lib()
    hdr = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    for name in ("ovp_active_tracks_create", "ovp_active_tracks_destroy", "ovp_active_tracks_reset", "ovp_active_tracks_update",
                 "ovp_active_tracks_debug"):
        assert hasattr(L, name) and name in hiplib.EXPORTS and re.search(r"\b(int|long) %s\s*\(" % name, hdr), name
    assert L.ovp_active_tracks_update.argtypes == [C.c_void_p, C.POINTER(hiplib.ActiveTracksIn), C.POINTER(hiplib.ActiveTracksOut)]
    for m in ("update", "reset", "close", "debug"):
        assert callable(getattr(hiplib.ActiveTracks, m)), m
    from ov_plane_amd.build import HEADERS, SOURCES

    assert "k_active_tracks.hip" in SOURCES and "k_tri3.h" in HEADERS
    for macro, val in (("OVP_AT_MAX_POINTS", hiplib.OVP_AT_MAX_POINTS), ("OVP_AT_MAX_LANDMARKS", hiplib.OVP_AT_MAX_LANDMARKS)):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == val == 1024


def test_struct_layouts_follow_the_header(hiplib):
    """field by field: name, order and type of the two structs of the entry, as the header declares them"""
    hdr = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    ctype = {"int": C.c_int, "double": C.c_double}
    for cname, cls in (("ovp_active_tracks_in", hiplib.ActiveTracksIn), ("ovp_active_tracks_out", hiplib.ActiveTracksOut)):
        body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} %s;" % cname, hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in [d.strip() for d in body.split(";") if d.strip()]:
            is_ptr = "*" in decl
            base = re.match(r"(?:const\s+)?(\w+)", decl).group(1)
            for name in re.split(r"\s*,\s*", re.sub(r"^(?:const\s+)?\w+\s+", "", decl)):
                arr = re.match(r"\*?(\w+)\[(\d+)\]", name)
                if arr:
                    fields.append((arr.group(1), ctype[base] * int(arr.group(2))))
                else:
                    fields.append((name.lstrip("*").strip(), C.c_void_p if is_ptr else ctype[base]))
        assert [(n, t) for n, t in fields] == [(n, t) for n, t in cls._fields_], cname


def test_entry_checks_that_need_no_device(hiplib):
    L = hiplib.lib()
    a, o = hiplib.ActiveTracksIn(), hiplib.ActiveTracksOut()
    assert L.ovp_active_tracks_create(None) == hiplib.OVP_E_ARG
    assert L.ovp_active_tracks_destroy(None) == hiplib.OVP_E_ARG
    assert L.ovp_active_tracks_reset(None) == hiplib.OVP_E_ARG
    assert L.ovp_active_tracks_update(None, C.byref(a), C.byref(o)) == hiplib.OVP_E_ARG


def test_host_mirror_option_and_session_entries():
    from ov_plane_amd import closed_loop, hostlib
    from ov_plane_amd.build import HOST_HEADERS, build_host

    lib = C.CDLL(build_host())
    assert hasattr(lib, "ovph_session_enable_active_tracks") and hasattr(lib, "ovph_session_active_tracks")
    assert callable(hostlib.Session.enable_active_tracks) and callable(hostlib.Session.active_tracks)
    assert inspect.signature(closed_loop.run_session).parameters["active_tracks"].default is False
    hdr = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "host", "ov_plane_host.h")).read()
    assert "bool gpu_active_tracks = false;" in hdr
    assert "ov_plane_activetracks.h" in HOST_HEADERS
    at = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "host", "ov_plane_activetracks.h")).read()
    for name in ("class ActiveTracks", "retriangulate(", "get_active_tracks(", "active_tracks_posinG", "active_tracks_uvd",
                 "active_tracks_time"):
        assert name in at, name


# ---- the restatement against cases computed by hand --------------------------------------------------------------------------------
I3 = np.eye(3)
CAL = {0: (I3, np.zeros(3)), 1: (I3, np.array([-0.5, 0.0, 0.0]))}   # camera 1 half a metre to the right of camera 0
POINT = np.array([0.3, -0.2, 4.0])


def _frame(x_imu, cams=(0,), ids=(7,), point=POINT):
    """the IMU at (x_imu, 0, 0) with identity orientation, the given cameras each seeing `point` exactly"""
    p_I = np.array([x_imu, 0.0, 0.0])
    obs = []
    for c in cams:
        pc = point - (p_I - CAL[c][1])              # p_CinG = p_IinG - R^T p_IinC with R = I
        uvn = np.array([[pc[0] / pc[2], pc[1] / pc[2]]] * len(ids))
        uv = (uvn * 400 + 300).astype(np.float32)
        obs.append((c, np.array(ids, dtype=np.int64), uv, uvn))
    return dict(cams=obs, R_GtoI=I3, p_IinG=p_I, calib=CAL, wh=(752, 480), slam=[])


def _term(cam_pos, point=POINT):
    b = (point - cam_pos) / np.linalg.norm(point - cam_pos)
    return np.eye(3) - np.outer(b, b)               # skew(b)^T skew(b) of a unit vector


def test_three_observations_give_no_position_four_give_one():
    r = ref.ActiveTracksRef()
    for k in range(3):
        r.retriangulate(_frame(0.2 * k))
        assert r.count[7] == k + 1 and 7 not in r.posinG
    assert not r.gate_log                           # (:304: nothing was solved)
    r.retriangulate(_frame(0.6))
    assert r.count[7] == 4 and np.allclose(r.posinG[7], POINT, rtol=0, atol=1e-12)
    A = sum(_term(np.array([x, 0.0, 0.0])) for x in (0.0, 0.2, 0.4, 0.6))
    assert np.allclose(r.A[7], A, rtol=0, atol=1e-15)
    # the pixel is inside the image and the depth is the camera's z
    assert np.allclose(r.uvd[7], [300 + 400 * (0.3 - 0.6) / 4.0, 300 + 400 * -0.2 / 4.0, 4.0], rtol=0, atol=1e-4)


def test_a_feature_absent_for_one_frame_restarts_at_one():
    r = ref.ActiveTracksRef()
    for k in range(4):
        r.retriangulate(_frame(0.2 * k))
    assert r.count[7] == 4 and 7 in r.posinG
    r.retriangulate(_frame(0.8, ids=(8,)))          # 7 is not seen
    assert 7 not in r.count and 7 not in r.A and 7 not in r.posinG and r.count[8] == 1
    r.retriangulate(_frame(1.0))
    assert r.count[7] == 1 and 7 not in r.posinG
    assert np.allclose(r.A[7], _term(np.array([1.0, 0.0, 0.0])), rtol=0, atol=1e-15)


def test_two_cameras_keep_the_last_term_and_count_old_plus_one():
    r = ref.ActiveTracksRef()
    r.retriangulate(_frame(0.0))                    # camera 0 alone: count 1
    A_old = r.A[7].copy()
    r.retriangulate(_frame(0.2, cams=(0, 1)))
    # (:297-301) old + camera 1's term, not old + both; the count rose by one, not by two
    assert r.count[7] == 2
    assert np.allclose(r.A[7], A_old + _term(np.array([0.7, 0.0, 0.0])), rtol=0, atol=1e-15)
    assert not np.allclose(r.A[7], A_old + _term(np.array([0.2, 0.0, 0.0])) + _term(np.array([0.7, 0.0, 0.0])), rtol=0, atol=1e-3)
    # a feature the previous frame did not leave is INSERTED (:293-296) and insert does not replace: camera 0's term stays
    r2 = ref.ActiveTracksRef()
    r2.retriangulate(_frame(0.2, cams=(0, 1)))
    assert r2.count[7] == 1 and np.allclose(r2.A[7], _term(np.array([0.2, 0.0, 0.0])), rtol=0, atol=1e-15)
    # from the fourth frame on it is solved after each of its two observations (two log entries per frame)
    for k in range(2, 4):
        r.retriangulate(_frame(0.2 * k, cams=(0, 1)))
    assert r.count[7] == 4 and len(r.gate_log) == 2 and 7 in r.posinG


def test_a_landmark_id_gives_its_pixel_but_no_row():
    r = ref.ActiveTracksRef()
    for k in range(4):
        r.retriangulate(_frame(0.2 * k))
    fr = _frame(0.8)
    fr["slam"] = [dict(id=7, xyz=POINT + [0.0, 0.0, 0.5], relative=False)]
    r.retriangulate(fr)
    assert 7 not in r.count and np.array_equal(r.posinG[7], POINT + [0.0, 0.0, 0.5]) and r.uvd[7][2] == 4.5
    # anchored in camera 1 of a clone at x = 2: p_FinG = R_GtoI^T R_ItoC^T (xyz - p_IinC) + p_IinG
    fr = _frame(1.0, ids=(8,))
    fr["slam"] = [dict(id=9, xyz=np.array([0.1, 0.2, 3.0]), relative=True, anchor_cam=1, anchor_R_GtoI=I3,
                       anchor_p_IinG=np.array([2.0, 0.0, 0.0]))]
    r.retriangulate(fr)
    assert np.allclose(r.posinG[9], [0.1 + 0.5 + 2.0, 0.2, 3.0], rtol=0, atol=1e-15) and 9 not in r.uvd  # (no camera-0 pixel)


# ---- the condition on the GPU tests' inputs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.SCENES))
def test_no_gated_quantity_of_a_gpu_scene_sits_at_its_threshold(name):
    make, gates = ref.SCENES[name]
    res, r = ref.run_reference(make(), **gates)    # (asserts min_margin() >= MARGIN itself)
    kinds = {k for k, _ in r.margins}
    print(name, "smallest margin %.3e over %d gated quantities" % (r.min_margin(), len(r.margins)), sorted(kinds))
    assert r.min_margin() >= ref.MARGIN
    assert {"cond", "min_dist", "max_dist", "depth", "u_lo", "u_hi", "v_lo", "v_hi"} <= kinds


def test_the_gate_scene_fails_each_gate_alone():
    frames = ref.gate_scene()
    res, r = ref.run_reference(frames, **ref.GATES)
    g = ref.GATES
    log = {f: [(c, z) for i, c, z in r.gate_log if i == f] for f in (1, 2, 3, 4)}
    assert len(frames) == 6 and len(frames[-1]["cams"][0][1]) == 40
    assert log[1] == [] and [x["count"].get(1) for x in res] == [None, None, None, 1, 2, 3]
    assert len(log[2]) == 3 and all(c <= g["max_cond_number"] and z < g["min_dist"] for c, z in log[2])
    assert len(log[3]) == 3 and all(c <= g["max_cond_number"] and z > g["max_dist"] for c, z in log[3])
    assert len(log[4]) == 3 and all(c > g["max_cond_number"] and g["min_dist"] <= z <= g["max_dist"] for c, z in log[4])
    assert not any(f in x["posinG"] for x in res for f in (1, 2, 3, 4))
    assert [x["count"].get(5) for x in res] == [1, 2, 3, None, 1, 2]                 # absent in frame 3: starts again
    assert [x["count"].get(6) for x in res] == [1, 2, 3, 4, None, None]              # a landmark from frame 4 on: no slot
    assert all(6 in x["posinG"] for x in res[3:]) and 6 in res[4]["uvd"]
    assert np.array_equal(res[4]["posinG"][6], frames[4]["slam"][0]["xyz"])          # ... and its position is the state's
    ordinary = [f for f in frames[-1]["cams"][0][1] if f >= 100]
    assert len(ordinary) == 34 and all(f in res[-1]["posinG"] for f in ordinary)


def test_the_other_scenes_hold_what_their_tests_look_for():
    res, _ = ref.run_reference(ref.stereo_scene())
    assert [x["count"][16] for x in res] == [1, 2, 3, 4, 5]
    assert sorted(res[-1]["posinG"]) == list(range(24)) and sorted(res[-1]["uvd"]) == list(range(8)) + list(range(16, 24))
    frames = ref.landmark_scene()
    res, _ = ref.run_reference(frames)
    assert sum(len(c[1]) for c in frames[-1]["cams"]) == 0 and len(res[-1]["posinG"]) == 12 and not res[-1]["uvd"]
    rel = [s["relative"] for s in frames[0]["slam"]]
    assert rel == [False] * 6 + [True] * 6
    assert len({(s["anchor_cam"], id(s["anchor_R_GtoI"])) for s in frames[0]["slam"][6:]}) == 4   # every anchor clone x camera
    for k in (1, 2, 3):
        got = {f for f in res[k]["uvd"] if f >= 500}
        assert got == {503, 504, 508, 509, 510}, (k, got)   # behind the camera: 500; outside on each side: 501, 502, 506, 507; unseen: 505, 511
    assert len(ref.big_scene()[0]["cams"][0][1]) == 300
