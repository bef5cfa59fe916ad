"""Plain numpy restatement of VioManager::retriangulate_active_tracks (core/VioManagerHelper.cpp:220-418), in the reference's
order and with its maps keyed by feature id (:244-334), and the synthetic scenes of the active-tracks tests.  Written from the
reference's text with numpy.linalg.solve / svd; it shares nothing with the device kernel.  Every thresholded quantity is logged with
its relative distance from the threshold, so a scene can assert that no decision is within rounding of flipping."""
import numpy as np

MARGIN = 1e-6
W, H = 752, 480
FX, FY, CX, CY = 458.0, 457.0, 367.0, 248.0


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


class ActiveTracksRef:
    """active_feat_linsys_A / _b / _count, active_tracks_posinG / _uvd of a VioManager"""

    def __init__(self, min_dist=0.1, max_dist=60.0, max_cond_number=10000.0):
        self.min_dist, self.max_dist, self.max_cond = min_dist, max_dist, max_cond_number
        self.A, self.b, self.count = {}, {}, {}
        self.posinG, self.uvd = {}, {}
        self.margins = []    # (kind, relative distance from the threshold)
        self.gate_log = []   # (feature id, condition number, z in the observing camera) of every solve

    def _thr(self, kind, value, thr, scale=None):
        if np.isfinite(value):
            self.margins.append((kind, abs(value - thr) / abs(thr if scale is None else scale)))

    def min_margin(self):
        return min([m for _, m in self.margins], default=np.inf)

    def retriangulate(self, frame):
        """frame: dict(cams = [(cam_id, ids, uv f32 [n, 2], uv_norm [n, 2]), ...] in sensor_ids order, R_GtoI, p_IinG (the newest
        clone), calib = {cam_id: (R_ItoC, p_IinC)}, wh = (w, h), slam = [dict(id, xyz, relative, anchor_cam, anchor_R_GtoI,
        anchor_p_IinG)] (the state's landmarks))"""
        self.posinG, self.uvd = {}, {}                                                  # :235-236
        A_new, b_new, count_new, pos_new = {}, {}, {}, {}                               # :244-247
        slam_ids = {int(s["id"]) for s in frame["slam"]}
        uvs_in_cam0 = {}
        R_GtoI, p_IinG = frame["R_GtoI"], frame["p_IinG"]
        for cam_id, ids, uv, uv_norm in frame["cams"]:                                  # :251
            R_ItoC, p_IinC = frame["calib"][cam_id]
            R_GtoCi = R_ItoC @ R_GtoI                                                   # :262-263
            p_CiinG = p_IinG - R_GtoCi.T @ p_IinC
            for i in range(len(ids)):                                                   # :268
                featid = int(ids[i])
                if cam_id == 0:                                                         # :273-275
                    uvs_in_cam0[featid] = np.asarray(uv[i], dtype=np.float32)
                if featid in slam_ids:                                                  # :278-280
                    continue
                b_i = R_GtoCi.T @ np.array([uv_norm[i][0], uv_norm[i][1], 1.0])         # :284-288
                b_i = b_i / np.linalg.norm(b_i)
                Bperp = _skew(b_i)
                Ai = Bperp.T @ Bperp                                                    # :291-292
                bi = Ai @ p_CiinG
                if featid not in self.A:                                                # :293-296 std::map::insert: does not replace
                    A_new.setdefault(featid, Ai)
                    b_new.setdefault(featid, bi)
                    count_new.setdefault(featid, 1)
                else:                                                                   # :297-301
                    A_new[featid] = Ai + self.A[featid]
                    b_new[featid] = bi + self.b[featid]
                    count_new[featid] = 1 + self.count[featid]
                if count_new[featid] > 3:                                               # :304
                    A, b = A_new[featid], b_new[featid]
                    with np.errstate(all="ignore"):
                        try:
                            p_FinG = np.linalg.solve(A, b)                              # :309
                        except np.linalg.LinAlgError:
                            p_FinG = np.full(3, np.nan)
                        sv = np.linalg.svd(A, compute_uv=False)                         # :313-317
                        condA = sv[0] / sv[-1]
                    p_FinCi = R_GtoCi @ (p_FinG - p_CiinG)                              # :310
                    self.gate_log.append((featid, abs(condA), p_FinCi[2]))
                    self._thr("cond", abs(condA), self.max_cond)
                    self._thr("min_dist", p_FinCi[2], self.min_dist)
                    self._thr("max_dist", p_FinCi[2], self.max_dist)
                    if (abs(condA) <= self.max_cond and p_FinCi[2] >= self.min_dist and p_FinCi[2] <= self.max_dist
                            and not np.isnan(np.linalg.norm(p_FinCi))):                 # :321-322
                        pos_new[featid] = p_FinG
        self.A, self.b, self.count, self.posinG = A_new, b_new, count_new, pos_new      # :331-334
        if not self.posinG and not frame["slam"]:                                       # :338
            return
        for s in frame["slam"]:                                                         # :342-357
            p_FinG = np.asarray(s["xyz"], float)
            if s["relative"]:
                R_ItoC, p_IinC = frame["calib"][s["anchor_cam"]]
                p_FinG = s["anchor_R_GtoI"].T @ R_ItoC.T @ (np.asarray(s["xyz"], float) - p_IinC) + s["anchor_p_IinG"]
            self.posinG[int(s["id"])] = p_FinG
        R_ItoC, p_IinC = frame["calib"][0]                                              # :360-368
        w, h = frame["wh"]
        for featid, p in self.posinG.items():                                           # :372
            if featid not in uvs_in_cam0:                                               # :376
                continue
            p_FinIi = R_GtoI @ (p - p_IinG)                                             # :381-383
            p_FinCi = R_ItoC @ p_FinIi + p_IinC
            depth = p_FinCi[2]
            u, v = float(uvs_in_cam0[featid][0]), float(uvs_in_cam0[featid][1])          # :386
            self._thr("depth", depth, 0.1)
            self._thr("u_lo", u, 0.0, w), self._thr("u_hi", u, float(w)), self._thr("v_lo", v, 0.0, h), self._thr("v_hi", v, float(h))
            if depth < 0.1:                                                             # :394
                continue
            if u < 0 or int(u) >= w or v < 0 or int(v) >= h:                            # :401
                continue
            self.uvd[featid] = np.array([u, v, depth])                                  # :407-409


def cam_pose(frame, cam_id):
    """R_GtoCi, p_CiinG of the newest clone (:262-263): what a caller of the device entry computes from the state"""
    R_ItoC, p_IinC = frame["calib"][cam_id]
    R = R_ItoC @ frame["R_GtoI"]
    return R, frame["p_IinG"] - R.T @ p_IinC


def run_reference(frames, **gates):
    """-> (per frame dict(posinG, uvd, count), the ActiveTracksRef); asserts the scene's margins"""
    ref = ActiveTracksRef(**gates)
    res = []
    for fr in frames:
        ref.retriangulate(fr)
        res.append(dict(posinG={k: v.copy() for k, v in ref.posinG.items()}, uvd={k: v.copy() for k, v in ref.uvd.items()},
                        count=dict(ref.count), A={k: v.copy() for k, v in ref.A.items()}, b={k: v.copy() for k, v in ref.b.items()}))
    assert ref.min_margin() >= MARGIN, sorted(ref.margins, key=lambda kv: kv[1])[:3]
    return res, ref


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = _skew(axis)
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


# camera 0 and a second camera 12 cm to its side, slightly toed in
CALIB = {0: (_rot([0.2, -0.5, 1.0], 0.31), np.array([0.05, -0.02, 0.01])),
         1: (_rot([0.0, 1.0, 0.0], 0.03) @ _rot([0.2, -0.5, 1.0], 0.31), np.array([-0.07, -0.02, 0.012]))}


def imu_path(n_frames, step=0.16, forward=0.14):
    """the IMU poses that put camera 0 on a curved path looking roughly along (1, 1, 0): [(R_GtoI, p_IinG)].  forward: the part of
    a step along the viewing direction (the rest goes sideways); points near the direction of motion have little parallax"""
    R_ItoC, p_IinC = CALIB[0]
    side = np.sqrt(1.0 - forward * forward)
    along = side * np.array([np.sqrt(0.5), -np.sqrt(0.5), 0.0]) + forward * np.array([np.sqrt(0.5), np.sqrt(0.5), 0.0])
    poses = []
    for k in range(n_frames):
        yaw = np.pi / 4 + 0.03 * np.sin(0.9 * k)
        fwd = np.array([np.cos(yaw), np.sin(yaw), 0.02 * k])
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, [0, 0, 1.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R_GtoC = np.stack([right, down, fwd])
        p_CinG = step * k * along + np.array([0.0, 0.015 * k * k, 0.05 * np.sin(0.7 * k) + 0.03 * k])
        poses.append((R_ItoC.T @ R_GtoC, p_CinG + R_GtoC.T @ p_IinC))
    return poses


def _observe(pose, cam_id, pts, rng, noise_px):
    """(uv f32 [n, 2], uv_norm [n, 2]) of a pinhole camera; the normalised coordinates are taken from the f32 pixels and rounded
    to f32, as the reference's undistort_cv returns them"""
    fr = dict(R_GtoI=pose[0], p_IinG=pose[1], calib=CALIB)
    R, p = cam_pose(fr, cam_id)
    pc = (pts - p) @ R.T
    uv = np.stack([FX * pc[:, 0] / pc[:, 2] + CX, FY * pc[:, 1] / pc[:, 2] + CY], 1) + noise_px * rng.standard_normal((len(pts), 2))
    uv = uv.astype(np.float32)
    uvn = np.stack([(uv[:, 0].astype(np.float64) - CX) / FX, (uv[:, 1].astype(np.float64) - CY) / FY], 1).astype(np.float32)
    return uv, uvn.astype(np.float64)


def _cloud(rng, n):
    """points 2 to 3.5 m in front of the path's first camera, spread over its image"""
    return np.stack([rng.uniform(1.6, 3.0, n), rng.uniform(1.6, 3.0, n), rng.uniform(-0.6, 0.6, n)], 1)


def _in_camera(pose, cam_id, xyz):
    """the point at camera coordinates xyz of the given pose's camera, in G"""
    R, p = cam_pose(dict(R_GtoI=pose[0], p_IinG=pose[1], calib=CALIB), cam_id)
    return p + R.T @ np.asarray(xyz, float)


def _frame(pose, cams, slam=()):
    return dict(cams=cams, R_GtoI=pose[0], p_IinG=pose[1], calib=CALIB, wh=(W, H), slam=list(slam))


GATES = dict(min_dist=0.9, max_dist=4.4, max_cond_number=2500.0)   # of gate_scene: each within reach of a point of the room


def gate_scene(seed=1, n_frames=6):
    """40 points over 6 frames of one camera that moves diagonally forward (little parallax towards the right of the image), six of
    them special:
       id 1 is seen in the last three frames only (never more than 3 observations: no solve);
       id 2 lies 0.6 m in front of the cameras (inside min_dist = 0.9, well conditioned);
       id 3 lies 5.5 m away on the left (beyond max_dist = 4.4, condition number below the limit);
       id 4 lies 3.2 m away near the direction of motion (inside both distances, condition number above 2500);
       id 5 is not seen in frame 3 (its history starts again in frame 4);
       id 6 is a SLAM landmark of the state from frame 4 on (still tracked: its slot goes, its position is the state's)."""
    rng = np.random.default_rng(seed)
    poses = imu_path(n_frames, forward=0.6)
    mid = poses[n_frames // 2]
    z = rng.uniform(2.0, 3.5, 37)
    cloud = np.array([_in_camera(mid, 0, [a * d, b * d, d]) for a, b, d in zip(rng.uniform(-0.7, 0.1, 37), rng.uniform(-0.4, 0.4, 37), z)])
    special = np.stack([cloud[0], _in_camera(mid, 0, [0.05, 0.02, 0.6]), _in_camera(mid, 0, [-2.0, -0.3, 5.5]),
                        _in_camera(mid, 0, [1.6, 0.1, 3.2]), cloud[1], cloud[2]])
    pts = np.concatenate([special, cloud[3:]])
    ids = np.concatenate([[1, 2, 3, 4, 5, 6], np.arange(100, 100 + len(cloud) - 3)]).astype(np.int64)
    frames = []
    for k, pose in enumerate(poses):
        uv, uvn = _observe(pose, 0, pts, rng, 0.05)
        sel = np.ones(len(ids), bool)
        sel[0] = k >= n_frames - 3
        sel[4] = k != 3
        slam = [dict(id=6, xyz=pts[5] + [0.01, -0.02, 0.015], relative=False)] if k >= 4 else []
        frames.append(_frame(pose, [(0, ids[sel], uv[sel], uvn[sel])], slam))
    return frames


def big_scene(seed=2, n=300, n_frames=5):
    """n points of one camera over n_frames frames: more than one workgroup of the kernel"""
    rng = np.random.default_rng(seed)
    pts = _cloud(rng, n)
    ids = np.arange(1000, 1000 + n, dtype=np.int64)
    frames = []
    for pose in imu_path(n_frames):
        uv, uvn = _observe(pose, 0, pts, rng, 0.05)
        frames.append(_frame(pose, [(0, ids, uv, uvn)]))
    return frames


def stereo_scene(seed=3, n_frames=5):
    """24 features over 5 frames of two cameras (sensor_ids = [0, 1]): ids 0-7 seen by camera 0 only, 8-15 by camera 1 only,
    16-23 by both.  A feature of both keeps, per frame, only camera 1's term (and in its first frame only camera 0's), so its count
    rises by one per frame like everyone's and it is solved twice per frame from the fourth on."""
    rng = np.random.default_rng(seed)
    pts = _cloud(rng, 24)
    ids = np.arange(24, dtype=np.int64)
    s0, s1 = np.r_[0:8, 16:24], np.r_[8:24]
    frames = []
    for pose in imu_path(n_frames):
        uv0, uvn0 = _observe(pose, 0, pts, rng, 0.05)
        uv1, uvn1 = _observe(pose, 1, pts, rng, 0.05)
        frames.append(_frame(pose, [(0, ids[s0], uv0[s0], uvn0[s0]), (1, ids[s1], uv1[s1], uvn1[s1])]))
    return frames


def landmark_scene(seed=4, n_frames=5):
    """20 tracked points and 12 landmarks of the state over 5 frames of two cameras: ids 500-505 global, 506-511 anchored - in
    the clone of frame 0 or 1 and in camera 0 or 1, every combination.  All landmarks are tracked by camera 0 except 505 and 511
    (a position, no uvd).  From frame 1 on: 500 lies behind camera 0 (depth < 0.1) while the tracker still reports a pixel for it,
    and 501 / 502 / 506 / 507 are reported at raw pixels left of, right of, above and below the image.  The last frame has
    no observation at all: the landmarks are still reported (:338)."""
    rng = np.random.default_rng(seed)
    poses = imu_path(n_frames)
    pts = _cloud(rng, 20)
    ids = np.arange(20, dtype=np.int64)
    lm_pts = _cloud(rng, 12)
    lm_ids = np.arange(500, 512, dtype=np.int64)
    lm_pts[0] = _in_camera(poses[2], 0, [0.1, 0.05, -1.0])
    anchors = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 1), (1, 0)]   # (anchor frame, anchor camera) of 506 .. 511
    slam = []
    for j in range(12):
        est = lm_pts[j] + 0.01 * rng.standard_normal(3)          # the state's estimate, a centimetre off the point
        if j < 6:
            slam.append(dict(id=int(lm_ids[j]), xyz=est, relative=False))
        else:
            fr0, cam = anchors[j - 6]
            aR, ap = poses[fr0]
            R_ItoC, p_IinC = CALIB[cam]
            slam.append(dict(id=int(lm_ids[j]), xyz=R_ItoC @ (aR @ (est - ap)) + p_IinC, relative=True, anchor_cam=cam,
                             anchor_R_GtoI=aR, anchor_p_IinG=ap))
    outside = {1: (-3.5, 200.0), 2: (W + 0.5, 100.0), 6: (300.0, -0.75), 7: (420.0, H + 12.25)}
    frames = []
    for k, pose in enumerate(poses):
        if k == n_frames - 1:
            frames.append(_frame(pose, [(0, ids[:0], np.zeros((0, 2), np.float32), np.zeros((0, 2)))], slam))
            continue
        uv0, uvn0 = _observe(pose, 0, pts, rng, 0.05)
        uv1, uvn1 = _observe(pose, 1, pts[10:], rng, 0.05)
        luv, luvn = _observe(pose, 0, lm_pts, rng, 0.05)
        if k >= 1:
            luv[0] = (333.25, 207.5)
            for j, px in outside.items():
                luv[j] = px
        seen = np.array([j not in (5, 11) for j in range(12)])
        c0 = (0, np.concatenate([ids, lm_ids[seen]]), np.concatenate([uv0, luv[seen]]), np.concatenate([uvn0, luvn[seen]]))
        frames.append(_frame(pose, [c0, (1, ids[10:], uv1, uvn1)], slam))
    return frames


SCENES = dict(gates=(gate_scene, GATES), big=(big_scene, {}), stereo=(stereo_scene, {}), landmarks=(landmark_scene, {}))
