"""Plain numpy restatement of TrackPlane::perform_plane_detection_monocular (track_plane/TrackPlane.cpp:580-1171), in the
reference's order, as the CPU truth of the device plane detector - and the small scenes its tests run on.

TrackPlaneRef keeps the same per-feature history (linear systems, positions, normal lists) and the same plane maps.  Every
quantity that is compared with a threshold is also recorded with its relative distance from that threshold (`margins`): the scene
generators assert that none sits closer than 1e-6, so that a difference in the last bits cannot flip a decision."""
import numpy as np

DEFAULTS = dict(max_tri_side_px=200, max_norm_count=5, max_norm_avg_max=25.0, max_norm_avg_var=25.0, max_norm_deg=25.0,
                max_dist_between_z=0.10, max_pairwise_px=100, min_norms=3, check_old_feats=1, filter_num_feat=4, filter_z_thresh=1.2,
                feat_init_min_obs=4, min_dist=0.10, max_dist=60.0, max_cond_number=8000.0)
MARGIN = 1e-6


# ---- Delaunay: incremental Bowyer-Watson with a ghost vertex for the point at infinity ------------------------------------------
def _orient(xy, a, b, c):
    return (xy[b, 0] - xy[a, 0]) * (xy[c, 1] - xy[a, 1]) - (xy[b, 1] - xy[a, 1]) * (xy[c, 0] - xy[a, 0])


def _incircle(xy, a, b, c, p):
    m = xy[[a, b, c]] - xy[p]
    return np.linalg.det(np.column_stack([m, (m * m).sum(1)]))


def canonical(tris, xy):
    """positively oriented in (x, y), smallest index first, sorted"""
    out = []
    for t in tris:
        t = [int(v) for v in t]
        if _orient(xy, *t) < 0:
            t = [t[0], t[2], t[1]]
        k = t.index(min(t))
        out.append((t[k], t[(k + 1) % 3], t[(k + 2) % 3]))
    return np.array(sorted(out), dtype=np.int32).reshape(-1, 3)


def delaunay(xy):
    xy = np.asarray(xy, dtype=np.float32).astype(np.float64).reshape(-1, 2)
    n = len(xy)
    if n < 3:
        return np.zeros((0, 3), np.int32)
    k1 = next((k for k in range(1, n) if tuple(xy[k]) != tuple(xy[0])), None)
    k0 = None if k1 is None else next((k for k in range(1, n) if k != k1 and _orient(xy, 0, k1, k) != 0.0), None)
    if k0 is None:
        return np.zeros((0, 3), np.int32)
    a, b, c = 0, k1, k0
    if _orient(xy, a, b, c) < 0:
        b, c = c, b
    G = -1
    tris = [(a, b, c), (b, a, G), (c, b, G), (a, c, G)]

    def inside(t, p):
        if G in t:
            k = t.index(G)
            return _orient(xy, t[(k + 1) % 3], t[(k + 2) % 3], p) > 0
        return _incircle(xy, t[0], t[1], t[2], p) > 0

    for p in range(1, n):
        if p in (k0, k1):
            continue
        bad = [t for t in tris if inside(t, p)]
        if not bad:
            continue
        edges = {(t[k], t[(k + 1) % 3]) for t in bad for k in range(3)}
        tris = [t for t in tris if t not in bad] + [(u, v, p) for (u, v) in sorted(edges) if (v, u) not in edges]
    return canonical([t for t in tris if G not in t and _orient(xy, *t) > 0], xy)


# ---- the stage --------------------------------------------------------------------------------------------------------------
def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


class TrackPlaneRef:
    def __init__(self, **opts):
        self.o = dict(DEFAULTS)
        self.o.update(opts)
        self.A, self.b, self.count, self.p, self.norms = {}, {}, {}, {}, {}
        self.feat2plane, self.plane2old, self.currplaneid = {}, {}, 0
        self.margins = []       # (kind, relative distance from the threshold)
        self.avg, self.filter_rows, self.max_appended = {}, [], 0
        self.gate_log = []      # (condition number, depth in the camera, feature id) of every solution that met the gates

    def _thr(self, kind, value, thr):
        if np.isfinite(value):
            self.margins.append((kind, abs(value - thr) / abs(thr)))

    def min_margin(self):
        return min([m for _, m in self.margins], default=np.inf)

    def avg_norm(self, norms):
        o = self.o
        if not norms:
            return np.zeros(3)
        keep = [v for v in norms if not np.linalg.norm(v) <= 0]
        s = np.sum(keep, axis=0) if keep else np.zeros(3)
        with np.errstate(all="ignore"):
            s = s / np.linalg.norm(s)
        if len(keep) < 2:
            return np.zeros(3)
        dots = [float(v @ s) for v in keep]
        for d in dots:
            self.margins.append(("acos", (1.0 - d) / 1e-10 * MARGIN))  # below 1 by 1e-10 at least: acos is no NaN on either side
        deg = [180.0 / np.pi * np.arccos(d) for d in dots]
        var = sum(d * d for d in deg) / (len(keep) - 1)
        self._thr("avg_var", np.sqrt(var), o["max_norm_avg_var"])
        self._thr("avg_max", max(deg), o["max_norm_avg_max"])
        if np.sqrt(var) > o["max_norm_avg_var"] or max(deg) > o["max_norm_avg_max"]:
            return np.zeros(3)
        return s

    def triangulate(self, ids, uv, uv_norm, R_GtoC, p_CinG):
        """TrackPlane.cpp:608-708 -> (has_est [n], p_FinG [n, 3], accepted [n])"""
        o = self.o
        ids = [int(i) for i in ids]
        self.ids, self.uv = ids, np.asarray(uv, dtype=np.float32).reshape(-1, 2)
        self.R, self.pc = np.asarray(R_GtoC, float).reshape(3, 3), np.asarray(p_CinG, float).reshape(3)
        for m in (self.A, self.b, self.count, self.p, self.norms):      # remove_feats
            for k in [k for k in m if k not in ids]:
                del m[k]
        acc = np.zeros(len(ids), bool)
        for i, f in enumerate(ids):
            bi = self.R.T @ np.array([uv_norm[i][0], uv_norm[i][1], 1.0])
            bi = bi / np.linalg.norm(bi)
            Ai = _skew(bi).T @ _skew(bi)
            self.A[f] = Ai + self.A.get(f, 0.0)
            self.b[f] = Ai @ self.pc + self.b.get(f, 0.0)
            self.count[f] = 1 + self.count.get(f, 0)
            if self.count[f] >= o["feat_init_min_obs"]:
                with np.errstate(all="ignore"):
                    try:
                        p = np.linalg.solve(self.A[f], self.b[f])
                    except np.linalg.LinAlgError:
                        p = np.full(3, np.nan)
                    sv = np.linalg.svd(self.A[f], compute_uv=False)
                    cond = sv[0] / sv[-1]
                pc = self.R @ (p - self.pc)
                self.gate_log.append((abs(cond), pc[2], f))
                self._thr("cond", abs(cond), o["max_cond_number"])
                self._thr("min_dist", pc[2], o["min_dist"])
                self._thr("max_dist", pc[2], o["max_dist"])
                if abs(cond) <= o["max_cond_number"] and o["min_dist"] <= pc[2] <= o["max_dist"] and not np.isnan(np.linalg.norm(pc)):
                    self.p[f] = p
                    acc[i] = True
        has = np.array([f in self.p for f in ids])
        pf = np.array([self.p.get(f, np.zeros(3)) for f in ids]).reshape(-1, 3)
        return has, pf, acc

    def planes(self, tris=None):
        """TrackPlane.cpp:696-1095 on the frame of the preceding triangulate(); tris over the vertices (None: delaunay())"""
        o = self.o
        keep = [i for i, f in enumerate(self.ids) if f in self.p]
        ids, px = [self.ids[i] for i in keep], self.uv[keep]
        if tris is None:
            tris = delaunay(px)
        self.tris = tris
        R, pc = self.R, self.pc

        def plen(a, b):  # cv::norm of a Point2f difference
            d = (px[a] - px[b]).astype(np.float64)
            return float(np.sqrt(d[0] * d[0] + d[1] * d[1]))

        close = {}
        appended = {}
        for t in tris:
            v = [int(x) for x in t]
            f = [ids[x] for x in v]
            for a in range(3):
                close.setdefault(f[a], set()).update({f[(a + 1) % 3], f[(a + 2) % 3]})
            lens = [plen(v[0], v[1]), plen(v[1], v[2]), plen(v[2], v[0])]
            for ln in lens:
                self._thr("tri_side", ln, o["max_tri_side_px"])
            if max(lens) > o["max_tri_side_px"]:
                continue
            with np.errstate(all="ignore"):
                d1 = self.p[f[1]] - self.p[f[0]]
                d1 = d1 / np.linalg.norm(d1)
                d2 = self.p[f[2]] - self.p[f[0]]
                d2 = d2 / np.linalg.norm(d2)
                nrm = np.cross(d1, d2)
                nrm = nrm / np.linalg.norm(nrm)
            if (R @ nrm) @ (R @ (self.p[f[0]] - pc)) < 0:
                nrm = nrm * -1.0
            for a in range(3):
                lst = self.norms.setdefault(f[a], [])
                lst.append(nrm)
                appended[f[a]] = appended.get(f[a], 0) + 1
                del lst[:max(0, len(lst) - o["max_norm_count"])]
        self.max_appended = max(appended.values(), default=0)
        self.avg = {f: self.avg_norm(lst) for f, lst in self.norms.items()}
        pts = {f: px[i] for i, f in enumerate(ids)}
        f2p = self.feat2plane
        if len(tris):
            done = set()
            for f in sorted(self.norms):
                norms, nrm = self.norms[f], self.avg[f]
                if len(norms) < o["min_norms"] or np.linalg.norm(nrm) <= 0:
                    continue
                d = self.p[f] @ nrm
                if not o["check_old_feats"] and f in f2p:
                    continue
                if f not in close:
                    continue
                matches = []
                for g in sorted(close[f]):
                    if g not in self.norms:
                        continue
                    n2 = self.avg[g]
                    if len(self.norms[g]) < o["min_norms"] or np.linalg.norm(n2) <= 0 or g in done:
                        continue
                    dp = (pts[f] - pts[g]).astype(np.float64)
                    ln = float(np.sqrt(dp[0] * dp[0] + dp[1] * dp[1]))
                    self._thr("pair_px", ln, o["max_pairwise_px"])
                    if ln > o["max_pairwise_px"]:
                        continue
                    plane_dist = self.p[g] @ nrm - d
                    dot = float(nrm @ n2)
                    self.margins.append(("acos", (1.0 - dot) / 1e-10 * MARGIN))
                    angle = 180.0 / np.pi * np.arccos(dot)
                    self._thr("angle", angle, o["max_norm_deg"])
                    self._thr("plane_dist", abs(plane_dist), o["max_dist_between_z"])
                    if not np.isnan(angle) and angle < o["max_norm_deg"] and abs(plane_dist) < o["max_dist_between_z"]:
                        matches.append(g)
                if not matches:
                    continue
                cand = ([f2p[f]] if f in f2p else []) + [f2p[g] for g in matches if g in f2p]
                if cand:
                    mn = min(cand)

                    def update(old):
                        if mn == old:
                            return
                        for k in f2p:
                            if f2p[k] == old:
                                f2p[k] = mn
                        self.plane2old.setdefault(mn, set()).add(old)
                        if old in self.plane2old:
                            self.plane2old[mn] |= self.plane2old.pop(old)

                    for g in matches:
                        if g in f2p:
                            update(f2p[g])
                    if f in f2p:
                        update(f2p[f])
                    for g in matches:
                        f2p[g] = mn
                    f2p[f] = mn
                    done.add(f)
                else:
                    self.currplaneid += 1
                    for g in matches:
                        f2p[g] = self.currplaneid
                    f2p[f] = self.currplaneid
        # spatial filter
        self.filter_rows = []
        k = o["filter_num_feat"]
        p2f = {}
        for f in sorted(f2p):
            if f in pts:
                p2f.setdefault(f2p[f], []).append(f)
        for pid in sorted(p2f):
            fs = p2f[pid]
            if len(fs) <= k:
                continue
            P = np.array([self.p[f] for f in fs]).astype(np.float32)
            dv = np.zeros(len(fs))
            for i in range(len(fs)):
                df = P - P[i]                                                     # f32 throughout, as KD_TREE::calc_dist
                d2 = (df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1]) + df[:, 2] * df[:, 2]
                d2 = np.sort(np.delete(d2, i))
                dv[i] = d2[:k].astype(np.float64).sum() / float(k)
            mean = dv.mean()
            std = np.sqrt(((dv - mean) ** 2).sum() / (len(dv) - 1.0))
            for i, f in enumerate(fs):
                with np.errstate(all="ignore"):
                    z = abs(dv[i] - mean) / std
                self._thr("zscore", z, o["filter_z_thresh"])
                self.filter_rows.append((f, pid, dv[i], float(z > o["filter_z_thresh"])))
                if z > o["filter_z_thresh"]:
                    del f2p[f]
        # planes that stay: more than three active features
        ct = {}
        for f in ids:
            if f in f2p:
                ct[f2p[f]] = ct.get(f2p[f], 0) + 1
        self.feat2plane = {f: f2p[f] for f in ids if f in f2p and ct[f2p[f]] > 3}
        self.plane2old = {p: s for p, s in self.plane2old.items() if p in set(self.feat2plane.values())}
        return dict(self.feat2plane)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
FX, FY, CX, CY = 458.0, 457.0, 367.0, 248.0


def camera_path(n_frames, step=0.16):
    """a curved path in front of the corner of the two walls x = 3 and y = 3, looking roughly along (1, 1, 0)"""
    poses = []
    for k in range(n_frames):
        yaw = np.pi / 4 + 0.03 * np.sin(0.9 * k)
        fwd = np.array([np.cos(yaw), np.sin(yaw), 0.02 * k])
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, [0, 0, 1.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])           # R_GtoC
        p = np.array([step * k * 0.8, -step * k * 0.6 + 0.015 * k * k, 0.05 * np.sin(0.7 * k) + 0.03 * k])
        poses.append((R, p))
    return poses


def observe(poses, pts, rng, noise_px=0.15):
    """-> per frame (uv f32 [n, 2], uv_norm f64 [n, 2]); pinhole camera, the normalised coordinates taken from the f32 pixels"""
    out = []
    for R, p in poses:
        pc = (pts - p) @ R.T
        uv = np.stack([FX * pc[:, 0] / pc[:, 2] + CX, FY * pc[:, 1] / pc[:, 2] + CY], 1) + noise_px * rng.standard_normal((len(pts), 2))
        uv = uv.astype(np.float32)
        uvn = np.stack([(uv[:, 0].astype(np.float64) - CX) / FX, (uv[:, 1].astype(np.float64) - CY) / FY], 1)
        out.append((uv, uvn))
    return out


def wall_points(rng, n, wall):
    a, z = rng.uniform(1.9, 2.9, n), rng.uniform(-0.45, 0.45, n)
    return np.stack([np.full(n, 3.0), a, z], 1) if wall == 0 else np.stack([a, np.full(n, 3.0), z], 1)


def two_wall_scene(seed, n_wall=20, n_off=8, n_frames=8):
    """two perpendicular walls of n_wall points each and n_off points off them; frames = [(ids, uv, uv_norm, R_GtoC, p_CinG)]"""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([wall_points(rng, n_wall, 0), wall_points(rng, n_wall, 1),
                          np.stack([rng.uniform(1.2, 2.2, n_off), rng.uniform(1.2, 2.2, n_off), rng.uniform(-0.4, 0.4, n_off)], 1)])
    poses = camera_path(n_frames)
    obs = observe(poses, pts, rng)
    ids = np.arange(100, 100 + len(pts), dtype=np.int64)
    return [(ids, uv, uvn, R, p) for (uv, uvn), (R, p) in zip(obs, poses)]


def run_reference(frames, **opts):
    """the restatement over a scene -> (per-frame results, the TrackPlaneRef); asserts the scene's margins"""
    ref = TrackPlaneRef(**opts)
    res = []
    for ids, uv, uvn, R, p in frames:
        has, pf, acc = ref.triangulate(ids, uv, uvn, R, p)
        m = ref.planes()
        res.append(dict(has=has, p=pf, acc=acc, map=m, tris=ref.tris, norms={f: np.array(v) for f, v in ref.norms.items()},
                        avg={f: v.copy() for f, v in ref.avg.items()}, filter=list(ref.filter_rows), max_appended=ref.max_appended,
                        merges={int(a): {int(x) for x in b} for a, b in ref.plane2old.items()}))
    assert ref.min_margin() >= MARGIN, sorted(ref.margins, key=lambda kv: kv[1])[:3]
    return res, ref


def triangulation_scene(seed, n_frames=6):
    """32 features over n_frames of the curved path: 29 ordinary points and three that meet a gate - id 1 is seen in the last
    three frames only (below feat_init_min_obs), id 2 lies a few centimetres in front of the last camera (inside min_dist), id 3
    lies 55 m away (a baseline too short for max_cond_number)"""
    rng = np.random.default_rng(seed)
    poses = camera_path(n_frames)
    Rl, pl = poses[-1]
    ordinary = np.concatenate([wall_points(rng, 12, 0), wall_points(rng, 12, 1),
                               np.stack([rng.uniform(1.2, 2.2, 5), rng.uniform(1.2, 2.2, 5), rng.uniform(-0.4, 0.4, 5)], 1)])
    Rm, pm = poses[n_frames - 3]
    near = pm + Rm.T @ np.array([0.004, 0.003, 0.05])
    assert all((R @ (near - p))[2] < 0.09 for R, p in poses[n_frames - 3:])  # from its fourth observation on, always inside min_dist
    special = np.stack([[2.5, 2.4, 0.1], near, pl + Rl.T @ np.array([1.0, 0.5, 55.0])])
    pts = np.concatenate([special, ordinary])
    ids = np.concatenate([[1, 2, 3], np.arange(100, 100 + len(ordinary))]).astype(np.int64)
    obs = observe(poses, pts, rng, noise_px=0.05)
    frames = []
    for k, ((uv, uvn), (R, p)) in enumerate(zip(obs, poses)):
        sel = np.arange(len(ids)) if k >= n_frames - 3 else np.arange(1, len(ids))
        frames.append((ids[sel], uv[sel], uvn[sel], R, p))
    return frames
