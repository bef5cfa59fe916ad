"""The epipolar check of TrackPlane::perform_matching (track_plane/TrackPlane.cpp:1331-1350) as a numpy restatement: undistort_cv of
both point sets, cv::findFundamentalMat(FM_RANSAC) on the normalised points, mask_out = status & mask_rsc.  OpenCV and ov_core are
not in the reference tree: every convention below is RECALLED from the published form of cv::undistortPoints,
cv::fisheye::undistortPoints, run7Point, computeError and RANSACPointSetRegistrator::run, and UNPINNED.  Each recalled convention
is one entry of CONV (mutant() flips one at a time); what is our own choice says so.

Our own choices (a device stage needs them; none is OpenCV's):
  * the draws: a stateless counter-based generator (draw()), since cv::RNG's sequence cannot be reproduced;
  * EPI_MAX_SUBSET_TRIES sets per hypothesis, EPI_MAX_DRAWS draws per hypothesis; a hypothesis without a valid set contributes no
    model and the loop goes on;
  * the null space of the 7 x 9 system: Gauss-Jordan elimination with complete pivoting (first largest |a| in row-major order of
    the remaining block, rows and columns swapped), F1 / F2 the null vectors of the two columns left over, in their final order.
    An SVD basis spans the same space and gives the same set of solutions (null="svd" shows that);
  * a zero or non-finite pivot gives no model; a root whose matrix has a non-finite entry is dropped;
  * the collinearity test and the error are evaluated in float64 on the float32 coordinates.
"""
import math

import numpy as np

EPI_MAX_SUBSET_TRIES = 8     # our own: sets tried per hypothesis
EPI_MAX_DRAWS = 256          # our own: draws per hypothesis, whatever they were spent on
EPI_MIN_POINTS = 10          # :1319
MODEL_POINTS = 7
MAX_ITERS_CAP = 1024
DBL_MIN = 2.2250738585072014e-308
DBL_EPSILON = 2.220446049250313e-16
FLT_EPSILON = 1.1920928955078125e-07

MODE_NORMALISED, MODE_RADTAN, MODE_EQUIDISTANT = 0, 1, 2

CONV = dict(
    radtan_iters=5,            # cv::undistortPoints: 5 fixed-point iterations (recalled)
    equi_max_iters=10,         # cv::fisheye::undistortPoints: at most 10 Newton steps (recalled)
    equi_eps=1e-8,             # ... stopping when |step| < 1e-8 (recalled)
    err_combine="max",         # computeError: the larger of the two squared distances (recalled)
    inlier_le=True,            # err <= t (recalled)
    thr_squared=True,          # t = threshold^2 (recalled)
    better_strict=True,        # goodCount > max(maxGoodCount, modelPoints - 1) (recalled)
    floor6=True,
    collinear_both=True,       # checkSubset: haveCollinearPoints on both images (recalled)
    root_order="forward",      # the models of a hypothesis in root order
    and_status=True,           # :1348 mask_klt && mask_rsc
    ransac_all_points=True,    # :1333-1344 does not look at mask_klt
    f33_eps=DBL_EPSILON,       # run7Point: F33 = 1 when |F33| > DBL_EPSILON (recalled)
    coll_eps=FLT_EPSILON,      # haveCollinearPoints: |cross| <= FLT_EPSILON * (|dx1| + |dy1| + |dx2| + |dy2|) (recalled)
)

MUTANTS = {
    "err_sum": dict(err_combine="sum"),
    "inlier_lt": dict(inlier_le=False),
    "thr_not_squared": dict(thr_squared=False),
    "better_ge": dict(better_strict=False),
    "no_floor6": dict(floor6=False),
    "radtan_4_iters": dict(radtan_iters=4),
    "radtan_6_iters": dict(radtan_iters=6),
    "collinear_first_image_only": dict(collinear_both=False),
    "roots_reversed": dict(root_order="reverse"),
    "status_not_anded": dict(and_status=False),
    "ransac_on_status1_only": dict(ransac_all_points=False),
}


def mutant(name):
    return dict(CONV, **MUTANTS[name])


# ---- (a) undistortion ----------------------------------------------------------------------------------------------------------
def undistort(pts, mode, intr, conv=CONV, dtype=np.float64, rounded=True):
    """pts [n, 2] f32 pixels -> normalised [n, 2]; rounded: to f32, as undistort_cv's cv::Point2f is"""
    p = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    if mode == MODE_NORMALISED:
        return p.copy() if rounded else p.astype(dtype)
    fx, fy, cx, cy, k1, k2, k3, k4 = (dtype(float(v)) for v in intr)
    x0, y0 = (p[:, 0].astype(dtype) - cx) / fx, (p[:, 1].astype(dtype) - cy) / fy
    one, two = dtype(1), dtype(2)
    if mode == MODE_RADTAN:
        p1, p2 = k3, k4   # (fx fy cx cy k1 k2 p1 p2)
        x, y = x0.copy(), y0.copy()
        for _ in range(conv["radtan_iters"]):
            r2 = x * x + y * y
            icdist = one / (one + (k2 * r2 + k1) * r2)
            dx = two * p1 * x * y + p2 * (r2 + two * x * x)
            dy = p1 * (r2 + two * y * y) + two * p2 * x * y
            x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
    elif mode == MODE_EQUIDISTANT:
        x, y = np.zeros_like(x0), np.zeros_like(y0)
        half_pi = dtype(math.pi) / two
        for i in range(len(x0)):
            th_d = min(max(np.sqrt(x0[i] * x0[i] + y0[i] * y0[i]), -half_pi), half_pi)
            scale = one
            if th_d > dtype(1e-8):
                th = th_d
                for _ in range(conv["equi_max_iters"]):
                    t2 = th * th
                    t4, t6, t8 = t2 * t2, t2 * t2 * t2, t2 * t2 * t2 * t2
                    fix = (th * (one + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8) - th_d) / (
                        one + dtype(3) * k1 * t2 + dtype(5) * k2 * t4 + dtype(7) * k3 * t6 + dtype(9) * k4 * t8)
                    th = th - fix
                    if abs(fix) < dtype(conv["equi_eps"]):
                        break
                scale = np.tan(th) / th_d
            x[i], y[i] = x0[i] * scale, y0[i] * scale
    else:
        raise ValueError("unknown camera mode")
    out = np.stack([x, y], axis=1)
    return out.astype(np.float32) if rounded else out


# ---- (d) sampling --------------------------------------------------------------------------------------------------------------
def draw(seed, h, t, n):
    x = (seed + 0x9E3779B9 * (h + 1) + 0x85EBCA6B * (t + 1)) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return (x * n) >> 32


def _collinear(px, py, idx, eps):
    """haveCollinearPoints: the last point against every pair of the others"""
    i = idx[-1]
    for j in range(len(idx) - 1):
        dx1, dy1 = px[idx[j]] - px[i], py[idx[j]] - py[i]
        for k in range(j):
            dx2, dy2 = px[idx[k]] - px[i], py[idx[k]] - py[i]
            if abs(dx2 * dy1 - dy2 * dx1) <= eps * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


def sample_sets(p0, p1, seed, max_iters, conv=CONV):
    """-> samples [H, 7] int32 (-1: no set), tries [H] (sets refused as collinear)"""
    n = len(p0)
    x0, y0, x1, y1 = ([float(v) for v in a] for a in (p0[:, 0], p0[:, 1], p1[:, 0], p1[:, 1]))
    S = np.full((max_iters, MODEL_POINTS), -1, dtype=np.int32)
    refused = np.zeros(max_iters, dtype=np.int32)
    eps = conv["coll_eps"]
    for h in range(max_iters):
        t, tries, idx = 0, 0, []
        while tries < EPI_MAX_SUBSET_TRIES and t < EPI_MAX_DRAWS:
            i = draw(seed, h, t, n)
            t += 1
            if i in idx:
                continue
            idx.append(i)
            if len(idx) < MODEL_POINTS:
                continue
            if _collinear(x0, y0, idx, eps) or (conv["collinear_both"] and _collinear(x1, y1, idx, eps)):
                tries += 1
                idx = []
                continue
            S[h] = idx
            break
        refused[h] = tries
    return S, refused


# ---- (b) the 7-point solver -----------------------------------------------------------------------------------------------------
def _system(p0, p1, S, dtype):
    q0, q1 = p0.astype(dtype)[np.maximum(S, 0)], p1.astype(dtype)[np.maximum(S, 0)]   # [H, 7, 2]
    x0, y0, x1, y1 = q0[..., 0], q0[..., 1], q1[..., 0], q1[..., 1]
    return np.stack([x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, np.ones_like(x0)], axis=-1)   # m1^T F m0 = 0


def _null_ge(A, backsub):
    """complete-pivoting elimination of [H, 7, 9] -> F1, F2 [H, 9], alive [H]"""
    A = A.copy()
    H = len(A)
    ar = np.arange(H)
    perm = np.tile(np.arange(9), (H, 1))
    alive = np.ones(H, dtype=bool)
    for k in range(7):
        blk = np.abs(A[:, k:, k:]).reshape(H, -1)
        idx = np.argmax(blk, axis=1)    # the first largest, row-major
        pr, pc = k + idx // (9 - k), k + idx % (9 - k)
        rk, rp = A[ar, k, :].copy(), A[ar, pr, :].copy()
        A[ar, k, :], A[ar, pr, :] = rp, rk
        ck, cp = A[ar, :, k].copy(), A[ar, :, pc].copy()
        A[ar, :, k], A[ar, :, pc] = cp, ck
        a, b = perm[ar, k].copy(), perm[ar, pc].copy()
        perm[ar, k], perm[ar, pc] = b, a
        piv = A[:, k, k].copy()
        ok = np.isfinite(piv) & (piv != 0)
        alive &= ok
        piv[~ok] = 1
        if backsub:   # the variant: forward elimination, sums in the back substitution
            for i in range(k + 1, 7):
                f = A[:, i, k] / piv
                A[:, i, k:] = A[:, i, k:] - f[:, None] * A[:, k, k:]
        else:
            A[:, k, k:] = A[:, k, k:] / piv[:, None]
            row = A[:, k, k:].copy()
            for i in range(7):
                if i != k:
                    f = A[:, i, k].copy()
                    A[:, i, k:] = A[:, i, k:] - f[:, None] * row
    V = np.zeros((H, 2, 9), dtype=A.dtype)
    for c in range(2):
        V[:, c, 7 + c] = 1
        if backsub:
            for i in range(6, -1, -1):
                s = A[:, i, 7 + c].copy()
                for j in range(i + 1, 7):
                    s = s + A[:, i, j] * V[:, c, j]
                with np.errstate(all="ignore"):
                    V[:, c, i] = -s / np.where(alive, A[:, i, i], 1)
        else:
            V[:, c, :7] = -A[:, :, 7 + c]
    F = np.zeros_like(V)
    for j in range(9):
        F[ar, :, perm[:, j]] = V[:, :, j]
    return F[:, 0], F[:, 1], alive


def _det3(m):
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])


def _mix_row(a, b, i):
    m = a.copy()
    m[3 * i:3 * i + 3] = b[3 * i:3 * i + 3]
    return m


def solve_cubic(c, dtype=np.float64):
    """c0 x^3 + c1 x^2 + c2 x + c3 = 0 in closed form (cv::solveCubic, recalled) -> the real roots in its order"""
    a0, a1, a2, a3 = (dtype(v) for v in c)
    zero, two, three = dtype(0), dtype(2), dtype(3)
    if a0 == zero:
        if a1 == zero:
            return [] if a2 == zero else [-a3 / a2]
        d = a2 * a2 - dtype(4) * a1 * a3
        if d < zero:
            return []
        d = np.sqrt(d)
        q1, q2 = (-a2 + d) * dtype(0.5), (a2 + d) * dtype(-0.5)
        r = [q1 / a1, a3 / q1] if abs(q1) > abs(q2) else [q2 / a1, a3 / q2]
        return r if d > zero else r[:1]
    b1, b2, b3 = a1 / a0, a2 / a0, a3 / a0
    Q = (b1 * b1 - three * b2) / dtype(9)
    R = (two * b1 * b1 * b1 - dtype(9) * b1 * b2 + dtype(27) * b3) / dtype(54)
    Q3 = Q * Q * Q
    d = Q3 - R * R
    t2 = b1 / three
    if d > zero:
        theta = np.arccos(R / np.sqrt(Q3))
        t0, t1 = -two * np.sqrt(Q), theta / three
        pi23 = dtype(2) * dtype(math.pi) / three
        return [t0 * np.cos(t1) - t2, t0 * np.cos(t1 + pi23) - t2, t0 * np.cos(t1 + pi23 + pi23) - t2]
    if d == zero:
        e = np.cbrt(abs(R))
        return [-two * e - t2, e - t2] if R >= zero else [two * e - t2, -e - t2]
    e = np.cbrt(np.sqrt(-d) + abs(R))
    if R > zero:
        e = -e
    return [(e + Q / e) - t2]


def scale_model(A, B, lam, conv=CONV):
    """F = lam A + (1 - lam) B written as run7Point does: A is f1 - f2, B is f2 -> (F [9], F33-tiny branch taken)"""
    mu = A.dtype.type(1)
    s = A[8] * lam + B[8]
    tiny = not abs(s) > conv["f33_eps"]
    if not tiny:
        mu = mu / s
        lam = lam * mu
    F = A * lam + B * mu
    F[8] = 0 if tiny else 1
    return F, tiny


def models(p0, p1, S, dtype=np.float64, null="ge", conv=CONV):
    """-> n_models [H], F [H, 3, 9] (dtype; zeros where there is none), report dict of [H] arrays"""
    H = len(S)
    have = S[:, 0] >= 0
    with np.errstate(all="ignore"):
        A = _system(p0, p1, S, dtype)
        if null == "svd":
            Vt = np.linalg.svd(A.astype(np.float64))[2]
            F1, F2, alive = Vt[:, 7].astype(dtype), Vt[:, 8].astype(dtype), np.ones(H, dtype=bool)
        else:
            F1, F2, alive = _null_ge(A, backsub=(null == "ge_backsub"))
    nm = np.zeros(H, dtype=np.int32)
    F = np.zeros((H, 3, 9), dtype=dtype)
    roots, tiny_any = np.zeros(H, dtype=np.int32), np.zeros(H, dtype=bool)
    with np.errstate(all="ignore"):
        for h in np.where(have & alive)[0]:
            Ad, B = F1[h] - F2[h], F2[h]
            c = [_det3(Ad), sum(_det3(_mix_row(Ad, B, i)) for i in range(3)), sum(_det3(_mix_row(B, Ad, i)) for i in range(3)), _det3(B)]
            if not all(np.isfinite(v) for v in c):
                continue
            r = solve_cubic(c, dtype)
            roots[h] = len(r)
            if conv["root_order"] == "reverse":
                r = r[::-1]
            for lam in r:
                Fm, tiny = scale_model(Ad, B, lam, conv)
                if not np.isfinite(Fm).all():
                    continue
                F[h, nm[h]] = Fm
                nm[h] += 1
                tiny_any[h] |= tiny
    return nm, F, dict(roots=roots, f33_tiny=tiny_any, dead=have & ~alive)


# ---- (c) the error --------------------------------------------------------------------------------------------------------------
def errors(F, p0, p1, conv=CONV):
    """F [..., 9], points [n, 2] -> err [..., n] in F's dtype (computeError rounds it to f32: inliers() does)"""
    dt = F.dtype
    x0, y0, x1, y1 = (a.astype(dt) for a in (p0[:, 0], p0[:, 1], p1[:, 0], p1[:, 1]))
    f = [F[..., k, None] for k in range(9)]
    with np.errstate(all="ignore"):
        a, b, c = f[0] * x0 + f[1] * y0 + f[2], f[3] * x0 + f[4] * y0 + f[5], f[6] * x0 + f[7] * y0 + f[8]
        s2 = 1 / (a * a + b * b)
        d2 = x1 * a + y1 * b + c
        a, b, c = f[0] * x1 + f[3] * y1 + f[6], f[1] * x1 + f[4] * y1 + f[7], f[2] * x1 + f[5] * y1 + f[8]
        s1 = 1 / (a * a + b * b)
        d1 = x0 * a + y0 * b + c
        e1, e2 = d1 * d1 * s1, d2 * d2 * s2
        return e1 + e2 if conv["err_combine"] == "sum" else np.maximum(e1, e2)   # (a NaN stays a NaN: no inlier)


def threshold_f32(threshold, conv=CONV):
    return np.float32(threshold * threshold if conv["thr_squared"] else threshold)


def inliers(err, threshold, conv=CONV):
    with np.errstate(all="ignore"):
        e, t = err.astype(np.float32), threshold_f32(threshold, conv)
        return e <= t if conv["inlier_le"] else e < t


# ---- (e) the sequential loop ----------------------------------------------------------------------------------------------------
def cv_round(v):
    return int(round(v))   # half to even, as cvRound's lrint


def update_num_iters(p, ep, model_points, max_iters):
    p, ep = min(max(p, 0.0), 1.0), min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - math.pow(1.0 - ep, model_points)
    if denom < DBL_MIN:
        return 0
    num, denom = math.log(num), math.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * (-denom) else cv_round(num / denom)


def table(n, confidence, max_iters):
    return np.array([update_num_iters(confidence, (n - c) / n, MODEL_POINTS, max_iters) for c in range(n + 1)], dtype=np.int32)


def replay(nm, counts, tab, max_iters, conv=CONV):
    """-> dict(best (h, m) or None, count, niters, stop: the first h not evaluated, updates)"""
    niters, best, best_count, updates, h = max_iters, None, 0, 0, 0
    while h < niters:
        for m in range(int(nm[h])):
            c = int(counts[h, m])
            floor = max(best_count, MODEL_POINTS - 1) if conv["floor6"] else best_count
            if c > floor if conv["better_strict"] else (c >= floor and c > 0):
                best, best_count, updates = (h, m), c, updates + 1
                niters = min(niters, int(tab[c]))
        h += 1
    return dict(best=best, count=best_count, niters=niters, stop=h, updates=updates)


# ---- (f) the frame around it ----------------------------------------------------------------------------------------------------
def defaults(**kw):
    o = dict(mode=MODE_NORMALISED, intrinsics=[1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], threshold=2.0 / 458.654, confidence=0.999,
             max_iters=1000, seed=0)
    o.update(kw)
    return o


def epipolar(pts0, pts1, status=None, opts=None, conv=CONV, dtype=np.float64, null="ge", stages=None):
    """the whole stage -> dict(mask, uvn0, uvn1, F, count, winner, niters, stop, n_with_model, too_few, no_model) plus the
    intermediate arrays (samples, n_models, models, counts, table, err_winner) and `branches`.  stages: a dict of arrays to use in
    place of the computed ones (the variants share the samples)."""
    o = defaults(**(opts or {}))
    p0, p1 = (np.asarray(p, dtype=np.float32).reshape(-1, 2) for p in (pts0, pts1))
    n = len(p0)
    st = np.ones(n, dtype=np.uint8) if status is None else (np.asarray(status).reshape(n) != 0).astype(np.uint8)
    out = dict(n=n, mask=np.zeros(n, dtype=np.uint8), F=np.zeros(9), count=0, winner=(-1, -1), niters=0, stop=0, n_with_model=0,
               too_few=False, no_model=False, branches={})
    if n == 0:
        out["uvn0"] = out["uvn1"] = np.zeros((0, 2), dtype=np.float32)
        return out
    u0, u1 = (undistort(p, o["mode"], o["intrinsics"], conv) for p in (p0, p1))
    out.update(uvn0=u0, uvn1=u1)
    if n < EPI_MIN_POINTS:
        out["too_few"] = True
        return out
    use = np.ones(n, dtype=bool) if conv["ransac_all_points"] else st != 0
    idx = np.where(use)[0]
    r0, r1, m = u0[idx], u1[idx], len(idx)
    H = o["max_iters"]
    if stages and "samples" in stages:
        S, refused = stages["samples"], stages["refused"]
    else:
        S, refused = sample_sets(r0, r1, o["seed"], H, conv) if m >= MODEL_POINTS else (np.full((H, 7), -1, np.int32), np.zeros(H, np.int32))
    nm, F, rep = models(r0, r1, S, dtype, null, conv)
    err = errors(F, r0, r1, conv)                                   # [H, 3, m]
    inl = inliers(err, o["threshold"], conv) & (np.arange(3)[None, :, None] < nm[:, None, None])
    counts = inl.sum(axis=2).astype(np.int32)
    tab = table(m, o["confidence"], H) if m else np.zeros(1, np.int32)
    rp = replay(nm, counts, tab, H, conv)
    out.update(samples=S, refused=refused, n_models=nm, models=F, counts=counts, table=tab, err=err, niters=rp["niters"], stop=rp["stop"],
               n_with_model=int((nm > 0).sum()), used=idx)
    mask_rsc = np.zeros(n, dtype=np.uint8)
    if rp["best"] is None:
        out["no_model"] = True
    else:
        h, k = rp["best"]
        mask_rsc[idx] = inl[h, k]
        out.update(F=F[h, k].astype(np.float64), count=rp["count"], winner=(h, k))
    out["mask"] = (mask_rsc & st) if conv["and_status"] else mask_rsc
    out["mask_rsc"] = mask_rsc
    before = slice(0, rp["stop"])
    out["branches"] = dict(
        roots_1=bool((rep["roots"] == 1).any()), roots_2=bool((rep["roots"] == 2).any()), roots_3=bool((rep["roots"] == 3).any()),
        collinear_redrawn=bool(((refused > 0) & (S[:, 0] >= 0)).any()), no_set=bool((S[:, 0] < 0).any()),
        early_stop=rp["stop"] < H, exhausted=rp["stop"] == H and rp["best"] is not None, no_model=rp["best"] is None,
        f33_tiny=bool(rep["f33_tiny"].any()), models_before_stop=int(nm[before].sum()))
    return out


def feed_monocular(ids_last, pts_last, track, width, height, mask, epi):
    """feed_monocular :505-567 behind the top-up, with the check on: track(pts) -> (pts_new, status) is perform_matching's KLT
    call, epi(pts0, pts1, status) -> mask_out its epipolar check.  -> (ids, pts, uv_norm of the kept points, reset)"""
    ids_last, pts_last = np.asarray(ids_last, dtype=np.int64), np.asarray(pts_last, dtype=np.float32).reshape(-1, 2)
    n = len(ids_last)
    none = (np.zeros(0, np.int64), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
    if n == 0:                                   # :1307 returns an empty mask -> :520-530 resets
        return none + (True,)
    if n < EPI_MIN_POINTS:                       # :1319-1323 all zeros, no KLT: nothing is kept
        return none + (False,)
    p, st = track(pts_last)
    r = epi(pts_last, p, st)
    x, y = p[:, 0], p[:, 1]
    keep = (r["mask"] != 0) & ~(x < 0) & ~(y < 0) & (np.trunc(x) < width) & (np.trunc(y) < height)
    if mask is not None:
        xi, yi = np.clip(x, 0, width - 1).astype(np.int64), np.clip(y, 0, height - 1).astype(np.int64)
        keep &= ~(np.asarray(mask)[yi, xi] > 127)
    return ids_last[keep], p[keep], r["uvn1"][keep], False
