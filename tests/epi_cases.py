"""The cases of the epipolar check (tests/epi_ref.py is the stage's definition) and what the GPU test asserts of a run.  Every case is
small: synthetic 3-D points under a known relative pose in normalised coordinates, a fixed seed, Gaussian noise of a hundredth of the
threshold, outliers displaced by 10 to 60 thresholds.

The restatement's variants - float64 as stated, numpy long double, the elimination with its sums re-associated (forward elimination
and back substitution), an SVD null space - define what a run may differ in:
  near [h, model, point]   the variants disagree on the decision, or the float64 error lies within 4 x its spread among the
                           variants (plus one f32 step of threshold^2, since the decision is taken on the f32-rounded error) of
                           threshold^2;
  unsettled [h]            the variants disagree on the number of models (every point of such a hypothesis counts as near).
A case whose replay is not the same for every count vector inside these allowances is replaced by another seed, never loosened.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epi_ref  # noqa: E402

THRESHOLD = 2.0 / 458.654          # :1341-1344 with the project's INTRINSICS
NOISE = THRESHOLD / 100.0
NEAR_CAP = 0.02                    # of the points for the winning model, of the hypotheses in front of the stop index
VARIANTS = (("float64", np.float64, "ge"), ("longdouble", np.longdouble, "ge"), ("reassociated", np.float64, "ge_backsub"),
            ("svd", np.float64, "svd"))


def _rot(w):
    th = np.linalg.norm(w)
    k = np.asarray(w) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scene(n, seed, outliers=0.0, status_zeros=0, special=None):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.3, 1.3, n), rng.uniform(3.0, 8.0, n)], axis=1)
    R, t = _rot([0.02, -0.03, 0.015]), np.array([0.25, -0.05, 0.08])
    Y = X @ R.T + t
    p0 = X[:, :2] / X[:, 2:] + rng.normal(0, NOISE, (n, 2))
    p1 = Y[:, :2] / Y[:, 2:] + rng.normal(0, NOISE, (n, 2))
    planted, unknown = np.ones(n, dtype=bool), np.zeros(n, dtype=bool)   # unknown: moved, but not by many thresholds
    k = int(round(outliers * n))
    if k:
        out = rng.choice(n, k, replace=False)
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        E = (tx @ R).reshape(1, 9)
        for i in out:   # displaced until the true epipolar error is above (5 thresholds)^2: no outlier slides along its line
            while True:
                ang, mag = rng.uniform(0, 2 * np.pi), rng.uniform(10, 60) * THRESHOLD
                q = p1[i] + mag * np.array([np.cos(ang), np.sin(ang)])
                if epi_ref.errors(E, p0[i:i + 1], q[None])[0, 0] > 25 * THRESHOLD ** 2:
                    break
            p1[i] = q
        planted[out] = False
    if special == "partline":    # ten points of the first image on one line, exactly: some sets are refused as collinear
        p0[:10, 1] = 0.125
        unknown[:10] = True
    if special == "partline1":   # the same in the second image alone
        p1[:10, 1] = 0.125
        unknown[:10] = True
    status = None
    if status_zeros:
        status = np.ones(n, dtype=np.uint8)
        status[rng.choice(np.where(planted)[0], status_zeros, replace=False)] = 0
    if special == "line":        # every point of the first image on one line, exactly
        p0[:, 1] = 0.125
    if special == "same":
        p1 = p0.copy()
    if special == "origin":      # one correspondence (0, 0) -> (0, 0): F33 = 0 for every set that holds it
        p0[0], p1[0], planted[0] = 0.0, 0.0, False
    return dict(pts0=p0.astype(np.float32), pts1=p1.astype(np.float32), status=status, planted=planted, unknown=unknown)


def _case(n, seed, max_iters=1000, rseed=7, **kw):
    c = scene(n, seed, **kw)
    c["opts"] = dict(mode=0, threshold=THRESHOLD, confidence=0.999, max_iters=max_iters, seed=rseed)
    return c


SPECS = {
    "n10_all_inliers": dict(n=10, seed=1, max_iters=200),
    "n9_too_few": dict(n=9, seed=2, max_iters=64),
    "n63": dict(n=63, seed=3, outliers=0.2, max_iters=200, special="partline"),
    "n64": dict(n=64, seed=4, outliers=0.2, max_iters=200),
    "n65": dict(n=65, seed=5, outliers=0.2, max_iters=200, special="partline1"),
    "n300_out30": dict(n=300, seed=6, outliers=0.3, max_iters=1000, special="origin"),
    "n120_out65": dict(n=120, seed=7, outliers=0.65, max_iters=1024, rseed=4),
    "n40_line": dict(n=40, seed=8, max_iters=64, special="line"),
    "n40_same": dict(n=40, seed=9, max_iters=64, special="same"),
    "n80_status": dict(n=80, seed=10, outliers=0.2, status_zeros=20, max_iters=200),
    "n100_iters1": dict(n=100, seed=11, outliers=0.2, max_iters=1),
    "n100_iters64": dict(n=100, seed=11, outliers=0.2, max_iters=64),
    "n100_iters65": dict(n=100, seed=11, outliers=0.2, max_iters=65),
    "n100_iters1024": dict(n=100, seed=11, outliers=0.2, max_iters=1024),
}
IDS = list(SPECS)
OUTLIER_CASES = ["n63", "n64", "n65", "n300_out30", "n120_out65", "n80_status", "n100_iters1024"]
UNCOMPARED = ["n40_same"]      # only finiteness, determinism and the return code


@functools.lru_cache(maxsize=None)
def case(cid):
    return _case(**SPECS[cid])


def run(cid, conv=epi_ref.CONV, dtype=np.float64, null="ge", stages=None):
    c = case(cid)
    return epi_ref.epipolar(c["pts0"], c["pts1"], c["status"], c["opts"], conv, dtype, null, stages)


@functools.lru_cache(maxsize=None)
def reference(cid):
    return run(cid)


def unit(F):
    """F [..., 9] at unit Frobenius norm, the entry of largest magnitude positive"""
    F = np.asarray(F, dtype=np.float64)
    with np.errstate(all="ignore"):
        F = F / np.sqrt((F * F).sum(axis=-1, keepdims=True))
    k = np.argmax(np.abs(np.nan_to_num(F)), axis=-1)
    s = np.sign(np.take_along_axis(F, k[..., None], axis=-1))
    return F * np.where(s == 0, 1, s)


@functools.lru_cache(maxsize=None)
def allowances(cid):
    """-> dict(near [H, 3, m] bool, unsettled [H] bool, near_in / near_out [H, 3], f_spread [H, 3]: the largest distance of a
    variant's matched unit F from the float64 one)"""
    return allowances_of(case(cid), reference(cid))


def allowances_of(c, ref):
    """the same for any inputs: c = dict(pts0, pts1, status, opts), ref = epi_ref.epipolar on them"""
    def run(cid, dtype, null, stages):
        return epi_ref.epipolar(c["pts0"], c["pts1"], c["status"], c["opts"], epi_ref.CONV, dtype, null, stages)
    cid = None
    thr = epi_ref.defaults(**c["opts"])["threshold"]
    t32 = epi_ref.threshold_f32(thr)
    nm, e_ref = ref["n_models"], ref["err"].astype(np.float64)
    H, _, m = e_ref.shape
    valid = np.arange(3)[None, :] < nm[:, None]
    dec_ref = epi_ref.inliers(ref["err"], thr) & valid[:, :, None]
    uF = unit(ref["models"])
    unsettled = np.zeros(H, dtype=bool)
    disagree = np.zeros(e_ref.shape, dtype=bool)
    spread = np.zeros(e_ref.shape)
    f_spread = np.zeros((H, 3))
    stages = dict(samples=ref["samples"], refused=ref["refused"])
    for name, dtype, null in VARIANTS[1:]:
        v = run(cid, dtype=dtype, null=null, stages=stages)
        unsettled |= v["n_models"] != nm
        vF = unit(v["models"])
        with np.errstate(all="ignore"):
            d = np.abs(uF[:, :, None, :] - vF[:, None, :, :]).max(axis=-1)        # [H, ref model, variant model]
        d = np.where(np.isfinite(d) & (np.arange(3)[None, None, :] < v["n_models"][:, None, None]), d, np.inf)
        k = np.argmin(d, axis=2)
        f_spread = np.maximum(f_spread, np.where(valid, np.take_along_axis(d, k[:, :, None], axis=2)[:, :, 0], 0))
        e_v = np.take_along_axis(v["err"].astype(np.float64), k[:, :, None], axis=1)
        dec_v = epi_ref.inliers(e_v, thr)
        disagree |= (dec_v != dec_ref) & valid[:, :, None]
        with np.errstate(all="ignore"):
            spread = np.fmax(spread, np.abs(e_v - e_ref))
    with np.errstate(all="ignore"):
        band = np.abs(e_ref - np.float64(t32)) <= 4 * spread + np.float64(np.spacing(t32))
    near = (disagree | band | ~np.isfinite(e_ref)) & valid[:, :, None]
    near |= unsettled[:, None, None]
    f_spread = np.where(np.isfinite(f_spread), f_spread, np.inf)
    return dict(near=near, unsettled=unsettled, near_in=(near & dec_ref).sum(axis=2), near_out=(near & ~dec_ref).sum(axis=2),
                f_spread=f_spread, dec_ref=dec_ref)


def replay_is_certain(cid):
    """the replay on count intervals [ref - near_in, ref + near_out] (an unsettled hypothesis: up to three models of any count):
    True when every count vector inside them gives the reference's winner and stop index"""
    ref, al = reference(cid), allowances(cid)
    n = len(ref["used"])
    tab, H = ref["table"], case(cid)["opts"]["max_iters"]
    lo, hi = ref["counts"] - al["near_in"], ref["counts"] + al["near_out"]
    bl = bh = 0
    nl = nh = H
    best = None
    h = 0
    while h < nl:
        k = 3 if al["unsettled"][h] else int(ref["n_models"][h])
        for m in range(k):
            a, b = (0, n) if al["unsettled"][h] else (int(lo[h, m]), int(hi[h, m]))
            if a > max(bh, 6):
                best, bl, bh = (h, m), a, b
                nl, nh = min(nl, int(tab[a:b + 1].min())), min(nh, int(tab[a:b + 1].max()))
            elif b > max(bl, 6):
                return False
        h += 1
    return nl == nh and h == ref["stop"] and (best or (-1, -1)) == tuple(ref["winner"])


def f32_step(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32)).astype(np.float32)).astype(np.float64)


def compare(cid, dev):
    """what the GPU test asserts of a run: dev = dict(samples, n_models, models, counts, table, mask, F, count, winner, niters,
    n_with_model, too_few, no_model) -> (failures [str], figures dict)"""
    ref, al, c = reference(cid), allowances(cid), case(cid)
    fail, fig = [], {}
    H = c["opts"]["max_iters"]
    if not np.array_equal(dev["samples"], ref["samples"]):
        fail.append("samples differ on %d hypotheses" % (dev["samples"] != ref["samples"]).any(axis=1).sum())
    if not np.array_equal(dev["table"], ref["table"]):
        fail.append("table differs")
    settled = ~al["unsettled"]
    if not np.array_equal(dev["n_models"][settled], ref["n_models"][settled]):
        fail.append("n_models differs on a settled hypothesis: %s" % np.where(settled & (dev["n_models"] != ref["n_models"]))[0][:8])
    valid = (np.arange(3)[None, :] < ref["n_models"][:, None]) & settled[:, None]
    low, high = ref["counts"] - al["near_in"], ref["counts"] + al["near_out"]
    bad = valid & ((dev["counts"] < low) | (dev["counts"] > high))
    if bad.any():
        fail.append("counts outside the near allowance at %s" % np.argwhere(bad)[:8].tolist())
    fig["counts_off_reference"] = int((valid & (dev["counts"] != ref["counts"])).sum())
    if tuple(dev["winner"]) != tuple(ref["winner"]) or dev["niters"] != ref["niters"] or dev["count"] < 0:
        fail.append("winner %s / niters %d, reference %s / %d" % (tuple(dev["winner"]), dev["niters"], tuple(ref["winner"]), ref["niters"]))
    if bool(dev["too_few"]) != ref["too_few"] or bool(dev["no_model"]) != ref["no_model"]:
        fail.append("too_few / no_model")
    if dev["n_with_model"] != ref["n_with_model"] and not al["unsettled"].any():
        fail.append("hypotheses with a model: %d, reference %d" % (dev["n_with_model"], ref["n_with_model"]))
    if ref["winner"][0] >= 0 and tuple(dev["winner"]) == tuple(ref["winner"]):
        h, m = ref["winner"]
        near_w = np.zeros(ref["n"], dtype=bool)
        near_w[ref["used"]] = al["near"][h, m]
        fig["near_winner"] = int(near_w.sum())
        if near_w.sum() > NEAR_CAP * ref["n"]:
            fail.append("%d near points for the winner" % near_w.sum())
        if not np.array_equal(dev["mask"][~near_w], ref["mask"][~near_w]):
            fail.append("mask differs outside the near points")
        bound = 4 * max(SPREAD_F[cid], 9 * np.finfo(np.float64).eps)   # floor: one rounding per entry of the unit F
        err = float(np.abs(unit(dev["F"]) - unit(ref["F"])).max())
        fig.update(f_err=err, f_bound=bound)
        if not err <= bound:
            fail.append("F: %.3e above %.3e" % (err, bound))
        if dev["count"] < low[h, m] or dev["count"] > high[h, m]:
            fail.append("best count")
    elif ref["winner"][0] < 0 and dev["mask"].any():
        fail.append("a mask without a model")
    return fail, fig


# ---- undistortion ---------------------------------------------------------------------------------------------------------------
def undistort_pixels():
    """a 9 x 7 grid over 752 x 480, the corners, the principal point itself"""
    from ov_plane_amd.synth import INTRINSICS

    xs, ys = np.meshgrid(np.linspace(0, 751, 9), np.linspace(0, 479, 7))
    grid = np.stack([xs.ravel(), ys.ravel()], axis=1)
    extra = np.array([[0, 0], [751, 0], [0, 479], [751, 479], [INTRINSICS[2], INTRINSICS[3]]])
    return np.concatenate([grid, extra]).astype(np.float32)


def undistort_cameras():
    from ov_plane_amd.synth import FISHEYE_INTRINSICS, INTRINSICS

    return {"radtan": (epi_ref.MODE_RADTAN, INTRINSICS), "equidistant": (epi_ref.MODE_EQUIDISTANT, FISHEYE_INTRINSICS)}


@functools.lru_cache(maxsize=None)
def undistort_reference(name):
    """-> (f32 result of the float64 restatement, bound [n, 2]: 4 x the recorded spread float64 / long double before rounding, and
    one f32 step, since two values that close may round to neighbouring floats; the spread as measured now)"""
    mode, intr = undistort_cameras()[name]
    px = undistort_pixels()
    a = epi_ref.undistort(px, mode, intr, dtype=np.float64, rounded=False)
    b = epi_ref.undistort(px, mode, intr, dtype=np.longdouble, rounded=False)
    spread = np.abs(a - b.astype(np.float64))
    want = a.astype(np.float32)
    return want, 4 * SPREAD_UNDISTORT[name] + f32_step(want), float(spread.max())


# ---- recorded figures (measured on the CPU by tests/test_epipolar_cpu.py, which re-measures them: a change of the restatement that
# moves a bound the device is held to fails there) ---------------------------------------------------------------------------------
# the winner's F: the largest distance of a variant's matched unit F from the float64 one
SPREAD_F = {
    "n10_all_inliers": 7.2720e-15,
    "n63": 2.4869e-14,
    "n64": 5.6899e-15,
    "n65": 3.6887e-14,
    "n300_out30": 4.3937e-14,
    "n120_out65": 8.9373e-15,
    "n80_status": 5.8287e-15,
    "n100_iters1": 1.2434e-14,
    "n100_iters64": 1.2434e-14,
    "n100_iters65": 1.2434e-14,
    "n100_iters1024": 1.2434e-14,
}
# the undistorted coordinates before rounding: float64 against long double, worst over the test pixels
SPREAD_UNDISTORT = {
    "radtan": 2.2204e-16,
    "equidistant": 2.6645e-15,
}
