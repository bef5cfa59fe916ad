"""The entries that keep P resident between updates (ovp_cov_upload / download / set_device / marginal / propagate / clone /
marginalize / augment_dt / initialize_invertible) against numpy indexing, bit for bit, where they copy, and against the long-double
restatements of oracle/ld_ref.py, inside the derived rounding bounds of tests/cov_bookkeeping_cases.py, where they sum.  Errors are
taken element by element on covariances whose scales spread over eight decades.  Every case runs in a context with n_max = n and
in one with n_max > n, checks cov_size() afterwards, and every refusal must leave the bits of P and the size as they were.  Then
the factor the plane loop keeps for the point update: every entry that writes P must drop it."""
import numpy as np
import pytest

import cov_bookkeeping_cases as B
from oracle import ld_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool(hiplib):
    """one small context per capacity, shared by the cases (each case uploads its own covariance first)"""
    made = {}

    def get(n_max):
        if n_max not in made:
            made[n_max] = hiplib.Context(n_max, 2, 4)
        made[n_max].cov_clone_jitter(0.0)
        return made[n_max]

    yield get
    for c in made.values():
        c.close()


def refused(hiplib, code, fn, *a, **kw):
    with pytest.raises(hiplib.OvpError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, code)


def unchanged(ctx, P):
    assert ctx.cov_size() == len(P) and np.array_equal(ctx.cov_download(), P)


def report(case, r):
    print("BOOKKEEPING %s %.3f" % (case, r))
    return r


# ---- copies ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", B.STATE_SIZES)
def test_upload_download_set_device(hiplib, pool, n):
    import torch

    P = B.spd(n, n)
    for n_max in B.capacities(n):
        ctx = pool(n_max)
        ctx.cov_upload(P)
        assert ctx.cov_size() == n and np.array_equal(ctx.cov_download(), P)
        ctx.cov_upload(2 * P, ld=n + 3)                             # host rows further apart than n, both ways
        assert np.array_equal(ctx.cov_download(ld=n + 7), 2 * P) and np.array_equal(ctx.cov_download(), 2 * P)
        # refusals: the covariance and its size stay
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_upload, P, ld=n - 1)
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_download, ld=n - 1)
        for wrong in (n - 1, n + 1):
            out = np.zeros((wrong + 1, wrong + 1))
            assert hiplib.lib().ovp_cov_download(ctx.handle, out.ctypes.data, wrong, wrong + 1) == hiplib.OVP_E_ARG and not out.any()
        refused(hiplib, hiplib.OVP_E_CAPACITY, ctx.cov_upload, B.spd(n_max + 1, 1))
        unchanged(ctx, 2 * P)
        # set_device from a tensor whose row stride is neither n nor the context's
        for stride in (n, n + 9):
            t = torch.full((n, stride), float("nan"), dtype=torch.float64, device="cuda")
            t[:, :n] = torch.from_numpy(3 * P).cuda()
            torch.cuda.synchronize()
            ctx.cov_set_device(t.data_ptr(), n, stride)
            assert ctx.cov_size() == n and np.array_equal(ctx.cov_download(), 3 * P)
        refused(hiplib, hiplib.OVP_E_CAPACITY, ctx.cov_set_device, t.data_ptr(), n_max + 1, n_max + 1)
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_set_device, t.data_ptr(), n, n - 1)
        unchanged(ctx, 3 * P)
        if n_max > n:                                               # a smaller covariance behind a larger one, and back
            ctx.cov_upload(B.spd(n_max, 2))
            ctx.cov_upload(P)
            unchanged(ctx, P)
        del t


@pytest.mark.parametrize("n", B.STATE_SIZES)
def test_marginal(hiplib, pool, n):
    rng = np.random.default_rng(n)
    P = B.spd(n, 10 + n)
    for n_max in B.capacities(n):
        ctx = pool(n_max)
        ctx.cov_upload(P)
        lists = [[(n - 1, 1)],                                       # m = 1
                 [(n - 4, 4), (0, 3), (5, 2)],                      # unsorted
                 [(2, 4), (0, 5), (2, 4)],                          # a variable listed twice (and overlapping another), m = 13 <= n_max
                 [(0, n)],                                           # m = n
                 [(int(i), 1) for i in rng.permutation(n)]]          # m = n, every column a variable of its own, shuffled
        if n >= 129:
            lists.append([(n - 100, 100), (0, 29)])                 # m = 129
        for vs in lists:
            cols = B.flat(vs)
            M = ctx.cov_marginal([v[0] for v in vs], [v[1] for v in vs])
            assert np.array_equal(M, P[np.ix_(cols, cols)]), vs
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_marginal, [0, n - 2], [3, 3])       # runs past the state
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_marginal, [n], [1])
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_marginal, [-1], [2])
        refused(hiplib, hiplib.OVP_E_CAPACITY, ctx.cov_marginal, [0, 0], [n, n_max - n + 1])  # m = n_max + 1
        unchanged(ctx, P)
        assert np.array_equal(ctx.cov_marginal([1], [2]), P[1:3, 1:3])


# ---- propagation ---------------------------------------------------------------------------------------------------------
def _propagate(hiplib, ctx, c, P, Phi, Q):
    """-> (verdict, P behind the call); the binding raises on the negative-diagonal verdict"""
    try:
        neg = ctx.cov_propagate(c["start"], [v[0] for v in c["old"]], [v[1] for v in c["old"]], Phi, Q)
    except hiplib.OvpError as e:
        assert e.code == hiplib.OVP_E_NEGDIAG
        neg = 1
    return neg, ctx.cov_download()


def _check_prop(c, P, Phi, Q, Pd, tag):
    n, a, phi = c["n"], c["start"], c["phi"]
    T, comp = ld_ref.ekf_propagation(P, a, B.flat(c["old"]), Phi, Q)
    K = B.prop_K(c)
    r = report("propagate/%s" % tag, B.ratio(Pd, T, comp, K))
    blk = np.zeros((n, n), dtype=bool)
    blk[a:a + phi, a:a + phi] = True
    # inside the block the two triangles are separate sums of the same value; outside it P is exactly symmetric
    r_sym = report("propagate/%s/symmetry" % tag, B.ratio(Pd[blk], Pd.T[blk], comp[blk], K[blk]))
    touched = np.zeros((n, n), dtype=bool)
    touched[a:a + phi, :] = touched[:, a:a + phi] = True
    assert np.array_equal(Pd[~touched], P[~touched])
    assert np.array_equal(Pd[~blk], Pd.T[~blk])
    assert r <= 1.0 and r_sym <= 1.0
    return T


@pytest.mark.parametrize("c", B.prop_cases(), ids=lambda c: c["name"])
def test_propagate(hiplib, pool, c):
    P, Phi, Q = B.prop_inputs(c)
    n = c["n"]
    assert c["phi"] == 1 or not np.array_equal(Q, Q.T)
    for n_max in B.capacities(n):
        ctx = pool(n_max)
        ctx.cov_upload(P)
        neg, Pd = _propagate(hiplib, ctx, c, P, Phi, Q)
        assert ctx.cov_size() == n
        T = _check_prop(c, P, Phi, Q, Pd, "%s/nmax%d" % (c["name"], n_max))
        assert neg == int((np.diag(T) < 0).any()) == 0


@pytest.mark.parametrize("name", ["front15", "anchor_change", "end64"])
def test_propagate_negative_diagonal_verdict_and_its_reset(hiplib, pool, name):
    c = [x for x in B.prop_cases() if x["name"] == name][0]
    n, a = c["n"], c["start"]
    P, Phi, Q = B.prop_inputs(c)
    T, _ = ld_ref.ekf_propagation(P, a, B.flat(c["old"]), Phi, Q)
    Qn = B.prop_inputs(c, qdiag=-4.0 * float(T[a, a]))[2]          # drives the block's first diagonal element to about -3x itself
    for n_max in B.capacities(n):
        ctx = pool(n_max)
        # a Q that drives a diagonal element of the block negative: the verdict, with P written as the truth says
        ctx.cov_upload(P)
        neg, Pd = _propagate(hiplib, ctx, c, P, Phi, Qn)
        Tn = _check_prop(c, P, Phi, Qn, Pd, "%s/negative_block/nmax%d" % (name, n_max))
        assert neg == 1 and Tn[a, a] < 0 and Pd[a, a] < 0 and ctx.cov_size() == n
        # a clean call straight after reports 0
        ctx.cov_upload(P)
        assert _propagate(hiplib, ctx, c, P, Phi, Q)[0] == 0
        # a negative diagonal element outside the block (the last row for a block in front, the first otherwise) is reported as well
        far = n - 1 if a == 0 else 0
        Pbad = P.copy()
        Pbad[far, far] = -Pbad[far, far]
        ctx.cov_upload(Pbad)
        neg, Pd = _propagate(hiplib, ctx, c, Pbad, Phi, Q)
        _check_prop(c, Pbad, Phi, Q, Pd, "%s/negative_outside/nmax%d" % (name, n_max))
        assert neg == 1 and Pd[far, far] == Pbad[far, far]
        ctx.cov_upload(P)
        assert _propagate(hiplib, ctx, c, P, Phi, Q)[0] == 0


def test_propagate_refusals(hiplib, pool):
    n = 129
    P = B.spd(n, 77)
    rng = np.random.default_rng(5)
    for n_max in B.capacities(n):
        ctx = pool(n_max)
        ctx.cov_upload(P)
        big = rng.standard_normal((65, 65))
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_propagate, 0, [0], [65], big, big)                       # phi = 65
        sq = rng.standard_normal((3, 3))
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_propagate, n - 2, [0], [3], sq, sq)                      # the block leaves the state
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_propagate, -1, [0], [3], sq, sq)
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_propagate, 0, [n - 2], [3], sq, sq)                      # an old variable does
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_propagate, 0, [-1], [3], sq, sq)
        unchanged(ctx, P)
        c = dict(name="after_refusals", n=n, start=n - 64, phi=64, old=[(n - 64, 64)], seed=78)          # phi = 64 goes through
        _, Phi, Q = B.prop_inputs(c)
        neg, Pd = _propagate(hiplib, ctx, c, P, Phi, Q)
        _check_prop(c, P, Phi, Q, Pd, "after_refusals/nmax%d" % n_max)


# ---- clone / marginalize ---------------------------------------------------------------------------------------------------
def _cloned(P, src, size):
    idx = np.concatenate([np.arange(len(P)), np.arange(src, src + size)])
    return P[np.ix_(idx, idx)]


def _without(P, vid, size):
    keep = np.r_[0:vid, vid + size:len(P)]
    return P[np.ix_(keep, keep)]


@pytest.mark.parametrize("n", B.STATE_SIZES)
def test_clone_up_to_capacity(hiplib, pool, n):
    """sources first / middle / last, sizes 1 / 3 / 6, until n = n_max exactly; one more is refused"""
    room = 20 if n < 700 else 0
    n0 = n if room else n - 20
    P = B.spd(n0, 20 + n)
    ctx = pool(n0 + 20)
    ctx.cov_upload(P)
    for size, where in ((6, "first"), (3, "middle"), (1, "last"), (6, "last"), (3, "first"), (1, "middle")):
        m = len(P)
        src = {"first": 0, "middle": (m - size) // 2, "last": m - size}[where]
        ctx.cov_clone(src, size)
        P = _cloned(P, src, size)
        unchanged(ctx, P)                                            # the whole matrix, bit for bit
    assert len(P) == n0 + 20 == ctx.n_state_max
    refused(hiplib, hiplib.OVP_E_CAPACITY, ctx.cov_clone, 0, 1)
    refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_clone, len(P) - 2, 3)
    refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_clone, -1, 3)
    refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_clone, 0, 0)
    unchanged(ctx, P)
    ctx.cov_marginalize(0, 6)                                        # the next valid call works, and a clone fits again
    ctx.cov_clone(len(P) - 12, 6)
    unchanged(ctx, _cloned(_without(P, 0, 6), len(P) - 12, 6))


@pytest.mark.parametrize("n", [17, 257])
def test_clone_jitter(hiplib, pool, n):
    P = B.spd(n, 30 + n)
    for n_max in (n + 6, n + 11):
        ctx = pool(n_max)
        ctx.cov_upload(P)
        for bad in (1.1e-6, -1e-12, float("nan")):
            refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_clone_jitter, bad)
        ctx.cov_clone(3, 6)                                          # (a refused jitter leaves the exact copy in force)
        unchanged(ctx, _cloned(P, 3, 6))
        ctx.cov_marginalize(n, 6)
        ctx.cov_clone_jitter(1e-11)
        src = n - 6
        ctx.cov_clone(src, 6)
        Pd = ctx.cov_download()
        want = _cloned(P, src, 6)
        dg = np.arange(n, n + 6)
        T, comp = B.jitter_truth(want[dg, dg], 1e-11)
        r = report("clone_jitter/n%d/nmax%d" % (n, n_max), B.ratio(Pd[dg, dg], T, comp, B.JITTER_K))
        assert (Pd[dg, dg] > want[dg, dg]).all()
        Pd[dg, dg] = want[dg, dg]
        assert np.array_equal(Pd, want) and r <= 1.0              # the new block's diagonal only
        ctx.cov_clone_jitter(0.0)


@pytest.mark.parametrize("n", B.STATE_SIZES)
def test_marginalize_down_to_one_and_clone_behind_it(hiplib, pool, n):
    P = B.spd(n, 40 + n)
    for n_max in B.capacities(n):
        ctx = pool(n_max)
        ctx.cov_upload(P)
        Q = P
        steps = [(1, "first"), (6, "middle"), (1, "last")] + ([(130, "middle"), (6, "last"), (6, "first")] if n >= 257 else [])
        for size, where in steps:
            m = len(Q)
            vid = {"first": 0, "middle": (m - size) // 2, "last": m - size}[where]
            ctx.cov_marginalize(vid, size)
            Q = _without(Q, vid, size)
            unchanged(ctx, Q)
        m = len(Q)
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_marginalize, m - 2, 3)
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_marginalize, -1, 1)
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_marginalize, 0, 0)
        unchanged(ctx, Q)
        # clone straight after a marginalize: the two buffers have been swapped, the new rows must not show old content
        ctx.cov_clone(1, 3)
        Q = _cloned(Q, 1, 3)
        unchanged(ctx, Q)
        ctx.cov_marginalize(1, len(Q) - 2)                           # down to n = 2, then 1
        Q = _without(Q, 1, len(Q) - 2)
        unchanged(ctx, Q)
        ctx.cov_marginalize(0, 1)
        Q = _without(Q, 0, 1)
        assert Q.shape == (1, 1)
        unchanged(ctx, Q)
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_marginalize, 0, 2)
        unchanged(ctx, Q)


# ---- augment_dt ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", B.augment_cases(), ids=lambda c: c["name"])
def test_augment_dt(hiplib, pool, c):
    P, d = B.augment_inputs(c)
    n, p, t = c["n"], c["pose"], c["dt"]
    T, comp = ld_ref.augment_dt(P, p, t, d)
    K = B.augment_K(c)
    for n_max in B.capacities(n):
        ctx = pool(n_max)
        ctx.cov_upload(P)
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_augment_dt, n - 5, t, d)           # pose_id + 6 > n
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_augment_dt, -1, t, d)
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_augment_dt, p, n, d)               # dt_id >= n
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_augment_dt, p, -1, d)
        for inside in (p, p + 3, p + 5):                                             # a dt inside the pose block has no meaning
            refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_augment_dt, p, inside, d)
        unchanged(ctx, P)
        ctx.cov_augment_dt(p, t, d)
        Pd = ctx.cov_download()
        r = report("augment_dt/%s/nmax%d" % (c["name"], n_max), B.ratio(Pd, T, comp, K))
        assert ctx.cov_size() == n and np.array_equal(Pd[K == 0], P[K == 0])
        assert r <= 1.0


# ---- initialize_invertible -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", B.init_cases(), ids=lambda c: c["name"])
def test_initialize_invertible(hiplib, pool, c):
    P, H_R, H_Linv, R = B.init_inputs(c)
    n, k, cols = c["n"], c["k"], c["cols"]
    assert k == 1 or not np.array_equal(R, R.T)
    T, comp = ld_ref.initialize_invertible(P, cols, H_R, H_Linv, R)
    Kb = B.init_K(c)
    rng = np.random.default_rng(1)
    for n_max in (n + k, n + k + 4):                                 # n + k = n_max exactly, and room to spare
        ctx = pool(n_max)
        ctx.cov_upload(P)
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_initialize_invertible, rng.standard_normal((7, 2)), [0, 1], np.eye(7), np.eye(7))
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_initialize_invertible, H_R, cols[:-1] + [n], H_Linv, R)   # a column id >= n
        refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_initialize_invertible, H_R, cols[:-1] + [-1], H_Linv, R)
        if k > 1:
            refused(hiplib, hiplib.OVP_E_ARG, ctx.cov_initialize_invertible, H_R, cols, H_Linv, R, ld=k - 1)
        unchanged(ctx, P)
        ctx.cov_initialize_invertible(H_R, cols, H_Linv, R, ld=c["ld"])
        Pd = ctx.cov_download()
        r = report("initialize_invertible/%s/nmax%d" % (c["name"], n_max), B.ratio(Pd, T, comp, Kb))
        assert ctx.cov_size() == n + k and np.array_equal(Pd[:n, :n], P)
        assert np.array_equal(Pd[:n, n:], Pd[n:, :n].T)             # the cross block is written twice from one value
        assert r <= 1.0
        if n_max == n + k:                                           # the state is full: one more column is refused
            refused(hiplib, hiplib.OVP_E_CAPACITY, ctx.cov_initialize_invertible, H_R[:1], cols, H_Linv[:1, :1], R[:1, :1])
            unchanged(ctx, Pd)
            ctx.cov_marginalize(n, k)
            unchanged(ctx, P)


# ---- the kept factor -------------------------------------------------------------------------------------------------------
KEPT_ENTRIES = ["cov_upload", "cov_set_device", "cov_propagate", "cov_clone", "cov_marginalize", "cov_marginalize_many", "cov_augment_dt",
                "cov_initialize_invertible", "cov_initialize", "ekf_update", "planes_merge_retire"]


@pytest.fixture(scope="module")
def kept_scene():
    from ov_plane_amd.synth import make_scene

    # the scene of tests/test_zupt_gpu.py's kept-factor test with two landmarks behind the clones (the columns the batch uses end
    # with the last clone): the entries that shrink the state retire the first of them
    return make_scene(C=8, F=96, seed=11, ragged=True, n_planes=3, feats_per_plane=14, chi2_mult=99999.0, n_slam=2)


def _entry(hiplib, name, c, sc, P):
    """one call of the entry on the covariance P the plane loop left (n = len(P)), on columns the point update does not use where
    it changes the size"""
    n = len(P)
    rng = np.random.default_rng(17)
    lm = int(sc.ids["slam"][0])
    cl = int(sc.ids["clones"][2])
    s = np.sqrt(np.diag(P))
    if name == "cov_upload":
        c.cov_upload(1.5 * P)
    elif name == "cov_set_device":
        import torch

        t = torch.from_numpy(np.ascontiguousarray(1.5 * P)).cuda()
        torch.cuda.synchronize()
        c.cov_set_device(t.data_ptr(), n, n)
        c.cov_download()  # (synchronises the copy before the tensor goes)
    elif name == "cov_propagate":
        Phi = np.eye(15) + 0.2 * rng.standard_normal((15, 15)) * np.outer(s[:15], 1 / s[:15])
        c.cov_propagate(0, [0], [15], Phi, 0.5 * P[:15, :15])
    elif name == "cov_clone":
        c.cov_clone(cl, 6)
    elif name == "cov_marginalize":
        c.cov_marginalize(lm, 3)
    elif name == "cov_marginalize_many":
        c.cov_marginalize_many([lm], [3])
    elif name == "cov_augment_dt":
        c.cov_augment_dt(cl, int(sc.ids["dt"]), 3.0 * s[cl:cl + 6] / s[sc.ids["dt"]])
    elif name in ("cov_initialize_invertible", "cov_initialize"):
        cols = list(range(cl, cl + 6))
        H_R = rng.standard_normal((3, 6)) / s[cols][None, :]
        Hinv = np.linalg.inv(rng.standard_normal((3, 3)) + 2 * np.eye(3))
        if name == "cov_initialize_invertible":
            c.cov_initialize_invertible(H_R, cols, Hinv, 0.1 * np.eye(3))
        else:
            acc, _, _ = c.cov_initialize(H_R, None, cols, Hinv, 0.1 * np.eye(3), None, 0.1, 1e9, do_update=False)
            assert acc
    elif name == "ekf_update":
        cols = list(range(cl, cl + 6))
        c.ekf_update(rng.standard_normal((4, 6)) / s[cols][None, :], cols, rng.standard_normal(4))
    elif name == "planes_merge_retire":
        c.planes_merge_retire([], [], [], np.zeros(0), 0.01, 1.0, 5.0, [lm], [3])
    else:
        raise KeyError(name)


def _fit(a, n):
    """dx or P of a state of another size, read at the size n: leading entries, zeros where there are none"""
    out = np.zeros((n,) * a.ndim)
    m = min(n, a.shape[0])
    out[(slice(0, m),) * a.ndim] = a[(slice(0, m),) * a.ndim]
    return out


@pytest.mark.parametrize("name", KEPT_ENTRIES)
def test_every_entry_that_writes_P_drops_the_kept_factor(hiplib, kept_scene, name):
    """Arm A: plane loop, the entry, point update.  Arm B: a fresh context handed the covariance behind the entry by upload, point
    update - the same arithmetic on the same bits, so A = B to 1e-9 (the bound of test_kept_factor_is_dropped_on_acceptance_...).
    Arm C: a fresh context handed the covariance from BEFORE the entry - what a point update on the stale factor amounts to; it
    must differ from B by more than 1e-6, or the parameter could not tell a stale factor from a fresh one.  Where the entry changes
    the size, C's dx and P are read at B's size (leading columns, zeros for columns C does not have): a stale factor is read at the
    new size, column by column."""
    from test_zupt_gpu import relP

    sc = kept_scene
    cap = sc.N + 6

    def point(c):
        c.state_upload(sc)  # every arm the same tables (the batch stays: a new one would void the loop's mask of consumed features)
        o = hiplib.opts_from_scene(sc)
        o.chi2_multiplier = 1.0
        o.skip_plane_used = 1
        out = c.msckf_update(o)
        return out, c.cov_download()

    a = hiplib.Context(cap, sc.C, sc.F)
    try:
        a.cov_upload(sc.P)
        a.state_upload(sc)
        a.batch_upload_scene(sc)
        o = hiplib.opts_from_scene(sc)
        pl = a.plane_update(o, sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id)
        assert pl["ok"].all() and len(pl["ok"]) == 3
        used = pl["used"].copy()
        P_before = a.cov_download()
        _entry(hiplib, name, a, sc, P_before)
        P_e = a.cov_download()
        assert not np.array_equal(_fit(P_before, len(P_e)), P_e)
        out_a, Pa = point(a)
    finally:
        a.close()

    def fresh(P):
        c = hiplib.Context(cap, sc.C, sc.F)
        try:
            # the same plane decisions (the mask of consumed features) without a kept factor: the loop, then the upload
            c.cov_upload(sc.P)
            c.state_upload(sc)
            c.batch_upload_scene(sc)
            o = hiplib.opts_from_scene(sc)
            pl = c.plane_update(o, sc.plane_id, sc.cp, sc.cp_fej, sc.plane_state_id)
            assert np.array_equal(pl["used"], used)
            c.cov_upload(P)
            return point(c)
        finally:
            c.close()

    out_b, Pb = fresh(P_e)
    out_c, Pc = fresh(P_before)
    n = len(P_e)
    e_dx, e_P = float(np.abs(out_a["dx"] - out_b["dx"]).max()), relP(Pa, Pb)
    d_dx, d_P = float(np.abs(_fit(out_c["dx"], n) - out_b["dx"]).max()), relP(_fit(Pc, n), Pb)
    print("KEPT %s: A vs B |d dx| %.1e, normalised |dP| %.1e; B vs C |d dx| %.1e, normalised |dP| %.1e" % (name, e_dx, e_P, d_dx, d_P))
    assert (out_a["accepted"] == out_b["accepted"]).all() and out_a["accepted"].sum() > 0
    assert e_dx < 1e-9 and e_P < 1e-9
    assert d_dx > 1e-6 and d_P > 1e-6
