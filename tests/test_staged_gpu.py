"""The staged upload on the device (csrc/ovp_staged.h): an entry that returns without waiting leaves its tables' copy behind, and the
next entry writes the same pinned block.  Back-to-back calls on one context give the bits of the same calls with a context
synchronisation between them (or of a fresh context that made only the last upload), and a growth of the shared staging block
between two calls changes nothing either."""
import numpy as np
import pytest

import retire_ref as R
from ov_plane_amd.synth import make_scene

pytestmark = pytest.mark.gpu

N_MAX, C_MAX, F_MAX = 64, 4, 16


def _both(run):
    """run(sync) with sync a no-op, and with sync the context's synchronisation: the two results"""
    return run(lambda ctx: None), run(lambda ctx: ctx.sync())


def _same(got, want, what=""):
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k)


def test_two_compactions_in_a_row(hiplib):
    """(a) ovp_cov_marginalize_many twice with different ranges on a 30-column covariance: the second call's ranges overwrite the
    first's in the pinned block (two ranges against three, so a late first copy would carry a range of the second)"""
    P = np.ascontiguousarray(R.small_state()[:30, :30])

    def run(sync):
        ctx = hiplib.Context(N_MAX, C_MAX, F_MAX)
        ctx.cov_upload(P)
        ctx.cov_marginalize_many([2, 11, 20], [3, 2, 4])
        sync(ctx)
        ctx.cov_marginalize_many([0, 9], [1, 6])
        out = dict(P=ctx.cov_download())
        ctx.close()
        return out

    got, want = _both(run)
    assert got["P"].shape == (14, 14)
    _same(got, want)
    assert np.array_equal(want["P"], R.compact_ref(R.compact_ref(P, [2, 11, 20], [3, 2, 4]), [0, 9], [1, 6]))


def test_state_and_batch_uploaded_twice_then_a_point_update(hiplib):
    """(b) table A immediately followed by table B, batch A immediately followed by batch B (fewer features than A), one point
    update: what a fresh context gives that uploaded only B"""
    A = make_scene(C=4, F=12, seed=1, chi2_mult=99999.0)
    B = make_scene(C=4, F=7, seed=2, chi2_mult=99999.0)
    assert A.N == B.N <= N_MAX and not np.array_equal(A["clone_p"], B["clone_p"])

    def run(first):
        ctx = hiplib.Context(N_MAX, C_MAX, F_MAX)
        ctx.cov_upload(B.P)
        for sc in first + [B]:
            ctx.state_upload(sc)
        for sc in first + [B]:
            ctx.batch_upload_scene(sc)
        out = ctx.msckf_update(hiplib.opts_from_scene(B))
        res = dict(dx=out["dx"], accepted=out["accepted"], chi2=out["chi2"], P=ctx.cov_download())
        ctx.close()
        return res

    got, want = run([A]), run([])
    assert want["accepted"].any()
    _same(got, want)


def test_two_feature_database_frames_in_a_row(hiplib):
    """(c) two appended frames, the second smaller and of other features in part, then the read-back of every track"""
    rng = np.random.default_rng(3)
    ids1, ids2 = np.arange(100, 140), np.arange(120, 150, 3)
    fr = lambda ids: (ids, rng.uniform(0, 600, (len(ids), 2)).astype(np.float32), rng.uniform(-1, 1, (len(ids), 2)).astype(np.float32))
    f1, f2 = fr(ids1), fr(ids2)

    def run(sync):
        ctx = hiplib.Context(N_MAX, C_MAX, F_MAX)
        db = hiplib.FeatureDatabase(ctx, max_slots=64, max_meas=8)
        db.update_feature(1.0, *f1)
        sync(ctx)
        db.update_feature(2.0, *f2)
        out = {}
        for fid in sorted(set(ids1) | set(ids2)):
            f = db.get_feature(fid)
            out.update({"%d_%s" % (fid, k): np.asarray(f[k]) for k in ("count", "ts", "uv", "uv_norm", "slot")})
        db.close()
        ctx.close()
        return out

    got, want = _both(run)
    assert int(want["120_count"]) == 2 and int(want["100_count"]) == 1 and int(want["147_count"]) == 1
    assert np.array_equal(want["123_uv"], np.stack([f1[1][23], f2[1][1]]))
    _same(got, want)


def test_compaction_only_retire_then_a_merge(hiplib):
    """(d) ovp_planes_merge_retire with no pair (it does not wait) directly followed by one with a pair"""
    P0 = R.small_state()
    kw = R.cases()["a_accepted"]
    E = R.PLANES[4]  # the last three columns: the merge's columns keep their places

    def run(sync):
        ctx = hiplib.Context(N_MAX, C_MAX, F_MAX)
        ctx.cov_upload(P0)
        none = ctx.planes_merge_retire([], [], [], [], 1.0, 1.0, 1.0, [E], [3])
        assert len(none["accepted"]) == 0 and ctx.cov_size() == R.N - 3
        sync(ctx)
        p = kw["pairs"]
        out = ctx.planes_merge_retire([q[0] for q in p], [q[1] for q in p], kw["plane_col"], kw["cp"], kw["sigma"], kw["chi2_mult"],
                                      kw["deg_max"], kw["retire_ids"], kw["retire_sizes"])
        res = dict(accepted=out["accepted"], chi2=out["chi2"], angle=out["angle_deg"], dx=out["dx"], P=ctx.cov_download())
        ctx.close()
        return res

    got, want = _both(run)
    assert want["accepted"].tolist() == [True] and want["P"].shape == (R.N - 6, R.N - 6)
    _same(got, want)


def _dense_update(hiplib, ctx, rows, cols, seed):
    sc = make_scene(C=4, F=4, seed=4)
    rng = np.random.default_rng(seed)
    ctx.cov_upload(sc.P)
    dx, info = ctx.ekf_update(rng.standard_normal((rows, cols)), sc.ids["clones"][0] + np.arange(cols), 1e-3 * rng.standard_normal(rows))
    return dict(dx=dx, P=ctx.cov_download(), info=np.array([info.n_rows, info.n_cols]))


def test_growth_of_the_staging_block_between_calls(hiplib):
    """(e) the dense update's tables travel in the block the plane loop and the SLAM entries share (8 (rows cols + rows + 8) +
    4 cols + 64 bytes): 12 x 12 sizes it with 4096 bytes of slack, 40 x 24 does not fit, then 12 x 12 again on the grown block"""
    calls = ((12, 12, 5), (40, 24, 6), (12, 12, 5))
    ctx = hiplib.Context(N_MAX, C_MAX, F_MAX)
    cap = lambda: int(ctx.debug_read("pl_stage_cap", (1,), dtype=np.uint64)[0])
    got, caps = [], []
    for rows, cols, seed in calls:
        got.append(_dense_update(hiplib, ctx, rows, cols, seed))
        caps.append(cap())
    ctx.close()
    print("pl_stage_cap behind each call:", caps)
    need = lambda rows, cols: 8 * (rows * cols + rows + 8) + 4 * cols + 64
    assert need(12, 12) <= caps[0] < need(40, 24) <= caps[1] == caps[2]
    fresh = {}
    for call, g in zip(calls, got):
        if call not in fresh:
            c2 = hiplib.Context(N_MAX, C_MAX, F_MAX)
            fresh[call] = _dense_update(hiplib, c2, *call)
            c2.close()
        _same(g, fresh[call], str(call))
    assert got[0]["info"].tolist() == [12, 12] and np.abs(got[1]["dx"]).max() > 0
