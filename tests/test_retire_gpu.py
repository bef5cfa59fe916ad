"""ovp_cov_marginalize_many and ovp_planes_merge_retire through capi, on the small state of tests/retire_ref.py (n = 63).
Compaction: bit-equal to ovp_cov_marginalize called once per range in descending order of id.  Merge: against the numpy
restatement of state/StateHelper.cpp:693-734 in retire_ref.py - identical decisions, chi2 / angle at 1e-9 relative, every accepted dx
at 1e-9 of its largest entry, P at 1e-9 normalised (max |dP_ij| / sqrt(P_ii P_jj)), the level the plane-detection and plane-front-end
tests hold their restatements to."""
import numpy as np
import pytest

import retire_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module")
def P0():
    return R.small_state()


def _ctx(hiplib, P):
    c = hiplib.Context(P.shape[0] + 8, 4, 8)
    c.cov_upload(P)
    return c


def _one_by_one(hiplib, P, ids, sizes):
    c = _ctx(hiplib, P)
    for i, s in sorted(zip(ids, sizes), reverse=True):
        c.cov_marginalize(i, s)
    out = c.cov_download()
    c.close()
    return out


A, B, Cc, D, E = R.PLANES
COMPACT = {
    "single": ([R.SLAM[1]], [3]),
    "adjacent": ([R.SLAM[0], R.SLAM[1]], [3, 3]),
    "ascending": ([R.CLONES[0], R.SLAM[2], B, E], [6, 3, 3, 3]),
    "descending": ([E, B, R.SLAM[2], R.CLONES[0]], [3, 3, 3, 6]),
    "shuffled": ([B, R.CLONES[0], E, R.SLAM[2]], [3, 6, 3, 3]),
    "last_columns": ([E], [3]),
    "six_and_threes": ([R.CLONES[1], R.SLAM[0], D], [6, 3, 3]),
    "single_columns": ([0, 62, 17], [1, 1, 1]),
}


@pytest.mark.parametrize("name", sorted(COMPACT))
def test_compaction_is_bit_equal_to_one_by_one(hiplib, P0, name):
    ids, sizes = COMPACT[name]
    c = _ctx(hiplib, P0)
    c.cov_marginalize_many(ids, sizes)
    assert c.cov_size() == R.N - sum(sizes)
    got = c.cov_download()
    c.close()
    assert np.array_equal(got, _one_by_one(hiplib, P0, ids, sizes))
    assert np.array_equal(got, R.compact_ref(P0, ids, sizes))  # ... which only copies


def test_compaction_49_to_31(hiplib, P0):
    """the three clones leave a state of 49 columns: n goes from above a multiple of 16 to below the one before it"""
    P = np.ascontiguousarray(P0[:49, :49])
    c = _ctx(hiplib, P)
    c.cov_marginalize_many(R.CLONES[::-1], [6, 6, 6])
    assert c.cov_size() == 31
    got = c.cov_download()
    c.close()
    assert np.array_equal(got, _one_by_one(hiplib, P, R.CLONES, [6, 6, 6]))


def test_compaction_of_nothing_and_bad_ranges_touch_nothing(hiplib, P0):
    c = _ctx(hiplib, P0)
    live = lambda: c.debug_read("live_bytes", 2, np.int64).tolist()  # noqa: E731
    before = live()
    c.cov_marginalize_many([], [])
    assert live() == before and c.cov_size() == R.N and np.array_equal(c.cov_download(), P0)
    for ids, sizes in (([B, B + 2], [3, 3]), ([R.N - 2], [3]), ([-1], [3]), ([R.N], [1]), ([A], [0]), ([A, A], [3, 3])):
        with pytest.raises(hiplib.OvpError) as e:
            c.cov_marginalize_many(ids, sizes)
        assert e.value.code == hiplib.OVP_E_ARG
        assert c.cov_size() == R.N and np.array_equal(c.cov_download(), P0)
    empty = hiplib.Context(16, 4, 8)
    with pytest.raises(hiplib.OvpError) as e:
        empty.cov_marginalize_many([0], [1])
    assert e.value.code == hiplib.OVP_E_STATE
    empty.close()
    c.close()


def _run(hiplib, P, kw):
    c = _ctx(hiplib, P)
    pairs = kw["pairs"]
    out = c.planes_merge_retire([p[0] for p in pairs], [p[1] for p in pairs], kw["plane_col"], kw["cp"], kw["sigma"], kw["chi2_mult"],
                                kw["deg_max"], kw["retire_ids"], kw["retire_sizes"])
    out["n"] = c.cov_size()
    out["P"] = c.cov_download()
    c.close()
    return out


@pytest.mark.parametrize("name", sorted(R.EXPECTED))
def test_merge_matches_restatement(hiplib, P0, name):
    kw = R.cases()[name]
    ref = R.merge_ref(P0, **kw)
    out = _run(hiplib, P0, kw)
    assert not out["neg_diag"] and out["n"] == ref["P"].shape[0] == R.N - sum(kw["retire_sizes"])
    e_chi2 = float((np.abs(out["chi2"] - ref["chi2"]) / ref["chi2"]).max())
    e_ang = float((np.abs(out["angle_deg"] - ref["angle_deg"]) / ref["angle_deg"]).max())
    e_dx = max([float(np.abs(out["dx"][k] - ref["dx"][k]).max() / np.abs(ref["dx"][k]).max()) for k in range(len(ref["dx"])) if ref["accepted"][k]],
               default=0.0)
    e_P = R.normalised(out["P"], ref["P"])
    print("%s: decisions %s, rel |d chi2| %.2e, rel |d angle| %.2e, |d dx| / max|dx| %.2e, normalised |dP| %.2e" % (
        name, out["accepted"].tolist(), e_chi2, e_ang, e_dx, e_P))
    assert out["accepted"].tolist() == ref["accepted"].tolist() == R.EXPECTED[name]
    assert e_chi2 < TOL and e_ang < TOL and e_dx < TOL and e_P < TOL
    for k in range(len(ref["dx"])):
        if not ref["accepted"][k]:
            assert not out["dx"][k].any()
    assert np.array_equal(out["P"], out["P"].T)
    if name == "d_chain":  # the dependency between the pairs is seen: the stale-value answer is not within the tolerance
        stale = R.merge_ref(P0, stale_cp=True, **kw)
        assert np.abs(out["dx"][1] - stale["dx"][1]).max() / np.abs(stale["dx"][1]).max() > 1e3 * TOL
        assert abs(out["chi2"][1] - stale["chi2"][1]) / stale["chi2"][1] > 1e3 * TOL


def test_merge_two_runs_give_the_same_bits(hiplib, P0):
    kw = R.cases()["e_chain_retire"]
    a, b = _run(hiplib, P0, kw), _run(hiplib, P0, kw)
    for k in ("accepted", "chi2", "angle_deg", "dx", "P"):
        assert np.array_equal(a[k], b[k]), k


def test_rejected_only_call_is_the_compaction(hiplib, P0):
    kw = dict(R.cases()["b_chi2"], retire_ids=[E, B, R.SLAM[0]], retire_sizes=[3, 3, 3])
    out = _run(hiplib, P0, kw)
    assert out["accepted"].tolist() == [False]
    c = _ctx(hiplib, P0)
    c.cov_marginalize_many(kw["retire_ids"], kw["retire_sizes"])
    assert np.array_equal(out["P"], c.cov_download())
    c.close()


def test_merge_argument_errors_touch_nothing(hiplib, P0):
    c = _ctx(hiplib, P0)
    cpA = R.cases()["a_accepted"]["cp"]
    call = lambda new, old, cols, cps, rid, rsz: c.planes_merge_retire(new, old, cols, cps, 0.001, 1.0, 1.0, rid, rsz)  # noqa: E731
    bad = [
        (hiplib.OVP_E_ARG, ([A], [A], [A, B], cpA, [B], [3])),                     # new == old
        (hiplib.OVP_E_ARG, ([A], [B], [A, B], cpA, [Cc], [3])),                    # the old plane is not retired
        (hiplib.OVP_E_ARG, ([A], [B], [A, B], cpA, [B, B + 1], [3, 3])),           # overlapping retire ranges
        (hiplib.OVP_E_ARG, ([A], [B], [A, Cc], cpA, [B], [3])),                    # a pair names a plane that is not in the table
        (hiplib.OVP_E_ARG, ([A], [R.N - 2], [A, R.N - 2], cpA, [R.N - 2], [2])),   # a column outside the state
        (hiplib.OVP_E_CAPACITY, ([A] * 65, [B] * 65, [A, B], cpA, [B], [3])),      # 65 pairs
        (hiplib.OVP_E_CAPACITY, ([A], [B], [A, B] + [0] * 127, np.zeros((129, 3)), [B], [3])),   # 129 planes in the table
        (hiplib.OVP_E_ARG, ([A], [A + 2], [A, A + 2], cpA, [A + 2], [3])),         # the two planes' columns overlap: |new - old| < 3
        (hiplib.OVP_E_ARG, ([A, Cc], [B, B], [A, B, Cc], np.zeros((3, 3)), [B], [3])),  # a plane already fused away is named again
    ]
    for code, args in bad:
        with pytest.raises(hiplib.OvpError) as e:
            call(*args)
        assert e.value.code == code, args
        assert c.cov_size() == R.N and np.array_equal(c.cov_download(), P0)
    c.close()
