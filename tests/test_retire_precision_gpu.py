"""ovp_planes_merge_retire and ovp_cov_marginalize_many (k_retire.hip) at the shapes tests/test_retire_gpu.py does not reach.
Merge: against the long-double truth oracle/ld_ref.py::plane_merge, inside the rounding bounds tests/retire_cases.py derives and
carries through a chain, element by element, on covariances whose scales spread over eight decades: chi2, the angle, dx and the
compacted P at error / bound <= 1, equal decisions, P exactly symmetric, a rejected pair's dx zero, a call without an accepted pair
the compaction of the input bit for bit, cov_size() right.  Compaction: bit-equal to numpy indexing.  The cases run the second
column of tiles of the downdate, the second and third workgroup of columns of the compaction, its scan with 256 and 257 ranges,
three strides of the gate's row loop, survivors before and behind the old plane, chains with a rejected pair in the middle, and
the limits of 64 pairs and 128 planes in one call.  One line per case and capacity: RETIRE <case> <worst ratio>."""
import numpy as np
import pytest

import cov_bookkeeping_cases as B
import retire_cases as RC
import retire_ref as R
from precision_helpers import capacities, context_pool

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool(hiplib):
    yield from context_pool(hiplib)


def run(ctx, c):
    ctx.cov_upload(c["P"])
    out = ctx.planes_merge_retire([p[0] for p in c["pairs"]], [p[1] for p in c["pairs"]], c["plane_col"], c["cp"], c["sigma"], c["chi2_mult"],
                                  c["deg_max"], c["retire_ids"], c["retire_sizes"])
    out["n"] = ctx.cov_size()
    out["P"] = ctx.cov_download()
    return out


@pytest.mark.parametrize("name", RC.names())
def test_merge_against_the_long_double_truth(hiplib, pool, name):
    c = RC.case(name)
    t, _, _ = RC.truth(name)
    n_out = c["n"] - sum(c["retire_sizes"])
    results = []
    for n_max in capacities(c["n"]):
        out = run(pool(n_max), c)
        same = out["accepted"].tolist() == t["accepted"].tolist()
        r = RC.ratios(name, out["chi2"], out["angle_deg"], out["dx"], out["P"]) if same and out["n"] == n_out else [float("inf")]
        print("RETIRE %s/nmax%d %.4f   (%s) decisions %s" % (name, n_max, max(r), " ".join("%.4f" % v for v in r),
                                                             "equal" if same else out["accepted"].tolist()))
        results.append((n_max, out, r))
    for n_max, out, r in results:
        assert out["accepted"].tolist() == t["accepted"].tolist() == RC.expected(c) and not out["neg_diag"]
        assert out["n"] == n_out and out["P"].shape == (n_out, n_out)
        assert np.array_equal(out["P"], out["P"].T)
        for k, kind in enumerate(c["kinds"]):
            if not t["accepted"][k]:
                assert not out["dx"][k].any()
            if kind == "parallel":
                assert out["angle_deg"][k] == 0.0
        if not t["accepted"].any():  # nothing was accepted: every entry is the input's, bit for bit
            assert np.array_equal(out["P"], R.compact_ref(c["P"], c["retire_ids"], c["retire_sizes"]))
        assert max(r) <= 1.0, (n_max, r)


def test_two_runs_of_the_64_pair_call_give_the_same_bits(hiplib, pool):
    c = RC.case("n399_limits")
    a, b = run(pool(399), c), run(pool(399), c)
    assert a["accepted"].sum() == 48
    for k in ("accepted", "chi2", "angle_deg", "dx", "P"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", list(RC.compact_cases()))
def test_compaction_is_bit_equal_to_indexing(hiplib, pool, name):
    n, ids, sizes = RC.compact_cases()[name]
    P = B.spd(n, 60 + n + len(ids))
    want = R.compact_ref(P, ids, sizes)
    for n_max in capacities(n):
        ctx = pool(n_max)
        ctx.cov_upload(P)
        ctx.cov_marginalize_many(ids, sizes)
        got = ctx.cov_download()
        ok = ctx.cov_size() == n - sum(sizes) and np.array_equal(got, want)
        print("RETIRE compact/%s/nmax%d %s" % (name, n_max, "0.0000" if ok else "inf"))
        assert ok
