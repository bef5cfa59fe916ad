"""ovp_zupt_update (k_zupt.hip) against the long-double truth oracle/ld_ref.py::zupt_compressed, inside the rounding bounds
tests/zupt_cases.py derives, element by element, on covariances whose scales spread over eight decades: chi2, dx and P at
error / bound <= 1, the decision and `rows` equal, P exactly symmetric, every element the update does not reach bit-equal to the
input (there is none in an accepted call: Y is dense; a rejected call leaves everything), cov_size() right, in a context with
n_max = n and in one with n_max = n + 5.  The cases reach what the parity tests (tests/test_zupt_gpu.py) do not: eleven row blocks
and 990 tiles at n = 700, more than one interval per thread of the gate (257 / 258 / 4096 readings), the IMU block at the end of
the state and across a 64-row border.  One line per case and capacity: ZUPT <case> <worst ratio>."""
import numpy as np
import pytest

import zupt_cases as ZC
import zupt_ref as Z
from precision_helpers import context_pool

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool(hiplib):
    yield from context_pool(hiplib)


def run(ctx, c):
    P, rd, kw = ZC.inputs(c)
    x = ZC.imu_state()
    ctx.cov_upload(P)
    out = ctx.zupt_update(rd, c["imu_id"], x["R"], x["Rj"], x["bg"], x["ba"], Z.PO, ZC.threshold(c), noise_mult=Z.NOISE_MULT, **kw)
    return out, ctx.cov_download()


@pytest.mark.parametrize("c", ZC.cases(), ids=lambda c: c["name"])
def test_zupt_against_the_long_double_truth(hiplib, pool, c):
    P, rd, _ = ZC.inputs(c)
    t, _, _ = ZC.truth(c)
    acc = ZC.expected(c)
    n = c["n"]
    results = []
    for n_max in ZC.capacities(n):
        ctx = pool(n_max)
        out, Pd = run(ctx, c)
        # (a result of the wrong size, or a decision that differs, still gets its line: inf)
        fits = Pd.shape == (n, n) and out["dx"].shape == (n,) and out["accepted"] == acc
        r = ZC.ratios(c, out["chi2"], out["dx"] if acc else None, Pd if acc else None) if fits else [float("inf")]
        print("ZUPT %s/nmax%d %.4f   (%s)" % (c["name"], n_max, max(r), " ".join("%.4f" % v for v in r)))
        results.append((n_max, out, Pd, r, ctx.cov_size()))
    for n_max, out, Pd, r, size in results:
        assert out["accepted"] == acc and out["rows"] == t["rows"] == 6 * (len(rd) - 1) and not out["neg_diag"]
        assert size == n and Pd.shape == (n, n)
        assert np.array_equal(Pd, Pd.T)
        if not acc:
            assert np.array_equal(Pd, P) and not out["dx"].any()
        assert max(r) <= 1.0, (n_max, r)


def test_two_runs_of_the_largest_call_give_the_same_bits(hiplib, pool):
    c = [x for x in ZC.cases() if x["name"] == "n700_r4096_end_accept"][0]
    ctx = pool(700)
    a, Pa = run(ctx, c)
    b, Pb = run(ctx, c)
    assert a["accepted"] and b["accepted"]
    assert a["chi2"] == b["chi2"] and np.array_equal(a["dx"], b["dx"]) and np.array_equal(Pa, Pb)
