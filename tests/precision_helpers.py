"""What the long-double precision tests of the zero-velocity update and of the retire / merge step share
(tests/zupt_cases.py, tests/retire_cases.py and their GPU tests): the covariance generator, the capacities a case runs in, and the
pool of device contexts."""
import numpy as np


def spd_with(n, seed, cols, scales):
    """cov_bookkeeping_cases.spd (the same stream of random numbers) with the standard deviations of `cols` replaced by `scales`:
    exactly symmetric, positive definite, every other column's scale spread over eight decades"""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n + 3))
    A = G @ G.T / (n + 3)
    A = (A + A.T) / 2 + 0.5 * np.eye(n)
    s = 10.0 ** rng.uniform(-4.0, 4.0, n)
    s[np.asarray(cols, dtype=np.int64)] = scales
    return np.outer(s, s) * A


def capacities(n):
    """n_max = n and n_max > n (700 is the largest context there is)"""
    return (n,) if n >= 700 else (n, n + 5)


def context_pool(hiplib):
    """generator behind a module-scoped fixture: yields get(n_max) -> one small context per capacity, shared by the cases (each
    case uploads its own covariance first); closes them at the end"""
    made = {}

    def get(n_max):
        if n_max not in made:
            made[n_max] = hiplib.Context(n_max, 2, 4)
        return made[n_max]

    yield get
    for c in made.values():
        c.close()
