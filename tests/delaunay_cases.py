"""Inputs of the Delaunay tests (tests/test_delaunay_cpu.py pins them on the host, tests/test_delaunay_gpu.py runs the device
kernel on them): pixel positions [n, 2] in f32, each generator deterministic."""
import numpy as np

W, H = 752, 480
RANDOM_N = (3, 4, 5, 48, 257, 1024)
GRID_G = (4, 8, 32)
NEAR_G = (16, 32)


def random_pixels(n, seed=48):
    rng = np.random.default_rng(seed + n)
    return np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1).astype(np.float32)


def collinear(n=64):
    i = np.arange(n, dtype=np.float32)
    return np.stack([3 * i, 2 * i], 1)  # exact in f32: every orientation is exactly zero


def identical(n=64):
    return np.tile(np.array([[100.5, 37.25]], dtype=np.float32), (n, 1))


def every_third_a_duplicate(n=1024):
    xy = random_pixels(n, seed=7)
    xy[3::3] = xy[0]
    return xy


def six_points():
    """a duplicate and a point exactly on a hull edge (tests/test_plane_detect_cpu.py)"""
    return np.array([[0, 0], [10, 0], [0, 10], [10, 0], [5, 5], [10, 10]], dtype=np.float32)


def collinear_but_the_last(n=1024):
    """n - 1 points on a line and the only point off it last: the seed search runs to the end"""
    i = np.arange(n, dtype=np.float32)
    xy = np.stack([i, np.zeros(n, dtype=np.float32)], 1)
    xy[-1] = [5.0, 7.0]
    return xy


def grid(g):
    """exactly cocircular: 10 (i % g, i // g); every product of the predicates is exact"""
    i = np.arange(g * g)
    return (10 * np.stack([i % g, i // g], 1)).astype(np.float32)


def near_grid(g):
    """(123.456f + 0.1f (i % g), 77.7f + 0.1f (i // g)) in f32 arithmetic: nearly cocircular, the signs hang on the last bits"""
    i = np.arange(g * g)
    x = np.float32(123.456) + np.float32(0.1) * (i % g).astype(np.float32)
    y = np.float32(77.7) + np.float32(0.1) * (i // g).astype(np.float32)
    assert x.dtype == np.float32 and y.dtype == np.float32
    return np.stack([x, y], 1)


def ellipse(n=1024):
    """every point on the hull: an insertion's cavity is a fan of up to a few hundred triangles.  The angle step is not a
    fraction of the turn: equally spaced angles put four points (+-x, +-y) on one circle exactly, and the sign of such a
    determinant is the arithmetic's choice (the numpy restatement's LU and the library's expansion then differ)"""
    a = 0.3 + 0.0061 * np.arange(n)
    return np.stack([400 + 300 * np.cos(a), 300 + 200 * np.sin(a)], 1).astype(np.float32)


def descending_x(n=1024):
    """x descending, y = i^2 mod 997: every insertion lies outside the hull.  x falls along a parabola, not a line: i and 997 - i
    share their y, so equally spaced x would make every two such pairs an isosceles trapezoid - four points on one circle"""
    i = np.arange(n)
    u = i / n
    x = (750 - 600 * u - 140 * u * u).astype(np.float32)
    assert (np.diff(x) < 0).all()
    return np.stack([x, ((i * i) % 997).astype(np.float32)], 1)


def all_cases():
    """name -> xy, every input of the GPU file's comparisons"""
    c = {"random_%d" % n: random_pixels(n) for n in RANDOM_N}
    c.update(n0=np.zeros((0, 2), np.float32), n1=random_pixels(1), n2=random_pixels(2), collinear=collinear(), identical=identical(),
             every_third_a_duplicate=every_third_a_duplicate(), six_points=six_points(), collinear_but_the_last=collinear_but_the_last(),
             ellipse=ellipse(), descending_x=descending_x())
    c.update({"grid_%d" % g: grid(g) for g in GRID_G})
    c.update({"near_grid_%d" % g: near_grid(g) for g in NEAR_G})
    return c
