"""CPU tests of the epipolar check's yardstick (tests/epi_ref.py, tests/epi_cases.py) and of the library's boundary: the new symbols
and struct layouts, the generator's draws and the iteration table against constants derived here, the branches the cases meet, the
mutants of the restatement - one convention changed at a time - that the GPU comparison must catch, the planted inlier sets, and
the caps on what the restatement's variants leave undecided.

Two branches no point case meets are met on probes of the restatement's own pieces: the cubic's two-root branch needs a
discriminant of exactly zero ((x - 1)^2 (x + 2)), and is met by epi_ref.solve_cubic alone."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epi_cases  # noqa: E402
import epi_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry(hiplib):
    hdr = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    assert "int ovp_klt_epipolar(ovp_ctx *ctx, const ovp_epipolar_opts *opts, int n, const float *pts0, const float *pts1" in hdr
    assert "void ovp_epipolar_defaults(ovp_epipolar_opts *o);" in hdr and "typedef struct ovp_epipolar_info" in hdr
    L = hiplib.lib()
    for s in ("ovp_klt_epipolar", "ovp_epipolar_defaults"):
        assert s in hiplib.EXPORTS and hasattr(L, s)
    # the struct layouts: every field of the header, in its order, at the offset a C compiler gives it
    for name, cls in (("ovp_epipolar_opts", hiplib.EpipolarOpts), ("ovp_epipolar_info", hiplib.EpipolarInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        fields = []
        for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
            d = decl.strip()
            if d:
                fields += [re.sub(r"\[\d+\]", "", f.strip()) for f in d.split(None, 1)[1].split(",")]
        assert fields == [f[0] for f in cls._fields_], (fields, cls._fields_)
    assert ctypes.sizeof(hiplib.EpipolarOpts) == 96 and ctypes.sizeof(hiplib.EpipolarInfo) == 104
    assert hiplib.EpipolarOpts.threshold.offset == 72 and hiplib.EpipolarInfo.best_count.offset == 72
    o = hiplib.EpipolarOpts()
    L.ovp_epipolar_defaults(ctypes.byref(o))
    assert (o.mode, o.max_iters, o.confidence, o.seed) == (0, 1000, 0.999, 0) and o.threshold == 2.0 / 458.654
    assert L.ovp_klt_epipolar(None, ctypes.byref(o), 0, None, None, None, None, None, None, None) == -1  # OVP_E_ARG on a null context


def test_first_draws_equal_constants():
    """x = seed + 0x9E3779B9 (h + 1) + 0x85EBCA6B (t + 1) mod 2^32, the 32-bit finaliser, (x n) >> 32.  The constants below come
    from a second implementation written from the issue's text (decimal multipliers, one loop for the two multiply rounds), not
    from epi_ref.draw."""
    def second(seed, h, t, n):
        m = (1 << 32) - 1
        x = (seed + 2654435769 * (h + 1) + 2246822507 * (t + 1)) & m
        for shift, mul in ((16, 2246822507), (13, 3266489909)):
            x = ((x ^ (x >> shift)) * mul) & m
        return ((x ^ (x >> 16)) * n) >> 32
    for seed, h, n in ((0, 0, 10), (7, 3, 300), (0xFFFFFFFF, 1023, 4096)):
        got = [epi_ref.draw(seed, h, t, n) for t in range(8)]
        assert got == [second(seed, h, t, n) for t in range(8)] and all(0 <= g < n for g in got)
    assert [epi_ref.draw(0, 0, t, 10) for t in range(4)] == FIRST_DRAWS_0_0_10
    assert [epi_ref.draw(7, 3, t, 300) for t in range(4)] == FIRST_DRAWS_7_3_300
    assert [epi_ref.draw(0xFFFFFFFF, 1023, t, 4096) for t in range(4)] == FIRST_DRAWS_MAX


FIRST_DRAWS_0_0_10 = [0, 5, 3, 7]
FIRST_DRAWS_7_3_300 = [274, 131, 236, 129]
FIRST_DRAWS_MAX = [3826, 274, 1251, 2037]


def test_table_equals_values_derived_by_hand():
    """niters(c) = log(1 - 0.999) / log(1 - (c / n)^7), rounded half to even, capped at max_iters; c = n gives 0 (the denominator
    1 - 1^7 is below DBL_MIN); c = 0 gives max_iters (log(1) = 0 is not negative)"""
    for n, H in ((10, 200), (300, 1000)):
        tab = epi_ref.table(n, 0.999, H)
        assert len(tab) == n + 1 and tab[n] == 0 and tab[0] == H
        for c in range(1, n):
            w = c / n
            want = math.log(0.001) / math.log(1.0 - w ** 7) if 1.0 - w ** 7 < 1.0 else math.inf   # (w^7 below an ulp of 1: log(1) = 0)
            assert tab[c] == (H if want >= H else int(round(want))), (n, c)
        assert (np.diff(tab) <= 0).all()
    # n = 10: 9 of 10 inliers: 0.9^7 = 0.4782969, log(0.001) / log(0.5217031) = 10.6 -> 11; 7 of 10: 0.7^7 = 0.0823543 -> 80.4 -> 80
    t10 = epi_ref.table(10, 0.999, 200)
    assert t10[9] == 11 and t10[7] == 80 and t10[6] == 200   # (0.6^7 -> 243.3: above max_iters)
    # n = 300: 210 inliers is the same ratio 0.7 -> 80; 150: 0.5^7 = 1 / 128 -> 6.9078 / 0.0078431 = 880.7 -> 881
    t300 = epi_ref.table(300, 0.999, 1000)
    assert t300[210] == 80 and t300[150] == 881 and t300[149] == 923


BRANCHES = ["roots_1", "roots_3", "collinear_redrawn", "no_set", "early_stop", "exhausted", "no_model", "f33_tiny"]


def test_branch_table():
    met = {}
    for cid in epi_cases.IDS:
        for k, v in epi_cases.reference(cid)["branches"].items():
            if v is True:
                met.setdefault(k, []).append(cid)
    for b in BRANCHES:
        print("%-18s %s" % (b, met.get(b, [])))
        assert met.get(b), "no case meets the branch %s" % b
    # the two-root branch: a discriminant of exactly zero, (x - 1)^2 (x + 2) = x^3 - 3 x + 2 - on the cubic alone
    assert [float(r) for r in epi_ref.solve_cubic([1.0, 0.0, -3.0, 2.0])] == [-2.0, 1.0]
    print("%-18s %s" % ("roots_2", "probe: solve_cubic on x^3 - 3 x + 2"))
    assert sorted(float(r) for r in epi_ref.solve_cubic([0.0, 1.0, -3.0, 2.0])) == [1.0, 2.0]      # the quadratic
    assert [float(r) for r in epi_ref.solve_cubic([0.0, 0.0, 2.0, -3.0])] == [1.5]                  # the linear one
    assert epi_cases.reference("n9_too_few")["too_few"] and not epi_cases.reference("n9_too_few")["mask"].any()
    assert epi_cases.reference("n10_all_inliers")["stop"] == 1
    mid = epi_cases.reference("n300_out30")
    assert 10 < mid["stop"] < 500, "the stop index lands in the middle"
    assert not epi_cases.reference("n40_line")["mask"].any()


def _fields(cid, conv):
    r = epi_cases.run(cid, conv=conv)
    F = np.round(epi_cases.unit(r["F"]), 6) if r["winner"][0] >= 0 else np.zeros(9)
    return (r["mask"].tobytes(), tuple(r["winner"]), r["niters"], r["stop"], r["count"], F.tobytes(), r["too_few"], r["no_model"],
            None if "samples" not in r else r["samples"].tobytes())


@pytest.mark.parametrize("name", list(epi_ref.MUTANTS))
def test_mutant_differs_on_a_case(name):
    conv = epi_ref.mutant(name)
    caught = [cid for cid in epi_cases.IDS if _fields(cid, conv) != _fields(cid, epi_ref.CONV)]
    if name.startswith("radtan"):
        for cam, (mode, intr) in epi_cases.undistort_cameras().items():
            px = epi_cases.undistort_pixels()
            if epi_ref.undistort(px, mode, intr, conv).tobytes() != epi_ref.undistort(px, mode, intr).tobytes():
                caught.append("undistort:" + cam)
    # two conventions no point case can meet - an error of exactly threshold^2 as a float, a model of fewer than 7 inliers (a
    # model fits its own seven points) - are met on the restatement's pieces, as the two-root branch is
    t32 = epi_ref.threshold_f32(epi_cases.THRESHOLD)
    if epi_ref.inliers(np.array([t32]), epi_cases.THRESHOLD, conv)[0] != epi_ref.inliers(np.array([t32]), epi_cases.THRESHOLD)[0]:
        caught.append("probe:error_equals_threshold")
    few = (np.array([1]), np.array([[5, 0, 0]]), epi_ref.table(20, 0.999, 1), 1)
    if epi_ref.replay(*few, conv)["best"] != epi_ref.replay(*few)["best"]:
        caught.append("probe:five_inliers")
    print("%s: differs on %s" % (name, caught))
    assert caught, "the mutant %s equals the restatement on every case" % name


@pytest.mark.parametrize("cid", epi_cases.OUTLIER_CASES)
def test_planted_inliers_are_recovered(cid):
    c, r, al = epi_cases.case(cid), epi_cases.reference(cid), epi_cases.allowances(cid)
    h, m = r["winner"]
    near = al["near"][h, m]
    sure = ~near & ~c["unknown"]
    print("%s: %d planted inliers, %d kept; %d planted outliers, %d kept; %d near" % (
        cid, c["planted"].sum(), r["mask_rsc"][c["planted"]].sum(), (~c["planted"]).sum(), r["mask_rsc"][~c["planted"] & ~c["unknown"]].sum(), near.sum()))
    assert r["mask_rsc"][c["planted"] & sure].all(), "a planted inlier is missing"
    assert not r["mask_rsc"][~c["planted"] & ~c["unknown"]].any(), "a planted outlier was kept"
    if c["status"] is not None:
        gone = c["status"] == 0
        assert gone.sum() == 20 and r["mask_rsc"][gone & c["planted"]].all() and not r["mask"][gone].any()
        assert np.isin(np.where(gone)[0], r["samples"]).any(), "the RANSAC draws among the status-0 points"


@pytest.mark.parametrize("cid", [c for c in epi_cases.IDS if c != "n9_too_few"])
def test_caps_on_what_the_variants_leave_open(cid):
    r, al = epi_cases.reference(cid), epi_cases.allowances(cid)
    if cid in epi_cases.UNCOMPARED:
        assert np.isfinite(r["F"]).all()
        return
    stop = max(r["stop"], 1)
    uns = int(al["unsettled"][:r["stop"]].sum())
    h, m = r["winner"]
    near_w = int(al["near"][h, m].sum()) if h >= 0 else 0
    fs = float(al["f_spread"][h, m]) if h >= 0 else 0.0
    print("%s: %d of %d hypotheses in front of the stop index unsettled, %d of %d points near for the winner, F spread %.3e" % (
        cid, uns, stop, near_w, r["n"], fs))
    assert uns <= epi_cases.NEAR_CAP * stop and near_w <= epi_cases.NEAR_CAP * r["n"]
    if h >= 0:   # the recorded figure the GPU test uses, re-measured
        rec = epi_cases.SPREAD_F[cid]
        assert fs <= rec * (1 + 1e-3) and rec * 0.95 <= fs, (fs, rec)
    assert epi_cases.replay_is_certain(cid), "another seed of the same shape is needed"
    # every variant passes the comparison the device is held to
    st = dict(samples=r["samples"], refused=r["refused"])
    for name, dtype, null in epi_cases.VARIANTS:
        v = epi_cases.run(cid, dtype=dtype, null=null, stages=st)
        if null == "svd":   # another basis: the same solutions, possibly in another order - the winner's set and F are compared
            assert v["count"] == r["count"] and np.array_equal(v["mask"], r["mask"]), "the SVD basis gives another inlier set"
            if h >= 0:
                assert np.abs(epi_cases.unit(v["F"]) - epi_cases.unit(r["F"])).max() <= 4 * max(epi_cases.SPREAD_F[cid], 2e-15)
            continue
        dev = dict(v, models=v["models"].astype(np.float64))
        fail, fig = epi_cases.compare(cid, dev)
        assert not fail, (name, fail)


@pytest.mark.parametrize("cam", ["radtan", "equidistant"])
def test_undistortion_inverts_the_camera_model(cam):
    """the recalled iteration counts against the generator's own 30-iteration inverses (synth.py, unchanged): 5 radtan iterations
    agree with 30 to 1e-6 inside r < 0.5 and to 5e-3 at the corners; the principal point maps to (0, 0)"""
    from ov_plane_amd import synth

    mode, intr = epi_cases.undistort_cameras()[cam]
    px = epi_cases.undistort_pixels()
    got = epi_ref.undistort(px, mode, intr)
    inv = synth.radtan_undistort if cam == "radtan" else synth.equi_undistort
    x, y = inv(px[:, 0].astype(np.float64), px[:, 1].astype(np.float64), intr)
    err = np.abs(got.astype(np.float64) - np.stack([x, y], axis=1)).max()
    want, bound, spread = epi_cases.undistort_reference(cam)
    print("%s: worst |5-or-10-step - 30-step| %.3e, float64 / long double spread %.3e" % (cam, err, spread))
    rec = epi_cases.SPREAD_UNDISTORT[cam]
    assert spread <= rec * (1 + 1e-3) and rec * 0.95 <= spread, (spread, rec)
    # five steps of a fixed-point iteration that contracts by about 2 |k1| r^2 (0.6 at the corners, r^2 = 1.07) leave about
    # 0.6^5 of the corner's distortion offset of 0.02: 1.5e-3; inside r < 0.5 the rate is below 0.15 and the offset below 0.002
    r = np.hypot(x, y)
    inner = np.abs(got.astype(np.float64) - np.stack([x, y], axis=1))[r < 0.5].max()
    assert err < 5e-3 and inner < 1e-6 and want.tobytes() == got.tobytes(), (err, inner)
    assert abs(got[-1]).max() < 1e-6   # (the principal point, as far as f32 pixels hold it)
    assert epi_ref.undistort(px, 0, intr).tobytes() == px.tobytes()


def test_frame_logic():
    """(f): nothing goes in -> the reset; fewer than 10 -> nothing kept and no KLT; otherwise the mask decides with the border rules"""
    calls = []

    def track(p):
        calls.append(len(p))
        q = p + np.float32(1.0)
        q[1, 0] = -0.5
        return q, np.ones(len(p), dtype=np.uint8)

    def epi(p0, p1, st):
        m = np.ones(len(p0), dtype=np.uint8)
        m[2] = 0
        return dict(mask=m & st, uvn1=p1 * np.float32(0.01))
    ids, pts, uvn, reset = epi_ref.feed_monocular([], np.zeros((0, 2)), track, 64, 48, None, epi)
    assert reset and not len(ids) and not calls
    ids, pts, uvn, reset = epi_ref.feed_monocular(np.arange(9), np.ones((9, 2)), track, 64, 48, None, epi)
    assert not reset and not len(ids) and not calls
    p = np.stack([np.arange(12) * 4.0 + 2, np.arange(12) * 3.0 + 2], axis=1).astype(np.float32)
    mask = np.zeros((48, 64), dtype=np.uint8)
    mask[int(p[5, 1]) + 1, int(p[5, 0]) + 1] = 255
    ids, pts, uvn, reset = epi_ref.feed_monocular(np.arange(12), p, track, 64, 48, mask, epi)
    assert calls == [12] and list(ids) == [0, 3, 4, 6, 7, 8, 9, 10, 11] and uvn.tobytes() == (pts * np.float32(0.01)).tobytes()


# ---- the host logic of the C++ mirror against the restatement's frame logic, without a device -------------------------------------
def test_mirror_compiles_and_the_harness_exports_the_sequence_entry():
    from ov_plane_amd.build import build_host

    L = ctypes.CDLL(build_host())
    assert hasattr(L, "ovph_run_klt_epipolar_sequence")
    hdr = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "host", "ov_plane_trackplane.h")).read()
    assert "int perform_matching(" in hdr and "int set_camera(int mode" in hdr and "bool epipolar = false" in hdr and "get_last_uv_norm" in hdr


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    import subprocess

    exe = str(tmp_path_factory.mktemp("epi_host") / "epi_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "ov_plane_amd", "csrc", "host"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "epi_host_main.cpp"), "-o", exe])
    return exe


def _bits(v):
    return "%08x" % int(np.float32(v).view(np.uint32))


def _mirror_frame(exe, tmp_path, w, h, mask, ids, pts, moved, status, rsc, uvn):
    import subprocess

    lines = ["%d %d %d" % (w, h, 0 if mask is None else 1)]
    if mask is not None:
        lines.append(" ".join(str(int(v)) for v in np.asarray(mask).ravel()))
    lines.append(str(len(ids)))
    lines += ["%d %s %s" % (i, _bits(p[0]), _bits(p[1])) for i, p in zip(ids, pts)]
    lines.append(str(len(moved)))
    lines += ["%s %s %d %d %s %s" % (_bits(q[0]), _bits(q[1]), s, r, _bits(u[0]), _bits(u[1])) for q, s, r, u in zip(moved, status, rsc, uvn)]
    f = tmp_path / "in.txt"
    f.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(f)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    out = run.stdout.split("\n")
    reset, calls, k = (int(v) for v in out[0].split())
    rows = [l.split() for l in out[1:1 + k]]
    got_ids = np.array([int(r[0]) for r in rows], dtype=np.int64)
    f32 = np.array([[int(v, 16) for v in r[1:5]] for r in rows], dtype=np.uint32).reshape(-1, 4).view(np.float32)
    return bool(reset), calls, got_ids, f32[:, :2], f32[:, 2:]


def test_host_logic_of_the_mirror_equals_the_frame_logic(host_exe, tmp_path):
    """the device calls stubbed by the restatement: the KLT's result is given, the epipolar check is epi_ref.epipolar on it"""
    rng = np.random.default_rng(5)
    w, h = 64, 48
    mask = np.zeros((h, w), dtype=np.uint8)
    mask[10:20, 30:40] = 255
    c = epi_cases.case("n80_status")
    n = 80
    pts = np.stack([rng.uniform(2, w - 6, n), rng.uniform(2, h - 6, n)], axis=1).astype(np.float32)
    moved = (pts + rng.uniform(-1, 4, (n, 2))).astype(np.float32)
    moved[3] = [-0.5, 10.0]            # leaves on the left: dropped though (int) x is 0
    moved[4] = [w - 0.5, 10.0]         # (int) x = w - 1: stays
    moved[5] = [w + 0.25, 10.0]        # leaves on the right
    moved[6] = [12.0, h]               # leaves below
    moved[7] = [33.5, 12.5]            # into the mask
    e = epi_ref.epipolar(c["pts0"], c["pts1"], c["status"], c["opts"])      # any mask and coordinates of 80 points will do
    ids = np.arange(500, 500 + n)

    def check(k):
        want = epi_ref.feed_monocular(ids[:k], pts[:k], lambda p: (moved[:k], c["status"][:k]), w, h, mask,
                                      lambda a, b, s: dict(mask=e["mask_rsc"][:k] & s, uvn1=e["uvn1"][:k]))
        got = _mirror_frame(host_exe, tmp_path, w, h, mask, ids[:k], pts[:k], moved[:k] if k >= 10 else moved[:0], c["status"][:k if k >= 10 else 0],
                            e["mask_rsc"][:k if k >= 10 else 0], e["uvn1"][:k if k >= 10 else 0])
        assert got[0] == want[3] and np.array_equal(got[2], want[0])
        assert got[3].tobytes() == want[1].tobytes() and got[4].tobytes() == want[2].tobytes()
        return got
    full = check(n)
    assert full[1] == 1 and 0 < len(full[2]) < n and not np.isin([503, 505, 506, 507], full[2]).any()
    assert (504 in full[2]) == bool(e["mask"][4]), "(int) x = w - 1 stays when its mask is set"
    few = check(9)
    assert not few[0] and few[1] == 0 and len(few[2]) == 0, "fewer than ten points: all zeros, no KLT, no reset"
    none = check(0)
    assert none[0] and none[1] == 0, "no points: the reset of :520-530"
    ten = check(10)
    assert ten[1] == 1 and not ten[0]
