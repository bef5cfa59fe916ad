"""CPU tests of the detection stage's yardstick (tests/fast_ref.py, tests/fast_cases.py) and of the library's boundary: the new
symbols, the branches the cases meet, the mutants of the restatement - one convention changed at a time - that the GPU test's
comparison must catch, the figures fast_cases.py records for the GPU test, and the host logic of the C++ mirror
(tests/fast_host_main.cpp, under the address and undefined-behaviour sanitizers) against the restatement.

Refinement branches: a FAST corner has gradients of two directions in its window, so no detected candidate is singular at its
integer start, and none of the small cases' candidates walks out of the image.  Those two branches are met on probe points
(fast_cases.probes), which the GPU test refines through the debug entry "refine"; the mutant "eps not squared" is caught by a
probe alone (test_mutant_differs_on_a_case says why)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fast_cases  # noqa: E402
import fast_ref  # noqa: E402
import klt_cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_detector(hiplib):
    hdr = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    assert "int ovp_klt_detect(ovp_ctx *ctx, int half, int num_features, int grid_x, int grid_y, int threshold" in hdr
    assert "OVP_FAST_MAX_K" in hdr and "OVP_FAST_MAX_CELLS" in hdr and "RECALLED" in hdr
    L = hiplib.lib()
    assert "ovp_klt_detect" in hiplib.EXPORTS and hasattr(L, "ovp_klt_detect")
    n = np.zeros(1, dtype=np.int32)
    assert L.ovp_klt_detect(None, 0, 10, 2, 2, 15, n.ctypes.data, None, None, None, None, 0) == -1  # OVP_E_ARG on a null context


def test_mirror_compiles_and_the_harness_exports_the_sequence_entry():
    from ov_plane_amd.build import build_host
    import ctypes

    L = ctypes.CDLL(build_host())
    assert hasattr(L, "ovph_run_klt_detect_sequence")
    hdr = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "host", "ov_plane_trackplane.h")).read()
    assert "perform_detection_monocular(int half" in hdr and "bool detect = false" in hdr


BRANCHES = ["bright_arc", "dark_arc", "wrapped_arc", "exactly_8", "diff_equals_t", "equal_neighbours_suppressed", "corner_next_to_border",
            "stronger_neighbour_in_next_cell", "tie_at_kth", "cell_smaller_than_7", "cell_exactly_7x7", "ct_cols_above_grid_x",
            "corner_in_leftover_strip", "regrid"]
# the drawn image's own patterns meet the forced branches (the textures meet most of them as well)
DRAWN_MEETS = ["bright_arc", "dark_arc", "wrapped_arc", "exactly_8", "diff_equals_t", "equal_neighbours_suppressed", "corner_next_to_border",
               "tie_at_kth"]


def test_branch_table():
    met = {}
    for cid in fast_cases.SMALL:
        for k, v in fast_cases.reference(cid)["report"].items():
            if v:
                met.setdefault(k, []).append(cid)
    for b in BRANCHES:
        print("%-34s %s" % (b, met.get(b, [])))
        assert met.get(b), "no small case meets the branch %s" % b
    for b in DRAWN_MEETS:
        assert "drawn64x48_g2x2_t15" in met[b], b
    img, mask, nf, gx, gy, th = fast_cases.masked_case()
    d = fast_ref.detect_candidates(img, nf, gx, gy, th, mask=mask)
    assert d["report"]["masked_point_uses_slot"]
    free = fast_cases.reference("drawn64x48_g2x2_t15")
    assert len(d["xy"]) == len(free["xy"]) - 1, "the masked point's slot went to nobody"
    # thresholds: 254 keeps the 0 / 255 corner, 255 nothing
    assert len(fast_cases.reference("strip64x48_g5x3_t254")["xy"]) == 1 and fast_cases.reference("strip64x48_g5x3_t254")["response"][0] == 254
    assert len(fast_cases.reference("strip64x48_g5x3_t255")["xy"]) == 0
    assert len(fast_cases.reference("constant64x48")["xy"]) == 0


def test_refinement_branches():
    met = {k: [] for k in ("converged", "exhausted", "singular", "left_image", "reverted")}
    for cid in fast_cases.REFINED:
        rep = fast_cases.variants(cid)["f32_numpy"][1]
        for k in met:
            if rep[k].any():
                met[k].append(cid)
    on_candidates = {k: list(v) for k, v in met.items()}
    for name, (img, pts) in fast_cases.probes().items():
        rep = fast_ref.corner_subpix(img, np.array(pts, dtype=np.float32))[1]
        for k in met:
            if rep[k].any():
                met[k].append("probe:" + name)
    for k, v in met.items():
        print("%-12s %s" % (k, v))
        assert v, "no case or probe meets the refinement branch %s" % k
    for k in ("converged", "exhausted", "reverted"):
        assert on_candidates[k], "no candidate list meets %s" % k


def _fields(img, mask, nf, gx, gy, th, conv):
    """everything the GPU comparison checks of a run: the two maps, the candidate list, the refined positions, and the points the
    host logic returns under a mask"""
    try:
        d = fast_ref.detect_candidates(img, nf, gx, gy, th, conv)
    except ValueError:
        return ("refused",)
    opts = dict(num_features=nf, grid_x=gx, grid_y=gy, threshold=th, min_px_dist=5)
    p, i, _ = fast_ref.detect_on_image(img, mask, np.zeros((0, 2), np.float32), np.zeros(0, np.int64), opts, 0, conv)
    return (d["score"].tobytes(), d["nms"].tobytes(), d["xy"].tobytes(), d["response"].tobytes(), d["cell"].tobytes(),
            np.round(d["refined"].astype(np.float64), 4).tobytes(), np.round(p.astype(np.float64), 4).tobytes(), i.tobytes())


@pytest.mark.parametrize("name", list(fast_ref.MUTANTS))
def test_mutant_differs_on_a_case(name):
    """a case is one of the small cases (all the fields the GPU test compares, the host logic under a mask included) or a probe of
    the refinement, which the GPU test refines through the debug entry "refine".  eps_not_squared is caught by the probe tiny_det
    alone: the window of a detected corner has gradients of two directions and of at least one grey level, and a determinant of
    order 1e3; exactly parallel gradients (an edge) give exactly 0, singular under both readings."""
    conv = fast_ref.mutant(name)
    img_m, mask_m, *rest = fast_cases.masked_case()
    runs = [(cid, fast_cases.CASES[cid][0], None) + tuple(fast_cases.CASES[cid][1:]) for cid in fast_cases.SMALL]
    runs.append(("drawn64x48_masked", img_m, mask_m) + tuple(rest))
    caught = []
    for cid, img, mask, nf, gx, gy, th in runs:
        if _fields(img, mask, nf, gx, gy, th, conv) != _fields(img, mask, nf, gx, gy, th, fast_ref.CONV):
            caught.append(cid)
    for pname, (img, pts) in fast_cases.probes().items():  # (the GPU test refines the probes through the debug entry)
        xy = np.array(pts, dtype=np.float32)
        if not np.array_equal(np.round(fast_ref.corner_subpix(img, xy, conv)[0], 4), np.round(fast_ref.corner_subpix(img, xy)[0], 4)):
            caught.append("probe:" + pname)
    print("%s: differs on %s" % (name, caught))
    assert caught, "the mutant %s equals the restatement on every case" % name


@pytest.mark.parametrize("cid", fast_cases.REFINED)
def test_recorded_spread_and_near_decision_cap(cid):
    sp = fast_cases.measure_spread(cid)
    ns, other = fast_cases.near_decision(cid, fast_cases.spread_px(cid))
    sure = ~ns & ~other
    worst = float(sp[sure].max()) if sure.any() else 0.0
    rec = fast_cases.SPREAD_PX[cid]
    cap = klt_cases.near_cap(len(sp))
    print("%s: %d points, spread %.4e px (recorded %.4e, floor %.3e), %d near the stop threshold, %d left out (cap %d)" % (
        cid, len(sp), worst, rec, fast_cases.spread_floor_px(cid), ns.sum(), other.sum(), cap))
    assert worst <= rec * (1 + 1e-3) and rec * 0.95 <= worst
    assert ns.sum() + other.sum() <= cap
    # every variant passes the comparison the device is held to
    for k, (pts, _) in fast_cases.variants(cid).items():
        assert not fast_cases.compare_refined(cid, pts)["failures"], k


# ---- the host logic of the C++ mirror against the restatement, without a device -------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fast_host") / "fast_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "ov_plane_amd", "csrc", "host"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "fast_host_main.cpp"), "-o", exe])
    return exe


def _bits(v):
    return "%08x" % int(np.float32(v).view(np.uint32))


def _run_host(exe, tmp_path, cols, rows, opts, mask, pts, ids, cand_xy, cand_ref, currid):
    lines = ["%d %d %d %d %d %d %d %d" % (cols, rows, opts["num_features"], opts["grid_x"], opts["grid_y"], opts["min_px_dist"], currid,
                                          0 if mask is None else 1)]
    if mask is not None:
        lines.append(" ".join(str(int(v)) for v in np.asarray(mask).ravel()))
    lines.append(str(len(ids)))
    lines += ["%d %s %s" % (i, _bits(p[0]), _bits(p[1])) for p, i in zip(pts, ids)]
    lines.append(str(len(cand_xy)))
    lines += ["%d %d %s %s" % (x, y, _bits(r[0]), _bits(r[1])) for (x, y), r in zip(cand_xy, cand_ref)]
    f = tmp_path / "in.txt"
    f.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(f)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    out = run.stdout.split("\n")
    det, cur, k = (int(v) for v in out[0].split())
    got_ids = np.array([int(l.split()[0]) for l in out[1:1 + k]], dtype=np.int64)
    got = np.array([[int(v, 16) for v in l.split()[1:3]] for l in out[1:1 + k]], dtype=np.uint32).reshape(-1, 2).view(np.float32)
    return det, cur, got_ids, got


def _check_host(exe, tmp_path, cols, rows, opts, mask, pts, ids, cand_xy, cand_ref, currid):
    want_p, want_i, want_cur, want_det = fast_ref.perform_detection(cols, rows, lambda: (cand_xy, cand_ref), mask, pts, ids, opts, currid)
    det, cur, got_i, got_p = _run_host(exe, tmp_path, cols, rows, opts, mask, pts, ids, cand_xy, cand_ref, currid)
    assert det == int(want_det) and cur == want_cur
    assert np.array_equal(got_i, want_i) and got_p.tobytes() == want_p.tobytes()
    return want_p, want_i, want_det


def test_host_logic_of_the_mirror_equals_the_restatement(host_exe, tmp_path):
    hc = fast_cases.host_case()
    img, mask, opts = hc["img"], hc["mask"], hc["opts"]
    rows, cols = img.shape
    d = fast_ref.detect_candidates(img, opts["num_features"], opts["grid_x"], opts["grid_y"], opts["threshold"])
    _, _, _, _, rep = fast_ref.occupancy_walk(cols, rows, hc["pts"], hc["ids"], mask, opts)
    print(rep)
    assert rep["edge"] >= 2 and rep["occupied"] >= 1 and rep["masked"] >= 1 and rep["painted"] >= 1
    # a rectangle that does not fit needs min_px_dist above the 10 px edge: 12
    wide = dict(opts, min_px_dist=12)
    rep = fast_ref.occupancy_walk(cols, rows, hc["pts"], hc["ids"], mask, wide)[4]
    assert rep["painted"] >= 1 and rep["not_painted"] >= 1, rep
    _check_host(host_exe, tmp_path, cols, rows, wide, mask, hc["pts"], hc["ids"], d["xy"], d["refined"], 7)
    p, i, det = _check_host(host_exe, tmp_path, cols, rows, opts, mask, hc["pts"], hc["ids"], d["xy"], d["refined"], 40)
    assert det and i.max() > 40 and list(i[i > 40]) == list(range(41, 41 + (i > 40).sum())), "ids continue at ++currid, in order"
    # no mask, no points: the first id is 1
    p, i, det = _check_host(host_exe, tmp_path, cols, rows, opts, None, np.zeros((0, 2), np.float32), np.zeros(0, np.int64), d["xy"], d["refined"], 0)
    assert det and len(i) and i[0] == 1
    # the 10 px edge: x = 9 goes, x = 10 stays; x = cols - 11 stays, cols - 10 goes
    e = np.array([[9.9, 24.0], [10.0, 24.0], [cols - 11 + 0.9, 30.0], [cols - 10, 30.0]], dtype=np.float32)
    p, i, det = _check_host(host_exe, tmp_path, cols, rows, opts, None, e, np.array([1, 2, 3, 4]), d["xy"][:0], d["refined"][:0], 4)
    assert list(i) == [2, 3]


def test_five_percent_return_at_exactly_the_boundary(host_exe, tmp_path):
    """num_features = 20: with 19 points kept 1 < 1.0000000000000009 (20 x (1 - 0.95) in double) returns, with 18 kept it detects;
    num_features = 40: 2 missing of 40 is not below 2.0000000000000018 -> returns as well, 3 missing detects"""
    cols, rows = 200, 120
    xs, ys = np.meshgrid(np.arange(15, 190, 12), np.arange(15, 110, 12))
    grid = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32) + np.float32(0.25)
    cand_xy = np.array([[100, 60]], dtype=np.int32)
    cand_ref = np.array([[100.4, 60.2]], dtype=np.float32)
    for nf, kept, want in ((20, 19, False), (20, 18, True), (40, 38, False), (40, 37, True)):
        opts = dict(num_features=nf, grid_x=4, grid_y=3, threshold=15, min_px_dist=5)
        assert fast_ref.enough(kept, nf) == (not want)
        pts = grid[:kept]
        p, i, det = _check_host(host_exe, tmp_path, cols, rows, opts, None, pts, np.arange(1, kept + 1), cand_xy, cand_ref, 100)
        assert det == want and len(i) == kept + (1 if want else 0)
