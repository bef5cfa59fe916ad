"""CPU tests of the intake options' yardstick (tests/clahe_ref.py, tests/clahe_cases.py) and of the library's boundary: the
restatement against closed forms, the branches the cases reach, the mutants of the restatement - one convention changed at a time -
that the GPU comparison must catch, the new symbols, the options struct and its defaults, the null-context refusals."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clahe_cases  # noqa: E402
import clahe_ref  # noqa: E402
import klt_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_header_declares_and_library_exports_the_entries(hiplib):
    hdr = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    assert "int ovp_klt_feed_image_opts(ovp_ctx *ctx, const uint8_t *img, int stride, const ovp_klt_intake *intake);" in hdr
    assert "void ovp_klt_intake_defaults(ovp_klt_intake *o);" in hdr
    assert "int ovp_klt_halve(ovp_ctx *ctx, const uint8_t *src, int stride, int src_width, int src_height, uint8_t *dst);" in hdr
    assert "parameters needed: use ovp_klt_feed_image_opts" in hdr and "not built: OVP_E_ARG" not in hdr
    L = hiplib.lib()
    for s in ("ovp_klt_intake_defaults", "ovp_klt_feed_image_opts", "ovp_klt_halve"):
        assert s in hiplib.EXPORTS and hasattr(L, s)
    # the struct: every field of the header, in its order, at the offset a C compiler gives it
    body = re.search(r"typedef struct ovp_klt_intake \{(.*?)\} ovp_klt_intake;", hdr, re.S).group(1)
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        d = decl.strip()
        if d:
            fields += [f.strip() for f in d.split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in hiplib.Intake._fields_], (fields, hiplib.Intake._fields_)
    assert ctypes.sizeof(hiplib.Intake) == 40
    assert [getattr(hiplib.Intake, f).offset for f in fields] == [0, 8, 16, 20, 24, 28, 32]
    o = hiplib.Intake()
    o.src_width = 7
    L.ovp_klt_intake_defaults(ctypes.byref(o))
    assert (o.hist_method, o.clahe_clip, o.clahe_tiles_x, o.clahe_tiles_y, o.downsample, o.src_width, o.src_height) == (1, 10.0, 8, 8, 0, 0, 0)
    L.ovp_klt_intake_defaults(None)   # (a null pointer is ignored)
    d = hiplib.intake_defaults(hist_method="CLAHE", downsample=1, clahe_clip=4.0)
    assert (d.hist_method, d.downsample, d.clahe_clip, d.clahe_tiles_x) == (2, 1, 4.0, 8)
    with pytest.raises(KeyError):
        hiplib.intake_defaults(tiles=3)
    # OVP_E_ARG on a null context, whatever else is handed over
    img, out = np.zeros((4, 4), dtype=np.uint8), np.zeros((2, 2), dtype=np.uint8)
    assert L.ovp_klt_feed_image_opts(None, img.ctypes.data, 4, ctypes.byref(o)) == -1
    assert L.ovp_klt_feed_image_opts(None, None, 4, None) == -1
    assert L.ovp_klt_halve(None, img.ctypes.data, 4, 4, 4, out.ctypes.data) == -1 and not out.any()


def test_mirror_compiles_and_the_harness_exports_the_sequence_entry():
    from ov_plane_amd.build import build_host

    L = ctypes.CDLL(build_host())
    for s in ("ovph_run_klt_intake_sequence", "ovph_run_klt_detect_sequence", "ovph_run_klt_sequence", "ovph_run_klt_epipolar_sequence"):
        assert hasattr(L, s)
    hdr = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "host", "ov_plane_trackplane.h")).read()
    assert "enum HistogramMethod { NONE, HISTOGRAM, CLAHE };" in hdr and "int set_intake(HistogramMethod method, bool downsample" in hdr


def _constant_value(v, area, clip):
    """what a constant tile of value v maps v to, written out from the issue's text: the one full bin is cut to clip, the excess
    goes batch-wise to every bin and one each to bins 0, step, 2 step, ..; the cumulative sum at v, scaled and rounded"""
    if clip <= 0 or clip >= area:
        cum = area
    else:
        excess = area - clip
        batch, residual = divmod(excess, 256)
        cum = clip + batch * (v + 1)
        if residual:
            step = max(256 // residual, 1)
            cum += min(residual, v // step + 1)
    return int(min(255.0, float(np.rint(F(cum) * (F(255.0) / F(area))))))


@pytest.mark.parametrize("v", [0, 91, 200, 255])
@pytest.mark.parametrize("shape,tiles,clip", [((64, 48), (8, 8), 10.0), ((64, 48), (8, 8), 0.0), ((64, 48), (1, 1), 42.7), ((47, 31), (4, 2), 10.0),
                                              ((752, 480), (8, 8), 10.0), ((752, 480), (8, 8), 12.0), ((9, 8), (8, 8), 0.01)])
def test_constant_image_maps_to_a_stated_constant(v, shape, tiles, clip):
    w, h = shape
    g = clahe_ref.geometry(w, h, tiles[0], tiles[1], clip)
    out, lut = clahe_ref.clahe(np.full((h, w), v, dtype=np.uint8), tiles[0], tiles[1], clip)
    want = _constant_value(v, g["area"], g["clip"])
    assert (lut[:, :, v] == want).all() and (out == want).all(), (want, np.unique(out))
    if clip == 0.0:
        assert want == 255   # without clipping the whole tile lies at or below v


def test_geometry_by_hand():
    G = lambda *a: clahe_ref.geometry(*a)  # noqa: E731
    g = G(64, 48, 8, 8, 10.0)
    assert (g["ext_w"], g["ext_h"], g["tile_w"], g["tile_h"], g["clip"]) == (64, 48, 8, 6, 1)        # 10 * 48 / 256 = 1.875
    g = G(47, 31, 8, 8, 10.0)
    assert (g["ext_w"], g["ext_h"], g["tile_w"], g["tile_h"], g["clip"]) == (48, 32, 6, 4, 1)        # 0.9375 -> 0 -> the floor
    g = G(64, 31, 8, 8, 10.0)
    assert (g["ext_w"], g["ext_h"], g["tile_w"], g["tile_h"]) == (72, 32, 9, 4)                       # the divisible axis grows by 8
    g = G(9, 8, 8, 8, 10.0)
    assert (g["ext_w"], g["ext_h"], g["tile_w"], g["tile_h"], g["area"]) == (16, 16, 2, 2, 4)
    g = G(8, 8, 8, 8, 0.01)
    assert (g["area"], g["clip"]) == (1, 1) and g["lut_scale"] == F(255.0)
    g = G(752, 480, 8, 8, 10.0)
    assert (g["tile_w"], g["tile_h"], g["clip"]) == (94, 60, 220)                                     # 10 * 5640 / 256 = 220.3
    assert G(752, 480, 8, 8, 12.0)["clip"] == 264 and (5640 - 264) % 256 == 0
    assert G(64, 48, 1, 1, 42.7)["clip"] == 512 and (3072 - 512) % 256 == 0
    assert G(47, 31, 4, 2, 10.0)["clip"] == 7                                                        # 7.5 truncated
    assert G(64, 48, 8, 8, 0.0)["clip"] == 0 and G(64, 48, 8, 8, 1e300)["clip"] == 48


def test_one_tile_without_clipping_is_equalize_hist_up_to_the_two_lut_formulas():
    """tiles 1 x 1, clip 0: both maps are the cumulative histogram scaled and rounded half to even;
    CLAHE: lut[i] = rint(cum[i] * (255 / N)), cum from bin 0; equalizeHist: lut[i] = rint((cum[i] - hist[first]) * (255 / (N - hist[first])))
    behind the first non-empty bin and 0 up to it"""
    for cid in ("15x17_t1x1_texture_clip0",):
        img = clahe_cases.cases()[cid]["img"]
        hist = np.bincount(img.reshape(-1), minlength=256)
        cum, n = np.cumsum(hist), img.size
        first = int(np.nonzero(hist)[0][0])
        lut_clahe = np.minimum(255, np.rint(cum.astype(F) * (F(255.0) / F(n)))).astype(np.uint8)
        lut_eq = np.minimum(255, np.rint((cum - hist[first]).astype(F) * (F(255.0) / F(n - hist[first])))).astype(np.uint8)
        out, lut = clahe_ref.clahe(img, 1, 1, 0.0)
        assert np.array_equal(lut[0, 0], lut_clahe) and np.array_equal(out, lut_clahe[img])
        assert np.array_equal(klt_ref.equalize_hist(img), lut_eq[img])
        assert not np.array_equal(lut_clahe[img], lut_eq[img]) and np.abs(lut_clahe[img].astype(int) - lut_eq[img]).max() <= 255 * hist[first] // n + 1


def test_weights_sum_to_one_and_indices_stay_in_the_table():
    for n, tile, tiles in ((64, 8, 8), (47, 6, 8), (64, 9, 8), (9, 2, 8), (8, 1, 8), (16, 1, 16), (15, 15, 1), (752, 94, 8), (480, 60, 8)):
        t1, t2, a, a1 = clahe_ref.axis_weights(n, tile, tiles)
        assert a.dtype == F and a1.dtype == F
        # (a = 1 exactly where the coordinate is a rounding error below an integer: 376 (1 / 94) - 0.5 = -1.5e-8, floor -1)
        assert (a >= 0).all() and (a <= 1).all() and np.abs((a + a1).astype(np.float64) - 1.0).max() <= 2.0 ** -23
        assert t1.min() >= 0 and t2.max() <= tiles - 1 and ((t2 - t1) <= 1).all() and ((t2 - t1) >= 0).all()
        # x (1 / tile) - 0.5 = 0 at x = tile / 2: an even tile has a pixel there, which takes tile 0's LUT alone (to rounding)
        if tile % 2 == 0 and tiles > 1:
            c = tile // 2
            assert min(float(a[c]), 1.0 - float(a[c])) <= 2.0 ** -20 and t2[c] <= 1
    # the four weights of a pixel
    _, _, xa, xa1 = clahe_ref.axis_weights(47, 6, 8)
    _, _, ya, ya1 = clahe_ref.axis_weights(31, 4, 8)
    s = ya1[:, None] * xa1[None, :] + ya1[:, None] * xa[None, :] + ya[:, None] * xa1[None, :] + ya[:, None] * xa[None, :]
    assert np.abs(s.astype(np.float64) - 1.0).max() <= 4 * 2.0 ** -23


def test_output_does_not_depend_on_the_padding_where_the_size_is_divisible():
    for cid in ("64x48_texture_clip10", "64x48_noise_clip40", "64x48_ramp_t4x4_clip10", "8x8_noise_clip10", "16x16_t16x16_noise_clip10"):
        pyr, lut = clahe_cases.reference(cid)
        for m in ("pad_needed_axis_only", "reflect_not_101", "tile_from_unpadded"):
            p2, l2 = clahe_cases.reference(cid, m)
            assert clahe_cases.same(lut, l2) and all(clahe_cases.same(a, b) for a, b in zip(pyr, p2)), (cid, m)


def test_cases_reach_the_branches():
    reach = {}
    for cid in clahe_cases.IDS:
        c = clahe_cases.cases()[cid]
        rep = []
        clahe_ref.lut_table(c["img"], c["tiles"][0], c["tiles"][1], c["clip"], report=rep)
        h, w = c["img"].shape
        g = clahe_ref.geometry(w, h, c["tiles"][0], c["tiles"][1], c["clip"])
        reach[cid] = dict(g=g, rep=rep, floor=c["clip"] > 0 and c["clip"] * g["area"] / 256 < 1)
    assert all(e > 0 and r > 0 for e, r in reach["64x48_const_clip10"]["rep"]), "every tile cut, residual non-zero"
    assert all(e > 0 and e % 256 == 0 and r == 0 for e, r in reach["64x48_const_t1x1_clip42.7"]["rep"]), "excess an exact multiple of 256"
    assert all(e == 0 for e, _ in reach["64x48_noise_clip40"]["rep"]) and reach["64x48_noise_clip40"]["g"]["clip"] > 1, "nothing cut"
    assert not reach["64x48_two_clip0"]["rep"], "no clipping at clip 0"
    assert reach["64x48_two_t2x2_clip0.01"]["floor"] and reach["47x31_texture_clip10"]["floor"] and reach["8x8_noise_clip10"]["floor"]
    assert any(0 < r < 128 for _, r in reach["47x31_strided_t4x2_clip10"]["rep"] + reach["752x480_texture_clip10"]["rep"]), "a stride above 1"
    assert any(r >= 128 for cid in clahe_cases.IDS for _, r in reach[cid]["rep"]), "a stride of 1"
    assert reach["9x8_ramp_clip10"]["g"]["area"] == 4 and reach["8x8_noise_clip10"]["g"]["area"] == 1
    assert reach["64x31_texture_clip10"]["g"]["ext_w"] == 72 and reach["47x32_noise_t4x4_clip40"]["g"]["ext_h"] == 36
    # a blended pixel that lands on a tie, or none: the rounding mutants are then caught by the LUT alone - say which
    print("branches reached: see the assertions; cases: %d" % len(reach))


def _differs(cid, name):
    pyr, lut = clahe_cases.reference(cid)
    p2, l2 = clahe_cases.reference(cid, name)
    return [k for k, (a, b) in dict(lut=(lut, l2), **{"level%d" % i: (a, b) for i, (a, b) in enumerate(zip(pyr, p2))}).items()
            if not clahe_cases.same(a, b)]


def test_every_mutant_differs_on_a_case():
    """what the GPU test compares - the LUT table and every pyramid level of every case, the halved images - told apart from each
    mutant's by at least one small case (so the 752 x 480 case is not what the comparison rests on)"""
    table = {}
    for name in clahe_ref.MUTANTS:
        if name == "halve_to_ceil":
            conv = clahe_ref.mutant(name)
            caught = [k for k, img in clahe_cases.halving_cases().items() if not clahe_cases.same(clahe_ref.halve(img), clahe_ref.halve(img, conv))]
        else:
            caught = ["%s (%s)" % (cid, ", ".join(d)) for cid in clahe_cases.SMALL for d in [_differs(cid, name)] if d]
        table[name] = caught
    for name, caught in table.items():
        print("%-22s differs on %2d: %s" % (name, len(caught), "; ".join(caught[:4]) + (" ..." if len(caught) > 4 else "")))
    for name, caught in table.items():
        assert caught, "the mutant %s equals the restatement on every case" % name


def test_halving_is_the_pyramid_kernel_at_the_floor_size():
    for k, img in clahe_cases.halving_cases().items():
        h, w = img.shape
        got = clahe_ref.halve(img)
        assert got.shape == (h // 2, w // 2)
        assert np.array_equal(got, klt_ref.pyr_down(img)[:h // 2, :w // 2]), k   # the same taps: an odd size drops the last row / column
        if k.endswith("mask"):
            assert set(np.unique(got)) - {0, 255}, "the halved mask has intermediate values at its edges: the keep rule's > 127 decides"
    assert clahe_ref.halve(clahe_cases.halving_cases()["3x2_noise"]).shape == (1, 1)
    pyr, lut = clahe_ref.intake(clahe_cases.halving_cases()["95x63_texture"], 3, "NONE", True)
    assert lut is None and [p.shape for p in pyr] == [(31, 47), (16, 24), (8, 12)]
