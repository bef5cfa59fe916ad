"""Deterministic images for the tests of the intake options (CLAHE, downsample_cameras): the smallest shapes at which the kernels
can go wrong, each with the content and the clip limit that reaches a branch.  CASES: {id: dict(img, levels, tiles (x, y), clip)}.

Shapes: 64 x 48 divides by 8 x 8; 47 x 31 divides on neither axis; 64 x 31 and 47 x 32 divide on one axis, so the other grows by a
whole tile count; 8 x 8 has tiles of one pixel (area 1: lut_scale 255, the clip limit's floor of 1), 9 x 8 extends to 16 x 16 (tiles
of 2 x 2: the extension is as large as the image and wraps it); 16 x 16 under 16 x 16 tiles and 15 x 17 under one tile are the two
ends of the tile count; one 752 x 480.  Contents: constant (every bin but one is cut and the residual is non-zero), two-valued, a
ramp, uniform noise (nothing is cut at clip 40), the texture of klt_cases, rows 64 bytes apart.  Clip limits: 0 (no clipping), 10,
0.01 (the floor), 40, and 42.7 on a constant 64 x 48 image under one tile, whose excess 3072 - 512 is 10 x 256 exactly."""
import functools

import numpy as np

import clahe_ref
import klt_cases


def _texture(width, height, seed):
    return klt_cases.render(klt_cases.texture(width, height, seed), width, height)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(29)
    noise = lambda w, h: rng.integers(0, 256, size=(h, w)).astype(np.uint8)  # noqa: E731
    two = lambda w, h: np.where(rng.random((h, w)) < 0.4, 30, 180).astype(np.uint8)  # noqa: E731
    ramp = lambda w, h: ((np.arange(w)[None, :] * 3 + np.arange(h)[:, None] * 5) % 256).astype(np.uint8)  # noqa: E731
    const = lambda w, h, v=91: np.full((h, w), v, dtype=np.uint8)  # noqa: E731
    t64, t47 = klt_cases.scene("subpixel_64x48").img0, klt_cases.scene("rot2_47x31").img0
    wide = noise(64, 31)
    wide[:, 3:50] = t47 // 2 + 40   # (a low-contrast texture, rows 64 bytes apart)
    c = {
        # 64 x 48: divisible, tiles of 8 x 6
        "64x48_texture_clip10": dict(img=t64, levels=3, tiles=(8, 8), clip=10.0),
        "64x48_const_clip10": dict(img=const(64, 48), levels=3, tiles=(8, 8), clip=10.0),
        "64x48_two_clip0": dict(img=two(64, 48), levels=3, tiles=(8, 8), clip=0.0),
        "64x48_noise_clip40": dict(img=noise(64, 48), levels=3, tiles=(8, 8), clip=40.0),
        "64x48_two_t2x2_clip0.01": dict(img=two(64, 48), levels=3, tiles=(2, 2), clip=0.01),
        "64x48_const_t1x1_clip42.7": dict(img=const(64, 48, 200), levels=3, tiles=(1, 1), clip=42.7),
        "64x48_ramp_t4x4_clip10": dict(img=ramp(64, 48), levels=3, tiles=(4, 4), clip=10.0),
        # 47 x 31: neither axis divisible
        "47x31_texture_clip10": dict(img=t47, levels=3, tiles=(8, 8), clip=10.0),
        "47x31_strided_t4x2_clip10": dict(img=wide[:, 3:50], levels=3, tiles=(4, 2), clip=10.0),
        "47x31_ramp_t3x5_clip40": dict(img=ramp(47, 31), levels=3, tiles=(3, 5), clip=40.0),
        "47x31_two_clip0": dict(img=two(47, 31), levels=3, tiles=(8, 8), clip=0.0),
        # one axis divisible: the other axis' whole extra tile count
        "64x31_texture_clip10": dict(img=np.ascontiguousarray(t64[:31]), levels=3, tiles=(8, 8), clip=10.0),
        "64x31_two_t4x4_clip0": dict(img=two(64, 31), levels=3, tiles=(4, 4), clip=0.0),
        "47x32_noise_t4x4_clip40": dict(img=noise(47, 32), levels=3, tiles=(4, 4), clip=40.0),
        # tile areas 1 and 4, the two ends of the tile count
        "8x8_noise_clip10": dict(img=noise(8, 8), levels=3, tiles=(8, 8), clip=10.0),
        "8x8_const_clip0": dict(img=const(8, 8), levels=3, tiles=(8, 8), clip=0.0),
        "9x8_ramp_clip10": dict(img=(ramp(9, 8).astype(np.int64) * 7 % 256).astype(np.uint8), levels=3, tiles=(8, 8), clip=10.0),
        "16x16_t16x16_noise_clip10": dict(img=noise(16, 16), levels=3, tiles=(16, 16), clip=10.0),
        "15x17_t1x1_texture_clip0": dict(img=np.ascontiguousarray(t47[:17, :15]), levels=3, tiles=(1, 1), clip=0.0),
        "15x17_t1x1_noise_clip10": dict(img=noise(15, 17), levels=1, tiles=(1, 1), clip=10.0),
        # the size the tracker runs at
        "752x480_texture_clip10": dict(img=klt_cases.scene("trans12_752x480").img0, levels=6, tiles=(8, 8), clip=10.0),
    }
    for v in c.values():
        v["img"].setflags(write=False)
    return c


IDS = ["64x48_texture_clip10", "64x48_const_clip10", "64x48_two_clip0", "64x48_noise_clip40", "64x48_two_t2x2_clip0.01",
       "64x48_const_t1x1_clip42.7", "64x48_ramp_t4x4_clip10", "47x31_texture_clip10", "47x31_strided_t4x2_clip10", "47x31_ramp_t3x5_clip40",
       "47x31_two_clip0", "64x31_texture_clip10", "64x31_two_t4x4_clip0", "47x32_noise_t4x4_clip40", "8x8_noise_clip10", "8x8_const_clip0",
       "9x8_ramp_clip10", "16x16_t16x16_noise_clip10", "15x17_t1x1_texture_clip0", "15x17_t1x1_noise_clip10", "752x480_texture_clip10"]
SMALL = IDS[:-1]


@functools.lru_cache(maxsize=None)
def reference(cid, mutant=None):
    """(pyramid, LUT table) of the restatement - or of one of its mutants - on a case, computed once and shared (do not write
    into it)"""
    c = cases()[cid]
    conv = clahe_ref.CONV if mutant is None else clahe_ref.mutant(mutant)
    pyr, lut = clahe_ref.intake(np.ascontiguousarray(c["img"]), c["levels"], "CLAHE", False, c["tiles"][0], c["tiles"][1], c["clip"], conv)
    for a in pyr + [lut]:
        a.setflags(write=False)
    return pyr, lut


@functools.lru_cache(maxsize=None)
def halving_cases():
    """{id: image} for the halving: an even and an odd size as image and as 0 / 255 mask, and 3 x 2, which halves to 1 x 1"""
    rng = np.random.default_rng(31)
    out = {}
    for w, h in ((94, 62), (95, 63)):
        out["%dx%d_texture" % (w, h)] = _texture(w, h, 41)
        m = np.zeros((h, w), dtype=np.uint8)
        m[11:40, 30:61] = 255
        m[h - 1, :] = 255
        m[:, w - 1] = 255
        out["%dx%d_mask" % (w, h)] = m
    out["3x2_noise"] = rng.integers(0, 256, size=(2, 3)).astype(np.uint8)
    for v in out.values():
        v.setflags(write=False)
    return out


def same(a, b):
    """bit-equal, shape included: what the GPU test asserts of every array"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def sequence():
    """the three frames, the mask and the pyramid depth of klt_cases.sequence() with detector options for step(detect=True), and
    the same scene at twice the size (192 x 128, mask doubled) for the run with downsampling"""
    q = klt_cases.sequence()
    width, height = 2 * q["width"], 2 * q["height"]
    sample = klt_cases.texture(width, height, 21, cell=10.0)
    big = [klt_cases.render(sample, width, height, klt_cases.homography(width, height, t=(k * 0.1852, 0.0, 0.0)) if k else None) for k in range(3)]
    return dict(frames=np.stack(q["frames"]), mask=q["mask"], levels=q["levels"], width=q["width"], height=q["height"],
                big_frames=np.stack(big), big_mask=np.kron(q["mask"], np.ones((2, 2), dtype=np.uint8)),
                detector=dict(num_features=40, grid_x=4, grid_y=3, threshold=15, min_px_dist=5))
