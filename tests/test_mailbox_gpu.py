"""The pinned-result handshake on the device (csrc/ovp_mailbox.h, k_publish.hip): what an entry point returns does not depend on
what earlier entry points left in the pinned block it shares with them.  Every call of a sequence on ONE context gives the bits of
the same call on a fresh context (tests/mailbox_calls.py: each call uploads its own inputs)."""
import numpy as np
import pytest

import mailbox_calls as mc

pytestmark = pytest.mark.gpu


def _fresh(capi, call, cache={}):
    """the call on a context of its own, computed once per call"""
    if call not in cache:
        ctx = mc.new_context(capi)
        cache[call] = call(capi, ctx)
        ctx.close()
    return cache[call]


def _same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k)


def test_a_sequence_on_one_context_gives_the_bits_of_fresh_contexts(hiplib):
    """plane loop with 2 planes, SLAM update, plane loop with 1 plane (the loop's flags move inside the block), dense update,
    propagation, the staged point update, delayed initialisation: the plane block's one channel and the point block's two."""
    seq = (mc.plane_loop, mc.slam_update, mc.plane_loop_one, mc.ekf_update, mc.cov_propagate, mc.point_update_async,
           mc.slam_delayed_init)
    ctx = mc.new_context(hiplib)
    got = [call(hiplib, ctx) for call in seq]
    ctx.close()
    for call, g in zip(seq, got):
        _same(g, _fresh(hiplib, call), call.__name__)


def test_growth_of_the_plane_result_block_between_calls(hiplib):
    """A one-plane loop sizes the block; a delayed initialisation of four candidates is the smallest call of this module that does
    not fit it (8 (12 + n_max) bytes per candidate, three candidates still fit the loop's 4096 bytes of slack); then a small call
    on the grown block."""
    seq = (mc.plane_loop_one, mc.slam_delayed_init_four, mc.ekf_update)
    ctx = mc.new_context(hiplib)
    cap = lambda: int(ctx.debug_read("pl_hres_cap", (1,), dtype=np.uint64)[0])
    got, caps = [], []
    for call in seq:
        got.append(call(hiplib, ctx))
        caps.append(cap())
    ctx.close()
    print("pl_hres_cap behind each call:", caps)
    assert 3 * 8 * (12 + mc.N_MAX) + 64 <= caps[0] < 4 * 8 * (12 + mc.N_MAX) + 64  # three candidates would have fitted
    assert caps[1] > caps[0] and caps[2] == caps[1]
    for call, g in zip(seq, got):
        _same(g, _fresh(hiplib, call), call.__name__)


def test_detector_frames_of_different_sizes(hiplib):
    """Frames of 12, 40 and 12 points on one detector, whose block a 300-point filter call has filled before: each frame bit for
    bit what a detector on a fresh context gives for it behind the same history."""
    history, frames = mc.detector_frames()
    assert [len(f[0]) for f in frames] == [12, 40, 12]

    def start(fill):
        ctx = hiplib.Context(64, 4, 8)
        det = hiplib.PlaneDetector(ctx)
        if fill:
            rng = np.random.default_rng(1)
            det.spatial_filter([rng.uniform(0, 4, (300, 3))], 4, 1.2)
        for fr in history:
            det.feed(*fr)
        return ctx, det

    ctx, det = start(True)
    got = [mc.detector_frame(det, fr) for fr in frames]
    det.close()
    ctx.close()
    assert all(g["has"].sum() == 12 and len(g["map"]) >= 6 and len(g["filter"]) >= 8 for g in got)
    for k in range(len(frames)):
        ctx, det = start(False)
        for fr in frames[:k]:
            det.feed(*fr)
        want = mc.detector_frame(det, frames[k])
        det.close()
        ctx.close()
        _same(got[k], want, "frame %d" % k)
