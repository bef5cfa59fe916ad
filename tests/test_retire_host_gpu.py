"""StateOptions::gpu_batched_retire through hostlib: the marg / merge harness entry and a closed-loop session with the option on
and off on the same inputs.  Ids, erased maps and decisions equal; state at 1e-9, covariance at 1e-9 normalised
(max |dP_ij| / sqrt(P_ii P_jj)); marginalize_slam alone only copies, so there every bit is equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hostlib(hiplib):
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib

    return hostlib


def _scene():
    """Plane 2 is a re-detection of plane 1 that passes its gate: its error is 0.9 x plane 1's plus a part of its own, so the merge
    corrects the survivor and its covariance (an exact copy of plane 1 would leave both as they are)."""
    from ov_plane_amd.synth import make_slam_scene

    sc = make_slam_scene(C=6, n_slam=5, seed=8, n_planes=4)
    i1, i2 = int(sc.plane_state_id[0]), int(sc.plane_state_id[1])
    P = sc.P.copy()
    P[i2:i2 + 3, :] = 0.9 * P[i1:i1 + 3, :]
    P[:, i2:i2 + 3] = 0.9 * P[:, i1:i1 + 3]
    P[i2:i2 + 3, i2:i2 + 3] = 0.81 * P[i1:i1 + 3, i1:i1 + 3] + 1e-5 * np.eye(3)
    sc["P"] = P
    sc.cp[1] = sc.cp[0] + np.array([4e-4, -3e-4, 2e-4])
    return sc


def _same_maps(a, b):
    assert a["n"] == b["n"]
    for k in ("plane_id", "slam_id", "slam_to_plane"):
        assert np.array_equal(a[k], b[k]), k


def test_marg_and_merge_with_the_option_on_and_off(hostlib):
    sc = _scene()
    should_marg = np.array([0, 1, 0, 1, 0], dtype=np.uint8)
    # landmarks flagged; plane 2 -> 1 merges, plane 3 takes the id 9, plane 4 has no observer left
    args = (sc, should_marg, [(2, 1), (3, 9)], [1, 9])
    off = hostlib.run_state_maintenance(*args)
    on = hostlib.run_state_maintenance(*args, batched_retire=True)
    _same_maps(on, off)
    assert on["n"] == sc.N - 6 - 6
    live = off["plane_id"] >= 0
    assert live.tolist() == [True, False, False, False] + [False] * 4 + [True] + [False] * 3
    e_cp = float(np.abs(on["plane_cp"][live] - off["plane_cp"][live]).max())
    d = np.sqrt(np.abs(np.diag(off["P"])))
    e_P = float((np.abs(on["P"] - off["P"]) / np.outer(d, d)).max())
    moved = float(np.abs(off["plane_cp"][0] - sc.cp[0]).max())
    print("merged plane moved by %.2e; on vs off: |d cp| %.2e, normalised |dP| %.2e" % (moved, e_cp, e_P))
    assert moved > 1e-5          # the merge was accepted in both arms: the survivor was corrected
    assert e_cp < 1e-9 and e_P < 1e-9
    # a rejected merge (the angle gate closed): the same maps, and nothing but copies - every bit equal
    off = hostlib.run_state_maintenance(*args, plane_merge_deg_max=0.0)
    on = hostlib.run_state_maintenance(*args, plane_merge_deg_max=0.0, batched_retire=True)
    _same_maps(on, off)
    assert np.array_equal(on["P"], off["P"]) and np.array_equal(on["plane_cp"], off["plane_cp"])
    assert np.array_equal(off["plane_cp"][0], sc.cp[0])


def test_marginalize_slam_alone_is_bit_equal(hostlib):
    sc = _scene()
    for flags in ([0, 1, 0, 1, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 1], [0, 0, 0, 0, 0]):
        args = (sc, np.array(flags, dtype=np.uint8), [], [1, 2, 3, 4])
        off = hostlib.run_state_maintenance(*args)
        on = hostlib.run_state_maintenance(*args, batched_retire=True)
        _same_maps(on, off)
        assert on["n"] == sc.N - 3 * sum(flags)
        assert np.array_equal(on["P"], off["P"]) and np.array_equal(on["plane_cp"], off["plane_cp"])


def test_closed_loop_session_with_the_option_on_and_off(hostlib):
    """40 frames of the session tests' scene with planes in the state (planes = 2) and 300 planar points, so that each half of a split
    plane has enough features to be initialised.  The detector puts no plane into the state on this scene within 40 frames, so the
    merges come from the tracker side instead: until frame 24 every plane is reported under two ids
    (run_session's split_planes_until), the state holds two variables per physical plane, and at frame 24 the tracker fuses them -
    accepted merges of re-detections, the case the detector produces as tracks grow.  From frame 32 on no plane is reported, so
    every plane left is retired.  With the option on and off: the same landmark ids and the same plane ids behind every frame,
    positions within 1e-6."""
    from ov_plane_amd import closed_loop
    from ov_plane_amd.sim import Simulator, synthetic_trajectory

    def run(**kw):
        sim = Simulator(synthetic_trajectory(duration=20.0), num_pts=60, num_pts_plane=300)
        return closed_loop.run_session(sim, n_frames=40, C=8, planes=2, max_slam=10, split_planes_until=24, forget_planes_at=32, **kw)

    off, on = run(), run(batched_retire=True)
    S = closed_loop.PLANE_SPLIT
    ids = off["plane_ids_per_frame"]
    print("plane ids per frame", ids)
    print("landmarks retired per frame", off["counts"][:, 3].tolist())
    # the scene does what the test is about: both ids of at least one plane are in the state before the merge frame, the merge
    # removes every second id and keeps its survivor, the planes leave at the end, and landmarks are retired along the way
    fused = [p for p in ids[23] if p < S and p + S in ids[23]]
    assert fused, ids[23]
    assert all(p < S for p in ids[24]) and all(p in ids[24] for p in fused)
    assert ids[31] and not ids[32] and not ids[39]
    assert off["counts"][:, 3].sum() > 0
    assert on["plane_ids_per_frame"] == ids
    assert on["slam_ids_per_frame"] == off["slam_ids_per_frame"]
    assert np.array_equal(on["counts"], off["counts"])
    e = float(np.abs(on["traj"][:, 4:7] - off["traj"][:, 4:7]).max())
    print("max position difference %.2e" % e)
    assert e < 1e-6
