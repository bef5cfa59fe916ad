"""The feature database on the device (k_featdb.hip through capi.FeatureDatabase) against the restatement (tests/featdb_ref.py) on the
scripted sequences of tests/featdb_cases.py: everything the stage produces is a copy or an integer decision, so every record - the
read-back table, the published class table, the gathered batch, the cleanup table, the refusals - is compared byte for byte."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import featdb_cases  # noqa: E402
import featdb_ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _select_dev(capi):
    return lambda ids, cls, *a: capi.featdb_select(ids, cls, *a)


def _device_records(capi, name):
    S, M = featdb_cases.dims(name)
    ctx = capi.Context(60, 32, 128, device=0)
    db = capi.FeatureDatabase(ctx, S, M)
    try:
        return featdb_cases.run(featdb_cases.case(name)[0], db, _select_dev(capi))
    finally:
        db.close()
        ctx.close()


_DEV = {}


def _dev(capi, name):
    if name not in _DEV:
        _DEV[name] = _device_records(capi, name)
    return _DEV[name]


@pytest.mark.parametrize("name", featdb_cases.IDS)
def test_every_record_equals_the_restatement(hiplib, name):
    got, want = _dev(hiplib, name), featdb_cases.reference(name)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "record %d (%s) of %s differs" % (k, w[0], name)
    if name == "s70_m8":
        assert 65 <= featdb_cases.case(name)[1] <= 70
    assert _device_records(hiplib, name) == got, "two runs give other bytes"


@pytest.mark.parametrize("mut", list(featdb_ref.MUTANTS))
def test_every_mutant_fails_the_device_comparison(hiplib, mut):
    caught = [c for c in featdb_cases.IDS if featdb_cases.reference(c, featdb_ref.mutant(mut)) != _dev(hiplib, c)]
    print("%s: differs from the device on %s" % (mut, caught))
    assert caught


def test_slots_are_reused_and_refusals_leave_the_context_usable(hiplib):
    capi = hiplib
    L = capi.lib()
    ctx = capi.Context(80, 32, 128, device=0)
    one = np.zeros(2, dtype=np.float32)
    i64 = np.array([1], dtype=np.int64)
    # calls before create
    assert L.ovp_featdb_append(ctx.handle, 1.0, 1, i64.ctypes.data, one.ctypes.data, one.ctypes.data) == featdb_ref.E_STATE
    assert L.ovp_featdb_cleanup(ctx.handle, 1, float("nan")) == featdb_ref.E_STATE and L.ovp_featdb_destroy(ctx.handle) == featdb_ref.E_STATE
    assert L.ovp_featdb_create(ctx.handle, 4097, 3) == featdb_ref.E_ARG and L.ovp_featdb_create(ctx.handle, 4, 33) == featdb_ref.E_ARG
    db = capi.FeatureDatabase(ctx, 2, 3)
    assert L.ovp_featdb_create(ctx.handle, 2, 3) == featdb_ref.E_STATE, "create twice"
    uv, uvn = featdb_cases.obs([7, 3], 0)
    db.update_feature(1.0, [7, 3], uv, uvn)
    slots = {i: db.get_feature(i)["slot"] for i in (7, 3)}
    assert sorted(slots.values()) == [0, 1]
    with pytest.raises(capi.OvpError) as e:
        db.update_feature(2.0, [9], uv[:1], uvn[:1])
    assert e.value.code == featdb_ref.E_CAPACITY
    with pytest.raises(capi.OvpError) as e:
        db.update_feature(2.0, [7, 7], uv, uvn)
    assert e.value.code == featdb_ref.E_ARG
    with pytest.raises(capi.OvpError) as e:
        db.gather([7] * 200, [1.0])     # above the context's n_feats_max
    assert e.value.code == featdb_ref.E_CAPACITY
    with pytest.raises(capi.OvpError) as e:
        db.triangulate()                  # nothing gathered
    assert e.value.code == featdb_ref.E_STATE
    db.mark_deleted([7])
    assert db.cleanup(True).tolist() == [[3, 1, 0], [7, 0, 1]]
    db.update_feature(2.0, [9], uv[:1], uvn[:1])
    assert db.get_feature(9)["slot"] == slots[7] and db.get_feature(7) is None and db.get_feature(9)["to_delete"] == 0
    assert db.dims() == [2, 3, 2, -1]
    db.reset()
    assert db.dims()[2] == 0 and db.get_feature(3) is None
    db.close()
    # the context is still good for an update
    from ov_plane_amd.synth import make_scene

    sc = make_scene(C=6, F=20, seed=3)
    ctx.cov_upload(sc.P)
    ctx.state_upload(sc)
    ctx.batch_upload_scene(sc)
    assert ctx.msckf_update(capi.opts_from_scene(sc))["rc"] == 0
    ctx.close()


def _scene_through_the_database(capi, sc, ctx):
    """the scene's measurements fed frame by frame (clone c is frame c), gathered over all clones: the batch the scene holds"""
    S, M = 32, 8
    db = capi.FeatureDatabase(ctx, S, M)
    times = [featdb_cases.T(c) for c in range(sc.C)]
    uvn_host = np.asarray(sc.uv_norm, dtype=np.float32)
    for c in range(sc.C):
        rows = [(f, k) for f in range(sc.F) for k in range(int(sc.n_meas[f])) if int(sc.clone_idx[f, k]) == c]
        ids = [100 + f for f, _ in rows]
        db.update_feature(times[c], ids, np.array([sc.uv[f, k] for f, k in rows], dtype=np.float32).reshape(-1, 2),
                          np.array([uvn_host[f, k] for f, k in rows], dtype=np.float32).reshape(-1, 2))
    return db, times


def _padded(sc, M):
    F = sc.F
    uv, uvn, ci = np.zeros((F, M, 2), dtype=np.float32), np.zeros((F, M, 2), dtype=np.float32), np.full((F, M), -1, dtype=np.int32)
    for f in range(F):
        n = int(sc.n_meas[f])
        order = np.argsort(sc.clone_idx[f, :n], kind="stable")
        uv[f, :n], uvn[f, :n], ci[f, :n] = sc.uv[f, order], np.asarray(sc.uv_norm, dtype=np.float32)[f, order], sc.clone_idx[f, order]
    return uv, uvn, ci


def test_triangulate_and_update_equal_the_uploaded_batch(hiplib):
    """6 clones, 20 features of the synthetic scene generator: ovp_featdb_triangulate against ovp_triangulate (the same batch
    uploaded with ovp_batch_upload, uv_norm from the host), then ovp_msckf_update on the bound batch against the uploaded one -
    p_FinG, ok, dx, the accept mask, chi2 and the covariance bit for bit; then the old_index form carries p_FinG bit for bit"""
    capi = hiplib
    from ov_plane_amd.synth import make_scene

    sc = make_scene(C=6, F=20, seed=5, ragged=True)
    assert "uv_norm" in sc and int(sc.n_meas.max()) <= 8
    M = 8
    uv, uvn, ci = _padded(sc, M)
    o = capi.opts_from_scene(sc)
    out = {}
    for arm in ("host", "device"):
        ctx = capi.Context(sc.N, sc.C, sc.F, device=0)
        ctx.cov_upload(sc.P)
        ctx.state_upload(sc)
        if arm == "host":
            ctx.batch_upload(uv, ci, sc.n_meas, np.zeros((sc.F, 3)))
            tri = ctx.triangulate(uvn)
        else:
            db, times = _scene_through_the_database(capi, sc, ctx)
            db.gather([100 + f for f in range(sc.F)], times)
            g = db.gathered()
            assert g["uv"].tobytes() == uv.tobytes() and g["uv_norm"].tobytes() == uvn.tobytes() and g["clone_idx"].tobytes() == ci.tobytes()
            assert g["n_meas"].tobytes() == np.asarray(sc.n_meas, dtype=np.int32).tobytes() and not g["p_FinG"].any()
            tri = db.triangulate()
            assert db.gathered()["p_FinG"].tobytes() == tri["p_FinG"].tobytes()
            keep = [int(f) for f in np.where(tri["ok"])[0]][::-1]
        upd = ctx.msckf_update(o, raise_on_error=False)
        out[arm] = (tri["p_FinG"].tobytes(), tri["ok"].tobytes(), upd["dx"].tobytes(), upd["accepted"].tobytes(), upd["chi2"].tobytes(),
                    ctx.cov_download().tobytes(), upd["rc"])
        if arm == "device":
            db.gather([100 + f for f in keep], times, old_index=keep)
            assert db.gathered()["p_FinG"].tobytes() == tri["p_FinG"][keep].tobytes(), "p_FinG is carried bit for bit"
            assert db.gathered()["uv"].tobytes() == uv[keep].tobytes()
            db.close()
        ctx.close()
    print("triangulated %d of %d, update rc %d" % (np.frombuffer(out["host"][1], dtype=bool).sum(), sc.F, out["host"][6]))
    assert np.frombuffer(out["host"][1], dtype=bool).sum() >= 10
    for k, what in enumerate(("p_FinG", "ok", "dx", "accepted", "chi2", "P", "rc")):
        assert out["host"][k] == out["device"][k], what


def test_simulated_tracks_through_select(hiplib):
    """20 frames of sim.Simulator's tracks, window 6: select on the device's table against the restatement's, every frame"""
    capi = hiplib
    from ov_plane_amd import sim

    tracks = _sim_tracks(sim, 20)
    W, S, M = 5, 128, 8
    ctx = capi.Context(60, 32, 128, device=0)
    dev, ref = capi.FeatureDatabase(ctx, S, M), featdb_ref.FeatureDatabase(S, M)
    landmarks, n_live, frames_ref = [], [], []
    for k, (t, ids, uv, uvn) in enumerate(tracks):
        times = [tr[0] for tr in tracks[max(0, k - W):k + 1]]
        dev.update_feature(t, ids, uv, uvn), ref.update_feature(t, ids, uv, uvn)
        got = dev.select(times, t, W, landmarks, max_slam_features=4)
        tr = ref.classify(times, t, times[0], W, len(times) > W or len(times) > 5)
        want = featdb_ref.select(tr["ids"], tr["cls"], tr["ids"], landmarks, 4, True)
        for key in ("ids", "cls", "count", "cleaned", "flags", "totals"):
            assert got["table"][key].tobytes() == tr[key].tobytes(), (k, key)
        for key in want:
            assert got[key] == want[key], (k, key)
        n_live.append(len(tr["ids"]))
        not_newer, containing = ref.features_not_containing_newer(t), ref.features_containing(times[0])
        f0 = ref.get_feature(tr["ids"][0])
        first = (f0["count"], f0["to_delete"])
        landmarks = [i for i in landmarks if i not in want["landmarks_marg"]] + want["slam_delayed"]
        chosen = want["lost"] + want["marg"] + want["maxtracks"] + want["slam_delayed"] + want["slam_update"]
        dev.mark_deleted(chosen), ref.mark_deleted(chosen)
        before = times[0] if len(times) > W else float("nan")
        assert dev.cleanup(True, before).tobytes() == ref.cleanup(True, before).tobytes()
        frames_ref.append(dict(want, table=tr, not_newer=not_newer, containing=containing, first=first))
    print("live features per frame:", n_live)
    assert max(n_live) >= 40
    dev.close()
    ctx.close()
    # the C++ mirror (ov_plane::FeatureDatabase) through the same frame loop: tables, lists, the two queries, a read-back
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib

    cpp = hostlib.run_featdb_sequence(tracks, S, M, W, max_slam_features=4)
    assert len(cpp) == len(frames_ref)
    for k, (g, w) in enumerate(zip(cpp, frames_ref)):
        for key in ("ids", "cls", "count", "cleaned", "flags", "totals"):
            assert g["table"][key].tobytes() == w["table"][key].tobytes(), (k, key)
        for key in ("lost", "marg", "maxtracks", "slam_delayed", "slam_update", "landmarks_marg", "not_newer", "containing"):
            assert g[key] == w[key], (k, key)
        assert g["first"] == w["first"], k
    assert any(w["slam_delayed"] for w in frames_ref) and any(w["marg"] for w in frames_ref) and any(w["lost"] for w in frames_ref)


def test_point_update_harness_is_bit_equal_with_gpu_featdb_on():
    """StateOptions::gpu_featdb: the existing point-update harness entry, features arriving untriangulated - every array it returns
    has the bytes it has with the option off"""
    from ov_plane_amd.build import build_host

    build_host()
    from ov_plane_amd import hostlib
    from ov_plane_amd.synth import make_scene

    for kw in (dict(C=6, F=20, seed=5, ragged=True), dict(C=10, F=70, seed=8, ragged=True, n_planes=2, feats_per_plane=10)):
        sc = make_scene(**kw)
        off = hostlib.run_msckf_update(sc, triangulate=True)
        on = hostlib.run_msckf_update(sc, triangulate=True, featdb=True)
        assert off["kept"].sum() >= 10
        for key in off:
            if isinstance(off[key], np.ndarray):
                assert np.asarray(on[key]).tobytes() == off[key].tobytes(), key
        assert on["shard"] == off["shard"]


def _sim_tracks(sim, frames):
    """per camera frame of sim.Simulator (about 60 tracked points): (time, ids, uv, uv_norm)"""
    s = sim.Simulator(sim.synthetic_trajectory(duration=6.0), num_pts=40, num_pts_plane=20)
    out = []
    while len(out) < frames:
        s.get_next_imu()
        cam = s.get_next_cam()
        if cam is None:
            continue
        ids = [int(i) for i, _ in cam[1]]
        uv = np.array([d[:2] for _, d in cam[1]], dtype=np.float32).reshape(-1, 2)
        uvn = ((uv - s.intr[2:4].astype(np.float32)) / s.intr[0:2].astype(np.float32)).astype(np.float32)
        out.append((float(cam[0]), ids, uv, uvn))
    return out
