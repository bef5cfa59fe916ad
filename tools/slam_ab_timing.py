"""The SLAM entries of two builds of libovplane_hip.so in ONE process, in interleaved windows, by the method of
tools/plane_loop_ab_timing.py: this checkout's and the one OVP_LIB_AB names (the build of the commit in front).  For a change of
csrc/ovp_api_slam.hip that must not cost anything.
    OVP_LIB_AB=path/to/parent/libovplane_hip.so python tools/slam_ab_timing.py --out profiles/slam_stages_timing.json

Host clock around the call (covariance and tables uploaded before it, outside the clock), ms; per build the median of `windows`
window means, the two builds interleaved window by window.  The scenes are those of tools/general_slam_timing.py,
tools/dinit_planes_timing.py and the closed loop's frame (tools/session_timing.py: 11 clones, 25 landmarks):
  update / update_general           25 landmarks at C = 11, mono / stereo with two in-state planes
  dinit / dinit_general / dinit_planes   4 mono candidates at C = 11 / 10 stereo candidates at C = 16 / 10 on-plane candidates at C = 11
Condition per figure: this.median <= other.median + (other.max - other.min)."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FIGURES = ("update_ms", "update_general_ms", "dinit_ms", "dinit_general_ms", "dinit_planes_ms")


class Entries:
    """the five calls on contexts of one build"""

    def __init__(self, capi):
        from ov_plane_amd.synth import make_dinit_plane_scene, make_scene, make_slam_scene, make_stereo_scene, make_stereo_slam_scene
        from slam_digest import plane_args

        self.capi = capi
        mono = make_slam_scene(C=11, n_slam=25, seed=6)
        st = make_stereo_slam_scene(C=11, n_slam=25, seed=11, n_planes=2, stereo_frac=1.0)
        cand = make_scene(C=11, F=4, seed=8, ragged=True, chi2_mult=0.6)
        gcand = make_stereo_scene(C=16, F=10, seed=3, stereo_frac=0.8, chi2_mult=1.0)
        pcand = make_dinit_plane_scene(C=11, F=10, n_planes=3, wrong_plane=0, outliers=0, seed=2, chi2_mult=2.0)
        sid, cp, cpf = plane_args(st)
        self.calls = {
            "update_ms": (mono, False, lambda c, o, s: c.slam_update(o, s.uv, s.clone_idx, s.n_meas, s.p_FinG, s.p_FinG_fej, s.lm_id)),
            "update_general_ms": (st, True, lambda c, o, s: c.slam_update_general(o, s.uv, s.clone_idx, s.cam_idx, s.n_meas, s.p_FinG,
                                                                                 s.p_FinG_fej, s.lm_id, sid, cp, cpf)),
            "dinit_ms": (cand, False, lambda c, o, s: c.slam_delayed_init(o, s.uv, s.clone_idx, s.n_meas, s.p_FinG)),
            "dinit_general_ms": (gcand, True, lambda c, o, s: c.slam_delayed_init_general(o, s.uv, s.clone_idx, s.cam_idx, s.n_meas, s.p_FinG)),
            "dinit_planes_ms": (pcand, False, lambda c, o, s: c.slam_delayed_init_planes(
                o, s.uv, s.clone_idx, s.n_meas, s.p_FinG, plane_of_cand=s.plane_id, plane_state_id=s.plane_state_id, cp=s.cp,
                cp_fej=s.cp_fej, p_FinG_noplane=s.p_FinG_noplane)),
        }
        self.ctx = {k: capi.Context(sc.N + 3 * sc.F, sc.C, max(sc.F, 32)) for k, (sc, _, _) in self.calls.items()}

    def window(self, reps):
        t = {k: 0.0 for k in FIGURES}
        for _ in range(reps):
            for name, (sc, cameras, call) in self.calls.items():
                ctx = self.ctx[name]
                ctx.cov_upload(sc.P)
                ctx.state_upload(sc)
                if cameras:
                    ctx.cameras_upload(sc)
                ctx.sync()
                o = self.capi.opts_from_scene(sc)
                t0 = time.perf_counter()
                call(ctx, o, sc)
                t[name] += time.perf_counter() - t0
        return {k: 1e3 * v / reps for k, v in t.items()}

    def close(self):
        for c in self.ctx.values():
            c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    other = os.environ.pop("OVP_LIB_AB", None)
    if not other:
        sys.exit("OVP_LIB_AB: the library to compare against")
    from ov_plane_amd import capi
    from ov_plane_amd.build import source_tree_hash
    from plane_loop_ab_timing import second_binding, stat

    small = {"this": Entries(capi), "other": Entries(second_binding(os.path.abspath(other)))}
    rows = {k: {f: [] for f in FIGURES} for k in small}
    for e in small.values():
        e.window(10)  # (a fresh device runs its first calls at ramping clocks)
    gc.collect()
    gc.disable()
    for w in range(a.windows):
        for name in (("this", "other") if w % 2 == 0 else ("other", "this")):
            for f, v in small[name].window(a.reps).items():
                rows[name][f].append(v)
    gc.enable()
    out = dict(what="the SLAM entries of this checkout's library and of the one in front of it in one process, interleaved windows "
                    "(tools/slam_ab_timing.py); host clock per call, ms; condition per figure: this.median <= other.median + "
                    "(other.max - other.min)",
               source_tree_hash=source_tree_hash(), other_library=os.path.basename(os.path.dirname(os.path.abspath(other))) + "/" +
               os.path.basename(other), reps=a.reps, windows=a.windows, figures={})
    ok = True
    for f in FIGURES:
        t, o = stat(rows["this"][f]), stat(rows["other"][f])
        spread = o["max"] - o["min"]
        fine = bool(t["median"] <= o["median"] + spread)
        ok &= fine
        out["figures"][f] = dict(this=t, other=o, other_spread=round(spread, 5), within=fine)
        print(f, json.dumps(out["figures"][f]))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    for e in small.values():
        e.close()
    if not ok:
        print("A FIGURE OF THIS BUILD IS ABOVE THE OTHER BUILD'S BY MORE THAN ITS SPREAD")
        sys.exit(1)


if __name__ == "__main__":
    main()
