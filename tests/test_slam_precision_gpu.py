"""ovp_slam_update and ovp_slam_update_general against the long-double truth, stage by stage (tests/slam_precision_cases.py has the
cases, the derivation of every bound and the float64 models; tests/test_slam_precision_cpu.py holds the bounds on the CPU):
rows, gate, M and the S-form tail, each from the device's own output of the stage before, read back through ovp_debug_read
"slam_Ht" / "slam_res" / "slam_M" / "slam_cols".  A case passes at ratio <= 1 in every stage; one line per case and stage:
SLAMPREC <case> <stage> <worst ratio>.  Every case runs with n_max = n and n_max = n + 5.

Not held here: delayed initialisation - single
candidates of ovp_slam_delayed_init, _general and _planes against the long-double chain remain to be written; multi-candidate loops
and the commit of the previous correction stay with the parity tests (tests/test_gpu_parity.py, test_general_slam_gpu.py,
test_dinit_planes_gpu.py)."""
import json
import os

import numpy as np
import pytest

import slam_precision_cases as S

CASES = S.cases()
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "slam_precision_ratios.json")


def run(hiplib, c, n_max):
    sc = S.scene(c)
    ctx = hiplib.Context(n_max, sc.C, sc.F)
    try:
        ctx.cov_upload(sc.P)
        ctx.state_upload(sc)
        sid, cp, cpf = S.plane_args(c, sc)
        pre = S.pre_blocks(c, sc) if c["pre"] else None
        opts = hiplib.opts_from_scene(sc)
        if c["kind"] in ("stereo", "cams"):
            ctx.cameras_upload(sc)
            out = ctx.slam_update_general(opts, sc.uv, sc.clone_idx, sc.cam_idx, sc.n_meas, sc.p_FinG, sc.p_FinG_fej, sc.lm_id, sid, cp, cpf, pre=pre)
        else:
            out = ctx.slam_update(opts, sc.uv, sc.clone_idx, sc.n_meas, sc.p_FinG, sc.p_FinG_fej, sc.lm_id, sid, cp, cpf, pre=pre)
        m_total, gcols, h_in_lds, sform = S.geometry(c, sc)
        # the device's own decisions: stacked rows, columns, S-form or information form, H of a block in LDS or in scratch
        assert ctx.debug_read("slam_dims", (4,), dtype=np.int32).tolist() == [m_total, gcols, int(sform), h_in_lds]
        assert h_in_lds == c.get("h_in_lds", h_in_lds)
        cols = ctx.debug_read("slam_cols", (gcols,), dtype=np.int32)
        got = dict(cols=cols, Ht=ctx.debug_read("slam_Ht", (gcols, m_total)), res=ctx.debug_read("slam_res", (m_total,)),
                   M=ctx.debug_read("slam_M", (sc.N, m_total)) if sform else None, chi2=out["chi2"], status=out["status"], dx=out["dx"],
                   P=ctx.cov_download())
        if not sform:
            with pytest.raises(hiplib.OvpError):
                ctx.debug_read("slam_M", (sc.N, m_total))
        return got
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_slam_update_stage_by_stage(hiplib, c):
    sc = S.scene(c)
    worst = {}
    for n_max in S.capacities(sc.N):
        got = run(hiplib, c, n_max)
        assert [int(s) for s in got["status"]] == c["expect"]
        assert sorted(int(i) for i in got["cols"]) == sorted(set(int(i) for b in S.layout(c, sc) for i in b["ids"]))
        r = S.ratios(c, got)
        for stage, v in r.items():
            print("SLAMPREC %s(n_max=%d) %s %.3g" % (c["name"], n_max, stage, v))
            worst[stage] = max(worst.get(stage, 0.0), v)
    if os.environ.get("OVP_WRITE_PRECISION_RECORD"):  # a record of a run, never an input of a bound; a subset keeps the other cases
        rec = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        rec[c["name"]] = worst
        with open(RECORD, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
    assert max(worst.values()) <= 1.0, worst
