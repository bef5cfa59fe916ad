"""CPU tests of the fused hand-over's boundary (ovp_klt_match_frame): the symbol is declared and exported, the ctypes structures
match the header's layout, and the pure survivor / slot plan of ov_plane_frame_plan.h - compiled into a stand-alone program under
-fsanitize=address,undefined - equals its numpy restatement (frame_cases.plan_reference) on the slot-order case and on random keep
vectors at the sizes of the compaction test.  No compute on a device is attempted here."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_cases  # noqa: E402


def test_symbol_is_declared_and_exported(hiplib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ovplane_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint ovp_klt_match_frame\s*\(ovp_ctx \*ctx, const ovp_klt_frame_in \*in, ovp_klt_frame_out \*out\);", txt)
    assert "typedef struct ovp_klt_frame_in" in txt and "typedef struct ovp_klt_frame_out" in txt
    assert hasattr(hiplib.lib(), "ovp_klt_match_frame") and "ovp_klt_match_frame" in hiplib.EXPORTS
    import inspect
    sig = inspect.signature(hiplib.KltTracker.step)
    for name, default in (("database", None), ("timestamp", None), ("fused", False)):
        assert sig.parameters[name].default is default, "step's new keywords are off by default"
    assert hasattr(hiplib.KltTracker, "match_frame")
    assert int(re.search(r"#define OVP_EPI_MIN_POINTS (\d+)", txt).group(1)) == hiplib.OVP_EPI_MIN_POINTS


def test_struct_layouts_match_header(hiplib, tmp_path):
    """sizes as tests/test_capi_cpu.py checks them, and every field's offset against the C compiler's"""
    assert C.sizeof(hiplib.KltFrameIn) == 64
    assert C.sizeof(hiplib.KltFrameOut) == 8 + 6 * 8 + C.sizeof(hiplib.EpipolarInfo) == 160
    fields = {"ovp_klt_frame_in": hiplib.KltFrameIn, "ovp_klt_frame_out": hiplib.KltFrameOut}
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "ovplane_hip.h"\nint main(void) {\n'
    for cname, cls in fields.items():
        src += '  printf("%s %%zu", sizeof(%s));\n' % (cname, cname)
        for f, _ in cls._fields_:
            src += '  printf(" %%zu", offsetof(%s, %s));\n' % (cname, f)
        src += '  printf("\\n");\n'
    src += "  return 0;\n}\n"
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(c), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.strip().split("\n")
    for line, (cname, cls) in zip(out, fields.items()):
        v = line.split()
        assert v[0] == cname and int(v[1]) == C.sizeof(cls)
        assert [int(x) for x in v[2:]] == [getattr(cls, f).offset for f, _ in cls._fields_], cname


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_plan") / "frame_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "ov_plane_amd", "csrc", "host"), os.path.join(ROOT, "tests", "frame_plan_main.cpp"),
                           "-o", exe])
    return exe


def _run_plan(exe, path, keep, fresh, slot, free_slots):
    path.write_text("%d %d\n" % (len(keep), len(free_slots)) + "".join("%d %d %d\n" % (k, f, s) for k, f, s in zip(keep, fresh, slot)) +
                    " ".join(str(int(v)) for v in free_slots) + "\n")
    run = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    rows = [[int(v) for v in line.split()] for line in run.stdout.strip("\n").split("\n")]
    body = np.array(rows[1:], dtype=np.int32).reshape(-1, 2)
    return rows[0][0], rows[0][1], body[:, 0], body[:, 1]


def test_plan_on_the_slot_order_case(plan_exe, tmp_path):
    c = frame_cases.slot_order_case()
    known = {1: 0, 4: 3, 6: 5}                     # what the case's docstring derives
    free_slots = [4, 2, 1, 6, 7]
    fresh = np.array([i not in known for i in c["frame_ids"]])
    slot = np.array([known.get(int(i), -1) for i in c["frame_ids"]])
    ok, nf, idx, sl = _run_plan(plan_exe, tmp_path / "slot.txt", c["frame_keep"], fresh, slot, free_slots)
    want = frame_cases.plan_reference(c["frame_keep"], fresh, slot, free_slots)
    assert ok == 1 and nf == want[2] == 3 and np.array_equal(idx, want[0]) and np.array_equal(sl, want[1])
    assert dict(zip(c["frame_ids"][idx].tolist(), sl.tolist())) == {11: 4, 1: 0, 13: 2, 6: 5, 15: 1}
    # more fresh survivors than free slots: the plan says so and stops
    ok, nf, idx, sl = _run_plan(plan_exe, tmp_path / "short.txt", c["frame_keep"], fresh, slot, free_slots[:2])
    assert ok == 0 and nf == 2


@pytest.mark.parametrize("n", frame_cases.EDGE_SIZES)
def test_plan_on_random_keep_vectors(plan_exe, tmp_path, n):
    rng = np.random.default_rng(4000 + n)
    for trial, p_keep in enumerate((0.5, 0.05, 0.95, 0.0, 1.0)):
        keep, fresh = rng.random(n) < p_keep, rng.random(n) < 0.4
        perm = rng.permutation(2 * n + 8)
        slot = np.where(fresh, -1, perm[:n])
        free_slots = perm[n:n + int(fresh.sum())]
        ok, nf, idx, sl = _run_plan(plan_exe, tmp_path / ("r%d.txt" % trial), keep, fresh, slot, free_slots)
        want = frame_cases.plan_reference(keep, fresh, slot, free_slots)
        assert ok == 1 and nf == want[2] and np.array_equal(idx, want[0]) and np.array_equal(sl, want[1]), (n, p_keep)
