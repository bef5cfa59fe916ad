"""The planner of the point update (csrc/ovp_point_plan.h) without a device: tests/point_plan_main.cpp, built with the address and
undefined-behaviour sanitizers and no HIP include path, compares every field of the plan with values written out in the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_point_planner_under_sanitizers(tmp_path):
    exe = str(tmp_path / "point_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "ov_plane_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "point_plan_main.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "point plan ok" in run.stdout
