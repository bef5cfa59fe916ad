"""The planner of the two SLAM entries (csrc/ovp_slam_plan.h) without a device: tests/slam_plan_main.cpp, built with the address and
undefined-behaviour sanitizers and no HIP include path, compares every field of the plans with values written out in the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slam_planner_under_sanitizers(tmp_path):
    exe = str(tmp_path / "slam_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "ov_plane_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "slam_plan_main.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "slam plan ok" in run.stdout
