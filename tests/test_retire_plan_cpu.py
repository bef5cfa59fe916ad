"""The planner of the batched plane merge (csrc/host/ov_plane_retire_plan.h) without a device: tests/retire_plan_main.cpp, built
with the address and undefined-behaviour sanitizers into a program of its own, compares every field of the plans with values
written out by hand in the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_retire_planner_under_sanitizers(tmp_path):
    exe = str(tmp_path / "retire_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "ov_plane_amd", "csrc", "host"),
                           os.path.join(ROOT, "tests", "retire_plan_main.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "retire plan ok" in run.stdout
