"""The host mirror's packing layer (csrc/host/ov_plane_pack.h) without a device: tests/host_pack_main.cpp, built with the address
and undefined-behaviour sanitizers, compares every packed array with values written out in the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_pack_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "ov_plane_amd", "csrc", "host"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host_pack_main.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "host pack ok" in run.stdout
