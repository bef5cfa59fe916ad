"""The staged upload (csrc/ovp_staged.h: OvpEvent, UploadFence, Staged) as a stand-alone host program: built from the header alone
against the HIP headers under AddressSanitizer (leak checker included) and UBSan, with the allocation calls defined over malloc and a
stream that only queues its copies until something synchronises.  The assertions are in tests/staged/staged_main.cpp."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.join(_HERE, "..")
_CSRC = os.path.join(_ROOT, "ov_plane_amd", "csrc")


def test_staged_under_sanitizers(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "staged_main")
    cmd = [os.path.join(rocm, "lib", "llvm", "bin", "clang++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + _CSRC,
           "-I" + os.path.join(_ROOT, "include"), os.path.join(_HERE, "staged", "staged_main.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"
