"""The owning buffer types of the device context (csrc/ovp_buf.h) as a stand-alone host program: built from the header alone
against the HIP headers, with the five allocation calls defined over malloc and a counter that makes the k-th allocation fail, under
AddressSanitizer (leak checker included) and UBSan.  The assertions are in tests/ctx_buffers/buf_main.cpp."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "ov_plane_amd", "csrc")


def test_owning_buffers_under_sanitizers(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "buf_main")
    cmd = [os.path.join(rocm, "lib", "llvm", "bin", "clang++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + _CSRC,
           os.path.join(_HERE, "ctx_buffers", "buf_main.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"
