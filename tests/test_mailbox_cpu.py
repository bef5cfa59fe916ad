"""The pinned-result handshake (csrc/ovp_mailbox.h: SeqChannel, Mailbox) as a stand-alone host program: built from the header alone
against the HIP headers, with the allocation calls defined over malloc and a std::thread in the device's place, once under
AddressSanitizer (leak checker included) and UBSan and once under ThreadSanitizer.  The assertions are in
tests/mailbox/mailbox_main.cpp."""
import os
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.join(_HERE, "..")
_CSRC = os.path.join(_ROOT, "ov_plane_amd", "csrc")


@pytest.mark.parametrize("sanitize,env", [("address,undefined", {"ASAN_OPTIONS": "detect_leaks=1"}), ("thread", {})],
                         ids=["asan_ubsan", "tsan"])
def test_mailbox_under_sanitizers(tmp_path, sanitize, env):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "mailbox_main")
    cmd = [os.path.join(rocm, "lib", "llvm", "bin", "clang++"), "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitize,
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + _CSRC,
           "-I" + os.path.join(_ROOT, "include"), os.path.join(_HERE, "mailbox", "mailbox_main.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, **env))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"
