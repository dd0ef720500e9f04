"""The rule of csrc/engine_host.h, checked on the CPU: a stand-alone program (tests/host/engine_host_check.cpp) includes the
scaffold and runs it against a fake of the HIP entry points it references, which keeps every copy pending until the stream is
waited on.  Nothing of the HIP runtime is linked, no GPU is needed and nothing is loaded into this process."""
import os
import subprocess

import pytest

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="no ROCm clang++ to compile the host check with")
def test_engine_host_check():
    built = subprocess.run(["make", "-C", HOST, "engine_host_check"], capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([os.path.join(HOST, "engine_host_check")], capture_output=True, text=True, timeout=60)
    print(ran.stdout)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "all 7 checks hold" in ran.stdout
