"""csrc/device_buffer.hpp on the host: ownership, ensure / reserve and the byte counter against counting stubs of the HIP
allocation calls.  The check is a stand-alone program (tests/device_buffer_stub/) built with AddressSanitizer and
UBSan and run as a child process; nothing sanitized is loaded into this interpreter."""

import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
STUB = os.path.join(HERE, "device_buffer_stub")
CSRC = os.path.join(os.path.dirname(HERE), "pde_opt_amd", "csrc")


def _compiler():
    for exe in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++", "c++"):
        path = exe if os.path.isabs(exe) and os.path.exists(exe) else shutil.which(exe)
        if path:
            return path
    return None


def test_device_buffer_ownership(tmp_path):
    cxx = _compiler()
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path / "device_buffer_check")
    # -isystem: the stub <hip/hip_runtime.h> stands in for the real one
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-isystem", STUB, "-I", CSRC, os.path.join(STUB, "device_buffer_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stdout}\n{r.stderr}"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, f"{r.stdout}\n{r.stderr}"
    assert "device_buffer ok: 7 device and 1 pinned blocks, all freed" in r.stdout


def test_header_stands_alone():
    """the header includes nothing of the project and calls only the four allocation functions"""
    src = open(os.path.join(CSRC, "device_buffer.hpp")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert all(i.startswith("<") for i in includes), includes
    assert set(re.findall(r"\bhip[A-Z]\w*(?=\()", src)) == {"hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree"}
