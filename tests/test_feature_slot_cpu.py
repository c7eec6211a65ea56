"""csrc/feature_slot.hpp on the host: the owning table of the ctx's feature states against dummy features that log
construction, invalidate and destruction.  The check is a stand-alone program (tests/feature_slot_stub/) built with
AddressSanitizer and UBSan and run as a child process; nothing sanitized is loaded into this interpreter."""

import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
STUB = os.path.join(HERE, "feature_slot_stub")
CSRC = os.path.join(os.path.dirname(HERE), "pde_opt_amd", "csrc")


def _compiler():
    for exe in ("/opt/rocm/llvm/bin/clang++", "clang++", "g++", "c++"):
        path = exe if os.path.isabs(exe) and os.path.exists(exe) else shutil.which(exe)
        if path:
            return path
    return None


def test_feature_table_ownership(tmp_path):
    cxx = _compiler()
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path / "feature_slot_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-I", CSRC, os.path.join(STUB, "feature_slot_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stdout}\n{r.stderr}"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, f"{r.stdout}\n{r.stderr}"
    assert "feature_slot ok: 10 states made, all destroyed" in r.stdout


def test_header_stands_alone():
    """the header includes standard headers only and calls nothing of HIP"""
    src = open(os.path.join(CSRC, "feature_slot.hpp")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<") for i in includes), includes
    assert re.findall(r"\bhip[A-Za-z_]\w*(?=\()", src) == []
