"""The engine's host code under AddressSanitizer + UBSan + LeakSanitizer for a stand-alone C program: one recipe for the tests that
run tests/*_sanitize.c.  CPU build only: the device code of this build is the ordinary gfx950 object and is never launched.  The
programs are executables of their own, linked against the sanitized library directly; nothing is loaded into Python."""
import glob
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gelato_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
CLANG = "/opt/rocm/lib/llvm/bin/clang"

needs_toolchain = pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(CLANG)), reason="ROCm toolchain not present")


def build(tmp_path):
    """the fused kernel's translation unit and every host file, sanitized, as one library in tmp_path -> its path"""
    lib = tmp_path / "libgelato_amd_asan.so"
    flags = ["-O1", "-g", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-fast-math", "-ffp-contract=on",
             "-mllvm", "-disable-machine-licm", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-w"]
    host = sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "gel_host*.hip")))
    subprocess.run([HIPCC, *flags, "-shared", "-o", str(lib), "gel_kernels.hip", *host], cwd=CSRC, check=True, capture_output=True, timeout=280)
    return lib


def run_program(tmp_path, lib, name):
    """compiles tests/<name>.c against the sanitized library, runs it, and asserts that it ended clean: exit status 0, its
    <NAME>_OK line, no UBSan report, no ASan / LeakSanitizer report"""
    exe = tmp_path / name
    subprocess.run([CLANG, "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", str(exe),
                    os.path.join(ROOT, "tests", name + ".c"), str(lib), "-lm",
                    "-Wl,-rpath,%s" % tmp_path, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, timeout=120)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and name.upper() + "_OK" in r.stdout, (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
