"""The engine's host code (LGR generator, pattern walker, index maps, descriptor validation, error paths) under
AddressSanitizer + UBSan + LeakSanitizer, through a host-only handle.  CPU build only: GPU ASan / xnack+ code
objects are not available on the pool, so the device code of this build is the ordinary gfx950 object and is
never launched here."""
import os
import shutil
import subprocess

import pytest

import sanitized_lib
from conftest import ROOT


@sanitized_lib.needs_toolchain
def test_host_code_under_asan_ubsan(tmp_path):
    sanitized_lib.run_program(tmp_path, sanitized_lib.build(tmp_path), "host_sanitize")


def test_oracle_under_asan_ubsan(tmp_path):
    """The CPU oracle itself (the checker every parity test leans on) with exactly sized heap buffers."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not present")
    exe = tmp_path / "oracle_sanitize"
    subprocess.run([gcc, "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fopenmp", "-o", str(exe),
                    os.path.join(ROOT, "tests", "oracle_sanitize.c"), os.path.join(ROOT, "oracle", "gelato_oracle.c"), "-lm"],
                   check=True, capture_output=True, timeout=240)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", OMP_NUM_THREADS="2")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "ORACLE_SANITIZE_OK" in r.stdout, (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
