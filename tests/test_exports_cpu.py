"""The library's dynamic C surface is exactly include/gelato_amd.h (no GPU): a helper of the host files that became a C-named
dynamic symbol would interpose, or be interposed by, a function of the same name in the host application.  What is looked at is
the library that the package loads (the Makefile's build, or GELATO_AMD_LIB); the sanitized and the variant builds, which compile
the same sources with other flags, are not."""
import os
import shutil
import subprocess

import pytest

from gelato_amd import _lib

LLVM_NM = "/opt/rocm/lib/llvm/bin/llvm-nm"


def test_dynamic_c_symbols_are_the_header():
    nm = shutil.which("nm") or (LLVM_NM if os.path.exists(LLVM_NM) else None)
    if nm is None:
        pytest.skip("neither nm nor llvm-nm present")
    out = subprocess.run([nm, "-D", "--defined-only", _lib.SO_PATH], check=True, capture_output=True, text=True, timeout=60).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert len(names) > len(_lib.SIGNATURES)          # (the launchers of namespace gel are there as well: the listing is not empty)
    # C++ names are mangled (_Z...); what is left has C linkage: the header's functions, the compiler's one id per .hip file, the loader's hooks
    c_names = {n for n in names if not n.startswith("_Z") and not n.startswith("__hip_") and n not in ("_init", "_fini")}
    declared = set(_lib.SIGNATURES)
    assert c_names == declared, "not in the header: %s; not exported: %s" % (sorted(c_names - declared), sorted(declared - c_names))
    internal = sorted(n for n in names if "7gelhost" in n)
    assert not internal, "host-internal functions exported: %s" % internal
