"""The chain agreement's result slab (csrc/gs_statplan.h: agreement_slab, agreement_bytes) under
host AddressSanitizer + UndefinedBehaviorSanitizer: tests/host/agreement_plan_main.cpp, a
program of its own that includes only that header and checks the parts' alignment and
disjointness, the zeroed prefix, which parts a call leaves out, and the bytes charged.  CPU
only; nothing is loaded into Python."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_agreement_plan_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = tmp_path / "agreement_plan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "gibbssampling_amd" / "csrc"),
                    str(ROOT / "tests" / "host" / "agreement_plan_main.cpp"), "-o", str(exe)],
                   check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.rstrip().endswith("all checks passed")
