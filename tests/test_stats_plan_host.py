"""The host-side plan of the chain statistics and summaries (csrc/gs_statplan.h: the
counted-sweep rule, the two slab layouts, the byte estimates) under host AddressSanitizer +
UndefinedBehaviorSanitizer: tests/host/stats_plan_main.cpp, a program of its own that includes
only that header, checks the rule against a brute-force loop, the layouts' alignment,
disjointness and zero prefix over every subset of the groups, and the estimates against the
expressions they replaced.  CPU only; nothing is loaded into Python."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_stats_plan_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = tmp_path / "stats_plan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "gibbssampling_amd" / "csrc"),
                    str(ROOT / "tests" / "host" / "stats_plan_main.cpp"), "-o", str(exe)],
                   check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.rstrip().endswith("all checks passed")
