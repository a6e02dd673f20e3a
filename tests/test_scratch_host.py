"""wsovod::Scratch (csrc/scratch.h), the grow-only device workspace, on the host alone: tests/host/scratch_main.cpp
instantiates it over a fake device API and checks the three growth rules, the behaviour under stream capture, a failed
allocation and the per-device blocks."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scratch_growth_rules_on_a_fake_device_api(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++, c++ or clang++) on PATH")
    exe = str(tmp_path / "scratch_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "host", "scratch_main.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "scratch ok", r.stdout + r.stderr
