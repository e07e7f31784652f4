"""The tile picker the four LDS-tile stage launchers share (tile_items, lol_amd/csrc/tile_host.h), on the CPU: the
stand-alone program tests/native/tile_items_host.cpp, compiled with g++ -fsanitize=address,undefined, checks it with each
launcher's cap rule against the arithmetic the launchers carried before they shared it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lol_amd", "csrc")


def test_tile_items_against_the_launchers_own_arithmetic(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs g++ and the ROCm headers")
    exe = tmp_path / "tile_items_host"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}",
           os.path.join(ROOT, "tests", "native", "tile_items_host.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "tile items host ok" in r.stdout
