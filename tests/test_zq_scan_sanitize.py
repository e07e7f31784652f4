"""The host side of the scan route of the prime ops (LOLHIP_ROUTE_SCAN_ZQ) under AddressSanitizer and UBSan: plan.cpp,
capi.cpp and the host sources they need, compiled with g++ -fsanitize=address,undefined against the device stubs and
driven by the stand-alone program tests/native/zq_scan_host.cpp — both creators over indices x moduli x flag and route
words, the route query for every op across the ZQ_SCAN and GENERIC_SCALAR switches, null and out-of-range arguments,
host-only compute calls answering LOLHIP_ERR_NO_DEVICE."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lol_amd", "csrc")


def test_zq_scan_host_code_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs g++ and the ROCm headers")
    exe = tmp_path / "zq_scan_host"
    srcs = [os.path.join(CSRC, f) for f in ("plan.cpp", "hostmath.cpp", "wire.cpp", "capi.cpp", "crtset.cpp", "khprf_api.cpp",
                                            "modswitch_api.cpp", "public_api.cpp", "ptround_api.cpp", "pttunnel_api.cpp",
                                            "ringmul_api.cpp")]
    srcs += [os.path.join(ROOT, "tests", "native", f) for f in ("device_stubs.cpp", "zq_scan_host.cpp")]
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}",
           *srcs, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "zq scan host ok" in r.stdout
