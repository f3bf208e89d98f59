"""The two owners of device memory (csrc/devmem.hpp: DevBuf for the temporaries of one call, DevArena for the blocks of
an initialisation) on the CPU, under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program with a stub
allocator and stub copies (tests/cxx/devmem_owners_driver.cpp) moves, re-allocates, fails an allocation in the middle
of a HIPCHK chain and of an arena, releases twice -- and counts the live blocks after every scope."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _have_gxx():
    if shutil.which("g++") is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        return False
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                       input="int main(){return 0;}", capture_output=True, text=True)
    return r.returncode == 0


@pytest.mark.skipif(not _have_gxx(), reason="g++ with the sanitizer runtimes (and the HIP headers devmem.hpp includes) not installed")
def test_owners_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "owners_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + SAN +
                          [os.path.join(ROOT, "tests", "cxx", "devmem_owners_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip().endswith("owners ok"), r.stdout[-2000:]
