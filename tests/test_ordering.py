"""The ordering of the reduced variables (csrc/ordering.cpp) as a stand-alone program: tests/cpp/test_ordering.cpp and ordering.cpp
compiled with a plain host compiler -- no hipcc, no HIP include path, nothing preloaded, which also shows that the unit is host-only --
and run twice: built plainly, and built with the address and undefined-behaviour sanitizers.  The program checks reverse Cuthill-McKee
and minimum degree against naive versions, nested dissection by its properties, the block- and tile-level flop counts against a naive
dense boolean Cholesky and the placement against layouts worked out by hand, on the smallest graphs that reach every branch; it prints
what failed and exits non-zero."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gtsam_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "cpp", "test_ordering.cpp"), os.path.join(CSRC, "ordering.cpp")]
DEPS = SRCS + [os.path.join(CSRC, "ordering.h")]


def _compiler():
    for cxx in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if cxx and os.path.exists(cxx):
            return cxx
    pytest.fail("no host C++ compiler (clang++ or g++) to build the ordering test with")


def _build(name, flags):
    path = os.path.join(ROOT, "tests", "_build", name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if not os.path.exists(path) or any(os.path.getmtime(path) < os.path.getmtime(d) for d in DEPS):
        tmp = f"{path}.{os.getpid()}.tmp"   # (renamed into place: a run in parallel never starts a half-written file)
        subprocess.run([_compiler(), "-std=c++17", "-Wall"] + flags + ["-o", tmp] + SRCS, check=True)
        os.replace(tmp, path)
    return path


@pytest.mark.parametrize("name,flags", [("test_ordering", ["-O2"]),
                                        ("test_ordering_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])],
                         ids=["plain", "address+undefined"])
def test_ordering_stand_alone(name, flags):
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([_build(name, flags)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith(" 0 failed")
