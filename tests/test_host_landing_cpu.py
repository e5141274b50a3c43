"""The host-side consumer of the packed value run (linkteller_amd/csrc/lt_host_landing.h) is plain C++: tests/host_landing_main.cpp
drives it with a producer thread in the GPU's place -- values in random block order with random pauses, all there before the
consumer starts, all after the ready word; one word held back until the settle callback (the stream wait), a value that equals the
sentinel, an index out of bounds, a run published late or never, a failing wait -- and checks the placed matrix, that the value
region is armed again afterwards, and that the budget path is taken exactly once where it must be and never where it need not.
Built with the system compiler under ThreadSanitizer and again under AddressSanitizer + UBSan, as stand-alone programs."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tests", "host_landing_main.cpp")
INC = os.path.join(REPO, "linkteller_amd", "csrc")


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_consumer_under_sanitizers(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler"
    exe = tmp_path / "host_landing"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", f"-fsanitize={sanitize}",
                        "-fno-sanitize-recover=all", "-pthread", "-I", INC, SRC, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ok 14 cases" in run.stdout, (run.stdout[-3000:], run.stderr[-3000:])
