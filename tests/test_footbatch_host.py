"""The host side of rbpf_check_footprints, thesis_amd/csrc/rbpf_footbatch.h, on the CPU: tests/host/footbatch_test.cpp includes
nothing but that header, is compiled by the host compiler with the address and undefined-behaviour sanitizers and runs as a
child process.  Its expectations (every message, the bounds' edges, the heading bins at negative headings, multiples of 2 pi and
half-bin points, the results of the three pairings) are literals; see the program."""
import os
import shutil
import subprocess

from tests.conftest import REPO


def test_footbatch_helpers_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "footbatch_test")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(REPO, "thesis_amd", "csrc"), os.path.join(REPO, "tests", "host", "footbatch_test.cpp"), "-o", exe]
    # the sanitizers' runtimes inside the program where the compiler has them as archives (gcc), so that it runs whatever the
    # process environment loads first; clang links them statically by itself and does not know the options
    for static in (["-static-libasan", "-static-libubsan"], []):
        built = subprocess.run(cmd + static, capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and ran.stdout.strip() == "footbatch ok", ran.stdout + ran.stderr
