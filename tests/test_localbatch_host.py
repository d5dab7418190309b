"""The host side of rbpf_local_map, thesis_amd/csrc/rbpf_localbatch.h, on the CPU: tests/host/localbatch_test.cpp includes
nothing but that header, is compiled by the host compiler with the address and undefined-behaviour sanitizers and runs as a
child process.  Its expectations (tables, reach at the limit's two sides, messages, the batch split) are literals, and it holds
the host copy of the placement to the square of half-side reach over 10^5 seeded windows and poses; see the program."""
import os
import shutil
import subprocess

from tests.conftest import REPO


def test_localbatch_helpers_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "localbatch_test")
    # -ffp-contract=off: the placement is six separately rounded operations, as the library is built
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(REPO, "thesis_amd", "csrc"), os.path.join(REPO, "tests", "host", "localbatch_test.cpp"), "-o", exe]
    # the sanitizers' runtimes inside the program where the compiler has them as archives (gcc), so that it runs whatever the
    # process environment loads first; clang links them statically by itself and does not know the options
    for static in (["-static-libasan", "-static-libubsan"], []):
        built = subprocess.run(cmd + static, capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0 and ran.stdout.strip() == "localbatch ok", ran.stdout + ran.stderr
