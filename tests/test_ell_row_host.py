"""Host build of csrc/ell_row.hpp (tests/host/ell_row.cpp) under AddressSanitizer and UBSan: the
SELL-64 element index every kernel and layout routine shares, against the formula written out and as
a bijection from (row, column) into the padded array, for N in {1, 63, 64, 65, 130} and row widths
4, 8 and 32."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "approximate-consensus-simulation_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ell_slot_under_sanitizers(tmp_path):
    exe = tmp_path / "ell_row"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "host", "ell_row.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "checks, 0 failed" in r.stderr, r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
