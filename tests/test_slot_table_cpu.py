"""The slot table and the capacity rule of the online modules' persistent state
(memgraph_amd/csrc/mgx_slot_table.h), checked on the CPU: a stand-alone host
program (tests/slot_table_check.cpp) is built with AddressSanitizer and UBSan
and run over 3000 seeded operation sequences against a naive std::map model.
What it checks is listed at the top of that file."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_slot_table_matches_the_naive_model(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found")
    exe = str(tmp_path / "slot_table_check")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    os.path.join(HERE, "slot_table_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "1", "3000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok 3000", r.stdout + r.stderr
