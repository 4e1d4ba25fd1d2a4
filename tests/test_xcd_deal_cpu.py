"""The dealt hot-first renumbering of the XCD-striped PageRank layout
(memgraph_amd/csrc/mgx_xcd_deal.h), checked on the CPU: a stand-alone host
program (tests/xcd_deal_check.cpp) is built with AddressSanitizer and UBSan and
run over every V in 0..4200 and V = 2^20 + 5. What it checks is listed at the
top of that file."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_dealt_map_is_a_striped_bijection(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found")
    exe = str(tmp_path / "xcd_deal_check")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    os.path.join(HERE, "xcd_deal_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    big = (1 << 20) + 5
    r = subprocess.run([exe, "0", "4200", str(big), str(big)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok 4202", r.stdout + r.stderr
