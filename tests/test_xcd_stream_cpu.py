"""The offset rule of the stripe-major column stream of the XCD-striped
PageRank sweep (memgraph_amd/csrc/mgx_xcd_stream.h), checked on the CPU: a
stand-alone host program (tests/xcd_stream_check.cpp) is built with
AddressSanitizer and UBSan and run over 2000 seeded layouts. What it checks is
listed at the top of that file."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_segments_keep_their_residue_and_do_not_overlap(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found")
    exe = str(tmp_path / "xcd_stream_check")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    os.path.join(HERE, "xcd_stream_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "1", "2000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok 2000", r.stdout + r.stderr
