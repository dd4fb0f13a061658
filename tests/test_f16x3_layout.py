"""The index functions of csrc/f16x3_tile.h, walked on the CPU by tools/f16x3_layout_check.cpp: the chunk and stream LDS images (the DMA's
source side fills every 16-byte slot once with the piece the fragment reads expect; ds_read_b128 lane groups free of bank conflicts), the
turn-round patch (every cell written once, read once) and mfma32_row.  The program includes the header the kernels include; it is built
with the host compiler under AddressSanitizer and UBSan and run once."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_f16x3_layout_check_under_sanitizers(tmp_path):
    cxx = next((c for c in (shutil.which(n) for n in ("c++", "g++", "clang++")) if c), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "f16x3_layout_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "unitspeech_amd", "csrc"), os.path.join(ROOT, "tools", "f16x3_layout_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
