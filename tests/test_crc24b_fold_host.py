"""Host checks of csrc/crc24b_fold.h (no GPU): the table-free CRC24B of the codeblock kernel and the range arithmetic of its
segmentation, compiled from the header the kernel includes into the stand-alone program tests/crc24b_fold_check.cpp.

The program compares, for every message length of 1 to 320 words with n % 32 in {0, 1, 8, 24, 31} (all-zero, all-one, single-bit
and random messages), the folded CRC -- in one pass and split over 64 lanes as build_codeblock() splits it, the lanes' shares
recombined by the x^(32 m) rule of GoldTables::crc24b_mul -- with bitwise long division by 0x1800063; and the segmentation of a
codeblock, aligned and unaligned path, for every (tb_pos & 31, used & 31) pair and for last codeblocks with a 16- and a 24-bit TB
CRC and zero padding, with a bit-by-bit model, counting any word read beyond the transport block's readable extent as a failure.
"""
import os
import shutil
import subprocess
import tempfile

import pytest

import backends

SRC = os.path.join(backends.ROOT, "tests", "crc24b_fold_check.cpp")
INC = os.path.join(backends.ROOT, "srsran-edgeric-5g_amd", "csrc")


def build_and_run(flags, nof_random):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "crc24b_fold_check")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", INC] + flags + [SRC, "-o", exe], check=True, timeout=300)
        r = subprocess.run([exe, str(nof_random)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("ok: "), r.stdout
        return r.stdout


def test_fold_equals_long_division_and_segmentation_equals_bit_model():
    """Two hundred random messages per length on top of the fixed patterns: 1600 lengths, 332,800 messages."""
    out = build_and_run(["-O2"], 200)
    assert "332800 messages" in out


def test_same_program_under_host_sanitizers():
    """The same text with -fsanitize=address,undefined (a stand-alone host program; fewer random messages per length): shifts,
    index arithmetic and array bounds of the header and of the lane split."""
    with tempfile.TemporaryDirectory() as d:
        probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.path.join(d, "probe")],
                               input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtimes")
    build_and_run(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 4)
