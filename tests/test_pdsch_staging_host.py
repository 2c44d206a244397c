"""Host checks of the device-free layout part of csrc/pdsch_staging_host.h (no GPU): where the asynchronous seams (pdsch_async.cpp,
dl_slot_async.cpp) put the transport blocks of a call and its plan tables, compiled from the header both include into the
stand-alone program tests/pdsch_staging_check.cpp.

The program lays out and copies calls of one, three and 64 PDUs with tb_size_bytes in {1, 3, 4, 5, 255, 256, 257} (every size
alone, every ordered triple, 64 of one size and 64 in rotation) and totals that land exactly on and one byte past a 256-byte
boundary, and asserts: every offset a multiple of 4; each block followed by 4 to 7 zero bytes, as (size + 7) & ~3 gives;
tables_at the first multiple of 256 at or after tb_total; no byte from tb_total on written by the block copy, beyond tables_at
included; the region before a block's offset left as it was; a null tbs[i] or a zero tb_size_bytes refused by the layout
step, which never sees the region.  Every block lives in a heap allocation of exactly its size.
"""
import os
import subprocess
import tempfile

import pytest

import backends

SRC = os.path.join(backends.ROOT, "tests", "pdsch_staging_check.cpp")
INC = [os.path.join(backends.ROOT, "srsran-edgeric-5g_amd", "csrc"), os.path.join(backends.ROOT, "include")]


def build_and_run(flags):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "pdsch_staging_check")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", INC[0], "-I", INC[1]] + flags + [SRC, "-o", exe],
                       check=True, timeout=300)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("ok: "), r.stdout
        return r.stdout


def test_layout_and_block_copy_of_one_three_and_64_pdus():
    out = build_and_run(["-O2"])
    # 7 + 7^3 + 2 * 7 + 3 * 4 calls
    assert "ok: 376 calls" in out


def test_same_program_under_host_sanitizers():
    """The same text with -fsanitize=address,undefined (a stand-alone host program): the reads of each block and the writes
    into the region."""
    with tempfile.TemporaryDirectory() as d:
        probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.path.join(d, "probe")],
                               input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtimes")
    build_and_run(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
