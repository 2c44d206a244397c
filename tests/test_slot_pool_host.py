"""Host checks of the slot life cycle that the downlink and the uplink slot pools share (no GPU).

csrc/slot_pool_host.h holds the device-free part of csrc/dl_slot_async.cpp and csrc/ul_slot_async.cpp: the states of a slot
(free, open, finishing, done), the locks and the condition variable of a pool, and the memory orders between the threads that
drive a pool and the threads of the HIP runtime that complete its slots.  tests/slot_pool_check.cpp compiles the header by
itself into a stand-alone program that

  * walks every transition on one thread for pools of 1, 2 and 64 slots: distinct ids until the pool is exhausted, look-up, poll
    and wait in each of the four states, completion with both statuses with and without a handler (which runs exactly once, with
    the slot's arguments, and already polls the final status), an armed slot failed without a handler, release and a fresh
    claim without stale handler or status, and the count of open slots after every step;
  * drives pools of 1, 2 and 4 slots from four submitting threads with fixed seeds, two threads that complete the armed slots
    some yields later and one that closes slots for the others, and checks that no slot ever has two owners, that the count of
    open slots stays within the depth and ends at zero, that as many handlers ran as were armed, that every wait and poll gives
    what its slot was completed with -- and that the run ends: a lost wake-up is the timeout below.

The program runs built with -O2, under the address and undefined-behaviour sanitizers, and under the thread sanitizer.
"""
import os
import platform
import shutil
import subprocess
import tempfile

import pytest

import backends

SRC = os.path.join(backends.ROOT, "tests", "slot_pool_check.cpp")
INC = [os.path.join(backends.ROOT, "srsran-edgeric-5g_amd", "csrc"), os.path.join(backends.ROOT, "include")]


# g++ 11's thread sanitizer gives up before main ("unexpected memory mapping") where the kernel places a program with more random
# address bits than that runtime knows, so the checker runs with address randomisation off for itself where setarch is installed.
FIXED_ADDRESSES = ["setarch", platform.machine(), "-R"] if shutil.which("setarch") else []


def build_and_run(flags):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "slot_pool_check")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", INC[0], "-I", INC[1]] + flags + [SRC, "-o", exe],
                       check=True, timeout=300)
        r = subprocess.run(FIXED_ADDRESSES + [exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("ok: "), r.stdout
        return r.stdout


def skip_unless_links(sanitize):
    """Skips only where this g++ cannot link a program with the flag at all."""
    with tempfile.TemporaryDirectory() as d:
        probe = subprocess.run(["g++", "-pthread", sanitize, "-x", "c++", "-", "-o", os.path.join(d, "probe")],
                               input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no runtime for " + sanitize)


def test_life_cycle_on_one_and_on_several_threads():
    out = build_and_run(["-O2"])
    assert int(out.split()[1]) > 20000, out


def test_same_program_under_address_and_undefined_sanitizers():
    skip_unless_links("-fsanitize=address,undefined")
    build_and_run(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_same_program_under_thread_sanitizer():
    """Every access that the life cycle leaves to a lock or to an acquire/release pair, seen by the thread sanitizer (a
    stand-alone host program; a report makes it exit with a status other than 0)."""
    skip_unless_links("-fsanitize=thread")
    build_and_run(["-O1", "-g", "-fsanitize=thread"])
