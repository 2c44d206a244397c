"""The measuring tools under profiles/: one timing method and one owner of "a GPU step runs under a limit and nothing starts
after a failure" (profiles/bench_harness.py), the A/B tool built on it (profiles/ab.py), and the *_bench.py scripts that use them.

CPU: run_steps with plain Python children (statuses, the time limit, an abort's status, order and environment); the command
lines ab.py hands to run_steps against the ones the shell loops it replaced ran, written out here; time_rounds, spread and settle
against a fake clock; every *_bench.py answers --help without a device or a built library, and none times or guards on its own.

GPU: copy_rate, settle and time_rounds with real events on an explicit stream around one small SrsPlan run."""
import contextlib
import ctypes as C
import glob
import io
import json
import os
import re
import runpy
import sys

import pytest

import backends

PROFILES = os.path.join(backends.ROOT, "profiles")
sys.path.insert(0, PROFILES)
import ab  # noqa: E402
import bench_harness as harness  # noqa: E402

BENCH_SCRIPTS = sorted(glob.glob(os.path.join(PROFILES, "*_bench.py")))


def child(code, *args):
    return [sys.executable, "-c", code] + list(args)


def exits(status, marker, say=""):
    """A child that leaves `marker`, writes `say` to stderr and ends with `status`."""
    return child("import sys; open(sys.argv[1], 'w').close(); sys.stderr.write(sys.argv[2]); sys.exit(int(sys.argv[3]))", marker, say, str(status))


def test_run_steps_stops_at_the_first_failure_and_keeps_its_stderr(tmp_path, capfd):
    marks = [str(tmp_path / ("mark%d" % i)) for i in range(3)]
    steps = [("first", exits(0, marks[0]), {}, 20), ("second", exits(3, marks[1], "the reason it failed\n"), {}, 20),
             ("third", exits(0, marks[2]), {}, 20)]
    assert harness.run_steps(steps, str(tmp_path / "logs")) == 3
    assert [os.path.exists(m) for m in marks] == [True, True, False]
    assert "the reason it failed" in (tmp_path / "logs" / "second.err").read_text()
    report = capfd.readouterr().err
    assert "second" in report and "status 3" in report and "the reason it failed" in report


def test_run_steps_ends_a_step_at_its_limit_and_starts_nothing_after(tmp_path):
    mark = str(tmp_path / "after")
    steps = [("sleeper", child("import time; time.sleep(30)"), {}, 1), ("after", exits(0, mark), {}, 20)]
    assert harness.run_steps(steps, str(tmp_path)) == 124
    assert not os.path.exists(mark)


def test_run_steps_ends_with_an_aborts_status(tmp_path):
    mark = str(tmp_path / "after")
    steps = [("aborts", child("import sys; sys.exit(134)"), {}, 20), ("after", exits(0, mark), {}, 20)]
    assert harness.run_steps(steps, str(tmp_path)) == 134
    assert not os.path.exists(mark)


def test_run_steps_runs_in_order_with_each_steps_environment_and_no_other(tmp_path, capfd, monkeypatch):
    monkeypatch.delenv("HARNESS_A", raising=False)
    monkeypatch.delenv("HARNESS_B", raising=False)
    order = str(tmp_path / "order")
    code = ("import json, os, sys, time\n"
            "open(sys.argv[1], 'a').write(sys.argv[2] + '\\n')\n"
            "json.dump(dict(os.environ), open(sys.argv[1] + '.' + sys.argv[2], 'w'))\n"
            "print('line from', sys.argv[2])\n")
    adds = {"a": {"HARNESS_A": "1"}, "b": {"HARNESS_B": "two"}, "c": {}}
    seen = []
    status = harness.run_steps([(k, child(code, order, k), env, 20) for k, env in adds.items()], str(tmp_path),
                               lambda label, last: seen.append((label, last)))
    assert status == 0
    assert open(order).read().split() == ["a", "b", "c"]
    for k, env in adds.items():
        got = json.load(open(order + "." + k))
        if "LC_CTYPE" not in os.environ:
            got.pop("LC_CTYPE", None)  # the child interpreter's own locale coercion
        assert got == dict(os.environ, **env)
    assert seen == [(k, "line from " + k) for k in adds]
    assert capfd.readouterr().out.split("\n")[:3] == ["line from a", "line from b", "line from c"]  # stdout is passed through


# What the shell loops ran at the parent commit (profiles/ab_variants.sh, ab_rx_variants.sh, ab_env.sh, slots_sweep.sh,
# stage_times.sh, ofdm_parts.sh), command line by command line.
QUIET = ["--no-cpu-baseline", "--no-secondary"]
AB_CASES = [
    (["lib", "2", "a.so", "b.so"], {"BENCH_ARGS": "--slots 512"},
     [(["python3", "bench.py", "--full"] + QUIET + ["--steps", "20", "--slots", "512"], {"NRPHY_LIB_SO": "$PWD/" + v}) for v in ("a.so", "b.so") * 2]),
    (["rx", "2", "a.so", "b.so"], {"RX_ARGS": "--steps 5"},
     [(["python3", "profiles/rx_chain_bench.py", "--steps", "5"], {"NRPHY_LIB_SO": "$PWD/" + v}) for v in ("a.so", "b.so") * 2]),
    (["env", "NRPHY_NO_DIAG_PRECODING"], {"NRPHY_NO_DIAG_PRECODING": "1"},
     [(["python3", "bench.py"] + QUIET + ["--steps", "20"], env) for env in ({}, {"NRPHY_NO_DIAG_PRECODING": "1"}) * 3]),
    (["env", "KNOB", "1"], {}, [(["python3", "bench.py"] + QUIET + ["--steps", "20"], env) for env in ({}, {"KNOB": "1"})]),
    (["slots", "--wire"], {},
     [(["python3", "bench.py", "--slots", str(s), "--steps", str(51200 // s), "--warmup", str(51200 // s // 2 + 30)] + QUIET + ["--wire"], {})
      for s in (64, 128, 192, 256, 384, 512, 768, 1024, 2048)]),
    (["slots"], {}, [(["python3", "bench.py", "--slots", "64", "--steps", "800", "--warmup", "430"] + QUIET, {})]),
    (["stages"], {}, [(["python3", "bench.py"] + QUIET, {"NRPHY_LIB_SO": "$PWD/build/variants/probes.so", "NRPHY_PROFILE_STAGE": st})
                      for st in "10 5 7 1 2 4 11 0".split()]),
    (["stages"], {"STAGES": "5 0", "NRPHY_LIB_SO": "/x/p.so"},
     [(["python3", "bench.py"] + QUIET, {"NRPHY_LIB_SO": "/x/p.so", "NRPHY_PROFILE_STAGE": st}) for st in ("5", "0")]),
    (["ofdm-parts", "--wire"], {}, [(["python3", "bench.py"] + QUIET + ["--steps", "20", "--wire"],
                                     {"NRPHY_LIB_SO": "$PWD/build/variants/probes.so", "NRPHY_OFDM_PROBE": pr}) for pr in "01230123"]),
]


@pytest.mark.parametrize("argv,environ,want", AB_CASES, ids=[" ".join(c[0] + sorted(c[1])) for c in AB_CASES])
def test_ab_hands_run_steps_the_command_lines_of_the_shell_loops(argv, environ, want, monkeypatch):
    for name in ("BENCH_ARGS", "RX_ARGS", "STAGES", "PROBES", "NRPHY_LIB_SO", "NRPHY_PROFILE_STAGE", "NRPHY_OFDM_PROBE", "KNOB"):
        monkeypatch.delenv(name, raising=False)
    for name, value in environ.items():
        monkeypatch.setenv(name, value)
    recorded = []
    monkeypatch.setattr(harness, "run_steps", lambda steps, log_dir, report=None: recorded.extend(steps) or 0)
    assert ab.main(argv) == 0
    here = os.getcwd()
    want = [(cmd, {k: v.replace("$PWD", here) for k, v in env.items()}) for cmd, env in want]
    assert [(cmd, env) for _, cmd, env, _ in recorded][:len(want)] == want
    assert len(recorded) == len(want) or argv == ["slots"]
    assert len({label for label, _, _, _ in recorded}) == len(recorded) and all(limit > 0 for _, _, _, limit in recorded)
    if argv[0] == "env":  # the run without the knob does not inherit it from the caller
        assert argv[1] not in os.environ


def test_ab_prints_the_lines_of_the_shell_loops(monkeypatch, capsys):
    record = {"kernel_ms": {"ofdm": 0.25, "prologue_tbcrc_scrambling_seq": 0.5, "codeblock_dmrs_zerofill": 1.0}, "value": 1234567.8,
              "verified_vs_oracle": True, "ms_per_step": 2.0}

    def last_line_of_each(steps, log_dir, report):
        for label, _, _, _ in steps[:1]:
            report(label, json.dumps(record))
        return 0

    monkeypatch.setattr(harness, "run_steps", last_line_of_each)
    monkeypatch.delenv("BENCH_ARGS", raising=False)
    ab.main(["lib", "1", "a.so"])
    ab.main(["env", "KNOB"])
    ab.main(["slots"])
    ab.main(["ofdm-parts"])
    ab.main(["stages"])
    assert capsys.readouterr().out.split("\n")[:5] == [
        "a.so %s 1234568 True" % record["kernel_ms"], "KNOB=0 %s 1234568" % record["kernel_ms"],
        "slots    64  value 1.2346 M/s  us per slot: prologue 7.8125 codeblock 15.6250 ofdm 3.9062  step 31.2500",
        "probe 0  ofdm 0.25 step 2.0", "stage 10 %s 1234568" % record["kernel_ms"]]


class FakeClock:
    """Stands in for the events: every launch costs what `cost` says, and the clock reads the sum since start()."""
    log = []
    now = 0.0

    def __init__(self, stream):
        self.t0 = None

    def start(self):
        self.t0 = FakeClock.now
        FakeClock.log.append("start")

    def elapsed_ms(self):
        FakeClock.log.append("stop")
        return FakeClock.now - self.t0


@pytest.fixture
def fake_clock(monkeypatch):
    monkeypatch.setattr(harness, "Clock", FakeClock)
    FakeClock.log, FakeClock.now = [], 0.0

    def launch(name, cost):
        def run():
            FakeClock.log.append(name)
            FakeClock.now += cost
        return run
    return launch


def test_time_rounds_is_round_major_and_divides_by_iters(fake_clock):
    launches = {"b": fake_clock("b", 3.0), "a": fake_clock("a", 0.5), "c": fake_clock("c", 1.25)}
    ms = harness.time_rounds(launches, None, rounds=2, iters=4)
    assert FakeClock.log == (["start"] + ["b"] * 4 + ["stop"] + ["start"] + ["a"] * 4 + ["stop"] + ["start"] + ["c"] * 4 + ["stop"]) * 2
    assert list(ms) == ["b", "a", "c"] and ms == {"b": [3.0, 3.0], "a": [0.5, 0.5], "c": [1.25, 1.25]}


def test_spread_is_the_median_min_and_max_to_five_places():
    assert harness.spread([0.1234567, 0.3000049, 0.2000051]) == (0.20001, 0.12346, 0.3)
    assert harness.spread([4.0, 1.0, 2.0, 3.0]) == (2.5, 1.0, 4.0)


def test_settle_stops_at_min_ms_and_at_the_cap(fake_clock):
    assert harness.settle({"x": fake_clock("x", 4.0), "y": fake_clock("y", 3.0)}, None) == 5  # 7 ms a pass: 35 >= 30 after five
    assert FakeClock.log.count("x") == 5 and FakeClock.log.count("y") == 5 and FakeClock.log.count("start") == 1
    assert harness.settle([fake_clock("x", 4.0)], None, min_ms=8.0) == 2
    assert harness.settle([fake_clock("z", 0.0)], None) == 2000  # the clock never gets there
    assert harness.settle([fake_clock("z", 0.0)], None, cap=7) == 7


@pytest.mark.parametrize("script", BENCH_SCRIPTS, ids=[os.path.basename(s) for s in BENCH_SCRIPTS])
def test_bench_script_answers_help_without_a_device_or_a_library(script, monkeypatch):
    monkeypatch.setattr(sys, "argv", [script, "--help"])
    monkeypatch.setattr(sys, "path", list(sys.path))
    monkeypatch.setenv("NRPHY_LIB_SO", "/nonexistent/libmi355nrphy.so")
    text = io.StringIO()
    with contextlib.redirect_stdout(text), pytest.raises(SystemExit) as stop:
        runpy.run_path(script, run_name="__main__")
    assert stop.value.code == 0 and "--help" in text.getvalue()


def test_the_bench_scripts_leave_timing_and_limits_to_the_harness():
    assert len(BENCH_SCRIPTS) == 19
    for script in BENCH_SCRIPTS:
        if os.path.basename(script) == "rx_chain_bench.py":
            continue  # bench.py imports it: it is part of how pull requests are measured and stays as it is
        text = open(script).read()
        assert "elapsed_time(" not in text and not re.search(r"""["']timeout["']""", text) and "subprocess" not in text, script
        assert "bench_harness" in text, script


@pytest.mark.gpu
def test_harness_times_one_srs_run_with_real_events(gpu_ctx):
    """One SRS, one symbol, one antenna port, one receive port on a 52-PRB grid of 4 ports (the M = 156 case of
    tests/test_srs_estimator.py's synthetic grids)."""
    import math
    import torch
    abi, lib = backends.abi, backends.pkg.lib
    nof_ports, nof_subc = 4, 12 * 52
    cfg = abi.make_srs(configuration_index=14, comb_size=4, comb_offset=2, start_symbol=2, numerology=1, sequence_id=30, rx_ports=(3,))
    plan = lib.SrsPlan(gpu_ctx, [cfg], [0], 1, nof_ports, nof_subc)
    d_grid = torch.randn((1, nof_ports, 14, nof_subc, 2), device="cuda").to(torch.bfloat16).view(torch.int32)
    d_grid = d_grid.reshape(1, nof_ports, 14, nof_subc).contiguous()
    d_result = torch.zeros(208 // 4, dtype=torch.int32, device="cuda")  # one nrphy_srs_result_t
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize()
    launches = {"srs": lambda: plan.run(d_grid, d_result, stream=sp), "srs_again": lambda: plan.run(d_grid, d_result, stream=sp)}
    rate = harness.copy_rate(stream)
    count = harness.settle(launches, stream, min_ms=5.0, cap=500)
    ms = harness.time_rounds(launches, stream, rounds=2, iters=2)
    plan.close()
    assert math.isfinite(rate) and rate > 0
    assert 1 <= count <= 500
    assert list(ms) == ["srs", "srs_again"] and all(len(v) == 2 for v in ms.values())
    assert all(math.isfinite(t) and t > 0 for v in ms.values() for t in v)
    assert all(math.isfinite(x) and x > 0 for v in ms.values() for x in harness.spread(v))
