#!/usr/bin/env python3
"""A/B runs on ONE box (box-to-box variance is +-4 %): lists of bench.py or rx_chain_bench.py command lines, alternating between
what is compared, run as guarded steps (profiles/bench_harness.py): every run is a child of its own under a time limit, its
stderr is kept under build/bench_logs/, and after a run that faults, aborts or hangs nothing more starts on the card.  A run's
own output is passed through; after it comes one line made from the JSON line the run ends with.  GPU box, repository root:

    python3 profiles/ab.py lib ROUNDS a.so b.so ...   builds of libmi355nrphy.so (profiles/make_variant.sh), chosen through
                                                      NRPHY_LIB_SO: the product library in the tree is never touched.  bench.py
                                                      --full; BENCH_ARGS adds arguments.  The same library twice gives the A/A
                                                      spread a difference has to beat.
    python3 profiles/ab.py rx ROUNDS a.so b.so ...    the same with the receive chain (profiles/rx_chain_bench.py); RX_ARGS adds
                                                      arguments
    python3 profiles/ab.py env KNOB [ROUNDS]          bench.py without and with the environment knob KNOB=1, 3 rounds by default
    python3 profiles/ab.py slots [--wire]             slots per launch from 64 to 2048: kernel times per slot and whole-path rate as
                                                      the batch shrinks (does a grid that fits the 256 MB memory-side cache make the
                                                      OFDM launch's grid reads cheaper?)
    python3 profiles/ab.py stages                     wall time of the codeblock launch when its codeblock waves stop after stage n
                                                      (see stage_pmc.sh for the stages; 10 = every wave returns at once, 11 =
                                                      everything but the data-RE stores), at bench.py's default step counts;
                                                      STAGES="10 5 7" selects
    python3 profiles/ab.py ofdm-parts [--wire]        the OFDM launch by parts, NRPHY_OFDM_PROBE: buffer ranges set to zero so that
                                                      loads / stores do not reach memory: 0 = everything, 1 = no IQ stores, 2 = no
                                                      grid loads, 3 = neither (arithmetic + LDS only), twice; PROBES="0 3" selects

stages and ofdm-parts need the profiling variant of the library, NRPHY_LIB_SO or build/variants/probes.so:
    bash profiles/make_variant.sh probes "pdsch_kernels.hip ofdm_kernels.hip nrphy_host.cpp ofdm_host.cpp pdsch_host.cpp pdsch_plan_build.cpp" "-DNRPHY_PROBES"
--timeout SECONDS in front of the subcommand replaces the limit per run (profiles/bench_harness.txt has the measured times).
"""
import json
import os
import sys

import bench_harness as harness

BENCH = ["python3", "bench.py"]
QUIET = ["--no-cpu-baseline", "--no-secondary"]
LIMITS = {"lib": 30, "rx": 30, "env": 30, "slots": 30, "stages": 30, "ofdm-parts": 30}  # seconds per run (profiles/bench_harness.txt)


def kernel_line(tag, verified=None, places=None):
    def line(d):
        kernel_ms = d["kernel_ms"] if places is None else {k: round(x, places) for k, x in d["kernel_ms"].items()}
        return " ".join(str(v) for v in [tag, kernel_ms, round(d["value"])] + ([d.get(verified)] if verified else []))
    return line


def slots_line(s):
    def line(d):
        k = d["kernel_ms"]
        return "slots %5d  value %.4f M/s  us per slot: prologue %.4f codeblock %.4f ofdm %.4f  step %.4f" % (
            s, d["value"] / 1e6, k["prologue_tbcrc_scrambling_seq"] / s * 1e3, k["codeblock_dmrs_zerofill"] / s * 1e3, k["ofdm"] / s * 1e3,
            d["ms_per_step"] / s * 1e3)
    return line


def runs(argv):
    """-> [(argv, environment additions, function from the run's JSON record to the line printed)] of a subcommand."""
    what, rest = argv[0], argv[1:]
    probes = os.environ.get("NRPHY_LIB_SO") or os.path.join(os.getcwd(), "build", "variants", "probes.so")
    if what == "lib":
        cmd = BENCH + ["--full"] + QUIET + ["--steps", "20"] + os.environ.get("BENCH_ARGS", "").split()
        return [(cmd, {"NRPHY_LIB_SO": os.path.join(os.getcwd(), v)}, kernel_line(v, "verified_vs_oracle"))
                for _ in range(int(rest[0])) for v in rest[1:]]
    if what == "rx":
        cmd = ["python3", "profiles/rx_chain_bench.py"] + os.environ.get("RX_ARGS", "").split()
        return [(cmd, {"NRPHY_LIB_SO": os.path.join(os.getcwd(), v)}, kernel_line(v, "verified", 4))
                for _ in range(int(rest[0])) for v in rest[1:]]
    if what == "env":
        knob = rest[0]
        os.environ.pop(knob, None)  # steps add to this process's environment: the run without the knob must not inherit it
        return [(BENCH + QUIET + ["--steps", "20"], {knob: "1"} if on else {}, kernel_line("%s=%d" % (knob, on)))
                for _ in range(int(rest[1]) if len(rest) > 1 else 3) for on in (0, 1)]
    if what == "slots":
        extra = ["--wire"] if rest else []
        return [(BENCH + ["--slots", str(s), "--steps", str(51200 // s), "--warmup", str(51200 // s // 2 + 30)] + QUIET + extra, {}, slots_line(s))
                for s in (64, 128, 192, 256, 384, 512, 768, 1024, 2048)]
    if what == "stages":
        return [(BENCH + QUIET, {"NRPHY_LIB_SO": probes, "NRPHY_PROFILE_STAGE": st}, kernel_line("stage " + st))
                for st in os.environ.get("STAGES", "10 5 7 1 2 4 11 0").split()]
    if what == "ofdm-parts":
        return [(BENCH + QUIET + ["--steps", "20"] + rest, {"NRPHY_LIB_SO": probes, "NRPHY_OFDM_PROBE": pr},
                 lambda d, pr=pr: "probe %s  ofdm %s step %s" % (pr, d["kernel_ms"]["ofdm"], d["ms_per_step"]))
                for _ in (1, 2) for pr in os.environ.get("PROBES", "0 1 2 3").split()]


def main(argv):
    limit = None
    if argv[:1] == ["--timeout"]:
        limit, argv = int(argv[1]), argv[2:]
    if not argv or argv[0] not in LIMITS:
        sys.exit(__doc__)
    todo = runs(argv)
    lines = {"%s_%02d" % (argv[0], i): line for i, (_, _, line) in enumerate(todo)}
    steps = [(label, cmd, env, limit or LIMITS[argv[0]]) for label, (cmd, env, _) in zip(lines, todo)]
    return harness.run_steps(steps, harness.LOG_DIR, lambda label, last: print(lines[label](json.loads(last)), flush=True))


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
