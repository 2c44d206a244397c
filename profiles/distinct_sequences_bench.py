#!/usr/bin/env python3
"""The case bench.py cannot make: a batch in which no two PDUs share a sequence -- 1024 config-3 PDUs with distinct RNTIs (1024
scrambling sequences) in 1024 distinct (slot, DM-RS identity) pairs (1024 DM-RS sets).  Times plan.run (PDSCH only); the library
under test through NRPHY_LIB_SO, as in profiles/ab.py.

    python3 profiles/distinct_sequences_bench.py [--steps 50] [--warmup 30]        (GPU box, repository root)

One GPU step in a child process under a time limit.  After `--warmup` launches and untimed launches until the clocks have had
about 30 ms of load, `--steps` runs are timed by the plan's own events around its launches (average ms of the prologue and the
codeblock launch, ms per run) and by the host clock; then rounds of runs are timed with HIP events on the same explicit stream,
median and spread (profiles/bench_harness.py).  Prints one JSON line, with the plan's sequence counts where the library reports
them and the rate of a device-to-device copy measured in the same process."""
import json
import os
import sys
import time

import numpy as np

import bench_harness as harness

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def step(rounds, iters, out, steps, warmup):
    import torch
    import backends
    import cases
    n = 1024
    lib = backends.pkg.lib
    ctx = lib.Context(0)
    pdus = []
    for i in range(n):
        pdu, ports, subc, _ = cases.baseline_config(3, rnti=1 + i, slot_index=i % 20)
        pdu.scrambling_id = i // 20
        pdus.append(pdu)
    stride = (pdus[0].tb_size_bytes + 255) & ~255
    plan = lib.PdschPlan(ctx, pdus, [i * stride for i in range(n)], list(range(n)), n, ports, subc)
    d_tb = torch.from_numpy(np.random.default_rng(0).integers(0, 256, n * stride + 64, dtype=np.uint8)).cuda()
    d_grid = torch.zeros((n, ports, 14, subc), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    copy_gbs = harness.copy_rate(stream)
    launch = lambda: plan.run(d_tb, d_grid, stream=stream.cuda_stream)
    for _ in range(warmup):
        launch()
    settle = harness.settle([launch], stream)
    plan.enable_timing(steps)
    t0 = time.perf_counter()
    for _ in range(steps):
        launch()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ms, runs = plan.kernel_times()
    rec = {"pdus": n, "steps": steps, "warmup": warmup, "prologue_ms": round(ms[0], 4), "codeblock_ms": round(ms[1], 4),
           "run_ms_events": round(ms[3], 4), "ms_per_run_wall": round(1e3 * (t1 - t0) / steps, 4), "timed_runs": runs}
    med, ms_min, ms_max = harness.spread(harness.time_rounds({"run": launch}, stream, rounds, iters)["run"])
    rec.update(rounds=rounds, iters=iters, settle_launches=settle, ms_per_run=med, ms_min=ms_min, ms_max=ms_max, copy_GBps=round(copy_gbs, 1))
    if hasattr(plan, "nof_sequences") and getattr(ctx.lib, "nrphy_pdsch_plan_nof_sequences", None) is not None:
        rec["nof_sequences"] = plan.nof_sequences
    if getattr(ctx.lib, "nrphy_pdsch_plan_scrambling_form", None) is not None:
        rec["scrambling_form"] = plan.scrambling_form
    print(json.dumps(rec), flush=True)
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=15, iters=20, timeout=30, out="", steps=50, warmup=30)))
