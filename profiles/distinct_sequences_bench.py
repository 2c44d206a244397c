#!/usr/bin/env python3
"""The case bench.py cannot make: a batch in which no two PDUs share a sequence -- 1024 config-3 PDUs with distinct RNTIs (1024
scrambling sequences) in 1024 distinct (slot, DM-RS identity) pairs (1024 DM-RS sets).  Times plan.run (PDSCH only) with HIP
events around its launches; the library under test through NRPHY_LIB_SO, as in profiles/ab_variants.sh.

    python3 profiles/distinct_sequences_bench.py [STEPS] [WARMUP]        (GPU box, repository root; defaults 50 and 30)

Prints one JSON line: average ms of the prologue and the codeblock launch, ms per run, and the plan's sequence counts (where
the library reports them)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import backends  # noqa: E402
import cases  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 30
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
torch.cuda.synchronize()
for _ in range(warmup):
    plan.run(d_tb, d_grid)
ctx.synchronize()
plan.enable_timing(steps)
t0 = time.perf_counter()
for _ in range(steps):
    plan.run(d_tb, d_grid)
ctx.synchronize()
t1 = time.perf_counter()
ms, runs = plan.kernel_times()
out = {"pdus": n, "steps": steps, "warmup": warmup, "prologue_ms": round(ms[0], 4), "codeblock_ms": round(ms[1], 4),
       "run_ms_events": round(ms[3], 4), "ms_per_run_wall": round(1e3 * (t1 - t0) / steps, 4), "timed_runs": runs}
if hasattr(plan, "nof_sequences") and getattr(ctx.lib, "nrphy_pdsch_plan_nof_sequences", None) is not None:
    out["nof_sequences"] = plan.nof_sequences
if getattr(ctx.lib, "nrphy_pdsch_plan_scrambling_form", None) is not None:
    out["scrambling_form"] = plan.scrambling_form
print(json.dumps(out))
