#!/usr/bin/env python3
"""Secondary measurement ("next" row): OFDM demodulator throughput at the config-3 numerology
(FFT 4096, 273 PRB, 4 ports), inputs resident in HBM.  One GPU step in a child process under a time limit: untimed launches until
the clocks have had about 30 ms of load, then rounds timed with HIP events on an explicit stream, median and spread
(profiles/bench_harness.py), next to the rate of a device-to-device copy measured in the same process.  Usage (GPU box,
repository root): python3 profiles/demod_bench.py [--slots 1024]"""
import os
import sys

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def step(rounds, iters, out, slots):
    import torch
    import backends
    import cases
    lib = backends.pkg.lib
    ctx = lib.Context(0)
    _, ports, subc, cfg = cases.baseline_config(3)
    plan = lib.OfdmPlan(ctx, cfg, ports)
    d_iq = torch.randn((slots, ports, plan.slot_stride, 2), dtype=torch.float32, device="cuda")
    d_grid = torch.zeros((slots, ports, 14, subc), dtype=torch.int32, device="cuda")
    d_slot = torch.tensor([i % 2 for i in range(slots)], dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()  # an explicit stream: a null handle would select the context's own stream
    torch.cuda.synchronize()
    copy_gbs = harness.copy_rate(s)
    launch = lambda: plan.demod_run(slots, d_iq, d_grid, d_slot_index=d_slot, stream=s.cuda_stream)
    settle = harness.settle([launch], s)
    ms, ms_min, ms_max = harness.spread(harness.time_rounds({"demod": launch}, s, rounds, iters)["demod"])
    nbytes = slots * ports * (plan.slot_stride * 8 + 14 * subc * 4)
    print("ofdm_demod_kernel<4096>: %.4f ms per %d slots -> %.0f k slots/s, %.1f GB/s (%.1f %% of 8 TB/s); median of %d rounds of %d "
          "(min %.4f, max %.4f) after %d settling launches; device-to-device copy %.1f GB/s" % (
              ms, slots, slots / ms, nbytes / ms / 1e6, nbytes / ms / 1e6 / 80.0, rounds, iters, ms_min, ms_max, settle, copy_gbs))


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=15, iters=20, timeout=30, out="", slots=1024)))
