#!/usr/bin/env python3
"""SRS channel estimator latency (nrphy_srs_run): batches of 1, 16 and 64 SRS of the largest shape -- 4 antenna ports x 4 receive
ports, 4 symbols, 272 PRB with comb 2 (M = 1632) --, every SRS on a received grid of its own, inputs resident in HBM.

Every batch size is one GPU step: a child process of its own under a time limit, and the next one starts only if the one before
ended well.  A step builds the plan, runs untimed launches until the engine clocks have had about 30 ms of load, then times rounds
of launches with HIP events on an explicit stream and reports the median round and the spread.  A run is two launches of 16
workgroups per SRS; the grid words it reads (each twice: once per launch) are set against the rate of a device-to-device copy
measured in the same process, though at these sizes the run is bound by latency, not by bytes.  After the timed region the first
SRS, whose grid carries a real transmission, is checked against the NumPy restatement (tests/srs_model.py).  Hardware counters
are not collected here.  Writes profiles/srs_bench.json.

    python3 profiles/srs_bench.py            (GPU box, repository root)
"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = (1, 16, 64)
PORTS, NOF_PRB, SYMBOLS = 4, 272, 4
NOF_SUBC = 12 * NOF_PRB
RESULT_BYTES = 208  # nrphy_srs_result_t


def step(n, rounds, iters, out):
    import torch
    import backends
    import srs_model as model
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    rng = np.random.default_rng(0)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    cfg = abi.make_srs(configuration_index=63, comb_size=2, nof_antenna_ports=4, nof_symbols=SYMBOLS, start_symbol=14 - SYMBOLS,
                       cyclic_shift=1, sequence_id=321, numerology=1, rx_ports=tuple(range(PORTS)))
    M = lib.srs_info(cfg, 0)["sequence_length"]
    gains = (0.5 + rng.random((PORTS, 4))) * np.exp(2j * np.pi * rng.random((PORTS, 4)))
    first = model.transmit(cfg, PORTS, NOF_SUBC, gains, delay_bins=5, noise_std=0.1, rng=rng)
    g = torch.randn((n, PORTS, 14, NOF_SUBC, 2), device="cuda", dtype=torch.float32) * (0.5 ** 0.5)
    d_grid = g.to(torch.bfloat16).view(torch.int32).reshape(n, PORTS, 14, NOF_SUBC).contiguous()
    del g
    d_grid[0] = torch.from_numpy(first.view(np.int32)).cuda()
    plan = lib.SrsPlan(ctx, [cfg] * n, list(range(n)), n, PORTS, NOF_SUBC)
    d_result = torch.zeros(n * RESULT_BYTES // 4, dtype=torch.int32, device="cuda")
    launch = lambda: plan.run(d_grid, d_result, stream=sp)
    copy_gbs = harness.copy_rate(stream)
    settle = harness.settle([launch], stream)  # about 30 ms of load before anything is timed
    ms = harness.time_rounds({"srs": launch}, stream, rounds, iters)["srs"]
    med = float(np.median(ms))
    ms_med, ms_min, ms_max = harness.spread(ms)
    nbytes = n * (2 * 16 * SYMBOLS * M * 4 + RESULT_BYTES)  # every path reads its grid words in both launches
    rec = {"leg": "srs", "n": n, "antenna_ports": 4, "rx_ports": PORTS, "nof_symbols": SYMBOLS, "nof_prb": NOF_PRB, "comb": 2, "M": M,
           "workgroups_per_launch": 16 * n, "launches_per_run": 2, "rounds": rounds, "iters": iters, "settle_launches": settle,
           "ms_per_run": ms_med, "ms_min": ms_min, "ms_max": ms_max, "us_per_srs": round(med * 1e3 / n, 2),
           "srs_per_s": round(n / (med * 1e-3)), "bytes_per_run": nbytes, "GBps": round(nbytes / (med * 1e-3) / 1e9, 2),
           "copy_GBps": round(copy_gbs, 1), "counters": "not measured"}
    torch.cuda.synchronize()
    got = d_result[:RESULT_BYTES // 4].cpu().numpy().tobytes()
    want = model.estimate(cfg, first)
    h = np.frombuffer(got, np.float32, 32).reshape(2, 4, 4)
    bins = np.frombuffer(got, np.int32, 16, 128).reshape(4, 4)
    rec["check_first_srs"] = {"ta_bins_equal": bool(np.array_equal(bins, want["ta_bins"])),
                              "h_error_over_rms_lse": float(np.abs(h[0] + 1j * h[1] - want["h"]).max() / want["lse_rms"])}
    print(json.dumps(rec), flush=True)
    plan.close()
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, SIZES, dict(rounds=15, iters=20, timeout=120, out=os.path.join(ROOT, "profiles", "srs_bench.json"))))
