#!/usr/bin/env python3
"""Times nrphy_llr_descramble on the receive-side bench shape (64 codewords of the 100 MHz / 4-layer / 256-QAM slot,
1,362,816 soft bits each).  One GPU step in a child process under a time limit: untimed launches until the clocks have had about
30 ms of load, then rounds timed with HIP events on the launch stream, median and spread (profiles/bench_harness.py), next to the
rate of a device-to-device copy measured in the same process.
Usage: python3 profiles/descramble_bench.py [--n-cw 64] [--iters 50]"""
import importlib
import json
import os
import sys

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step(rounds, iters, out, n_cw):
    import torch
    lib = importlib.import_module("srsran-edgeric-5g_amd.lib")
    length = 273 * 12 * 13 * 8 * 4
    stride = (length + 255) // 256 * 256
    ctx = lib.Context(0)
    rng = np.random.default_rng(1)
    d_ci = torch.from_numpy(rng.integers(0, 1 << 31, n_cw).astype(np.int32)).cuda()
    d_in = torch.from_numpy(rng.integers(-127, 128, (n_cw, stride)).astype(np.int8)).cuda()
    d_out = torch.empty_like(d_in)
    stream = torch.cuda.Stream()  # a real stream: 0 would select the context's own stream, which the events do not see
    torch.cuda.synchronize()
    copy_gbs = harness.copy_rate(stream)
    launch = lambda: ctx.llr_descramble(d_ci, n_cw, length, d_in, stride, d_out, stride, stream.cuda_stream)
    settle = harness.settle([launch], stream)
    ms, ms_min, ms_max = harness.spread(harness.time_rounds({"descramble": launch}, stream, rounds, iters)["descramble"])
    rec = {"kernel": "llr_descramble_kernel", "codewords": n_cw, "soft_bits_each": length, "rounds": rounds, "iters": iters,
           "settle_launches": settle, "ms_per_launch": ms, "ms_min": ms_min, "ms_max": ms_max, "soft_bits_per_sec": n_cw * length / ms * 1e3,
           "algorithmic_bytes_per_launch": 2 * n_cw * length, "GB_per_s": round(2 * n_cw * length / ms / 1e6, 1),
           "hbm_frac": round(2 * n_cw * length / ms / 1e6 / 8000, 3), "copy_GBps": round(copy_gbs, 1)}
    print(json.dumps(rec), flush=True)
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=15, iters=50, timeout=30, out="", n_cw=64)))
