#!/usr/bin/env python3
"""PRACH detector throughput (nrphy_prach_run): 1024 occasions per launch on 4 receive ports, format 0 at zeroCorrelationZone 0
(64 root sequences per occasion, the worst case) and format B4 (15 kHz) at zeroCorrelationZone 11, inputs resident in HBM, with and
without the metric output.  One GPU step in a child process under a time limit; per format untimed launches until the clocks have
had about 30 ms of load, then the two launches in alternating rounds timed with HIP events on an explicit stream, median and spread
(profiles/bench_harness.py), and the rate of a device-to-device copy measured in the same process.  The occasions are unit-variance
noise; every eighth carries one preamble.  Where the table's row for a configuration is red its threshold and margin are passed
as the caller's.  After the timed region one occasion is checked against the NumPy restatement (tests/prach_model.py).
Writes profiles/prach_detect_bench.json.  Usage (GPU box, repository root): python3 profiles/prach_detect_bench.py [--n 1024]"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def step(rounds, iters, out, n):
    import torch
    import backends
    import prach_model as model
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    ports = 4
    rng = np.random.default_rng(0)
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    copy_gbs = harness.copy_rate(s)
    records = []
    for fmt, scs, zcz in (("0", "1.25", 0), ("B4", "15", 11)):
        cfg = dict(format=fmt, ra_scs=scs, root_sequence_index=0, zero_correlation_zone=zcz, start_preamble_index=0,
                   nof_preamble_indices=64, nof_rx_ports=ports)
        th, margin, flag = model.thresholds()[(ports, scs, fmt, zcz)]
        if flag == "red":
            cfg.update(threshold=float(th), win_margin=margin)
        d = model.derive(cfg)
        L, nsym = d["L"], d["nof_symbols"]
        cfgs, x = [], np.zeros((n, ports, nsym, L), np.complex64)
        for i in range(n):
            c = dict(cfg, root_sequence_index=int(rng.integers(0, L - 1)))
            tx = [(int(rng.integers(0, 64)), 0.3 * d["max_delay"], 1.0)] if i % 8 == 0 else []
            x[i] = model.transmit(c, tx, rng, noise_std=1.0)
            cfgs.append(c)
        d_x = torch.from_numpy(x.view(np.float32)).cuda()
        plan = lib.PrachPlan(ctx, [abi.make_prach(**c) for c in cfgs], [i * ports * nsym * L for i in range(n)], nsym * L, L)
        d_res = torch.zeros((n, 24), dtype=torch.uint8, device="cuda")
        d_pre = torch.zeros((n, 64, 5), dtype=torch.int32, device="cuda")
        d_met = torch.zeros((n, 64, plan.metric_stride), dtype=torch.float32, device="cuda")
        rec = {"leg": "prach_detect", "format": fmt, "ra_scs_kHz": scs, "zero_correlation_zone": zcz, "rx_ports": ports, "n": n,
               "table_flag": flag, "root_sequences": d["nof_sequences"], "shifts_per_root": d["nof_shifts"],
               "window": d["win_width"], "transforms_per_launch": n * d["nof_sequences"] * ports,
               "input_bytes": int(x.nbytes)}
        launches = {"ms_per_launch": lambda: plan.run(d_x, d_res, d_pre, None, stream=sp),
                    "ms_per_launch_with_metric": lambda: plan.run(d_x, d_res, d_pre, d_met, stream=sp)}
        torch.cuda.synchronize()
        rec.update(rounds=rounds, iters=iters, settle_rounds=harness.settle(launches, s), copy_GBps=round(copy_gbs, 1))
        for key, ms in harness.time_rounds(launches, s, rounds, iters).items():
            rec[key], rec[key.replace("ms_per_launch", "ms_min")], rec[key.replace("ms_per_launch", "ms_max")] = harness.spread(ms)
        rec["us_per_occasion"] = round(rec["ms_per_launch"] * 1e3 / n, 3)
        rec["ns_per_transform"] = round(rec["ms_per_launch"] * 1e6 / rec["transforms_per_launch"], 2)
        # one occasion against the restatement, after the timed region
        i = 8 * (n // 24)
        m = model.detect(cfgs[i], x[i], np.float64)
        pre = d_pre[i].cpu().numpy()
        rec["check_detected_equal"] = bool([bool(v) for v in pre[:, 0]] == m["detected"])
        rec["check_delay_equal"] = bool([int(v) for v in pre[:, 1]] == m["delay"])
        got = d_met[i].cpu().numpy()[:, :d["win_width"]]
        rec["check_metric_rel_err"] = float(max((np.abs(got[k] - m["metric"][k]) / np.maximum(np.abs(m["metric"][k]), 1e-3)).max()
                                                for k in range(64)))
        print(json.dumps(rec), flush=True)
        records.append(rec)
        plan.close()
        del d_x, d_met
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=15, iters=20, timeout=30, out=os.path.join(ROOT, "profiles", "prach_detect_bench.json"),
                                               n=1024)))
