#!/usr/bin/env python3
"""PRACH detector throughput (nrphy_prach_run): 1024 occasions per launch on 4 receive ports, format 0 at zeroCorrelationZone 0
(64 root sequences per occasion, the worst case) and format B4 (15 kHz) at zeroCorrelationZone 11, timed with HIP events on an
explicit stream after warm-up, inputs resident in HBM, with and without the metric output.  The occasions are unit-variance
noise; every eighth carries one preamble.  Where the table's row for a configuration is red its threshold and margin are passed
as the caller's.  After the timed region one occasion is checked against the NumPy restatement (tests/prach_model.py).
Writes profiles/prach_detect_bench.json.  Usage (GPU box, repository root): python3 profiles/prach_detect_bench.py [--n 1024]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prach_detect_bench.json"))
    args = ap.parse_args()
    import torch
    import backends
    import prach_model as model
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    n, ports = args.n, 4
    rng = np.random.default_rng(0)
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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
        for key, met in (("ms_per_launch", None), ("ms_per_launch_with_metric", d_met)):
            torch.cuda.synchronize()
            for _ in range(3):
                plan.run(d_x, d_res, d_pre, met, stream=sp)
            e0.record(s)
            for _ in range(args.iters):
                plan.run(d_x, d_res, d_pre, met, stream=sp)
            e1.record(s)
            torch.cuda.synchronize()
            rec[key] = round(e0.elapsed_time(e1) / args.iters, 4)
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
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    main()
