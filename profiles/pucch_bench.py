#!/usr/bin/env python3
"""PUCCH receiver throughput (nrphy_pucch_run): 1,024 and 16,384 PUCCHs per launch on 4 receive ports -- format 1 with 14 symbols
without and with frequency hopping, and format 0 with 2 symbols (2 ACK bits and an SR opportunity: 8 candidates) --, 16 PUCCHs
per received grid on PRBs of their own, inputs resident in HBM.

Every batch size is one GPU step: a child process of its own under a time limit, and the next one starts only if the one before
ended well.  A step builds the three plans, runs untimed launches until the engine clocks have had about 30 ms of load (what
bench.py's --settle does), then times the plans in alternating rounds with HIP events on an explicit stream and reports the
median round and the spread.  The bytes a launch has to move (grid rows read, descriptors read, records written) are set
against the rate of a device-to-device copy measured in the same process.  After the timed region the PUCCHs of the first grid,
which carry real transmissions, are checked against the NumPy restatement (tests/pucch_model.py).  Hardware counters are not
collected here.  Writes profiles/pucch_bench.json.

    python3 profiles/pucch_bench.py            (GPU box, repository root)
"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = (1024, 16384)
PORTS, NOF_PRB, PER_GRID = 4, 52, 16
NOF_SUBC = 12 * NOF_PRB
RESULT_BYTES, DESC_BYTES = 40, 88  # nrphy_pucch_result_t, the plan's descriptor


def legs(model):
    base = dict(bwp_start_rb=0, bwp_size_rb=NOF_PRB, slot_index=3, n_id=77, ports=tuple(range(PORTS)))
    return [("format1_14sym", lambda prb: model.make_cfg(1, prb, 14, 0, nof_harq_ack=2, time_domain_occ=1, initial_cyclic_shift=prb % 12,
                                                         **base), 14),
            ("format1_14sym_hopping", lambda prb: model.make_cfg(1, prb, 14, 0, second_hop_prb=prb + 1, nof_harq_ack=2,
                                                                 time_domain_occ=1, initial_cyclic_shift=prb % 12, **base), 14),
            ("format0_2sym", lambda prb: model.make_cfg(0, prb, 2, 12, nof_harq_ack=2, sr_opportunity=True,
                                                        initial_cyclic_shift=prb % 12, **base), 2)]


def step(n, rounds, iters, out):
    import torch
    import backends
    import pucch_model as model
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    n_grids = n // PER_GRID
    rng = np.random.default_rng(0)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    # Unit-variance noise in every grid; the first grid of every leg also carries its 16 UEs at 6 dB.
    noise = torch.randn((n_grids, PORTS, 14, NOF_SUBC, 2), device="cuda", dtype=torch.float32) * (0.5 ** 0.5)
    runs = []
    for name, make, nsym in legs(model):
        cfgs = [make(3 * (i % PER_GRID)) for i in range(n)]
        first = np.zeros((PORTS, 14, NOF_SUBC), complex)
        sent = []
        for i in range(PER_GRID):
            bits = [int(b) for b in rng.integers(0, 2, 2)]
            sr = int(rng.integers(0, 2))
            model.add_to_grid(first, model.transmit(cfgs[i], bits, sr), [2.0 * np.exp(1j * (0.4 + p)) for p in range(PORTS)], delay=2.0)
            sent.append((bits, sr))
        g = noise.clone()
        g[0] += torch.from_numpy(np.stack([first.real, first.imag], axis=-1).astype(np.float32)).cuda()
        d_grid = g.to(torch.bfloat16).view(torch.int32).reshape(n_grids, PORTS, 14, NOF_SUBC).contiguous()
        del g
        plan = lib.PucchPlan(ctx, [model.to_abi(abi, c) for c in cfgs], [i // PER_GRID for i in range(n)], n_grids, PORTS, NOF_SUBC)
        d_res = torch.zeros((n, RESULT_BYTES // 4), dtype=torch.int32, device="cuda")
        rows = PORTS * nsym * 48
        runs.append(dict(name=name, plan=plan, grid=d_grid, res=d_res, cfgs=cfgs, sent=sent,
                         bytes=n * (rows + DESC_BYTES + RESULT_BYTES)))
    del noise
    copy_gbs = harness.copy_rate(stream)
    launches = {r["name"]: (lambda r=r: r["plan"].run(r["grid"], r["res"], stream=sp)) for r in runs}
    settle = harness.settle(launches, stream)  # about 30 ms of load before anything is timed
    times = harness.time_rounds(launches, stream, rounds, iters)  # alternating: every round times every leg once
    records = []
    for r in runs:
        ms = float(np.median(times[r["name"]]))
        ms_med, ms_min, ms_max = harness.spread(times[r["name"]])
        rec = {"leg": "pucch", "case": r["name"], "n": n, "rx_ports": PORTS, "pucch_per_grid": PER_GRID, "rounds": rounds, "iters": iters,
               "settle_launches": settle, "ms_per_launch": ms_med, "ms_min": ms_min, "ms_max": ms_max,
               "pucch_per_s": round(n / (ms * 1e-3)), "ns_per_pucch": round(ms * 1e6 / n, 2), "bytes_per_launch": r["bytes"],
               "GBps": round(r["bytes"] / (ms * 1e-3) / 1e9, 2), "copy_GBps": round(copy_gbs, 1),
               "share_of_copy_rate": round(r["bytes"] / (ms * 1e-3) / 1e9 / copy_gbs, 4), "counters": "not measured"}
        # the first grid's PUCCHs against the restatement, after the timed region
        got = r["res"][:PER_GRID].cpu().numpy().view(model.RESULT_DTYPE).reshape(-1)
        words = r["grid"][0].cpu().numpy().view(np.uint32)
        ok_bits = ok_model = 0
        for i in range(PER_GRID):
            want = model.process(r["cfgs"][i], words, np.float32)
            bits, sr = r["sent"][i]
            ok_bits += int(got[i]["status"] == 1 and list(got[i]["harq_ack"]) == bits and (r["cfgs"][i]["format"] == 1 or got[i]["sr"] == sr))
            ok_model += int(got[i]["status"] == want["status"] and list(got[i]["harq_ack"]) == want["harq_ack"] and
                            abs(float(got[i]["detection_metric"]) - float(want["metric"])) <= 1e-3 * abs(float(want["metric"])))
        rec["check_sent_bits_returned"] = "%d of %d" % (ok_bits, PER_GRID)
        rec["check_equal_restatement"] = "%d of %d" % (ok_model, PER_GRID)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        r["plan"].close()
    with open(out, "a") as f:
        f.write("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, SIZES, dict(rounds=15, iters=20, timeout=240, out=os.path.join(ROOT, "profiles", "pucch_bench.json"))))
