#!/usr/bin/env python3
"""PUSCH DM-RS channel estimator throughput (nrphy_pusch_chest_run): 1024 PUSCHs of 273 PRB on 4 receive ports, 1 and 2 layers,
DM-RS in symbols {2, 11} and {2, 7, 11}, inputs resident in HBM; then the estimator followed by nrphy_pusch_demod_run (grid to soft
bits, the demodulator reading the estimator's output).  One GPU step in a child process under a time limit; per shape untimed
launches until the clocks have had about 30 ms of load, then rounds timed with HIP events on an explicit stream, median and spread
(profiles/bench_harness.py); the copy rate is measured in the same process, next to the 6.29 TB/s constant of earlier records.  The grids
are random (bf16 normal).  After the timed region one PUSCH is checked against the NumPy restatement (tests/pusch_chest_model.py).
Algorithmic bytes: the DM-RS RE read (twice: LS and noise passes) and the estimate written.  Usage (GPU box, repository root):
python3 profiles/pusch_chest_bench.py [--n 1024] [--rounds 15] [--iters 20]"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_COPY = 6.29e12


def step(rounds, iters, out, n):
    import torch
    import backends
    import pusch_chest_model as model
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    nprb, ports = 273, 4
    nsubc = 12 * nprb
    torch.manual_seed(0)
    d_grid = torch.randn((n, ports, 14, nsubc, 2), device="cuda").to(torch.bfloat16).view(torch.int32).squeeze(-1).contiguous()
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    copy_gbs = harness.copy_rate(s)
    records = []
    for layers in (1, 2):
        for dmrs in ((2, 11), (2, 7, 11)):
            cfgs = [abi.make_pusch_chest(prbs=range(nprb), slot_index=i % 10, scrambling_id=i % 1008, scaling=1.4125,
                                         dmrs_symbols=dmrs, nof_layers=layers, rx_ports=(0, 1, 2, 3), dc_position=nsubc // 2)
                    for i in range(n)]
            ce_elems = layers * ports * 14 * nsubc
            d_ce = torch.zeros(n * ce_elems, dtype=torch.int32, device="cuda")
            d_nv = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            d_meas = torch.zeros((n, 4, 2, 32), dtype=torch.uint8, device="cuda")
            plan = lib.PuschChestPlan(ctx, cfgs, list(range(n)), n, ports, nsubc, [i * ce_elems for i in range(n)])
            torch.cuda.synchronize()
            chest = lambda: plan.run(d_grid, d_ce, d_nv, d_meas, stream=sp)
            settle = harness.settle([chest], s)
            ms, ms_min, ms_max = harness.spread(harness.time_rounds({"chest": chest}, s, rounds, iters)["chest"])
            write = n * ce_elems * 4
            read = n * ports * len(dmrs) * 6 * nprb * 4 * 2
            nbytes = write + read
            rec = {"leg": "pusch_chest", "layers": layers, "dmrs_symbols": list(dmrs), "rx_ports": ports, "nof_prb": nprb, "n": n,
                   "rounds": rounds, "iters": iters, "settle_launches": settle,
                   "ms_per_launch": ms, "ms_min": ms_min, "ms_max": ms_max, "copy_GBps": round(copy_gbs, 1),
                   "algorithmic_bytes": nbytes, "estimate_bytes": write,
                   "GBps": round(nbytes / ms / 1e6, 1), "frac_copy_6p29TBps": round(nbytes / ms / 1e-3 / HBM_COPY, 3),
                   "floor_ms_at_copy_rate": round(nbytes / HBM_COPY * 1e3, 4)}
            # estimator + demodulator back to back (grid to soft bits)
            qm = 8 if layers == 1 else 6
            dcfgs = [abi.make_pusch_demod(prbs=range(nprb), qm=qm, rnti=0x4601 + i, n_id=i % 1008, dmrs_symbols=dmrs,
                                          nof_cdm_groups_without_data=2, nof_layers=layers, rx_ports=(0, 1, 2, 3),
                                          equalizer=abi.EQ_ZF) for i in range(n)]
            dplan = lib.PuschDemodPlan(ctx, dcfgs, list(range(n)), n, ports, nsubc, [i * ce_elems for i in range(n)])
            G = dplan.codeword_bits(0)
            stride = (G + 63) & ~63
            d_llr = torch.zeros((n, stride), dtype=torch.int8, device="cuda")
            def both():
                chest()
                dplan.run(d_grid, d_ce, d_nv, d_llr, stride, None, stream=sp)

            harness.settle([both], s)
            rec["chest_plus_demod_ms"] = harness.spread(harness.time_rounds({"both": both}, s, rounds, max(2, iters // 2))["both"])[0]
            dplan.close()
            del d_llr
            # one PUSCH against the restatement, after the timed region
            plan.run(d_grid, d_ce, d_nv, d_meas, stream=sp)
            torch.cuda.synchronize()
            i = n // 3
            grid = d_grid[i].cpu().numpy().view(np.uint32)
            want_ce, want_nv, _ = model.estimate(cfgs[i], grid)
            got = d_ce[i * ce_elems:(i + 1) * ce_elems].cpu().numpy().view(np.uint32).reshape(layers, ports, 14, nsubc)
            rec["check_words_equal_frac"] = float(np.mean(got[:, :, 0:14] == want_ce[:, :, 0:14]))
            rec["check_noise_var_rel_err"] = float(np.max(np.abs(d_nv[i].cpu().numpy() - want_nv) / want_nv))
            print(json.dumps(rec), flush=True)
            records.append(rec)
            plan.close()
            del d_ce
            torch.cuda.empty_cache()


    with open(out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=15, iters=20, timeout=30, out=os.path.join(ROOT, "profiles", "pusch_chest_bench.json"),
                                               n=1024)))
