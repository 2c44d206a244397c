#!/usr/bin/env python3
"""nrphy_pusch_chest_run with Gold and with low-PAPR DM-RS on one batch shape: the shape of profiles/pusch_chest_bench.py restricted
to a size transform precoding allows -- 1024 PUSCHs of 270 PRB on 4 receive ports, 1 layer, DM-RS in symbols {2, 11}, inputs
resident in HBM, random grids (bf16 normal).  One GPU step per pilot source, each in a child process under a time limit; untimed
launches until the clocks have had about 30 ms of load, then rounds timed with HIP events on an explicit stream, median and spread
(profiles/bench_harness.py).  NRPHY_LIB_SO names another build of the library (the parent commit's, for its Gold figure; a variant,
for an A/B of the kernel); --pilots gold runs there too, for it uses nothing this commit added.  Usage (GPU box, repository root):
python3 profiles/pusch_lowpapr_measure.py [--pilots both|gold|lowpapr] [--n 1024] [--rounds 15] [--iters 20]"""
import ctypes as C
import json
import os
import sys

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
SOURCES = ("gold", "lowpapr")


def step(source, rounds, iters, out, n, pilots):
    import torch
    import backends
    lib, abi = backends.pkg.lib, backends.abi
    name = SOURCES[source - 1]
    if pilots not in ("both", name):
        return
    ctx = lib.Context(0)
    nprb, ports, dmrs = 270, 4, (2, 11)
    nsubc = 12 * 273
    torch.manual_seed(0)
    d_grid = torch.randn((n, ports, 14, nsubc, 2), device="cuda").to(torch.bfloat16).view(torch.int32).squeeze(-1).contiguous()
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    cfgs = [abi.make_pusch_chest(prbs=range(nprb), slot_index=i % 10, scrambling_id=i % 1008, scaling=1.4125, dmrs_symbols=dmrs,
                                 rx_ports=(0, 1, 2, 3), dc_position=nsubc // 2) for i in range(n)]
    ce_elems = ports * 14 * nsubc
    d_ce = torch.zeros(n * ce_elems, dtype=torch.int32, device="cuda")
    d_nv = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    d_meas = torch.zeros((n, 4, 2, 32), dtype=torch.uint8, device="cuda")
    lps = [abi.PuschChestLowpapr(1, i % 1008) for i in range(n)] if name == "lowpapr" else None
    plan = lib.PuschChestPlan(ctx, cfgs, list(range(n)), n, ports, nsubc, [i * ce_elems for i in range(n)], lowpapr=lps)
    torch.cuda.synchronize()
    chest = lambda: plan.run(d_grid, d_ce, d_nv, d_meas, stream=sp)
    settle = harness.settle([chest], s)
    ms, ms_min, ms_max = harness.spread(harness.time_rounds({"chest": chest}, s, rounds, iters)["chest"])
    rec = {"leg": "pusch_chest", "pilots": name, "library": os.environ.get("NRPHY_LIB_SO", "this commit"), "layers": 1,
           "dmrs_symbols": list(dmrs), "rx_ports": ports, "nof_prb": nprb, "n": n, "rounds": rounds, "iters": iters,
           "settle_launches": settle, "ms_per_launch": ms, "ms_min": ms_min, "ms_max": ms_max}
    print(json.dumps(rec), flush=True)
    plan.close()
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (1, 2), dict(rounds=15, iters=20, timeout=120, out=os.path.join(ROOT, "profiles", "pusch_lowpapr_measure.json"),
                                                   n=1024, pilots="both")))
