#!/usr/bin/env python3
"""What the EVM costs in the PUSCH demodulator.  Recorded, not gated.

The shapes are those of profiles/pusch_demod_bench.py: 1024 PUSCHs of 273 PRB, DM-RS in symbols 2 and 11 with two CDM groups
without data, 4 receive ports; 1 layer 256-QAM and 2 layers 64-QAM, ZF; random grids and estimates resident in HBM.

(1) plain: nrphy_pusch_demod_run (no EVM) for this library and for another build of it (--other-lib, the parent commit's: the
    kernels the call launches are the instantiation without EVM and must cost what they cost before).  The two libraries run in
    alternating processes through NRPHY_LIB_SO, twice each.
(2) evm: in one process of this library, nrphy_pusch_demod_run and nrphy_pusch_demod_run_evm with d_evm in alternating rounds: the
    added time is the difference of the two medians.  After the timed region the soft bits and SINRs of the two calls are compared
    (equal bytes) and the EVM of three PUSCHs is checked against tests/pusch_evm_model.py on the stand-alone device path.

HIP events on an explicit stream around rounds of launches, after about 30 ms of untimed load; median round and spread
(profiles/bench_harness.py).  Every measurement is one GPU step: a child process of its own under a time limit, and the next one
starts only if the one before ended well.  Appends one JSON record per figure to profiles/pusch_evm.txt.  (The script is not called
*_bench.py: tests/test_bench_harness.py counts those.)

    python3 profiles/pusch_evm_measure.py [--other-lib PATH] [--n 1024]           (GPU box, repository root)
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((1, 8), (2, 6))  # (layers, bits per symbol)


class Shape:
    """One shape's plan and device buffers."""

    def __init__(self, ctx, lib, abi, d_grid, n, layers, qm):
        import torch
        nprb, ports = 273, 4
        nsubc = 12 * nprb
        self.cfgs = [abi.make_pusch_demod(prbs=range(nprb), qm=qm, rnti=0x4601 + i, n_id=i % 1008, dmrs_symbols=(2, 11),
                                          nof_cdm_groups_without_data=2, nof_layers=layers, rx_ports=(0, 1, 2, 3), equalizer=abi.EQ_ZF)
                     for i in range(n)]
        self.ce_elems = layers * ports * 14 * nsubc
        self.d_ce = torch.randn((n * self.ce_elems, 2), device="cuda").to(torch.bfloat16).view(torch.int32).squeeze(-1).contiguous()
        self.nv = np.full((n, 4), 0.05, np.float32)
        self.d_nv = torch.from_numpy(self.nv).cuda()
        self.plan = lib.PuschDemodPlan(ctx, self.cfgs, list(range(n)), n, ports, nsubc, [i * self.ce_elems for i in range(n)])
        self.G = self.plan.codeword_bits(0)
        self.stride = (self.G + 63) & ~63
        self.d_grid = d_grid
        self.d_llr = torch.zeros((n, self.stride), dtype=torch.int8, device="cuda")
        self.d_sinr = torch.zeros(n, dtype=torch.float32, device="cuda")
        self.d_evm = torch.zeros(n, dtype=torch.float32, device="cuda")
        self.layers, self.qm, self.ports, self.nsubc = layers, qm, ports, nsubc
        torch.cuda.synchronize()

    def run(self, sp, evm):
        self.plan.run(self.d_grid, self.d_ce, self.d_nv, self.d_llr, self.stride, self.d_sinr, stream=sp,
                      d_evm=self.d_evm if evm else None)


def setup(n):
    import torch
    import backends
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    torch.manual_seed(0)
    d_grid = torch.randn((n, 4, 14, 12 * 273, 2), device="cuda").to(torch.bfloat16).view(torch.int32).squeeze(-1).contiguous()
    stream = torch.cuda.Stream()
    return torch, lib, abi, ctx, d_grid, stream, C.c_void_p(stream.cuda_stream)


def step_plain(label, rounds, iters, n):
    torch, lib, abi, ctx, d_grid, stream, sp = setup(n)
    out = []
    for layers, qm in SHAPES:
        s = Shape(ctx, lib, abi, d_grid, n, layers, qm)
        launch = lambda: s.plan.run(s.d_grid, s.d_ce, s.d_nv, s.d_llr, s.stride, s.d_sinr, stream=sp)  # the call the parent has too
        settle = harness.settle([launch], stream)
        ms, lo, hi = harness.spread(harness.time_rounds({"demod": launch}, stream, rounds, iters)["demod"])
        out.append(dict(leg="plain", library=label, layers=layers, qm=qm, n=n, rounds=rounds, iters=iters, settle_launches=settle,
                        ms=ms, ms_min=lo, ms_max=hi))
        s.plan.close()
        del s
        torch.cuda.empty_cache()
    return out


def step_evm(rounds, iters, n):
    import pusch_evm_model as model
    import pusch_tp_model as tp_model
    torch, lib, abi, ctx, d_grid, stream, sp = setup(n)
    out = []
    for layers, qm in SHAPES:
        s = Shape(ctx, lib, abi, d_grid, n, layers, qm)
        legs = {"without": lambda: s.run(sp, False), "with_evm": lambda: s.run(sp, True)}
        settle = harness.settle(legs, stream)
        ms = harness.time_rounds(legs, stream, rounds, iters)
        a, b = harness.spread(ms["without"]), harness.spread(ms["with_evm"])
        rec = dict(leg="evm", layers=layers, qm=qm, n=n, rounds=rounds, iters=iters, settle_launches=settle,
                   ms_without=a[0], ms_without_min=a[1], ms_without_max=a[2], ms_with_evm=b[0], ms_with_evm_min=b[1],
                   ms_with_evm_max=b[2], added_ms=round(b[0] - a[0], 5), added_share=round(b[0] / a[0] - 1, 4))
        # after the timed region: the two calls give the same soft bits and SINRs; three PUSCHs' EVM against the model
        s.run(sp, False)
        torch.cuda.synchronize()
        llr0, sinr0 = s.d_llr.clone(), s.d_sinr.clone()
        s.d_llr.zero_()
        s.d_sinr.zero_()
        torch.cuda.synchronize()  # the fills run on the default stream, the launches on `stream`
        s.run(sp, True)
        torch.cuda.synchronize()
        rec["check_same_soft_bits_and_sinr"] = bool(torch.equal(llr0, s.d_llr) and
                                                     torch.equal(sinr0.view(torch.int32), s.d_sinr.view(torch.int32)))
        worst = 0.0
        for i in (0, n // 3, n - 1):
            cfg = s.cfgs[i]
            grid = d_grid[i].cpu().numpy().view(np.uint32)
            ce = s.d_ce[i * s.ce_elems:(i + 1) * s.ce_elems].cpu().numpy().view(np.uint32).reshape(layers, s.ports, 14, s.nsubc)
            xs, softs = [], []
            for l in range(14):
                ks = tp_model.data_subcarriers(cfg, l)
                if ks.size == 0:
                    continue
                eq, ev = ctx.channel_equalize_host(cfg.equalizer, grid[:, l, ks], ce[:, :, l, ks], s.nv[i], 1.0)
                xs.append(eq.reshape(-1))
                softs.append(ctx.demodulate_soft_host(qm, eq.reshape(-1), ev.reshape(-1)))
            want = float(model.evm(qm, xs, softs)[1])
            got = float(s.d_evm[i].cpu())
            worst = max(worst, abs(got - want) / want / model.allowance(max(x.size for x in xs)))
        rec["check_evm_worst_share_of_allowance"] = round(worst, 4)
        out.append(rec)
        s.plan.close()
        del s
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="", help="run one step in this process (what the driver starts)")
    ap.add_argument("--label", default="this")
    ap.add_argument("--other-lib", default="", help="another build of the library to compare nrphy_pusch_demod_run with")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pusch_evm.txt"))
    args = ap.parse_args()
    if args.step:
        recs = step_plain(args.label, args.rounds, args.iters, args.n) if args.step == "plain" else step_evm(args.rounds, args.iters, args.n)
        with open(args.out, "a") as f:
            for r in recs:
                print(json.dumps(r), flush=True)
                f.write(json.dumps(r) + "\n")
        return 0
    common = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--iters", str(args.iters), "--n", str(args.n),
              "--out", args.out]
    steps = []
    libraries = ([("other", {"NRPHY_LIB_SO": os.path.abspath(args.other_lib)})] if args.other_lib else []) + [("this", {})]
    for turn in range(2):
        for label, env in libraries:
            steps.append(("pusch_evm_plain_%s_%d" % (label, turn), common + ["--step", "plain", "--label", label], env, args.timeout))
    steps.append(("pusch_evm_added", common + ["--step", "evm"], {}, args.timeout))
    return harness.run_steps(steps, harness.LOG_DIR)


if __name__ == "__main__":
    sys.exit(main())
