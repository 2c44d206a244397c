#!/usr/bin/env python3
"""PUSCH demodulator throughput (nrphy_pusch_demod_run): 1024 PUSCHs of 273 PRB, DM-RS in symbols 2 and 11 with two CDM groups
without data (12 data symbols), 4 receive ports, in two shapes -- 1 layer 256-QAM (ZF) and 2 layers 64-QAM (ZF) --, inputs resident
in HBM; then the same launch followed by nrphy_pusch_decode_batch (grid to transport blocks).  One GPU step in a child process
under a time limit; per shape untimed launches until the clocks have had about 30 ms of load, then rounds timed with HIP events
on an explicit stream, median and spread (profiles/bench_harness.py); the copy rate is measured in the same process, next to the
6.3 TB/s constant of earlier records.  The grids and estimates are random (bf16 normal): the decoder sees noise-like soft bits,
so every codeblock runs its
full iteration count and that leg is the decoder's worst case.  After the timed region one PUSCH is checked against the composed
path (equaliser -> soft demodulator per OFDM symbol -> descrambler).  Usage (GPU box, repository root):
python3 profiles/pusch_demod_bench.py [--n 1024] [--rounds 15] [--iters 20]"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12
HBM_COPY = 6.3e12


def step(rounds, iters, out, n):
    import torch
    import backends
    import test_pusch_demodulator as t
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
    for layers, qm in ((1, 8), (2, 6)):
        cfgs = [abi.make_pusch_demod(prbs=range(nprb), qm=qm, rnti=0x4601 + i, n_id=i % 1008, dmrs_symbols=(2, 11),
                                     nof_cdm_groups_without_data=2, nof_layers=layers, rx_ports=(0, 1, 2, 3), equalizer=abi.EQ_ZF)
                for i in range(n)]
        ce_elems = layers * ports * 14 * nsubc
        d_ce = torch.randn((n * ce_elems, 2), device="cuda").to(torch.bfloat16).view(torch.int32).squeeze(-1).contiguous()
        nv = np.zeros((n, 4), np.float32)
        nv[:] = 0.05
        d_nv = torch.from_numpy(nv).cuda()
        plan = lib.PuschDemodPlan(ctx, cfgs, list(range(n)), n, ports, nsubc, [i * ce_elems for i in range(n)])
        G = plan.codeword_bits(0)
        stride = (G + 63) & ~63
        d_llr = torch.zeros((n, stride), dtype=torch.int8, device="cuda")
        d_sinr = torch.zeros(n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        demod = lambda: plan.run(d_grid, d_ce, d_nv, d_llr, stride, d_sinr, stream=sp)
        settle = harness.settle([demod], s)
        ms, ms_min, ms_max = harness.spread(harness.time_rounds({"demod": demod}, s, rounds, iters)["demod"])
        nre = G // (layers * qm)                    # data RE per PUSCH
        nbytes = n * (nre * ports * 4 * (1 + layers) + G + 4 * 4 + 4)
        rec = {"leg": "pusch_demod", "layers": layers, "qm": qm, "rx_ports": ports, "nof_prb": nprb, "n": n,
               "rounds": rounds, "iters": iters, "settle_launches": settle,
               "ms_per_launch": ms, "ms_min": ms_min, "ms_max": ms_max, "copy_GBps": round(copy_gbs, 1),
               "algorithmic_bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1),
               "frac_8TBps": round(nbytes / ms / 1e-3 / HBM_PEAK, 3), "frac_copy_6p3TBps": round(nbytes / ms / 1e-3 / HBM_COPY, 3)}
        # grid to transport blocks: the same launch, then the decoder
        tbs = int(lib.load().nrphy_tbs_calculate(12, 0, 0, qm, 0.75 * 1024, layers, nprb))
        tb_bytes = tbs // 8
        bg = 1
        cfg = abi.PuschDecoderCfg(bg, qm, 0, layers, 0, tb_bytes, G // qm, 10, 1, 1)
        soft_bytes, state_bytes, ncb = ctx.pusch_decoder_sizes(cfg, n)
        d_soft = torch.zeros((n, soft_bytes), dtype=torch.int8, device="cuda")
        d_state = torch.zeros((state_bytes,), dtype=torch.uint8, device="cuda")
        tb_stride = (tb_bytes + 3) & ~3
        d_tb = torch.zeros((n, tb_stride), dtype=torch.uint8, device="cuda")
        d_res = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        def grid_to_tb():
            demod()
            ctx.pusch_decode_batch(cfg, n, d_llr, stride, d_soft, d_state, d_tb, tb_stride, d_res, stream=sp)

        harness.settle([grid_to_tb], s)
        rec["grid_to_tb_ms"] = harness.spread(harness.time_rounds({"tb": grid_to_tb}, s, rounds, max(2, iters // 4))["tb"])[0]
        rec["tb_bytes"], rec["codeblocks_per_tb"] = tb_bytes, ncb
        # one PUSCH against the composed path, after the timed region
        plan.run(d_grid, d_ce, d_nv, d_llr, stride, d_sinr, stream=sp)
        torch.cuda.synchronize()
        i = n // 3
        grid = d_grid[i].cpu().numpy().view(np.uint32)
        ce = d_ce[i * ce_elems:(i + 1) * ce_elems].cpu().numpy().view(np.uint32).reshape(layers, ports, 14, nsubc)
        want, want_sinr = t.composed(ctx, cfgs[i], grid, ce, nv[i])
        got = d_llr[i, :G].cpu().numpy()
        rec["check_bit_exact"] = bool(np.array_equal(got, want))
        rec["check_sinr_err_db"] = float(abs(float(d_sinr[i].cpu()) - want_sinr))
        print(json.dumps(rec), flush=True)
        records.append(rec)
        plan.close()
        del d_ce, d_soft, d_state
        torch.cuda.empty_cache()


    with open(out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=15, iters=20, timeout=30, out=os.path.join(ROOT, "profiles", "pusch_demod_bench.json"),
                                               n=1024)))
