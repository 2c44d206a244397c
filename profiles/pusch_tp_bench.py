#!/usr/bin/env python3
"""Transform-precoded PUSCH demodulation: the fused launch against the composed device calls, inputs resident in HBM.

1. The 28 recorded reference cases (tests/golden/pusch_tp_reference_*, the transform-precoded configurations of the reference's
   unit test with ZF and MMSE) as ONE plan run, next to the composed path for the same cases: per case nrphy_channel_equalize
   (one batch entry per OFDM symbol with data), nrphy_transform_deprecode, nrphy_demodulate_soft and nrphy_llr_descramble, 112
   launches in all, on RE already gathered.  `--rounds` alternating rounds of 20 x `--iters` fused runs and `--iters` composed
   passes; the median and the spread are printed.
2. A size a cell would run: 16 PUSCHs of 270 PRB, 256-QAM, 4 ports, 12 symbols with data -- the fused launch alone, with the
   bytes it has to move (grid and estimate words in, soft bits out).

One GPU step in a child process under a time limit.  Each part runs untimed until the clocks have had about 30 ms of load and is
then timed with HIP events on an explicit stream (profiles/bench_harness.py); the rate of a device-to-device copy measured in
the same process is printed with it.

Usage (GPU box, repository root): python3 profiles/pusch_tp_bench.py
"""
import os
import statistics
import sys

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def step(rounds, iters, out):
    import torch
    import backends
    import pusch_tp_model as model
    import test_pusch_transform_precoding as T
    from pusch_chest_model import as_i32, dev
    abi, lib = backends.abi, backends.pkg.lib
    ctx = lib.Context(0)
    s = torch.cuda.Stream()
    sp = s.cuda_stream

    rows, blobs = T.recording()
    nports, nsubc = 4, 25 * 12
    cases = [T.Recorded(r, blobs, nports=nports, nsubc=nsubc) for r in rows if r["group"] == 0 and r["transform_precoding"]]
    assert len(cases) == 28
    ce_off = np.cumsum([0] + [c.ce.size for c in cases])[:-1]
    plan = lib.PuschDemodPlan(ctx, [c.cfg for c in cases], list(range(len(cases))), len(cases), nports, nsubc,
                              [int(o) for o in ce_off], features=T.BOTH)
    G = [plan.codeword_bits(i) for i in range(len(cases))]
    stride = (max(G) + 15) & ~15
    d_grid = dev(as_i32(np.stack([c.grid for c in cases])))
    d_ce = dev(as_i32(np.concatenate([c.ce.reshape(-1) for c in cases])))
    d_nv = dev(np.stack([c.noise_vars for c in cases]))
    d_llr = torch.zeros(len(cases) * stride, dtype=torch.int8, device="cuda")
    d_sinr = torch.zeros(len(cases), dtype=torch.float32, device="cuda")

    def fused():
        plan.run(d_grid, d_ce, d_nv, d_llr, stride, d_sinr, stream=sp)

    # The composed path on gathered RE: per case [symbol][port][re] and [symbol][layer = 1][port][re].
    work = []
    for i, c in enumerate(cases):
        P = c.cfg.nof_rx_ports
        ports = [c.cfg.rx_ports[k] for k in range(P)]
        syms = [l for l in range(14) if model.data_subcarriers(c.cfg, l).size]
        ks = model.data_subcarriers(c.cfg, syms[0])
        rx = np.stack([c.grid[ports][:, l, ks] for l in syms])
        ch = np.stack([c.ce[:, :, l, ks] for l in syms])
        n, nre = len(syms), ks.size
        work.append(dict(eq_alg=c.cfg.equalizer, n=n, nre=nre, P=P, nprb=nre // 12, mod=0 if c.cfg.qm == 1 else c.cfg.qm,
                         bits=n * nre * c.cfg.qm, d_rx=dev(as_i32(rx)), d_ch=dev(as_i32(ch)),
                         d_nv=dev(np.tile(c.noise_vars[:P], (n, 1))),
                         d_eq=torch.zeros((n, nre, 2), dtype=torch.float32, device="cuda"),
                         d_ev=torch.zeros((n, nre), dtype=torch.float32, device="cuda"),
                         d_soft=torch.zeros(n * nre * c.cfg.qm + 16, dtype=torch.int8, device="cuda"),
                         d_out=torch.zeros(n * nre * c.cfg.qm + 16, dtype=torch.int8, device="cuda"),
                         d_ci=dev(np.array([c.cfg.rnti * 2 ** 15 + c.cfg.n_id], np.uint32).view(np.int32))))

    def composed():
        for w in work:
            ctx.channel_equalize(w["eq_alg"], w["n"], w["nre"], 1, w["P"], w["d_rx"], w["d_ch"], w["d_nv"], 1.0, w["d_eq"], w["d_ev"],
                                 stream=sp)
            ctx.transform_deprecode(w["nprb"], w["n"], w["d_eq"], w["d_eq"], stream=sp)
            ctx.demodulate_soft(w["mod"], w["n"], w["nre"], w["d_eq"], w["d_ev"], w["d_soft"], stream=sp)
            ctx.llr_descramble(w["d_ci"], 1, w["bits"], w["d_soft"], w["bits"], w["d_out"], w["bits"], stream=sp)

    torch.cuda.synchronize()
    fused()
    composed()
    torch.cuda.synchronize()
    for i, w in enumerate(work):  # the two paths compute the same soft bits
        assert torch.equal(w["d_out"][:w["bits"]], d_llr[i * stride: i * stride + G[i]]), i
    print("device-to-device copy %.1f GB/s" % harness.copy_rate(s))
    settle = harness.settle([fused, composed], s)
    f, c = [], []
    for _ in range(rounds):  # alternating; microseconds per call
        f += [1e3 * t for t in harness.time_rounds({"fused": fused}, s, 1, 20 * iters)["fused"]]
        c += [1e3 * t for t in harness.time_rounds({"composed": composed}, s, 1, iters)["composed"]]
    nre = sum(w["n"] * w["nre"] for w in work)
    print("28 recorded reference cases (%d data RE, %d soft bits): fused run %.1f us (min %.1f, max %.1f), composed device calls "
          "%.1f us (min %.1f, max %.1f), ratio %.1f; %d rounds after %d settling passes"
          % (nre, sum(G), statistics.median(f), min(f), max(f), statistics.median(c), min(c), max(c),
             statistics.median(c) / statistics.median(f), rounds, settle))
    plan.close()

    # A cell-sized launch.
    n, nprb, nsubc, qm = 16, 270, 273 * 12, 8
    cfg = abi.make_pusch_demod(prbs=range(nprb), qm=qm, rnti=0x4601, n_id=5, dmrs_symbols=(2, 11), nof_cdm_groups_without_data=2,
                               rx_ports=(0, 1, 2, 3), equalizer=abi.EQ_MMSE, transform_precoding=1)
    rng = np.random.default_rng(1)
    from pusch_chest_model import to_cbf16
    grid = to_cbf16((rng.standard_normal((n, 4, 14, nsubc)) + 1j * rng.standard_normal((n, 4, 14, nsubc))).astype(np.complex64))
    ce = to_cbf16((rng.standard_normal((1, 4, 14, nsubc)) + 1j * rng.standard_normal((1, 4, 14, nsubc))).astype(np.complex64))
    plan = lib.PuschDemodPlan(ctx, [cfg] * n, list(range(n)), n, 4, nsubc, [0] * n, features=T.BOTH)
    bits = plan.codeword_bits(0)
    d_grid, d_ce, d_nv = dev(as_i32(grid)), dev(as_i32(ce)), dev(np.full((n, 4), 0.01, np.float32))
    d_llr = torch.zeros(n * bits, dtype=torch.int8, device="cuda")
    d_sinr = torch.zeros(n, dtype=torch.float32, device="cuda")

    def big():
        plan.run(d_grid, d_ce, d_nv, d_llr, bits, d_sinr, stream=sp)

    settle = harness.settle([big], s)
    t = [1e3 * ms for ms in harness.time_rounds({"big": big}, s, rounds, 5 * iters // 2)["big"]]
    re = n * 12 * nprb * 12
    nbytes = re * (4 * 4 + 4 * 4) + n * bits
    us = statistics.median(t)
    print("%d PUSCHs x %d PRB x 12 symbols, 256-QAM, 4 ports, MMSE: fused run %.1f us (min %.1f, max %.1f), %.2f G RE/s, %.0f GB/s of "
          "grid + estimate words in and soft bits out; %d rounds after %d settling launches"
          % (n, nprb, us, min(t), max(t), re / us / 1e3, nbytes / us / 1e3, rounds, settle))
    plan.close()


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=5, iters=200, timeout=30, out="")))
