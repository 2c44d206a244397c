#!/usr/bin/env python3
"""OFDM PRACH demodulator throughput (nrphy_prach_demod_run) against what the library offered before it for the same job.

Workloads, each one launch of 64 occasions on 4 receive ports, inputs resident in HBM: format 0 at 30.72 MHz with 1 and with 8
frequency-domain occasions (24576 points = 6 x 4096), format 3 at 30.72 MHz (6144 points, 4 symbols), B4 at 30 kHz and 61.44 MHz
(2048 points, 12 symbols).

Yardstick: nrphy_dft_run over the same symbols read in place -- per (occasion, port) one call whose batch is the occasion's
back-to-back symbols behind the cyclic prefix, writing every bin; the gather of the L_RA bins per frequency-domain occasion would
still be to do after it.  A stricter figure is reported next to it: ONE nrphy_dft_run call over a packed copy of all the symbols
(no prefix between them), which needs a copy the timing leaves out.

Method: one GPU step in a child process of its own under a time limit.  The legs run untimed until the engine clocks have had
`--settle` seconds of load; then `--rounds` rounds alternate between the legs, each timing `--iters` back-to-back repetitions with
HIP events on one explicit stream (profiles/bench_harness.py); median and spread (largest - smallest) over the rounds.  The
demodulator passes a workload when its median does not exceed the yardstick's by more than the larger spread of the two.  After
the timed region one (occasion, port) is compared with the float64 restatement (tests/prach_demod_model.py).
Writes profiles/prach_demod_bench.json.  Usage (GPU box, repository root): python3 profiles/prach_demod_bench.py"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKLOADS = (("format 0, 1 fd", dict(srate_hz=30720000, format="0", nof_fd_occasions=1, rb_offset=4, nof_prb_ul_grid=79, pusch_numerology=0)),
             ("format 0, 8 fd", dict(srate_hz=30720000, format="0", nof_fd_occasions=8, rb_offset=4, nof_prb_ul_grid=79, pusch_numerology=0)),
             ("format 3", dict(srate_hz=30720000, format="3", nof_fd_occasions=1, rb_offset=4, nof_prb_ul_grid=79, pusch_numerology=0)),
             ("B4 at 30 kHz", dict(srate_hz=61440000, format="B4", nof_fd_occasions=1, rb_offset=4, nof_prb_ul_grid=106, pusch_numerology=1)))


def step(rounds, iters, out, n, settle):
    import torch
    import backends
    import prach_demod_model as model
    lib, abi = backends.pkg.lib, backends.abi
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    ctx = lib.Context(0)
    ports = 4
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    # The copy rate every "bytes over copy rate" below refers to: a 256 MiB device-to-device copy, read + write counted.
    copy_gbs = harness.copy_rate(stream)
    records = []
    for name, base in WORKLOADS:
        cfg = dict(base, nof_td_occasions=1, start_symbol=0, nof_rx_ports=ports)
        d = model.derive(cfg)
        N, L, nsym, nfd, window = d["dft_size"], d["L"], d["nof_symbols"], cfg["nof_fd_occasions"], d["window_samples"]
        rng = np.random.default_rng(1)
        x = (rng.uniform(-1, 1, (n, ports, window)) + 1j * rng.uniform(-1, 1, (n, ports, window))).astype(np.complex64)
        d_x = torch.from_numpy(x.view(np.float32)).cuda()
        d_buf = torch.zeros((n, ports, 1, nfd, nsym, L, 2), dtype=torch.float32, device="cuda")
        plan = lib.PrachDemodPlan(ctx, [abi.make_prach_demod(**cfg)] * n, [i * ports * window for i in range(n)], window,
                                  [i * ports * nfd * nsym * L for i in range(n)], nfd * nsym * L, nsym * L, nfd * nsym * L, L)
        d_all = torch.empty((n * ports * nsym, N, 2), dtype=torch.float32, device="cuda")
        first = d["symbol_offset"][0]
        d_packed = torch.from_numpy(np.ascontiguousarray(x[:, :, first:first + nsym * N]).view(np.float32)).cuda()
        x_ptr, all_ptr = d_x.data_ptr(), d_all.data_ptr()

        def demod():
            plan.run(d_x, d_buf, stream=sp)

        def dft_in_place():
            for k in range(n * ports):
                rc = ctx.lib.nrphy_dft_run(ctx.handle, N, 0, nsym, C.c_void_p(x_ptr + 8 * (k * window + first)),
                                           C.c_void_p(all_ptr + 8 * k * nsym * N), sp)
                assert rc == abi.OK

        def dft_packed():
            assert ctx.lib.nrphy_dft_run(ctx.handle, N, 0, n * ports * nsym, C.c_void_p(d_packed.data_ptr()), C.c_void_p(all_ptr), sp) == abi.OK

        legs = {"demod": demod, "dft_in_place": dft_in_place, "dft_packed": dft_packed}
        harness.settle(legs, stream, min_ms=1000 * settle)
        times = harness.time_rounds(legs, stream, rounds, iters)
        med = {k: float(np.median(v)) for k, v in times.items()}
        spread = {k: float(max(v) - min(v)) for k, v in times.items()}
        symbols = n * ports * nsym
        read_bytes = symbols * N * 8
        rec = {"leg": "prach_demod", "workload": name, "srate_hz": cfg["srate_hz"], "format": cfg["format"], "fd_occasions": nfd,
               "occasions": n, "rx_ports": ports, "dft_size": N, "symbols_per_launch": symbols, "rounds": rounds, "iters": iters,
               "ms_per_launch": round(med["demod"], 4), "ms_spread": round(spread["demod"], 4),
               "ns_per_symbol": round(med["demod"] * 1e6 / symbols, 1),
               "dft_run_in_place_ms": round(med["dft_in_place"], 4), "dft_run_in_place_spread": round(spread["dft_in_place"], 4),
               "dft_run_in_place_calls": n * ports,
               "dft_run_packed_ms": round(med["dft_packed"], 4), "dft_run_packed_spread": round(spread["dft_packed"], 4),
               "input_bytes": read_bytes, "output_bytes": symbols * nfd * L * 8, "copy_rate_GBps": round(copy_gbs, 1),
               "input_bytes_over_copy_rate_ms": round(read_bytes / copy_gbs / 1e6, 4),
               "pass_vs_in_place": bool(med["demod"] <= med["dft_in_place"] + max(spread["demod"], spread["dft_in_place"])),
               "pass_vs_packed": bool(med["demod"] <= med["dft_packed"] + max(spread["demod"], spread["dft_packed"]))}
        # one (occasion, port) against the restatement, and the yardstick's bins against the same
        got = d_buf.cpu().numpy().view(np.complex64).reshape(n, ports, 1, nfd, nsym, L)
        i, p = n // 3, ports - 1
        want = model.demodulate(cfg, x[i, p])
        rec["check_rel_err"] = float(np.abs(got[i, p] - want).max() / np.abs(want).max())
        dft_in_place()
        torch.cuda.synchronize()
        spectrum = d_all.cpu().numpy().view(np.complex64).reshape(n, ports, nsym, N)[i, p]
        bins = (d["first_bin"][0] + np.arange(L)) % N
        rec["check_dft_run_rel_err"] = float(np.abs(spectrum[:, bins] - want[0, 0]).max() / np.abs(want).max())
        print(json.dumps(rec), flush=True)
        records.append(rec)
        plan.close()
        del d_x, d_buf, d_all, d_packed
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=9, iters=10, timeout=30, out=os.path.join(ROOT, "profiles", "prach_demod_bench.json"),
                                               n=64, settle=1.0)))
