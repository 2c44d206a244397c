#!/usr/bin/env python3
"""The PRACH window pipeline, 4 receive ports: format 0 at 30.72 MHz (24576 = 6 x 4096 points, one symbol) and B4 at 61.44 MHz /
30 kHz (2048 points, twelve symbols).  Recorded, not gated.

(a) kernel: the demodulation launch (nrphy_prach_window_demod_run) from complex float and from complex int16 samples resident in
    HBM, for one window -- what a pool enqueues -- and for a plan of 64 windows.  HIP events on an explicit stream around rounds of
    launches, after about 30 ms of untimed load; median round and spread.  The bytes a launch must move (the symbols' samples in,
    the occasions' elements out) are set against a device-to-device copy timed in the same process.
(b) pool: the same window again and again -- one preamble in noise on every port -- through nrphy_prach_windows at depth 1 and 4,
    delivered in runs of one PUSCH slot, float and int16 samples, against the window driven by hand with the two blocking entry
    points of this library: nrphy_prach_demodulate_host (an int16 stream widened in numpy first), then nrphy_prach_detect_host per
    occasion.  Host microseconds per window are the time spent inside the calls that submit a window; windows per second are
    windows over wall time, waits included.

Every measurement is one GPU step: a child process of its own under a time limit, and the next one starts only if the one before
ended well.  Hardware counters are not collected here.  Writes profiles/prach_window_bench.json: one JSON record per line, a line
per figure, as profiles/ul_slot_bench.json is written.  (The script is not called *_bench.py: tests/test_bench_harness.py counts those.)

    python3 profiles/prach_window_measure.py            (GPU box, repository root)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
PORTS = 4
CI16_SCALE = 10000.0
BATCH = 64
CASES = {
    "format0": (dict(srate_hz=30720000, format="0", nof_td_occasions=1, nof_fd_occasions=1, start_symbol=0, rb_offset=12, nof_prb_ul_grid=79,
                     pusch_numerology=0, nof_rx_ports=PORTS),
                dict(format="0", ra_scs="1.25", root_sequence_index=40, zero_correlation_zone=5, nof_rx_ports=PORTS), 32, 240),
    "B4": (dict(srate_hz=61440000, format="B4", nof_td_occasions=1, nof_fd_occasions=1, start_symbol=2, rb_offset=30, nof_prb_ul_grid=106,
                pusch_numerology=1, nof_rx_ports=PORTS),
           dict(format="B4", ra_scs="30", root_sequence_index=9, zero_correlation_zone=11, nof_rx_ports=PORTS), 12, 40),
}


def timed(launch, stream, rounds, iters):
    settle = harness.settle([launch], stream)  # about 30 ms of load before anything is timed
    ms, ms_min, ms_max = harness.spread(harness.time_rounds({"launch": launch}, stream, rounds, iters)["launch"])
    return {"ms": ms, "ms_min": ms_min, "ms_max": ms_max, "settle_launches": settle}


def configurations(case):
    """(abi.PrachDemodCfg, abi.PrachCfg, abi.PrachDemodSizes); the detector takes the table's threshold where the table has a row
    for four ports and a threshold of its own where it has none."""
    import backends
    lib, abi = backends.pkg.lib, backends.abi
    demod, det, _, _ = CASES[case]
    d, p = abi.make_prach_demod(**demod), abi.make_prach(**det)
    if lib.prach_validate(p) != abi.OK:
        p = abi.make_prach(threshold=0.3, win_margin=5, **det)
    assert lib.prach_demod_validate(d) == abi.OK and lib.prach_validate(p) == abi.OK
    return d, p, lib.prach_demod_sizes(d)


def window(ctx, case):
    """complex64 [ports][window_samples]: the preamble of the case, delayed, a phase per port, in noise."""
    import prach_demod_model as model
    demod, _, preamble, delay = CASES[case]
    _, p, sz = configurations(case)
    rng = np.random.default_rng(3)
    start, occasion = model.modulate(demod, 0, 0, ctx.prach_generate_host(p, preamble), delay)
    sigma = 0.05 * np.sqrt(np.mean(np.abs(occasion) ** 2))
    x = sigma * (rng.standard_normal((PORTS, sz.window_samples)) + 1j * rng.standard_normal((PORTS, sz.window_samples)))
    for port in range(PORTS):
        x[port, start:start + len(occasion)] += occasion * np.exp(0.7j * port)
    return x.astype(np.complex64), preamble


def to_ci16(x):
    return np.clip(np.rint(np.stack([x.real, x.imag], axis=-1).astype(np.float64) * CI16_SCALE), -32768, 32767).astype(np.int16)


def step_kernel(case, rounds, iters):
    import torch
    import backends
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    d, _, sz = configurations(case)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    copy_gbs = harness.copy_rate(stream)
    out = []
    for windows in (1, BATCH):
        n_in = PORTS * sz.window_samples
        n_out = PORTS * sz.nof_symbols * sz.sequence_length
        plan = lib.PrachDemodPlan(ctx, [d] * windows, [w * n_in for w in range(windows)], sz.window_samples, [w * n_out for w in range(windows)],
                                  port_stride=sz.nof_symbols * sz.sequence_length, fd_stride=sz.nof_symbols * sz.sequence_length,
                                  td_stride=sz.nof_symbols * sz.sequence_length, symbol_stride=sz.sequence_length)
        d_iq = torch.randn((windows * n_in, 2), device="cuda", dtype=torch.float32) * 0.3
        d_x = (d_iq * CI16_SCALE).round().clamp(-32768, 32767).to(torch.int16)
        d_buf = torch.zeros((windows * n_out, 2), device="cuda", dtype=torch.float32)
        torch.cuda.synchronize()
        read = windows * PORTS * sz.nof_symbols * sz.dft_size  # samples the symbols cover; the prefixes are not read
        legs = [("cf32", 8, lambda: plan.run_iq(d_iq, d_buf, abi.IQ_CF32, 1.0, stream=sp)),
                ("ci16", 4, lambda: plan.run_iq(d_x, d_buf, abi.IQ_CI16, CI16_SCALE, stream=sp))]
        for _ in range(2):  # the legs in turn, twice: the spread between the two passes is run-to-run spread inside one process
            for name, sample_bytes, launch in legs:
                assert launch() == abi.OK
                t = timed(launch, stream, rounds, iters)
                nbytes = read * sample_bytes + windows * n_out * 8
                out.append(dict(t, leg="kernel", case=case, iq_format=name, windows=windows, ports=PORTS, dft_size=sz.dft_size,
                                symbols=sz.nof_symbols, workgroups=windows * PORTS * sz.nof_symbols, rounds=rounds, iters=iters,
                                bytes_per_launch=nbytes, GBps=round(nbytes / (t["ms"] * 1e-3) / 1e9, 1), copy_GBps=round(copy_gbs, 1),
                                counters="not measured"))
        plan.close()
    return out


def step_hand(case, nwindows):
    import backends
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    d, p, _ = configurations(case)
    x, preamble = window(ctx, case)
    x16 = to_ci16(x)
    gain = np.float32(1.0) / np.float32(CI16_SCALE)
    out = []
    for fmt in ("cf32", "ci16"):
        def one():
            samples = x if fmt == "cf32" else np.ascontiguousarray(x16.astype(np.float32) * gain).view(np.complex64)[..., 0]
            buffer = ctx.prach_demodulate_host(d, samples)
            return ctx.prach_detect_host(p, buffer[:, 0, 0])
        for _ in range(3):
            res, pre, _ = one()
        assert res.nof_detected == 1 and pre[preamble].detected
        t0 = time.perf_counter()
        for _ in range(nwindows):
            one()
        dt = time.perf_counter() - t0
        out.append(dict(leg="hand", case=case, iq_format=fmt, windows=nwindows, host_us_per_window=round(dt / nwindows * 1e6, 1),
                        windows_per_s=round(nwindows / dt, 1)))
    return out


def step_pool(case, depth, nwindows):
    import backends
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    d, p, sz = configurations(case)
    x, preamble = window(ctx, case)
    run = d.srate_hz // (1000 << d.pusch_numerology)  # the samples of one PUSCH slot
    out = []
    for fmt, name, radio in ((abi.IQ_CF32, "cf32", x), (abi.IQ_CI16, "ci16", to_ci16(x))):
        pool = lib.PrachWindows(ctx, d.srate_hz, PORTS, depth, sz.window_samples, iq_format=fmt, iq_scale=CI16_SCALE, max_ports=PORTS)
        spans = [[radio[r, at:at + run] for r in range(PORTS)] for at in range(0, sz.window_samples, run)]

        def submit():
            rc, wid = pool.open(d, range(PORTS), p)
            assert rc == abi.OK
            for span in spans:
                assert pool.samples(wid, span)[0] == abi.OK
            return wid

        def retire(wid, check=False):
            assert pool.wait(wid) == abi.OK
            if check:
                assert pool.results(wid)[0].nof_detected == 1 and pool.preambles(wid, 0)[preamble].detected
            pool.close(wid)

        for _ in range(3):
            retire(submit(), check=True)
        open_ids, host = [], 0.0
        t0 = time.perf_counter()
        for _ in range(nwindows):
            if len(open_ids) == depth:
                retire(open_ids.pop(0))
            h0 = time.perf_counter()
            open_ids.append(submit())
            host += time.perf_counter() - h0
        for wid in open_ids:
            retire(wid)
        dt = time.perf_counter() - t0
        out.append(dict(leg="pool", case=case, iq_format=name, depth=depth, runs_per_window=len(spans), windows=nwindows,
                        host_us_per_window=round(host / nwindows * 1e6, 1), windows_per_s=round(nwindows / dt, 1),
                        sample_bytes_per_window=int(radio.nbytes), plans_made=pool.plans_made()))
        pool.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="", help="run one step in this process (what the driver starts)")
    ap.add_argument("--case", default="format0")
    ap.add_argument("--depth", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--windows", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prach_window_bench.json"))
    args = ap.parse_args()
    if args.step:
        recs = {"kernel": lambda: step_kernel(args.case, args.rounds, args.iters), "hand": lambda: step_hand(args.case, args.windows),
                "pool": lambda: step_pool(args.case, args.depth, args.windows)}[args.step]()
        with open(args.out, "a") as f:
            for r in recs:
                print(json.dumps(r), flush=True)
                f.write(json.dumps(r) + "\n")
        return 0
    if os.path.exists(args.out):
        os.remove(args.out)
    steps = []
    for case in CASES:
        steps += [["--step", "kernel", "--case", case], ["--step", "hand", "--case", case]]
        steps += [["--step", "pool", "--case", case, "--depth", str(depth)] for depth in (1, 4)]
    common = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--iters", str(args.iters), "--windows", str(args.windows),
              "--out", args.out]
    return harness.run_steps([("prach_window_%d_%s_%s" % (i, extra[1], extra[3]), common + extra, {}, args.timeout)
                              for i, extra in enumerate(steps)], harness.LOG_DIR)


if __name__ == "__main__":
    sys.exit(main())
