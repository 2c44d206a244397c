#!/usr/bin/env python3
"""The uplink slot pipeline at 100 MHz / 30 kHz (273 PRB, 4096-point transform, 4 receive ports).  Recorded, not gated.

(a) kernel: one OFDM demodulation launch over 14 symbols x 4 ports x 64 slots, samples and grids resident in HBM --
    nrphy_ofdm_demod_symbols from complex float and from complex int16, and the whole-slot nrphy_ofdm_demod_run next to them.
    HIP events on an explicit stream around rounds of launches, after about 30 ms of untimed load; median round and spread.  The
    bytes a launch must move (samples in, cbf16 rows out) are set against a device-to-device copy timed in the same process.
(b) pool: the same slot again and again -- one 273-PRB 16-QAM PUSCH and four format 1 PUCCHs, transmitted by the tests'
    transmitters and modulated by the library -- through nrphy_ul_slots at depth 1 and 4 (one run of 14 symbols per slot, and at
    depth 4 also 14 runs of one symbol), float and int16 samples, against the slot driven by hand with the blocking entry points:
    nrphy_ofdm_demodulate_slot_host (an int16 stream widened in numpy first), nrphy_pusch_proc_host and four nrphy_pucch_host.
    Host microseconds per slot are the time spent inside the calls that submit a slot; slots per second are slots over wall time,
    waits included.  The pool makes one plan per receiver call, as nrphy_dl_slot_pdsch does: that is what the host time is.

Every measurement is one GPU step: a child process of its own under a time limit, and the next one starts only if the one before
ended well.  --parent-lib names a build of the parent commit's library: its steps (the whole-slot launch, the hand-driven slot)
then alternate with this build's, parent first, twice each.  Hardware counters are not collected here.  Writes
profiles/ul_slot_bench.json.

    python3 profiles/ul_slot_bench.py [--parent-lib PATH]            (GPU box, repository root)
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
PORTS, NOF_PRB, DFT, MU = 4, 273, 4096, 1
NOF_SUBC = 12 * NOF_PRB
SLOTS = 64
CI16_SCALE = 10000.0


def ofdm_cfg(abi):
    return abi.OfdmConfig(MU, NOF_PRB, DFT, 0, 1.0 / np.sqrt(DFT), 3.5e9)


def timed(launch, stream, rounds, iters):
    settle = harness.settle([launch], stream)  # about 30 ms of load before anything is timed
    ms, ms_min, ms_max = harness.spread(harness.time_rounds({"launch": launch}, stream, rounds, iters)["launch"])
    return {"ms": ms, "ms_min": ms_min, "ms_max": ms_max, "settle_launches": settle}


def step_kernel(tag, rounds, iters):
    import torch
    import backends
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    cfg = ofdm_cfg(abi)
    plan = lib.OfdmPlan(ctx, cfg, PORTS)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    d_iq = torch.randn((SLOTS, PORTS, plan.slot_stride, 2), device="cuda", dtype=torch.float32)
    d_x = (d_iq * 3000.0).round().clamp(-32768, 32767).to(torch.int16)
    d_grid = torch.zeros((SLOTS, PORTS, 14, NOF_SUBC), dtype=torch.int32, device="cuda")
    d_slot = torch.from_numpy((np.arange(SLOTS) % 2).astype(np.int32)).cuda()
    torch.cuda.synchronize()
    samples = SLOTS * PORTS * lib.slot_size(cfg, 1)
    grid_bytes = SLOTS * PORTS * 14 * NOF_SUBC * 4
    copy_gbs = harness.copy_rate(stream)
    legs = [("demod_run", 8, lambda: plan.demod_run(SLOTS, d_iq, d_grid, d_slot_index=d_slot, stream=sp))]
    if hasattr(ctx.lib, "nrphy_ofdm_demod_symbols"):
        legs.append(("demod_symbols_cf32", 8, lambda: plan.demod_symbols(SLOTS, d_iq, d_grid, 0, 14, d_slot_index=d_slot, stream=sp)))
        legs.append(("demod_symbols_ci16", 4, lambda: plan.demod_symbols(SLOTS, d_x, d_grid, 0, 14, iq_format=abi.IQ_CI16, iq_scale=CI16_SCALE,
                                                                           d_slot_index=d_slot, stream=sp)))
    out = []
    for _ in range(2):  # the legs in turn, twice: the spread between the two passes is run-to-run spread inside one process
        for name, sample_bytes, launch in legs:
            t = timed(launch, stream, rounds, iters)
            nbytes = samples * sample_bytes + grid_bytes
            out.append(dict(t, leg="kernel", library=tag, call=name, slots=SLOTS, ports=PORTS, symbols=14, dft_size=DFT, nof_prb=NOF_PRB,
                            rounds=rounds, iters=iters, bytes_per_launch=nbytes, GBps=round(nbytes / (t["ms"] * 1e-3) / 1e9, 1),
                            copy_GBps=round(copy_gbs, 1), counters="not measured"))
    plan.close()
    return out


def build_slot(ctx, lib, abi):
    """One slot's PDUs and its samples (complex64 [ports][n]).  The PUSCH takes PRBs 0-268 of the 273 and the four PUCCHs PRBs 269-272,
    so that nothing overlaps."""
    import pucch_model
    import test_pusch_processor as tp
    from pusch_chest_model import to_cbf16
    rng = np.random.default_rng(1)
    prbs = range(0, NOF_PRB - 4)
    tb_bits = lib.tbs_calculate(14, 24, 0, 4, 616.0, 1, len(prbs))
    pdu = abi.make_pusch_pdu(prbs=prbs, modulation=4, target_code_rate=616.0, numerology=MU, slot_index=0, rnti=0x4601, n_id=11,
                             scrambling_id=100, tb_size_bytes=tb_bits // 8, ldpc_base_graph=tp.base_graph(tb_bits, 616.0), tbs_lbrm_bytes=159749,
                             dmrs_symbols=(2, 11), rx_ports=(0, 1, 2, 3))
    opts = tp.OPTIONS
    assert lib.pusch_proc_validate(pdu, opts, PORTS, NOF_SUBC) == abi.OK
    sent = tp.transmit(ctx, pdu, lib.pusch_proc_derive(pdu, opts, PORTS, NOF_SUBC), rng, nsubc=NOF_SUBC)
    grid = sent.clean.copy()
    pucch = []
    for i in range(4):
        c = pucch_model.make_cfg(1, NOF_PRB - 4 + i, 14, 0, bwp_size_rb=NOF_PRB, numerology=MU, n_id=40 + i, slot_index=0, initial_cyclic_shift=i,
                                 nof_harq_ack=2, ports=(0, 1, 2, 3))
        pucch_model.add_to_grid(grid, pucch_model.transmit(c, [i & 1, i >> 1]), [1.0, 0.8j, -0.9, 0.7 - 0.2j], delay=1.0, numerology=MU)
        pucch.append(pucch_model.to_abi(abi, c))
    plan = lib.OfdmPlan(ctx, ofdm_cfg(abi), PORTS)
    iq = plan.modulate_slot_host(to_cbf16(grid.astype(np.complex64)).view(np.uint16).reshape(PORTS, 14, NOF_SUBC, 2), 0)
    sigma = np.sqrt(0.5 * 10 ** (-25.0 / 10))
    iq = (iq + sigma * (rng.standard_normal(iq.shape) + 1j * rng.standard_normal(iq.shape))).astype(np.complex64)
    return pdu, opts, pucch, plan, iq, sent.tb


def step_hand(tag, nslots):
    import backends
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    pdu, opts, pucch, plan, iq, tb = build_slot(ctx, lib, abi)
    x16 = np.clip(np.rint(iq.view(np.float32).astype(np.float64) * CI16_SCALE), -32768, 32767).astype(np.int16)
    gain = np.float32(1.0) / np.float32(CI16_SCALE)
    out = []
    for fmt in ("cf32", "ci16"):
        def one():
            samples = iq if fmt == "cf32" else (x16.astype(np.float32) * gain).view(np.complex64)
            words = plan.demodulate_slot_host(samples, 0).view(np.uint32).reshape(PORTS, 14, NOF_SUBC)
            r, got, _ = ctx.pusch_proc_host(pdu, opts, words)
            return r, got, [ctx.pucch_host(c, words)[0] for c in pucch]
        for _ in range(3):
            r, got, acks = one()
        assert r.tb_crc_ok == 1 and got.tobytes() == tb.tobytes() and all(a.status == abi.PUCCH_STATUS_VALID for a in acks)
        t0 = time.perf_counter()
        for _ in range(nslots):
            one()
        dt = time.perf_counter() - t0
        out.append(dict(leg="hand", library=tag, iq_format=fmt, slots=nslots, host_us_per_slot=round(dt / nslots * 1e6, 1),
                        slots_per_s=round(nslots / dt, 1), tb_bytes=pdu.tb_size_bytes))
    return out


def step_pool(depth, symbols_per_run, nslots):
    import torch
    import backends
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    pdu, opts, pucch, plan, iq, tb = build_slot(ctx, lib, abi)
    x16 = np.clip(np.rint(iq.view(np.float32).astype(np.float64) * CI16_SCALE), -32768, 32767).astype(np.int16).reshape(PORTS, -1, 2)
    soft, state = lib.pusch_proc_harq_bytes(pdu, opts)
    state_at = (soft + 255) // 256 * 256
    stride = state_at + (state + 255) // 256 * 256
    off = [0]
    for l in range(14):
        off.append(off[-1] + lib.symbol_size(ofdm_cfg(abi), l))
    out = []
    for fmt, name, x in ((abi.IQ_CF32, "cf32", iq), (abi.IQ_CI16, "ci16", x16)):
        d_harq = torch.zeros(depth * stride, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pool = lib.UlSlots(ctx, ofdm_cfg(abi), PORTS, depth, iq_format=fmt, iq_scale=CI16_SCALE, max_pusch=1, max_pucch=4,
                           max_tb_bytes=pdu.tb_size_bytes, max_uci_bits=16, d_harq=d_harq)
        runs = [(f, min(symbols_per_run, 14 - f)) for f in range(0, 14, symbols_per_run)]
        spans = [[x[p, off[f]: off[f + n]] for p in range(PORTS)] for f, n in runs]

        def submit():
            sid = pool.open(0)
            for (f, n), span in zip(runs, spans):
                assert pool.samples(sid, f, n, span) == abi.OK
            assert pool.pucch(sid, pucch) == abi.OK
            assert pool.pusch(sid, [pdu], opts, [sid * stride], [sid * stride + state_at]) == abi.OK
            assert pool.finish(sid) == abi.OK
            return sid

        def retire(sid, check=False):
            assert pool.wait(sid) == abi.OK
            if check:
                r = pool.pusch_results(sid)[0]
                assert r.tb_crc_ok == 1 and pool.tb(sid, 0).tobytes() == tb.tobytes()
                assert all(a.status == abi.PUCCH_STATUS_VALID for a in pool.pucch_results(sid))
            pool.close(sid)

        for _ in range(3):
            retire(submit(), check=True)
        open_ids, host = [], 0.0
        t0 = time.perf_counter()
        for _ in range(nslots):
            if len(open_ids) == depth:
                retire(open_ids.pop(0))
            h0 = time.perf_counter()
            open_ids.append(submit())
            host += time.perf_counter() - h0
        for sid in open_ids:
            retire(sid)
        dt = time.perf_counter() - t0
        out.append(dict(leg="pool", library="new", iq_format=name, depth=depth, symbols_per_run=symbols_per_run, slots=nslots,
                        host_us_per_slot=round(host / nslots * 1e6, 1), slots_per_s=round(nslots / dt, 1), tb_bytes=pdu.tb_size_bytes,
                        sample_bytes_per_slot=int(x.nbytes)))
        pool.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="", help="run one step in this process (what the driver starts)")
    ap.add_argument("--tag", default="new")
    ap.add_argument("--depth", type=int, default=1)
    ap.add_argument("--symbols-per-run", type=int, default=14)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--slots", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per GPU step")
    ap.add_argument("--parent-lib", default="", help="libmi355nrphy.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ul_slot_bench.json"))
    args = ap.parse_args()
    if args.step:
        recs = {"kernel": lambda: step_kernel(args.tag, args.rounds, args.iters), "hand": lambda: step_hand(args.tag, args.slots),
                "pool": lambda: step_pool(args.depth, args.symbols_per_run, args.slots)}[args.step]()
        with open(args.out, "a") as f:
            for r in recs:
                print(json.dumps(r), flush=True)
                f.write(json.dumps(r) + "\n")
        return 0
    if os.path.exists(args.out):
        os.remove(args.out)
    libs = [("parent", args.parent_lib), ("new", "")] * 2 if args.parent_lib else [("new", "")] * 2
    steps = [(["--step", "kernel", "--tag", tag], lib) for tag, lib in libs]
    steps += [(["--step", "hand", "--tag", tag], lib) for tag, lib in libs[:2]]
    steps += [(["--step", "pool", "--depth", str(d), "--symbols-per-run", str(s)], "") for d, s in ((1, 14), (4, 14), (4, 1))]
    common = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--iters", str(args.iters), "--slots", str(args.slots),
              "--out", args.out]
    rc = harness.run_steps([("ul_slot_%d_%s" % (i, extra[1]), common + extra, {"NRPHY_LIB_SO": os.path.abspath(lib)} if lib else {}, args.timeout)
                            for i, (extra, lib) in enumerate(steps)], harness.LOG_DIR)
    if rc != 0:
        return rc
    if not args.parent_lib:
        with open(args.out, "a") as f:
            f.write(json.dumps({"leg": "kernel", "library": "parent", "ms": "not measured"}) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
