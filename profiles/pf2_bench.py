#!/usr/bin/env python3
"""PUCCH format 2 receiver throughput (nrphy_pf2_run): 1,024 and 16,384 PUCCHs per launch on 4 receive ports, in three shapes --
1 PRB x 1 symbol with A = 4, 4 PRB x 2 symbols with A = 20 and 16 PRB x 2 symbols with A = 100 --, every PUCCH on PRBs of its own
(16, 12 or 3 per received grid), inputs resident in HBM.

Every batch size is one GPU step: a child process of its own under a time limit, and the next one starts only if the one before
ended well.  A step builds the plans, runs untimed launches until the engine clocks have had about 30 ms of load, then times, in
alternating rounds with HIP events on an explicit stream, per shape: the receiver launch alone (nrphy_pf2_run without decoder
outputs), the decoder launch alone (a UCI decoder plan over the same soft bits) and both together (nrphy_pf2_run); it reports the
median round and the spread.  The bytes a launch has to move (grid rows and descriptors read, soft bits, records and payload
written, soft bits read again by the decoder) are set against the rate of a device-to-device copy measured in the same process;
the 8 KB twiddle table every workgroup reads comes from cache and is listed apart.  After the timed region the PUCCHs of the first
grid, which carry real transmissions, are checked against the NumPy restatement (tests/pucch2_model.py).  Hardware counters are
not collected here.  Writes profiles/pf2_bench.json.

    python3 profiles/pf2_bench.py            (GPU box, repository root)
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
PORTS, NOF_PRB = 4, 52
NOF_SUBC = 12 * NOF_PRB
CSI_BYTES, DESC_BYTES, UCI_DESC_BYTES, TWIDDLE_BYTES = 32, 152, 40, 8192  # nrphy_pf2_csi_t, the two plans' descriptors, the table
SHAPES = (("1prb_1sym_A4", 1, 1, 4, 16), ("4prb_2sym_A20", 4, 2, 20, 12), ("16prb_2sym_A100", 16, 2, 100, 3))  # name, PRB, symbols, A, per grid


def step(n, rounds, iters, out):
    import torch
    import backends
    import pucch2_model as model
    lib, abi = backends.pkg.lib, backends.abi
    oracle = backends.oracle()
    ctx = lib.Context(0)
    rng = np.random.default_rng(0)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    runs = []
    for name, nprb, nsym, A, per_grid in SHAPES:
        n_grids = (n + per_grid - 1) // per_grid
        E = 16 * nprb * nsym
        cfgs = [model.make_cfg(nprb * (i % per_grid) * (3 if nprb == 1 else 1), nprb, nsym, 14 - nsym, bwp_size_rb=NOF_PRB, slot_index=3,
                               rnti=1 + i % 60000, n_id=77, n_id_0=500, nof_harq_ack=A, rx_ports=tuple(range(PORTS))) for i in range(n)]
        # Unit-variance noise in every grid; the first grid also carries its UEs at 6 dB per port.
        g = torch.randn((n_grids, PORTS, 14, NOF_SUBC, 2), device="cuda", dtype=torch.float32) * (0.5 ** 0.5)
        first = np.zeros((PORTS, 14, NOF_SUBC), complex)
        sent = []
        for i in range(min(per_grid, n)):
            bits = rng.integers(0, 2, A).astype(np.uint8)
            model.add_to_grid(first, model.transmit(cfgs[i], bits), [2.0 * np.exp(1j * (0.4 + p)) for p in range(PORTS)], delay=2.0)
            sent.append(bits)
        g[0] += torch.from_numpy(np.stack([first.real, first.imag], axis=-1).astype(np.float32)).cuda()
        d_grid = g.to(torch.bfloat16).view(torch.int32).reshape(n_grids, PORTS, 14, NOF_SUBC).contiguous()
        del g
        llr_off, msg_off = [i * E for i in range(n)], [i * A for i in range(n)]
        plan = lib.Pf2Plan(ctx, [model.to_abi(abi, c) for c in cfgs], [i // per_grid for i in range(n)], n_grids, PORTS, NOF_SUBC, llr_off,
                           msg_off)
        decoder = lib.UciDecoderPlan(ctx, [abi.make_uci_decoder(A, E, 2)] * n, llr_off, msg_off)
        bufs = dict(llr=torch.zeros(n * E, dtype=torch.int8, device="cuda"), msg=torch.zeros(n * A, dtype=torch.uint8, device="cuda"),
                    status=torch.zeros(n, dtype=torch.int32, device="cuda"), csi=torch.zeros(n * CSI_BYTES // 4, dtype=torch.int32, device="cuda"))
        rows = PORTS * nsym * nprb * 48
        rx_bytes, dec_bytes = n * (rows + DESC_BYTES + E + CSI_BYTES), n * (E + UCI_DESC_BYTES + A + 4)
        launches = {"receiver": (lambda p=plan, b=bufs, d=d_grid: p.run(d, b["llr"], None, None, b["csi"], stream=sp), rx_bytes),
                    "decoder": (lambda p=decoder, b=bufs: p.run(b["llr"], b["msg"], b["status"], stream=sp), dec_bytes),
                    "both": (lambda p=plan, b=bufs, d=d_grid: p.run(d, b["llr"], b["msg"], b["status"], b["csi"], stream=sp), rx_bytes + dec_bytes)}
        runs.append(dict(name=name, plan=plan, decoder=decoder, grid=d_grid, bufs=bufs, cfgs=cfgs, sent=sent, launches=launches,
                         shape=(nprb, nsym, A, per_grid)))
    copy_gbs = harness.copy_rate(stream)
    settle = harness.settle([r["launches"]["both"][0] for r in runs], stream)  # about 30 ms of load before anything is timed
    # alternating: every round times every launch of every shape once
    ms = harness.time_rounds({(r["name"], kind): launch for r in runs for kind, (launch, _) in r["launches"].items()}, stream, rounds, iters)
    records = []
    for r in runs:
        nprb, nsym, A, per_grid = r["shape"]
        E = 16 * nprb * nsym
        rec = {"leg": "pf2", "case": r["name"], "n": n, "rx_ports": PORTS, "nof_prb": nprb, "nof_symbols": nsym, "A": A, "E": E,
               "pucch_per_grid": per_grid, "rounds": rounds, "iters": iters, "settle_launches": settle, "copy_GBps": round(copy_gbs, 1),
               "twiddle_bytes_per_pucch_from_cache": TWIDDLE_BYTES, "counters": "not measured"}
        for kind, (_, nbytes) in r["launches"].items():
            med = float(np.median(ms[r["name"], kind]))
            ms_med, ms_min, ms_max = harness.spread(ms[r["name"], kind])
            rec[kind] = {"ms_per_launch": ms_med, "ms_min": ms_min, "ms_max": ms_max,
                         "ns_per_pucch": round(med * 1e6 / n, 2), "bytes_per_launch": nbytes, "GBps": round(nbytes / (med * 1e-3) / 1e9, 2),
                         "share_of_copy_rate": round(nbytes / (med * 1e-3) / 1e9 / copy_gbs, 4)}
        rec["pucch_per_s"] = round(n / (rec["both"]["ms_per_launch"] * 1e-3))
        # the first grid's PUCCHs against the restatement, after the timed region (the last launch was `both`)
        r["launches"]["both"][0]()
        torch.cuda.synchronize()
        k = len(r["sent"])
        llr = r["bufs"]["llr"][:k * E].cpu().numpy().reshape(k, E)
        msg = r["bufs"]["msg"][:k * A].cpu().numpy().reshape(k, A)
        status = r["bufs"]["status"][:k].cpu().numpy()
        words = r["grid"][0].cpu().numpy().view(np.uint32)
        ok_bits = ok_model = 0
        for i in range(k):
            want = model.process(r["cfgs"][i], words, oracle)
            ok_bits += int(status[i] == 1 and (msg[i] == r["sent"][i]).all())
            ok_model += int(status[i] == want["status"] and (msg[i] == want["message"]).all() and (llr[i] == want["llr"]).all())
        rec["check_sent_bits_returned"] = "%d of %d" % (ok_bits, k)
        rec["check_equal_restatement"] = "%d of %d" % (ok_model, k)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        r["plan"].close()
        r["decoder"].close()
    with open(out, "a") as f:
        f.write("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, SIZES, dict(rounds=15, iters=20, timeout=240, out=os.path.join(ROOT, "profiles", "pf2_bench.json"))))
