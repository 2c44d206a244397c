#!/usr/bin/env python3
"""UCI on PUSCH launch times.  nrphy_uci_decoder_run: 4096 messages per launch, inputs resident in HBM, three legs --

  polar_n512    A = 100, E = 512   (one block, K = 111, N = 512, no rate matching)
  polar_n1024   A = 300, E = 1087  (one block, K = 311, N = 1024, repetition)
  short_11bit   A = 11,  E = 64    (the 1024 even-valued codewords of the (32, 11) code)

every message its own random payload through noise of standard deviation 8 on +-20.  nrphy_ulsch_demux_run: one leg --

  ulsch_demux   64 codewords of 273 PRB x 13 data symbols x 4 layers x 256-QAM (1.36 MB each) with 2 HARQ-ACK bits puncturing a
                reserved set, 40 CSI part 1 bits and 20 CSI part 2 bits, next to a device-to-device copy of the same bytes
                (torch's copy_), timed in the same rounds: the leg's traffic (input read, streams written) over its time as a
                fraction of the copy's rate.

The GPU step is a child process of its own under a time limit.  It builds the three plans, runs untimed launches until the engine
clocks have had about 30 ms of load (what bench.py's --settle does), then times the plans in alternating rounds with HIP events on
an explicit stream and reports the median round and the spread.  After the timed region every message of every leg is checked:
status VALID and the sent bits, and the first 64 of each leg against the NumPy restatement (tests/uci_model.py).  Hardware counters
are not collected here.  Writes profiles/uci_bench.json.

    python3 profiles/uci_bench.py            (GPU box, repository root)
"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_MESSAGES = 4096
LEGS = (("polar_n512", 100, 512), ("polar_n1024", 300, 1087), ("short_11bit", 11, 64))


def step(rounds, iters, out):
    import torch
    import backends
    import uci_model as model
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    rng = np.random.default_rng(0)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    runs = []
    for name, A, E in LEGS:
        n = N_MESSAGES
        sent = rng.integers(0, 2, (n, A), dtype=np.uint8)
        clean = np.stack([model.codeword_llr(model.encode(sent[i], E, 2)) for i in range(n)]).astype(np.float64)
        llr = np.clip(np.rint(clean + 8.0 * rng.standard_normal(clean.shape)), -120, 120).astype(np.int8)
        plan = lib.UciDecoderPlan(ctx, [abi.make_uci_decoder(A, E, 2)] * n, [i * E for i in range(n)], [i * A for i in range(n)])
        runs.append(dict(name=name, A=A, E=E, n=n, plan=plan, sent=sent, llr=llr, d_llr=torch.from_numpy(llr).cuda(),
                         d_msg=torch.zeros((n, A), dtype=torch.uint8, device="cuda"),
                         d_status=torch.zeros(n, dtype=torch.int32, device="cuda")))
    for r in runs:
        r["launch"] = lambda r=r: r["plan"].run(r["d_llr"], r["d_msg"], r["d_status"], stream=sp)
    # The demultiplexer and the copy it is compared with.
    nbre = 32
    dcfg = dict(modulation=8, nof_layers=4, nof_prb=273, start_symbol_index=0, nof_symbols=14, dmrs_type=0, dmrs_symbol_mask=1 << 2,
                nof_cdm_groups_without_data=2, nof_harq_ack_rvd=60 * nbre, nof_harq_ack_bits=2, nof_enc_harq_ack_bits=40 * nbre,
                nof_csi_part1_bits=40, nof_enc_csi_part1_bits=120 * nbre, nof_csi_part2_bits=20, nof_enc_csi_part2_bits=90 * nbre,
                rnti=0x4601, n_id=77)
    n_cw = 64
    nof_sch, total = lib.ulsch_demux_sizes(abi.make_ulsch_demux(**dcfg))
    sizes = (total, nof_sch, dcfg["nof_enc_harq_ack_bits"], dcfg["nof_enc_csi_part1_bits"], dcfg["nof_enc_csi_part2_bits"])
    offs = [[i * ((sz + 255) // 256 * 256) for i in range(n_cw)] for sz in sizes]
    cw = rng.integers(-127, 128, total).astype(np.int8)
    host_in = np.zeros(offs[0][-1] + total, np.int8)
    for o in offs[0]:
        host_in[o:o + total] = cw
    d_cw = torch.from_numpy(host_in).cuda()
    d_streams = [torch.zeros(o[-1] + sz, dtype=torch.int8, device="cuda") for o, sz in zip(offs[1:], sizes[1:])]
    dplan = lib.UlschDemuxPlan(ctx, [abi.make_ulsch_demux(**dcfg)] * n_cw, *offs)
    d_copy = torch.empty_like(d_cw)
    demux = dict(name="ulsch_demux", launch=lambda: dplan.run(d_cw, *d_streams, stream=sp))

    def copy_launch():
        with torch.cuda.stream(stream):
            d_copy.copy_(d_cw)
    copy = dict(name="copy", launch=copy_launch)
    uci_runs = list(runs)
    runs = uci_runs + [demux, copy]
    launches = {r["name"]: r["launch"] for r in runs}
    settle = harness.settle(launches, stream)  # about 30 ms of load before anything is timed
    times = harness.time_rounds(launches, stream, rounds, iters)  # alternating: every round times every leg once
    records = []
    for r in uci_runs:
        ms = float(np.median(times[r["name"]]))
        ms_med, ms_min, ms_max = harness.spread(times[r["name"]])
        got, status = r["d_msg"].cpu().numpy(), r["d_status"].cpu().numpy()
        ok_sent = int(((status == 1) & (got == r["sent"]).all(axis=1)).sum())
        ok_model = 0
        for i in range(64):
            want, want_status = model.decode(r["llr"][i], r["A"], 2)
            ok_model += int(status[i] == want_status and np.array_equal(got[i], want))
        rec = {"leg": "uci_decoder", "case": r["name"], "message_length": r["A"], "llr_length": r["E"], "n": r["n"], "rounds": rounds,
               "iters": iters, "settle_launches": settle, "ms_per_launch": ms_med, "ms_min": ms_min,
               "ms_max": ms_max, "messages_per_s": round(r["n"] / (ms * 1e-3)), "ns_per_message": round(ms * 1e6 / r["n"], 2),
               "input_GBps": round(r["n"] * r["E"] / (ms * 1e-3) / 1e9, 3), "counters": "not measured",
               "check_valid_with_sent_bits": "%d of %d" % (ok_sent, r["n"]), "check_equal_restatement": "%d of 64" % ok_model}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        r["plan"].close()
    # The demultiplexer: every codeword's streams against the restatement's answer for the one codeword they all carry.
    want = model.ulsch_demultiplex(dcfg, cw)
    got = [t.cpu().numpy() for t in d_streams]
    ok = sum(all(got[k][offs[k + 1][i]:offs[k + 1][i] + sizes[k + 1]].tobytes() == want[k].tobytes() for k in range(4)) for i in range(n_cw))
    ms, ms_copy = float(np.median(times["ulsch_demux"])), float(np.median(times["copy"]))
    ms_med, ms_min, ms_max = harness.spread(times["ulsch_demux"])
    moved = n_cw * (total + sum(sizes[1:]))  # bytes read and written by the demultiplexer
    rate, copy_rate = moved / (ms * 1e-3) / 1e9, 2 * d_cw.numel() / (ms_copy * 1e-3) / 1e9
    rec = {"leg": "ulsch_demux", "case": "273prb_13sym_4layers_256qam", "n": n_cw, "codeword_bytes": total, "rounds": rounds, "iters": iters,
           "ms_per_launch": ms_med, "ms_min": ms_min, "ms_max": ms_max,
           "GBps_read_plus_written": round(rate, 1), "copy_ms": round(ms_copy, 5), "copy_GBps_read_plus_written": round(copy_rate, 1),
           "fraction_of_copy_rate": round(rate / copy_rate, 3), "counters": "not measured",
           "check_equal_restatement": "%d of %d" % (ok, n_cw)}
    print(json.dumps(rec), flush=True)
    records.append(rec)
    dplan.close()
    with open(out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in records))


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=15, iters=20, timeout=300, out=os.path.join(ROOT, "profiles", "uci_bench.json"))))
