#!/usr/bin/env python3
"""PUSCH processor (nrphy_pusch_proc_run) against the same PDUs driven through the existing entry points by hand: 16 slots of 8
PDUs of 52 PRB each -- QPSK / 16-QAM / 64-QAM, 1 and 2 layers, 1 to 4 receive ports, with and without HARQ-ACK and CSI part 1, one
PDU without codeword (24 PRB, what its polar codeword can fill): the mix of tests/test_pusch_processor.py at 52 PRB -- as one plan of 128 PDUs, every PDU on a grid of its
own (52 PRB, 4 ports), received at the SNR of the estimator's link cases so that the decoders do a receiver's work.  The hand chain
is the parent's way and the yardstick: nrphy_pusch_chest_run, nrphy_pusch_demod_run, nrphy_ulsch_demux_run, nrphy_uci_decoder_run
and one nrphy_pusch_decode_batch per PDU with a codeword, the configurations from nrphy_pusch_proc_derive.  Both are timed with
HIP events on an explicit stream after warm-up, inputs resident in HBM, `--repeats` times each in alternation; the record holds the
median and the spread.  Launches are counted as the nodes of one captured run (kernels, memsets and copies).  The two outputs are
compared byte for byte after the timed region.  Usage (GPU box, repository root):
python3 profiles/pusch_proc_bench.py [--slots 16] [--iters 10] [--repeats 7]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NPRB = 52


def hip_runtime():
    """The HIP runtime this process has loaded (PyTorch's)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    return None


def count_nodes(hip, stream, run):
    """Nodes of one captured run, or None where the runtime cannot tell."""
    if hip is None:
        return None
    graph, n = C.c_void_p(), C.c_size_t(0)
    if hip.hipStreamBeginCapture(C.c_void_p(stream), 0) != 0:
        return None
    run()
    if hip.hipStreamEndCapture(C.c_void_p(stream), C.byref(graph)) != 0:
        return None
    rc = hip.hipGraphGetNodes(graph, None, C.byref(n))
    hip.hipGraphDestroy(graph)
    return int(n.value) if rc == 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    import torch
    import backends
    import test_pusch_processor as T
    lib, abi = backends.pkg.lib, backends.abi
    nsubc = 12 * NPRB  # the test's transmitter and hand chain take the grid's width
    ctx = lib.Context(0)
    opts = T.OPTIONS
    base = T.pdu_args()
    slot = []
    for k, name in enumerate("abcdefac"):
        # the PDU without codeword fills its allocation with CSI part 1, and a polar codeword holds at most 8192 soft bits: 24 PRB
        a = dict(base[name], prbs=range(NPRB if name != "e" else 24), n_id=20 + k, scrambling_id=200 + k)
        if "dc_position" in a:
            a["dc_position"] = 12 * NPRB // 2
        if a.get("tb_size_bytes"):
            has_uci = a.get("nof_harq_ack", 0) + a.get("nof_csi_part1", 0) > 0
            tb_bits = lib.tbs_calculate(14, 12 * len(a["dmrs_symbols"]), 18 if has_uci else 0, a["modulation"], a["target_code_rate"],
                                        a["nof_layers"], NPRB)
            a.update(tb_size_bytes=tb_bits // 8, ldpc_base_graph=T.base_graph(tb_bits, a["target_code_rate"]))
        slot.append(abi.make_pusch_pdu(**a))
    derived8 = [lib.pusch_proc_derive(p, opts, T.NPORTS, nsubc) for p in slot]
    assert None not in derived8
    rng = np.random.default_rng(1)
    sent8 = [T.transmit(ctx, p, d, rng, nsubc) for p, d in zip(slot, derived8)]
    pdus = slot * args.slots
    derived = derived8 * args.slots
    n = len(pdus)
    grids = np.stack([T.noisy(sent8[i % 8], T.GOOD_SNR[(pdus[i].modulation, pdus[i].nof_tx_layers)], rng) for i in range(n)])
    d_grid = T.dev(T.as_i32(grids))
    layout = T.Layout(pdus, opts)
    gidx = list(range(n))
    plan = lib.PuschProcPlan(ctx, pdus, opts, gidx, n, T.NPORTS, nsubc, layout.soft, layout.state, layout.tb, layout.uci)
    chain = T.HandChain(ctx, pdus, derived, layout, n, gidx, nsubc)
    P, H = T.Buffers(layout, n), T.Buffers(layout, n)
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    legs = {"processor": lambda: plan.run(d_grid, P.harq, P.tb, P.uci, P.result, stream=sp),
            "hand_chain": lambda: chain.run(d_grid, H, stream=sp)}
    torch.cuda.synchronize()
    for run in legs.values():
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in legs}
    for r in range(args.repeats):
        for name in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            e0.record(s)
            for _ in range(args.iters):
                legs[name]()
            e1.record(s)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters)
    hip = hip_runtime()
    nodes = {name: count_nodes(hip, s.cuda_stream, run) for name, run in legs.items()}
    torch.cuda.synchronize()
    # the two ways agree, and the blocks decode
    for run in legs.values():
        run()
    torch.cuda.synchronize()
    got, want = P.read(), H.read()
    res = got["result"]
    rec = {"leg": "pusch_proc", "slots": args.slots, "pdus_per_slot": 8, "nof_prb": NPRB, "grid_ports": T.NPORTS, "n": n,
           "pdus_with_codeword": int(sum(p.has_codeword for p in pdus)), "pdus_with_uci": int(sum(d.nof_uci != 0 for d in derived)),
           "codeblocks": int(res["nof_codeblocks"].sum()), "iters": args.iters, "repeats": args.repeats}
    for name in legs:
        t = sorted(times[name])
        rec[name + "_ms_per_run"] = round(t[len(t) // 2], 4)
        rec[name + "_ms_min_max"] = [round(t[0], 4), round(t[-1], 4)]
        rec[name + "_us_per_slot"] = round(1e3 * t[len(t) // 2] / args.slots, 2)
        rec[name + "_launches_per_run"] = nodes[name]
        rec[name + "_launches_per_slot"] = None if nodes[name] is None else round(nodes[name] / args.slots, 2)
    rec["processor_over_hand_chain"] = round(rec["processor_ms_per_run"] / rec["hand_chain_ms_per_run"], 4)
    rec["check_bytes_equal"] = bool(all(got[k].tobytes() == want[k].tobytes() for k in ("tb", "uci", "harq")))
    rec["check_tb_crc_ok"] = int(res["tb_crc_ok"].sum())
    rec["check_uci_valid"] = int((res["harq_ack_status"] == abi.UCI_STATUS_VALID).sum() + (res["csi_part1_status"] == abi.UCI_STATUS_VALID).sum())
    print(json.dumps(rec), flush=True)
    plan.close()
    chain.close()


if __name__ == "__main__":
    main()
