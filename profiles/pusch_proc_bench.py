#!/usr/bin/env python3
"""PUSCH processor (nrphy_pusch_proc_run) against the same PDUs driven through the existing entry points by hand: 16 slots of 8
PDUs of 52 PRB each -- QPSK / 16-QAM / 64-QAM, 1 and 2 layers, 1 to 4 receive ports, with and without HARQ-ACK and CSI part 1, one
PDU without codeword (24 PRB, what its polar codeword can fill): the mix of tests/test_pusch_processor.py at 52 PRB -- as one plan of 128 PDUs, every PDU on a grid of its
own (52 PRB, 4 ports), received at the SNR of the estimator's link cases so that the decoders do a receiver's work.  The hand chain
is the parent's way and the yardstick: nrphy_pusch_chest_run, nrphy_pusch_demod_run, nrphy_ulsch_demux_run, nrphy_uci_decoder_run
and one nrphy_pusch_decode_batch per PDU with a codeword, the configurations from nrphy_pusch_proc_derive.  One GPU step in a
child process under a time limit, inputs resident in HBM: both run untimed until the clocks have had about 30 ms of load, then
`--rounds` alternating rounds time them with HIP events on an explicit stream (profiles/bench_harness.py); the record holds the
median and the spread, and the rate of a device-to-device copy measured in the same process.  Launches are counted as the nodes
of one captured run (kernels, memsets and copies).  The two outputs are
compared byte for byte after the timed region.  Usage (GPU box, repository root):
python3 profiles/pusch_proc_bench.py [--slots 16] [--iters 10] [--rounds 7]"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_harness as harness

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


def step(rounds, iters, out, slots):
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
    pdus = slot * slots
    derived = derived8 * slots
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
    copy_gbs = harness.copy_rate(s)
    settle = harness.settle(legs, s)
    times = harness.time_rounds(legs, s, rounds, iters)
    hip = hip_runtime()
    nodes = {name: count_nodes(hip, s.cuda_stream, run) for name, run in legs.items()}
    torch.cuda.synchronize()
    # the two ways agree, and the blocks decode
    for run in legs.values():
        run()
    torch.cuda.synchronize()
    got, want = P.read(), H.read()
    res = got["result"]
    rec = {"leg": "pusch_proc", "slots": slots, "pdus_per_slot": 8, "nof_prb": NPRB, "grid_ports": T.NPORTS, "n": n,
           "pdus_with_codeword": int(sum(p.has_codeword for p in pdus)), "pdus_with_uci": int(sum(d.nof_uci != 0 for d in derived)),
           "codeblocks": int(res["nof_codeblocks"].sum()), "iters": iters, "repeats": rounds, "rounds": rounds,
           "settle_rounds": settle, "copy_GBps": round(copy_gbs, 1)}
    for name in legs:
        t = sorted(times[name])
        rec[name + "_ms_per_run"] = round(t[len(t) // 2], 4)
        rec[name + "_ms_min_max"] = [round(t[0], 4), round(t[-1], 4)]
        rec[name + "_us_per_slot"] = round(1e3 * t[len(t) // 2] / slots, 2)
        rec[name + "_launches_per_run"] = nodes[name]
        rec[name + "_launches_per_slot"] = None if nodes[name] is None else round(nodes[name] / slots, 2)
    rec["processor_over_hand_chain"] = round(rec["processor_ms_per_run"] / rec["hand_chain_ms_per_run"], 4)
    rec["check_bytes_equal"] = bool(all(got[k].tobytes() == want[k].tobytes() for k in ("tb", "uci", "harq")))
    rec["check_tb_crc_ok"] = int(res["tb_crc_ok"].sum())
    rec["check_uci_valid"] = int((res["harq_ack_status"] == abi.UCI_STATUS_VALID).sum() + (res["csi_part1_status"] == abi.UCI_STATUS_VALID).sum())
    print(json.dumps(rec), flush=True)
    plan.close()
    chain.close()
    with open(out, "w") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=7, iters=10, timeout=30, out=os.path.join(ROOT, "profiles", "pusch_proc_bench.json"),
                                               slots=16)))
