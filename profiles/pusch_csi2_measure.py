#!/usr/bin/env python3
"""What the CSI part 2 route of the PUSCH processor costs.  Recorded, not gated.

(1) proc: nrphy_pusch_proc_run on the batch (a)-(f) of tests/test_pusch_processor.py, for this library and for another build of it
    (--other-lib, the parent commit's: the null-pointer tests that the demultiplexer, UCI decoder and rate-dematcher kernels gained
    must not show).  The two libraries run in alternating processes through NRPHY_LIB_SO, twice each.
(2) csi2: (h) and (i) of tests/pusch_csi2_cases.py through nrphy_pusch_csi2_run against the same PDUs without description through
    nrphy_pusch_proc_run: the price of the extra launches -- per PDU one select (shared by the plan), one demultiplex and one UCI
    decode (shared by the plan), and the rate-dematcher launches of every variant.

HIP events on an explicit stream around rounds of runs, after about 30 ms of untimed load; median round and spread.  Every
measurement is one GPU step: a child process of its own under a time limit, and the next one starts only if the one before ended
well.  Appends one JSON record per figure to profiles/pusch_csi2.txt.  (The script is not called *_bench.py:
tests/test_bench_harness.py counts those.)

    python3 profiles/pusch_csi2_measure.py [--other-lib PATH]            (GPU box, repository root)
"""
import argparse
import ctypes as C
import json
import os
import sys

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(launch, stream, rounds, iters):
    settle = harness.settle([launch], stream)  # about 30 ms of load before anything is timed
    ms, ms_min, ms_max = harness.spread(harness.time_rounds({"launch": launch}, stream, rounds, iters)["launch"])
    return {"ms": ms, "ms_min": ms_min, "ms_max": ms_max, "settle_runs": settle}


def step_proc(label, rounds, iters):
    import torch
    import backends
    import test_pusch_processor as T
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    sc = T.Scenario(ctx, "abcdef", T.OPTIONS)
    d_grid = T.dev(T.as_i32(sc.grids(True)))
    plan = sc.plan(ctx)
    B = T.Buffers(sc.layout, len(sc.names))
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    launch = lambda: plan.run(d_grid, B.harq, B.tb, B.uci, B.result, stream=sp)
    launch()
    torch.cuda.synchronize()
    assert all(B.read()["result"]["tb_crc_ok"] == [p.has_codeword for p in sc.pdus])
    t = timed(launch, stream, rounds, iters)
    plan.close()
    return [dict(t, leg="proc", library=label, pdus="abcdef", rounds=rounds, iters=iters)]


def step_csi2(rounds, iters):
    import torch
    import backends
    import test_pusch_csi2 as M
    lib = backends.pkg.lib
    ctx = lib.Context(0)
    sizes = dict(h=36, i=150)
    sc = M.Scenario(ctx, "hi", sizes)

    plain = M.Scenario(ctx, "hi", {}, described=False)  # (h) and (i) without description, sent without part 2
    d_grid, d_plain = M.dev(M.as_i32(sc.grids())), M.dev(M.as_i32(plain.grids()))
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    L, PL = sc.layout, plain.layout
    with_plan = sc.plan(ctx)
    without_plan = lib.PuschProcPlan(ctx, plain.pdus, M.OPTIONS, plain.gidx, 2, M.NPORTS, M.NSUBC, PL.soft, PL.state, PL.tb, PL.uci)
    B, P = M.Buffers(L, 2), M.Buffers(PL, 2)
    legs = [("pusch_csi2_run", lambda: with_plan.run(d_grid, B.harq, B.tb, B.uci, B.result, B.csi2, stream=sp)),
            ("pusch_proc_run without description", lambda: without_plan.run(d_plain, P.harq, P.tb, P.uci, P.result, stream=sp))]
    out = []
    variants = [len(v.sizes) for v in sc.sent_as]
    for _ in range(2):  # the legs in turn, twice: the spread between the two passes is run-to-run spread inside one process
        for name, launch in legs:
            launch()
            torch.cuda.synchronize()
            t = timed(launch, stream, rounds, iters)
            out.append(dict(t, leg="csi2", run=name, pdus="hi", sizes=sizes, variants=variants, rounds=rounds, iters=iters))
    got, ref = B.read(), P.read()
    assert [int(r["variant"]) for r in got["csi2"]] == [v.index for v in sc.sent_as]
    assert (got["result"]["tb_crc_ok"] == 1).all() and (ref["result"]["tb_crc_ok"] == 1).all()  # both routes decode what they time
    with_plan.close()
    without_plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="", help="run one step in this process (what the driver starts)")
    ap.add_argument("--label", default="this")
    ap.add_argument("--other-lib", default="", help="another build of the library to compare nrphy_pusch_proc_run with")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pusch_csi2.txt"))
    args = ap.parse_args()
    if args.step:
        recs = step_proc(args.label, args.rounds, args.iters) if args.step == "proc" else step_csi2(args.rounds, args.iters)
        with open(args.out, "a") as f:
            for r in recs:
                print(json.dumps(r), flush=True)
                f.write(json.dumps(r) + "\n")
        return 0
    common = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--iters", str(args.iters), "--out", args.out]
    steps = []
    libraries = ([("other", {"NRPHY_LIB_SO": os.path.abspath(args.other_lib)})] if args.other_lib else []) + [("this", {})]
    for turn in range(2):
        for label, env in libraries:
            steps.append(("pusch_csi2_proc_%s_%d" % (label, turn), common + ["--step", "proc", "--label", label], env, args.timeout))
    steps.append(("pusch_csi2_routes", common + ["--step", "csi2"], {}, args.timeout))
    return harness.run_steps(steps, harness.LOG_DIR)


if __name__ == "__main__":
    sys.exit(main())
