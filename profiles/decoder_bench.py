"""LDPC decoder throughput (BASELINE config 5 shape: the 104 codeblocks of a config-3 slot, BG1 Zc=384, E=8960), and the rate
dematcher in front of it.  One GPU step in a child process under a time limit; every leg runs untimed until the clocks have had
about 30 ms of load and is then timed in rounds with HIP events on an explicit stream, median and spread
(profiles/bench_harness.py); the rate of a device-to-device copy is measured in the same process.
Usage: python3 profiles/decoder_bench.py [--n-slots 64] [--max-iterations 6]   (run on the GPU box)"""
import importlib
import json
import os
import sys
import time

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step(rounds, iters, out, n_slots, max_iterations):
    import torch
    pkg = importlib.import_module("srsran-edgeric-5g_amd")
    abi, lib = pkg.abi, pkg.lib
    ctx = lib.Context(0)
    bg, zc, e, n_cb = 1, 384, 8960, 104 * n_slots
    k = 22 * zc
    rng = np.random.default_rng(5)
    msgs = rng.integers(0, 256, (n_cb, k // 8), dtype=np.uint8)
    d_msg = torch.from_numpy(msgs).cuda()
    d_cb = torch.zeros((n_cb, e // 8), dtype=torch.uint8, device="cuda")
    ctx.ldpc_encode(bg, zc, d_msg, k // 8, e, d_cb, e // 8, n_cb)
    torch.cuda.synchronize()
    bits = np.unpackbits(d_cb.cpu().numpy(), axis=1).astype(np.float32)
    nof_llr = 66 * zc
    llr = np.zeros((n_cb, nof_llr), np.int8)
    llr[:, :e] = np.clip(np.rint((1 - 2 * bits) * 20 + rng.normal(0, 8.0, bits.shape)), -120, 120).astype(np.int8)
    d_llr = torch.from_numpy(llr).cuda()
    out_bits = torch.zeros((n_cb, k // 8), dtype=torch.uint8, device="cuda")
    its = torch.zeros((n_cb,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    copy_gbs = harness.copy_rate(stream)

    def timed(launch):
        def on_stream():
            with torch.cuda.stream(stream):
                launch()
        settle = harness.settle([on_stream], stream)
        ms, ms_min, ms_max = harness.spread(harness.time_rounds({"leg": on_stream}, stream, rounds, iters)["leg"])
        return ms, {"ms_min": ms_min, "ms_max": ms_max, "settle_launches": settle}

    res = {}
    for crc, label in ((0, "fixed_iterations"), (0x24B, "early_stop")):
        cfg = abi.LdpcDecoderCfg(bg, zc, 0, crc, nof_llr, max_iterations, 0.8)
        ms, more = timed(lambda: ctx.ldpc_decode(cfg, n_cb, d_llr, nof_llr, out_bits, k // 8, its, stream.cuda_stream))
        res[label] = {"ms": ms, "codeblocks_per_s": n_cb / ms * 1e3, "slots_per_s": n_slots / ms * 1e3,
                      "info_gbps": n_cb * (k - 24) / ms * 1e-6, "mean_iterations": float(its.float().mean()), **more}
    # rate dematcher in front (256-QAM, rv 0, new data, then a retransmission combined into the same soft buffers)
    rm_in = torch.from_numpy(np.ascontiguousarray(llr[:, :e])).cuda()
    soft = torch.zeros((n_cb, nof_llr), dtype=torch.int8, device="cuda")
    dcfg = abi.LdpcRateDematcherCfg(bg, zc, 0, 8, 0, 72, e)
    for new_data, label in ((True, "rate_dematch_new_data"), (False, "rate_dematch_combine")):
        ms, more = timed(lambda: ctx.ldpc_rate_dematch(dcfg, n_cb, rm_in, e, soft, nof_llr, new_data, stream.cuda_stream))
        gb = n_cb * (e + nof_llr * (1 if new_data else 2)) * 1e-9
        res[label] = {"ms": ms, "codeblocks_per_s": n_cb / ms * 1e3, "algorithmic_GBps": gb / ms * 1e3, **more}
    # without a CRC in the random messages early stop never fires: the second leg is the CRC cost on top
    # CPU context: the reference's own decoder (oracle/_ref, AVX2 and generic) on a few of the same codeblocks, 1 thread
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import backends
        ref = backends.ref()
        if ref is None:
            raise RuntimeError("oracle/_ref not built")
        for simd, label in ((1, "reference_avx2"), (0, "reference_generic")):
            t0, n = time.perf_counter(), 0
            while time.perf_counter() - t0 < 2.0:
                ref.ldpc_decode(bg, zc, 0, 0, max_iterations, 0.8, llr[n % n_cb], simd=simd)
                n += 1
            dt = time.perf_counter() - t0
            res[label] = {"codeblocks_per_s": n / dt, "info_gbps": n * (k - 24) / dt * 1e-9, "threads": 1}
    except Exception as e:  # the compiled reference is optional here
        res["reference"] = "unavailable: %s" % e
    rec = {"n_slots": n_slots, "n_cb": n_cb, "max_iterations": max_iterations, "rounds": rounds, "iters": iters,
           "copy_GBps": round(copy_gbs, 1), **res}
    print(json.dumps(rec), flush=True)
    if out:
        with open(out, "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=15, iters=5, timeout=30, out="", n_slots=64, max_iterations=6)))
