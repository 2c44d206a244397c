#!/usr/bin/env python3
"""Open Fronthaul uplink receive throughput: 64 grids x 4 ports x 14 symbols x 273 PRB of BFP-9 records, one section per (grid,
port, symbol) -- 3584 sections --, payload and grids resident in HBM.

One GPU step in a child process of its own under a time limit.  The step compresses a random batch of grids with
nrphy_ofh_compress (so that the bytes are what a radio unit would send), runs untimed launches until the engine clocks have had
about 30 ms of load, then times in alternating rounds with HIP events on an explicit stream: nrphy_ofh_ul_write_grid (which
includes its validation on the host and the staging of the 3584 descriptors), nrphy_ofh_decompress on the same bytes, and, for
context, nrphy_ofh_compress at the same shape, the mirror kernel.  It reports the median round and the spread, the bytes in plus the
bytes out, the rate, and its share of the 8 TB/s HBM roof and of a device-to-device copy measured in the same process.  After the
timed region both outputs are checked against each other and, on the first grid, against the NumPy restatement
(tests/ofh_ul_model.py).  Hardware counters are not collected here.  Writes profiles/ofh_ul_bench.json.

    python3 profiles/ofh_ul_bench.py            (GPU box, repository root)
"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GRIDS, PORTS, NSYMB, NOF_PRB, WIDTH = 64, 4, 14, 273, 9
HBM_ROOF_GBPS = 8000.0


def step(rounds, iters, out):
    import torch
    import backends
    import ofh_ul_model as model
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    cfg = abi.OfhCompressionCfg(1, WIDTH, 1.0)
    rec, rows, nsubc = 3 * WIDTH + 1, GRIDS * PORTS * NSYMB, 12 * NOF_PRB
    torch.manual_seed(0)
    d_src = (torch.randn((rows, nsubc, 2), device="cuda") * 0.2).to(torch.bfloat16).view(torch.int32).reshape(rows, nsubc).contiguous()
    d_bytes = torch.zeros(rows * NOF_PRB * rec, dtype=torch.uint8, device="cuda")
    d_grid = torch.zeros((GRIDS, PORTS, NSYMB, nsubc), dtype=torch.int32, device="cuda")
    d_rows = torch.zeros((rows, nsubc), dtype=torch.int32, device="cuda")
    sections = [abi.OfhUlSection(r * NOF_PRB * rec, r // (PORTS * NSYMB), (r // NSYMB) % PORTS, r % NSYMB, 0, NOF_PRB, 1, WIDTH, 0)
                for r in range(rows)]
    arr = (abi.OfhUlSection * rows)(*sections)
    torch.cuda.synchronize()
    ctx.ofh_compress(cfg, rows, NOF_PRB, d_src, d_bytes, stream=sp)
    stream.synchronize()

    def write_grid():
        rc = ctx.lib.nrphy_ofh_ul_write_grid(ctx.handle, rows, arr, C.c_void_p(d_bytes.data_ptr()), d_bytes.numel(), C.c_void_p(d_grid.data_ptr()),
                                             GRIDS, PORTS, nsubc, sp)
        assert rc == abi.OK, rc

    nbytes = rows * NOF_PRB * (rec + 48)
    launches = {"ofh_ul_write_grid": write_grid,
                "ofh_decompress": lambda: ctx.ofh_decompress(cfg, rows, NOF_PRB, d_bytes, d_rows, stream=sp),
                "ofh_compress": lambda: ctx.ofh_compress(cfg, rows, NOF_PRB, d_src, d_bytes, stream=sp)}
    copy_gbs = harness.copy_rate(stream)
    settle = harness.settle(launches, stream)  # about 30 ms of load before anything is timed
    ms = harness.time_rounds(launches, stream, rounds, iters)  # alternating: every round times every launch once
    result = {"leg": "ofh_ul", "grids": GRIDS, "ports": PORTS, "symbols": NSYMB, "nof_prb": NOF_PRB, "type": "BFP", "data_width": WIDTH,
              "sections": rows, "record_bytes": rec, "bytes_in_plus_out": nbytes, "rounds": rounds, "iters": iters, "settle_rounds": settle,
              "copy_GBps": round(copy_gbs, 1), "hbm_roof_GBps": HBM_ROOF_GBPS, "counters": "not measured",
              "note": "ofh_ul_write_grid is the whole call: host validation and the staging of the descriptors included"}
    for kind in launches:
        m = float(np.median(ms[kind]))
        ms_med, ms_min, ms_max = harness.spread(ms[kind])
        gbs = nbytes / (m * 1e-3) / 1e9
        result[kind] = {"ms_per_call": ms_med, "ms_min": ms_min, "ms_max": ms_max, "GBps": round(gbs, 1),
                        "share_of_hbm_roof": round(gbs / HBM_ROOF_GBPS, 4), "share_of_copy_rate": round(gbs / copy_gbs, 4)}
    write_grid()
    launches["ofh_decompress"]()
    stream.synchronize()
    result["check_grid_equals_rows"] = bool(torch.equal(d_grid.reshape(rows, nsubc), d_rows))
    wire = d_bytes[:PORTS * NSYMB * NOF_PRB * rec].cpu().numpy()
    want = model.words(model.decompress(wire, 1, WIDTH)).reshape(PORTS, NSYMB, nsubc)
    result["check_first_grid_equals_restatement"] = bool(np.array_equal(d_grid[0].cpu().numpy().view(np.uint32), want))
    print(json.dumps(result), flush=True)
    with open(out, "w") as f:
        f.write(json.dumps(result) + "\n")


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=15, iters=20, timeout=240, out=os.path.join(ROOT, "profiles", "ofh_ul_bench.json"))))
