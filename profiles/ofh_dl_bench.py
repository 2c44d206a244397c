#!/usr/bin/env python3
"""Open Fronthaul downlink transmit throughput: slots of 4 ports x 14 symbols x 273 PRB, BFP 9, one descriptor per (slot, port,
symbol), static compression header, frames for an MTU of 9000 (one 7678-byte frame per symbol) and of 1500 (five 1490-byte frames
and one of 398), batches of 1 and of 16 slots; grids and frames resident in HBM.

One GPU step in a child process of its own under a time limit.  It runs untimed launches until the engine clocks have had about
30 ms of load, then times in alternating rounds with HIP events on an explicit stream: nrphy_ofh_dl_write_frames (the whole call:
validation on the host, the staging of the descriptors, one launch) at both MTUs, and as the baseline nrphy_ofh_compress over the
same rows -- the same arithmetic without headers or fragments, and a bare launch without descriptors.  It reports the median round
and the spread, the bytes written (frames, or records for the baseline), bytes written per second, and bytes read plus written per
second against the 8 TB/s HBM roof.  After the timed region the MTU-9000 frames are checked against the baseline's records (one
fragment per symbol is one compress() call of the whole row) and the first symbol of both against the NumPy restatement
(tests/ofh_dl_model.py).  Hardware counters are not collected here.  Writes profiles/ofh_dl_bench.json.

    python3 profiles/ofh_dl_bench.py            (GPU box, repository root)
"""
import ctypes as C
import json
import os
import sys

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
PORTS, NSYMB, NOF_PRB, WIDTH = 4, 14, 273, 9
HBM_ROOF_GBPS = 8000.0


def step(rounds, iters, out):
    import torch
    import backends
    import ofh_dl_model as model
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    cfg = abi.OfhCompressionCfg(1, WIDTH, 1.0)
    rec, nsubc, max_slots = 3 * WIDTH + 1, 12 * NOF_PRB, 16
    torch.manual_seed(0)
    max_rows = max_slots * PORTS * NSYMB
    d_grid = (torch.randn((max_rows, nsubc, 2), device="cuda") * 0.2).to(torch.bfloat16).view(torch.int32).reshape(max_rows, nsubc).contiguous()
    d_records = torch.zeros(max_rows * NOF_PRB * rec, dtype=torch.uint8, device="cuda")
    mac = lambda *b: (C.c_uint8 * 6)(*b)
    launches, info, keep = {}, {}, {}
    for mtu in (9000, 1500):
        flow = abi.OfhDlFlow(mac(0xAA, 0xBB, 0xCC, 0xDD, 0xEE, 0x11), mac(0xAA, 0xBB, 0xCC, 0xDD, 0xEE, 0x22), 1, 0xAEFE, mtu, NOF_PRB, 1, cfg)
        frags = lib.ofh_dl_fragments(flow)
        stride = (mtu + 15) // 16 * 16
        frame_bytes = sum(f[2] for f in frags)
        d_frames = torch.zeros(max_rows * len(frags) * stride, dtype=torch.uint8, device="cuda")
        keep[mtu] = (flow, frags, stride, d_frames)
        for slots in (1, 16):
            rows = slots * PORTS * NSYMB
            symbols = [abi.OfhDlSymbol(r * len(frags) * stride, 0, r // (PORTS * NSYMB), (r // NSYMB) % PORTS, (r // NSYMB) % PORTS, r // (PORTS * NSYMB) // 20,
                                       (r // (PORTS * NSYMB) // 2) % 10, r // (PORTS * NSYMB) % 2, r % NSYMB, (r * len(frags)) & 0xFF,
                                       (C.c_uint8 * 2)(0, 0)) for r in range(rows)]
            arr = (abi.OfhDlSymbol * rows)(*symbols)
            flows = (abi.OfhDlFlow * 1)(flow)

            def write_frames(arr=arr, flows=flows, rows=rows, slots=slots, d_frames=d_frames, stride=stride):
                rc = ctx.lib.nrphy_ofh_dl_write_frames(ctx.handle, 1, flows, rows, arr, C.c_void_p(d_grid.data_ptr()), slots, PORTS, nsubc,
                                                       C.c_void_p(d_frames.data_ptr()), d_frames.numel(), stride, sp)
                assert rc == abi.OK, rc

            name = "ofh_dl_write_frames_mtu%d_slots%d" % (mtu, slots)
            launches[name] = write_frames
            info[name] = dict(rows=rows, frames=rows * len(frags), bytes_written=rows * frame_bytes)
    for slots in (1, 16):
        rows = slots * PORTS * NSYMB
        name = "ofh_compress_slots%d" % slots
        launches[name] = lambda rows=rows: ctx.ofh_compress(cfg, rows, NOF_PRB, d_grid, d_records, stream=sp)
        info[name] = dict(rows=rows, frames=0, bytes_written=rows * NOF_PRB * rec)
    torch.cuda.synchronize()
    settle = harness.settle(launches, stream)  # about 30 ms of load before anything is timed
    ms = harness.time_rounds(launches, stream, rounds, iters)  # alternating: every round times every launch once
    result = {"leg": "ofh_dl", "ports": PORTS, "symbols": NSYMB, "nof_prb": NOF_PRB, "type": "BFP", "data_width": WIDTH, "record_bytes": rec,
              "static_compression": 1, "rounds": rounds, "iters": iters, "settle_rounds": settle, "hbm_roof_GBps": HBM_ROOF_GBPS,
              "counters": "not measured",
              "fragments": {str(mtu): keep[mtu][1] for mtu in keep},
              "note": "ofh_dl_write_frames is the whole call: host validation, the staging of the descriptors and one launch; "
                      "ofh_compress is a bare launch over the same rows"}
    for kind in launches:
        m = float(np.median(ms[kind]))
        ms_med, ms_min, ms_max = harness.spread(ms[kind])
        written, read = info[kind]["bytes_written"], info[kind]["rows"] * NOF_PRB * 48
        result[kind] = {"rows": info[kind]["rows"], "frames": info[kind]["frames"], "bytes_written": written, "ms_per_call": ms_med,
                        "ms_min": ms_min, "ms_max": ms_max, "GBps_written": round(written / (m * 1e-3) / 1e9, 2),
                        "ns_per_byte_written": round(m * 1e6 / written, 5),
                        "share_of_hbm_roof_read_plus_written": round((read + written) / (m * 1e-3) / 1e9 / HBM_ROOF_GBPS, 4)}
    for kind, launch in launches.items():
        if kind.endswith("slots16"):
            launch()
    stream.synchronize()
    rows = max_rows
    flow, frags, stride, d_frames = keep[9000]
    body = d_frames.reshape(rows, stride)[:, 34:34 + NOF_PRB * rec]
    result["check_mtu9000_records_equal_ofh_compress"] = bool(torch.equal(body, d_records.reshape(rows, NOF_PRB * rec)))
    oracle = backends.oracle()
    compress = lambda typ, width, s, prbs: oracle.ofh_compress(abi.OfhCompressionCfg(typ, width, s), prbs)
    row0 = d_grid[0].cpu().numpy().view(np.uint16).reshape(nsubc, 2)
    ok = True
    for mtu in keep:
        flow, frags, stride, d_frames = keep[mtu]
        fd = dict(mac_dst=list(flow.mac_dst), mac_src=list(flow.mac_src), tci=1, eth_type=0xAEFE, mtu=mtu, ru_nof_prbs=NOF_PRB, static_compression=1,
                  type=1, data_width=WIDTH, iq_scaling=1.0)
        want = model.symbol_frames(fd, dict(eaxc=0, sfn=0, subframe=0, slot=0, symbol=0, seq_id=0), row0, compress)
        got = d_frames[:len(frags) * stride].cpu().numpy()
        ok = ok and all(np.array_equal(got[k * stride:k * stride + w.size], w) for k, w in enumerate(want))
    result["check_first_symbol_equals_restatement"] = bool(ok)
    print(json.dumps(result), flush=True)
    with open(out, "w") as f:
        f.write(json.dumps(result) + "\n")


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=15, iters=20, timeout=240, out=os.path.join(ROOT, "profiles", "ofh_dl_bench.json"))))
