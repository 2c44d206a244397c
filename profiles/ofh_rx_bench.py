#!/usr/bin/env python3
"""Open Fronthaul uplink frame receiver: one slot's worth of Ethernet frames -- 4 eAxC x 14 symbols x 273 PRB of BFP-9 records under
static compression, cut into frames of at most MTU 1500 (6 frames of up to 52 PRBs per symbol, 336 frames) and MTU 9000 (one frame
per symbol, 56 frames) -- resident in HBM, through nrphy_ofh_rx_run into one grid of 4 ports.

One GPU step in a child process of its own under a time limit.  Per MTU the step builds the frames with the test suite's frame
builder (tests/ofh_rx_model.py), runs untimed calls until the clocks have had about 30 ms of load, then times in alternating
rounds with HIP events on an explicit stream:
  ofh_rx_run          nrphy_ofh_rx_reset + nrphy_ofh_rx_run: the whole call -- host validation, staging of the two descriptor
                      arrays, the ownership table's reset, three launches.  (The reset is there because the same frames are sent
                      again: without it their sequence identifiers are from the past.)
  ofh_ul_write_grid   the section path of the same commit on the same sections, its descriptors built on the host beforehand from
                      the receiver's own records: what a caller pays on the device when all parsing stays on the CPU.
and, with a host clock around the call alone (no synchronise), the host time of each.  After the timed region the two grids are
compared and every record is checked to be accepted.  Hardware counters are not collected here.  Writes profiles/ofh_rx_bench.json.

    python3 profiles/ofh_rx_bench.py            (GPU box, repository root)
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

import bench_harness as harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
EAXC, NSYMB, NOF_PRB, WIDTH = 4, 14, 273, 9
REC = 3 * WIDTH + 1
HEADERS = 14 + 8 + 4 + 4  # Ethernet without a tag, eCPRI, radio application header, section header


def slot_frames(model, cfg, mtu, rng):
    """-> (buffer, [(offset, length)]): symbol by symbol, eAxC by eAxC, fragment by fragment, back to back."""
    per_frame = (mtu - HEADERS) // REC
    frames = []
    seq = [0] * EAXC
    for symbol in range(NSYMB):
        for eaxc in range(EAXC):
            for start in range(0, NOF_PRB, per_frame):
                n = min(per_frame, NOF_PRB - start)
                records = rng.integers(0, 256, n * REC, dtype=np.uint8)
                records[::REC] = rng.integers(0, 8, n)
                frames.append(model.build_frame(cfg, eaxc=eaxc, seq_id=(seq[eaxc] & 0xFF) << 8 | 0x80, sfn8=1, subframe=2, slot=1, symbol=symbol,
                                                sections=[model.section_bytes(start, n if n < 256 else 0, records)]))
                seq[eaxc] += 1
    ranges, pos = [], 0
    for f in frames:
        ranges.append((pos, f.size))
        pos += f.size
    return np.concatenate(frames), ranges


def measure(ctx, lib, abi, model, mtu, rounds, iters):
    import torch
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    cfg = model.default_cfg(ru_nof_prbs=NOF_PRB, ul_eaxc=tuple(range(EAXC)), prach_eaxc=(), compression=(1, WIDTH), prach_compression=(1, WIDTH))
    expects = [model.expect(sfn8=1, subframe=2, slot=1, eaxc=e, nof_prb=NOF_PRB) for e in range(EAXC)]
    buf, ranges = slot_frames(model, cfg, mtu, np.random.default_rng(mtu))
    n, nsubc = len(ranges), 12 * NOF_PRB
    comp = abi.OfhCompressionCfg(1, WIDTH, 1.0)
    pad = lambda v: (C.c_uint16 * 4)(*(list(v) + [0] * (4 - len(v))))
    rx = lib.OfhRx(ctx, abi.OfhRxCfg((C.c_uint8 * 6)(*cfg["mac_dst"]), (C.c_uint8 * 6)(*cfg["mac_src"]), cfg["eth_type"], 0, 0, 0, 1, 1, 14, NOF_PRB, 1,
                                     EAXC, 0, pad(range(EAXC)), pad([]), comp, comp))
    f_arr = (abi.OfhRxFrame * n)(*[abi.OfhRxFrame(o, length, 0) for o, length in ranges])
    e_arr = (abi.OfhRxExpect * EAXC)(*[abi.OfhRxExpect(e["grid_index"], e["sfn8"], e["eaxc"], e["prb_start"], e["nof_prb"], e["context_symbols"],
                                                       e["subframe"], e["slot"], e["filter_index"], e["start_symbol"], e["nof_symbols"], 0)
                                       for e in expects])
    d_frames = torch.from_numpy(buf).cuda()
    d_grid = torch.zeros((1, EAXC, NSYMB, nsubc), dtype=torch.int32, device="cuda")
    d_second = torch.zeros_like(d_grid)
    d_records = torch.zeros(n * C.sizeof(abi.OfhRxRecord), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def rx_run():
        rc = ctx.lib.nrphy_ofh_rx_reset(rx.handle, sp)
        assert rc == abi.OK, rc
        rc = ctx.lib.nrphy_ofh_rx_run(rx.handle, n, f_arr, EAXC, e_arr, C.c_void_p(d_frames.data_ptr()), d_frames.numel(),
                                      C.c_void_p(d_grid.data_ptr()), 1, EAXC, nsubc, C.c_void_p(d_records.data_ptr()), sp)
        assert rc == abi.OK, rc

    rx_run()
    stream.synchronize()
    records = (abi.OfhRxRecord * n).from_buffer_copy(d_records.cpu().numpy().tobytes())
    accepted = all(r.status == 0 and r.seq_skipped == 0 for r in records)
    sections = (abi.OfhUlSection * n)(*[abi.OfhUlSection(r.payload_offset, r.grid_index, r.port, r.symbol, r.start_prb, r.nof_prbs, r.type,
                                                         r.data_width, 0) for r in records])

    def write_grid():
        rc = ctx.lib.nrphy_ofh_ul_write_grid(ctx.handle, n, sections, C.c_void_p(d_frames.data_ptr()), d_frames.numel(),
                                             C.c_void_p(d_second.data_ptr()), 1, EAXC, nsubc, sp)
        assert rc == abi.OK, rc

    launches = {"ofh_rx_run": rx_run, "ofh_ul_write_grid": write_grid}
    settle = harness.settle(launches, stream)  # about 30 ms of load before anything is timed
    ms = {k: [] for k in launches}
    host_us = {k: [] for k in launches}
    for _ in range(rounds):  # alternating: every round times every launch once
        for kind, t in harness.time_rounds(launches, stream, 1, iters).items():
            ms[kind] += t
        for kind, launch in launches.items():  # the host's share: the call alone on an idle stream
            t0 = time.perf_counter()
            launch()
            host_us[kind].append((time.perf_counter() - t0) * 1e6)
            torch.cuda.synchronize()
    payload = EAXC * NSYMB * NOF_PRB * REC
    result = {"mtu": mtu, "frames": n, "frame_bytes_total": int(buf.size), "payload_bytes": payload, "grid_bytes_written": EAXC * NSYMB * nsubc * 4,
              "settle_rounds": settle}
    for kind in launches:
        m = float(np.median(ms[kind]))
        ms_med, ms_min, ms_max = harness.spread(ms[kind])
        result[kind] = {"ms_per_call": ms_med, "ms_min": ms_min, "ms_max": ms_max,
                        "host_us_per_call": round(float(np.median(host_us[kind])), 1),
                        "GBps_payload_plus_grid": round((payload + EAXC * NSYMB * nsubc * 4) / (m * 1e-3) / 1e9, 1)}
    rx_run()
    write_grid()
    stream.synchronize()
    result["check_all_frames_accepted_in_order"] = bool(accepted)
    result["check_grid_equals_section_path"] = bool(torch.equal(d_grid, d_second)) and bool((d_grid != 0).any())
    rx.close()
    return result


def step(rounds, iters, out):
    import backends
    import ofh_rx_model as model
    lib, abi = backends.pkg.lib, backends.abi
    ctx = lib.Context(0)
    result = {"leg": "ofh_rx", "eaxc": EAXC, "symbols": NSYMB, "nof_prb": NOF_PRB, "type": "BFP", "data_width": WIDTH, "static_compression": 1,
              "rounds": rounds, "iters": iters, "counters": "not measured",
              "note": "ofh_rx_run is nrphy_ofh_rx_reset + the whole nrphy_ofh_rx_run call; ofh_ul_write_grid is the whole call with descriptors "
                      "prebuilt on the host; host_us_per_call is the call alone, without a synchronise",
              "cases": [measure(ctx, lib, abi, model, mtu, rounds, iters) for mtu in (1500, 9000)]}
    print(json.dumps(result), flush=True)
    with open(out, "w") as f:
        f.write(json.dumps(result) + "\n")


if __name__ == "__main__":
    sys.exit(harness.bench_main(step, (), dict(rounds=15, iters=20, timeout=240, out=os.path.join(ROOT, "profiles", "ofh_rx_bench.json"))))
