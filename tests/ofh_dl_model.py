"""NumPy restatement of the Open Fronthaul downlink transmit (include/mi355_nrphy.h: nrphy_ofh_dl_fragments,
nrphy_ofh_dl_write_frames): srsRAN-5G-ER's ofh_uplane_fragment_size_calculator as data_flow_uplane_downlink_data_impl drives it, and
the bytes vlan_frame_builder_impl, ecpri::packet_builder_impl and the static / dynamic user-plane message builders put in front of
the PRB records.  The records themselves are not restated: they come from a compressor the caller passes (the oracle's
ofh_compress, pinned to the reference's AVX2 compressors), called once per fragment as the reference calls compress().
tests/test_ofh_downlink.py pins this to recordings of the reference."""
import numpy as np

from ofh_ul_model import mix

NONE, BFP = 0, 1
ETH_HEADER, ECPRI_HEADER = 18, 8
MIN_FRAME, MAX_FRAME = 64, 9600


def record_bytes(typ, width):
    return 3 * width + (1 if typ == BFP else 0)


def header_bytes(static_compression):
    return ETH_HEADER + ECPRI_HEADER + (8 if static_compression else 10)


def fragments(mtu, ru_nof_prbs, static_compression, typ, width):
    """[(start_prb, nof_prbs, frame_bytes)], or None where the reference never finishes (a frame that cannot hold one record).

    The calculator's loop, statement by statement: frame_size = mtu - headers for every frame."""
    frame_size, prb_size = mtu - header_bytes(static_compression), record_bytes(typ, width)
    if frame_size < prb_size:
        return None
    out, next_start = [], 0
    while True:
        fit = frame_size // prb_size
        remaining = ru_nof_prbs - next_start
        last = fit >= remaining
        n = remaining if last else fit
        used = header_bytes(static_compression) + n * prb_size
        out.append((next_start, n, max(MIN_FRAME, used)))  # frame_buffer::set_size
        next_start += n
        if last:
            return out


def frame(flow, sym, frag_index, start_prb, nof_prbs, records):
    """One frame: flow and sym are dicts with the fields of nrphy_ofh_dl_flow_t (compression flattened to type, data_width) and
    nrphy_ofh_dl_symbol_t; records the fragment's PRB records (uint8)."""
    typ, width, static = flow["type"], flow["data_width"], flow["static_compression"]
    records = np.asarray(records, np.uint8).reshape(-1)
    assert records.size == nof_prbs * record_bytes(typ, width)
    ofh = [0x90,                                            # downlink << 7 | payload version 1 << 4 | filter index 0
           sym["sfn"] & 0xFF,
           (sym["subframe"] << 4 | sym["slot"] >> 2) & 0xFF,
           ((sym["slot"] & 3) << 6 | sym["symbol"]) & 0xFF,
           0,                                               # section identifier
           (start_prb >> 8) & 3,                            # every RB << 3 | this symbol << 2 | 2 MSBs of startPrbu
           start_prb & 0xFF,
           0 if nof_prbs > 255 else nof_prbs]
    if not static:
        ofh += [(width << 4 | typ) & 0xFF, 0]               # udCompHdr, reserved
    payload_size = 4 + len(ofh) + records.size              # what follows the eCPRI common header: pc_id, seq_id, the message
    seq = (sym["seq_id"] + frag_index) & 0xFF
    ecpri = [0x10, 0x00, payload_size >> 8, payload_size & 0xFF, sym["eaxc"] >> 8, sym["eaxc"] & 0xFF, seq, 0x80]
    eth = list(flow["mac_dst"]) + list(flow["mac_src"]) + [0x81, 0x00, flow["tci"] >> 8, flow["tci"] & 0xFF,
                                                          flow["eth_type"] >> 8, flow["eth_type"] & 0xFF]
    out = np.concatenate([np.array(eth + ecpri + ofh, np.uint8), records])
    if out.size < MIN_FRAME:
        out = np.concatenate([out, np.zeros(MIN_FRAME - out.size, np.uint8)])
    return out


def symbol_frames(flow, sym, row, compress):
    """The frames of one symbol: row is the grid row, raw cbf16 as uint16 [grid_nof_subc][2]; compress(typ, width, iq_scaling, prbs
    uint16 [n][12][2]) -> the records of ONE compress() call.  PRBs beyond the row are zero samples."""
    row = np.asarray(row, np.uint16).reshape(-1, 2)
    assert row.shape[0] % 12 == 0 and row.shape[0] <= 12 * flow["ru_nof_prbs"]
    full = np.zeros((12 * flow["ru_nof_prbs"], 2), np.uint16)
    full[:row.shape[0]] = row
    frags = fragments(flow["mtu"], flow["ru_nof_prbs"], flow["static_compression"], flow["type"], flow["data_width"])
    out = []
    for f, (start, n, frame_bytes) in enumerate(frags):
        records = compress(flow["type"], flow["data_width"], flow["iq_scaling"], full[12 * start:12 * (start + n)].reshape(n, 12, 2))
        out.append(frame(flow, sym, f, start, n, records))
        assert out[-1].size == frame_bytes
    return out


def to_bf16_exact(values):
    """float32 values that bf16 holds exactly -> raw bf16 (uint16)."""
    bits = np.asarray(values, np.float32).view(np.uint32)
    assert (bits & 0xFFFF == 0).all()
    return (bits >> 16).astype(np.uint16)


def seeded_grid(seed, ports, nof_subc):
    """The recorder's grid: uint16 [ports][14][nof_subc][2] (see tests/golden/record_ofh_dl_reference.cpp)."""
    n_re = ports * 14 * nof_subc
    re = np.arange(n_re, dtype=np.uint64)
    cls = (mix((31 * seed + (re % nof_subc) // 12 + 0x51ED) & 0xFFFFFFFF) & 3)[:, None]
    h = mix((seed + 2 * re[:, None] + np.arange(2, dtype=np.uint64)[None, :]) & 0xFFFFFFFF)
    sel, m = h & 15, h >> 4
    small, medium, large = (m & 31).astype(np.float32), 64.0 * (m & 127).astype(np.float32), 8192.0 * (1 + (m & 7)).astype(np.float32)
    mag = np.where((sel < 12) | (cls < 2), small, np.where((sel < 14) | (cls == 2), medium, large)).astype(np.float32)
    v = np.where(h >> 31 != 0, -mag, mag).astype(np.float32)
    return to_bf16_exact(v).reshape(ports, 14, nof_subc, 2)
