"""NumPy restatement of the Open Fronthaul uplink receive (include/mi355_nrphy.h: nrphy_ofh_decompress, nrphy_ofh_ul_write_grid,
nrphy_ofh_ul_write_prach): unpacking, sign extension, the BFP scaler rule, the division in float32, the bf16 rounding, the grid
clipping and the PRACH trimming of srsRAN-5G-ER's iq_compression_{none,bfp}_impl::decompress, uplane_rx_symbol_data_flow_writer and
uplane_prach_symbol_data_flow_writer.  tests/test_ofh_uplink.py pins it to recordings of the reference."""
import numpy as np

NONE, BFP = 0, 1
MAX_NOF_PRBS = 275


def mix(h):
    """The recorder's 32-bit finaliser, on uint32 arrays."""
    h = np.asarray(h, np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def seeded_bytes(seed, n):
    return (mix((seed + np.arange(n, dtype=np.uint64)) & 0xFFFFFFFF) & 0xFF).astype(np.uint8)


def record_bytes(typ, width):
    return 3 * width + (1 if typ == BFP else 0)


def section_payload(seed, nof_prbs, typ, width):
    """The recorder's payload of a writer section: seeded bytes, the udCompParam byte of every BFP record & 0x0F."""
    rec = record_bytes(typ, width)
    data = seeded_bytes(seed, nof_prbs * rec)
    if typ == BFP:
        data[::rec] &= 0x0F
    return data


def unpack(data, typ, width):
    """records -> (values int32 [nof_prb][24], sign-extended data_width-bit fields MSB first; udCompParam uint8 [nof_prb])."""
    rec = record_bytes(typ, width)
    data = np.asarray(data, np.uint8).reshape(-1, rec)
    params = data[:, 0].copy() if typ == BFP else np.zeros(len(data), np.uint8)
    bits = np.unpackbits(data[:, rec - 3 * width:], axis=1).reshape(len(data), 24, width).astype(np.int64)
    raw = (bits << np.arange(width - 1, -1, -1)).sum(axis=2)
    return (raw - ((raw >> (width - 1)) << width)).astype(np.int32), params


def pack(values, typ, width, params=None):
    """The inverse of unpack: the low data_width bits of every value."""
    values = np.asarray(values, np.int64).reshape(-1, 24) & ((1 << width) - 1)
    bits = ((values[:, :, None] >> np.arange(width - 1, -1, -1)) & 1).astype(np.uint8).reshape(len(values), 24 * width)
    body = np.packbits(bits, axis=1)
    if typ == BFP:
        body = np.concatenate([np.asarray(params, np.uint8).reshape(-1, 1), body], axis=1)
    return body.reshape(-1)


def scaler(params):
    """int16_t scaler = 1 << udCompParam as the reference built by gcc evaluates it; 0 from 16 on (the library's rule from 31 on)."""
    e = np.asarray(params, np.int64)
    s = np.where(e <= 15, np.int64(1) << np.minimum(e, 15), 0)
    return np.where(s == 32768, -32768, s).astype(np.int32)


def to_bf16(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def decompress(data, typ, width):
    """records -> [nof_prb][12][2] uint16, raw cbf16."""
    if typ not in (NONE, BFP) or not (1 if typ == BFP else 2) <= width <= 16:
        raise ValueError("compression %r width %r" % (typ, width))
    v, params = unpack(data, typ, width)
    if typ == BFP:
        p = (v.astype(np.int64) * scaler(params)[:, None]).astype(np.int32)
        x = p.astype(np.float32) / np.float32(32767.0)
    else:
        x = v.astype(np.float32) / np.float32((1 << (width - 1)) - 1)
    assert x.dtype == np.float32
    return to_bf16(x).reshape(-1, 12, 2)


def words(prbs):
    """[..][2] uint16 -> cbf16 words uint32."""
    prbs = np.asarray(prbs, np.uint16)
    return prbs[..., 0].astype(np.uint32) | (prbs[..., 1].astype(np.uint32) << 16)


def widen(prbs):
    """srsvec::convert(cf, cbf16): [..][2] uint16 -> complex64."""
    f = (np.asarray(prbs, np.uint16).astype(np.uint32) << 16).view(np.float32)
    return (f[..., 0] + 1j * f[..., 1]).astype(np.complex64)


# ---- a compressor of the model's own (for round trips; the library's is nrphy_ofh_compress) -----------------------------
def quantise(x):
    """float in [-1, 1] -> int16 at 16 bits."""
    return np.rint(np.clip(np.asarray(x, np.float64), -1, 1) * 32767).astype(np.int32)


def bfp_compress(q, width):
    """int16 values [nof_prb][24] -> records: the smallest exponent that makes every value of the PRB fit `width` bits."""
    q = np.asarray(q, np.int32).reshape(-1, 24)
    e = np.full(len(q), -1, np.int64)
    for k in range(16):
        fits = ((q >> k) >= -(1 << (width - 1))).all(axis=1) & ((q >> k) < (1 << (width - 1))).all(axis=1)
        e = np.where((e < 0) & fits, k, e)
    return pack(q >> e[:, None], BFP, width, e), e


# ---- the two writers ---------------------------------------------------------------------------------------------------
def grid_range(start_prb, nof_prbs, du_nof_prbs):
    """-> (first subcarrier, PRBs written) or None: ofh_uplane_rx_symbol_data_flow_writer.cpp:53-80."""
    if start_prb >= du_nof_prbs:
        return None
    n = du_nof_prbs - start_prb
    if start_prb + nof_prbs < du_nof_prbs:
        n = nof_prbs
    return 12 * start_prb, n


def write_grid(grid, sections, payload):
    """grid: uint32 [nof_grids][ports][14][subc] cbf16 words, written in place, sections in order.  A section is a dict with the
    fields of nrphy_ofh_ul_section_t."""
    du = grid.shape[3] // 12
    for s in sections:
        r = grid_range(s["start_prb"], s["nof_prbs"], du)
        if r is None:
            continue
        rec = record_bytes(s["type"], s["data_width"])
        data = payload[s["payload_offset"]:s["payload_offset"] + r[1] * rec]
        grid[s["grid_index"], s["port"], s["symbol"], r[0]:r[0] + 12 * r[1]] = words(decompress(data, s["type"], s["data_width"])).reshape(-1)


def prach_range(start_prb, nof_prbs, prach_nof_re, offset_to_first_re):
    """-> (start_re, iq_start_re, iq_size_re) or None: ofh_uplane_prach_symbol_data_flow_writer.cpp:56-104, with its unsigned
    32-bit wrap-around, its float division and its max<int>."""
    u = lambda v: int(v) & 0xFFFFFFFF
    prach_nof_prbs = int(np.ceil(np.float32(u(prach_nof_re + offset_to_first_re)) / np.float32(12)))
    after = u(prach_nof_prbs * 12 - (prach_nof_re + offset_to_first_re))
    data_start_prb = offset_to_first_re // 12
    if start_prb >= prach_nof_prbs or start_prb + nof_prbs <= data_start_prb:
        return None
    to_write = u(prach_nof_prbs - start_prb)
    if start_prb + nof_prbs < prach_nof_prbs:
        to_write = nof_prbs
    diff = u(start_prb * 12 - offset_to_first_re)
    start_re = max(0, diff - (1 << 32) if diff >= (1 << 31) else diff)
    section_start_re = u(start_prb * 12)
    section_nof_re = u(to_write * 12)
    if start_prb + nof_prbs >= prach_nof_prbs:
        section_nof_re = u(section_nof_re - after)
    iq_start_re = 0
    if section_start_re < offset_to_first_re:
        iq_start_re = offset_to_first_re - section_start_re
        section_nof_re = u(section_nof_re - iq_start_re)
    return start_re, iq_start_re, min(section_nof_re, prach_nof_re)


def write_prach(symbols, sections, payload):
    """symbols: complex64, flat, written in place.  A section is a dict with the fields of nrphy_ofh_ul_prach_section_t (the
    inner section's fields alongside)."""
    for s in sections:
        r = prach_range(s["start_prb"], s["nof_prbs"], s["prach_nof_re"], s["offset_to_first_re"])
        if r is None or r[2] == 0:
            continue
        rec = record_bytes(s["type"], s["data_width"])
        data = payload[s["payload_offset"]:s["payload_offset"] + s["nof_prbs"] * rec]
        iq = widen(decompress(data, s["type"], s["data_width"])).reshape(-1)
        first = s["dst_offset"] + r[0]
        symbols[first:first + r[2]] = iq[r[1]:r[1] + r[2]]
