"""Python/NumPy restatement of the Open Fronthaul uplink frame receiver (include/mi355_nrphy.h: nrphy_ofh_rx_run): srsRAN-5G-ER's
message_receiver_impl::process_new_frame with vlan_frame_decoder_impl, the two eCPRI packet decoders, sequence_id_checker_impl,
uplane_peeker, the static and the dynamic uplane_message_decoder, data_flow_uplane_uplink_data_impl's filter and
uplane_rx_symbol_data_flow_writer, check by check in the reference's order, one status per way out.  The PRB arithmetic is
tests/ofh_ul_model.py's.  Frames are taken one after another, so checker state and "later message wins" come by themselves.
tests/test_ofh_frame_receiver.py pins it to a recording of the reference."""
import numpy as np

import ofh_ul_model as ul

RECORD_FIELDS = ("payload_offset", "status", "seq_skipped", "grid_index", "expect_index", "eaxc", "seq_id", "start_prb", "nof_prbs",
                 "nof_prbs_written", "port", "sfn8", "filter_index", "subframe", "slot", "symbol", "type", "data_width")
EXPECT_FIELDS = ("grid_index", "sfn8", "eaxc", "prb_start", "nof_prb", "context_symbols", "subframe", "slot", "filter_index",
                 "start_symbol", "nof_symbols")


def default_cfg(**kw):
    """The fields of nrphy_ofh_rx_cfg_t; compressions as (type, data_width)."""
    cfg = dict(mac_dst=bytes([0x00, 0x11, 0x22, 0x33, 0x44, 0x55]), mac_src=bytes([0x66, 0x77, 0x88, 0x99, 0xAA, 0xBB]), eth_type=0xAEFE,
               vlan_tag_present=0, ignore_ecpri_payload_size=0, seq_id_check=1, numerology=1, nof_symbols=14, ru_nof_prbs=9,
               static_compression=1, ul_eaxc=(4, 5), prach_eaxc=(0, 1), compression=(ul.BFP, 9), prach_compression=(ul.BFP, 9))
    cfg.update(kw)
    return cfg


def expect(**kw):
    e = dict(grid_index=0, sfn8=0, eaxc=4, prb_start=0, nof_prb=9, context_symbols=0x3FFF, subframe=0, slot=0, filter_index=0,
             start_symbol=0, nof_symbols=14)
    e.update(kw)
    return e


def has_param(typ):
    """is_ud_comp_param_present."""
    return typ in (1, 2, 3, 5, 6)


def section_bytes(start_prb, nof_prbs, records, comp=None, section_id=0, rb=0, sym_inc=0, comp_len=None):
    """One section as sent: header, [udCompHdr, reserved byte] when comp = (type, width) is given (dynamic compression),
    [udCompLen] when comp_len is given, the PRB records.  nof_prbs is the field's value (0 = all of the RU's)."""
    out = [section_id >> 4, (section_id & 0xF) << 4 | rb << 3 | sym_inc << 2 | (start_prb >> 8) & 3, start_prb & 0xFF, nof_prbs & 0xFF]
    if comp is not None:
        out += [(comp[1] & 0xF) << 4 | comp[0], 0]
    if comp_len is not None:
        out += [comp_len >> 8, comp_len & 0xFF]
    return bytes(out) + bytes(np.asarray(records, np.uint8).tobytes())


def build_frame(cfg, eaxc=4, seq_id=0, sfn8=0, subframe=0, slot=0, symbol=0, sections=(), filter_index=0, direction=0, version=1,
                revision=1, concatenation=0, msg_type=0, payload_size=None, mac_dst=None, mac_src=None, eth_type=None, tci=None,
                message=None, pad_to=64, trailing=b""):
    """One Ethernet frame as uint8: addresses, [802.1Q tag when tci is given], type, eCPRI common header, pc_id, seq_id, the
    user-plane header, `sections` (bytes objects of section_bytes) -- or `message` in place of header and sections --, zeros up
    to pad_to, `trailing`.  seq_id is the 16-bit field (sequence in the high byte, E bit and subsequence in the low)."""
    if message is None:
        message = bytes([direction << 7 | version << 4 | filter_index, sfn8, subframe << 4 | slot >> 2, (slot & 3) << 6 | symbol])
        message += b"".join(sections)
    size = 4 + len(message) if payload_size is None else payload_size
    out = bytes(cfg["mac_dst"] if mac_dst is None else mac_dst) + bytes(cfg["mac_src"] if mac_src is None else mac_src)
    if tci is not None:
        out += bytes([0x81, 0x00, tci >> 8, tci & 0xFF])
    et = cfg["eth_type"] if eth_type is None else eth_type
    out += bytes([et >> 8, et & 0xFF, revision << 4 | concatenation, msg_type, size >> 8, size & 0xFF, eaxc >> 8, eaxc & 0xFF,
                  seq_id >> 8, seq_id & 0xFF]) + message
    out += bytes(max(0, pad_to - len(out))) + bytes(trailing)
    return np.frombuffer(out, np.uint8).copy()


def check_seq_id(state, eaxc, seq):
    """sequence_id_checker_impl::update_and_compare_seq_id; state: {eaxc: counter}."""
    if eaxc not in state:
        state[eaxc] = seq
        return 0
    expected = (state[eaxc] + 1) & 0xFF
    if seq == expected:
        state[eaxc] = expected
        return 0
    a = seq - expected
    if a >= 128:
        a -= 256
    elif a < -128:
        a += 256
    if a > 0:
        state[eaxc] = seq
    return a


class Receiver:
    def __init__(self, cfg):
        self.cfg = cfg
        self.state = {}

    def reset(self):
        self.state = {}

    def frame(self, buf, offset, length, expects, grid):
        """One frame -> its record; an accepted section is written into grid (uint32 [grids][ports][14][subc]) at once."""
        c = self.cfg
        r = dict.fromkeys(RECORD_FIELDS, 0)

        def out(status):
            r["status"] = status
            return r

        f = [int(v) for v in buf[offset:offset + length]]
        if length < 64:
            return out(1)
        h = 18 if c["vlan_tag_present"] else 14
        if bytes(f[6:12]) != bytes(c["mac_src"]) or bytes(f[0:6]) != bytes(c["mac_dst"]) or (f[h - 2] << 8 | f[h - 1]) != c["eth_type"]:
            return out(2)
        at = h
        if f[at] >> 4 != 1 or f[at] & 1:
            return out(3)
        msg_type, size = f[at + 1], f[at + 2] << 8 | f[at + 3]
        at += 4
        rem = length - at
        if not c["ignore_ecpri_payload_size"] and (size > rem or size < 5):
            return out(4)
        if msg_type != 0:
            return out(5)
        eaxc, seq_id = f[at] << 8 | f[at + 1], f[at + 2] << 8 | f[at + 3]
        at += 4
        m = f[at:at + ((rem if c["ignore_ecpri_payload_size"] else size) - 4)]
        r["eaxc"], r["seq_id"] = eaxc, seq_id
        if eaxc not in c["ul_eaxc"] and eaxc not in c["prach_eaxc"]:
            return out(6)
        skipped = check_seq_id(self.state, eaxc, seq_id >> 8) if c["seq_id_check"] else 0
        r["seq_skipped"] = skipped
        if skipped < 0:
            return out(7)
        if len(m) < 4:
            return out(8)
        subframe, slot, symbol, filt = m[2] >> 4, (m[2] & 0xF) << 2 | m[3] >> 6, m[3] & 0x3F, m[0] & 0xF
        if subframe >= 10 or slot >= 1 << c["numerology"]:
            return out(8)
        r.update(sfn8=m[1], subframe=subframe, slot=slot, symbol=symbol, filter_index=filt)
        if filt >= 8:
            return out(9)
        if m[0] >> 7:
            return out(10)
        if (m[0] >> 4) & 7 != 1:
            return out(11)
        if symbol >= c["nof_symbols"]:
            return out(12)
        # decode_all_sections
        static = c["prach_compression"] if filt else c["compression"]
        q, sections = 4, []
        while q < len(m):
            if len(m) - q < 4:
                break
            s1, start, n = m[q + 1], (m[q + 1] & 3) << 8 | m[q + 2], m[q + 3]
            if n == 0:
                n, start = c["ru_nof_prbs"], 0
            q += 4
            typ, width = static
            if not c["static_compression"]:
                if len(m) - q < 2:
                    break
                typ = m[q] & 0xF
                if typ >= 7:
                    return out(13)
                width = (m[q] >> 4) or 16
                q += 2
            if typ in (5, 6):
                if len(m) - q < 2:
                    break
                q += 2
            nbytes = (3 * width + (1 if has_param(typ) else 0)) * n
            if len(m) - q < nbytes:
                break
            sections.append(dict(rb=(s1 >> 3) & 1, sym_inc=(s1 >> 2) & 1, start_prb=start, nof_prbs=n, type=typ, data_width=width, at=q))
            q += nbytes
            if len(sections) == 2:
                return out(14)
        if not sections:
            return out(15)
        s = sections[0]
        r.update(start_prb=s["start_prb"], nof_prbs=s["nof_prbs"], type=s["type"], data_width=s["data_width"],
                 payload_offset=offset + at + s["at"])
        if s["type"] > 1 or (s["type"] == 0 and s["data_width"] < 2):
            return out(16)
        if filt:
            return out(22)
        found = [k for k, e in enumerate(expects)
                 if (e["sfn8"], e["subframe"], e["slot"], e["eaxc"]) == (r["sfn8"], subframe, slot, eaxc)]
        if not found:
            return out(17)
        e = expects[found[0]]
        if not e["start_symbol"] <= symbol < e["start_symbol"] + e["nof_symbols"] or e["filter_index"] != 0:
            return out(17)
        r.update(expect_index=found[0], grid_index=e["grid_index"], port=list(c["ul_eaxc"]).index(eaxc))
        if s["rb"]:
            return out(18)
        if s["sym_inc"]:
            return out(19)
        if s["start_prb"] < e["prb_start"] or s["start_prb"] + s["nof_prbs"] > e["prb_start"] + e["nof_prb"]:
            return out(20)
        if not (e["context_symbols"] >> symbol) & 1:
            return out(21)
        rng = ul.grid_range(s["start_prb"], s["nof_prbs"], grid.shape[3] // 12)
        if rng is not None:
            r["nof_prbs_written"] = rng[1]
            ul.write_grid(grid, [dict(payload_offset=r["payload_offset"], grid_index=r["grid_index"], port=r["port"], symbol=symbol,
                                      start_prb=s["start_prb"], nof_prbs=s["nof_prbs"], type=s["type"], data_width=s["data_width"])], buf)
        return out(0)

    def run(self, buf, frames, expects, grid):
        """frames: [(offset, length)] in batch order -> the records."""
        return [self.frame(buf, off, length, expects, grid) for off, length in frames]
