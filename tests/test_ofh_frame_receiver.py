"""Open Fronthaul uplink frame receiver (nrphy_ofh_rx_create, _reset, _validate, _run, _host): received Ethernet frames in device
memory to the receive grid.

The reference's answers were recorded once by tests/golden/record_ofh_rx_reference.cpp, which sends frames it builds through
srsRAN-5G-ER's message_receiver_impl::on_new_frame with the reference's own decoders, sequence checker, repositories and data
flow, and notes per frame how far it got and what it wrote.  tests/golden/ofh_rx_reference_* hold the frames, the cases and the
written words.  The path is integer parsing, one float division and one bf16 rounding, so every comparison is exact: the
restatement (tests/ofh_rx_model.py) against the recording on the CPU, the device against the restatement and the recording on
the GPU."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import backends
import ofh_rx_model as model
import ofh_ul_model as ul

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
POISON = 0x5A5AA5A5
GRID_SHAPE = (2, 2, 14, 72)


# =======================================================================================================================
# helpers
# =======================================================================================================================
def make_cfg(c, **change):
    c = dict(c, **change)
    comp = lambda t: abi.OfhCompressionCfg(t[0], t[1], 1.0)
    pad = lambda v: (C.c_uint16 * 4)(*(list(v) + [0] * (4 - len(v))))
    return abi.OfhRxCfg((C.c_uint8 * 6)(*c["mac_dst"]), (C.c_uint8 * 6)(*c["mac_src"]), c["eth_type"], c.get("reserved_", 0),
                        c["vlan_tag_present"], c["ignore_ecpri_payload_size"], c["seq_id_check"], c["numerology"], c["nof_symbols"],
                        c["ru_nof_prbs"], c["static_compression"], c.get("n_ul_eaxc", len(c["ul_eaxc"])),
                        c.get("n_prach_eaxc", len(c["prach_eaxc"])), pad(c["ul_eaxc"][:4]), pad(c["prach_eaxc"][:4]), comp(c["compression"]),
                        comp(c["prach_compression"]))


def make_expect(e):
    return abi.OfhRxExpect(e["grid_index"], e["sfn8"], e["eaxc"], e["prb_start"], e["nof_prb"], e["context_symbols"], e["subframe"],
                           e["slot"], e["filter_index"], e["start_symbol"], e["nof_symbols"], e.get("reserved_", 0))


def make_frames(ranges):
    return [abi.OfhRxFrame(off, length, 0) for off, length in ranges]


def record_dict(rec):
    return {f: int(getattr(rec, f)) for f in model.RECORD_FIELDS}


def pack(frames, gaps=None):
    """Frames back to back (or with `gaps[i]` bytes of 0xEE in front of frame i) -> (buffer, [(offset, length)])."""
    parts, ranges, pos = [], [], 0
    for i, f in enumerate(frames):
        gap = 0 if gaps is None else gaps[i]
        parts.append(np.full(gap, 0xEE, np.uint8))
        pos += gap
        ranges.append((pos, f.size))
        parts.append(f)
        pos += f.size
    return np.concatenate(parts), ranges


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


class Recording:
    def __init__(self):
        self.frames = np.load(os.path.join(GOLDEN, "ofh_rx_reference_frames.npy"))
        self.values = np.load(os.path.join(GOLDEN, "ofh_rx_reference_values.npy"))
        self.cases = json.load(open(os.path.join(GOLDEN, "ofh_rx_reference_cases.json")))
        self.batches = self.cases["batches"]
        self.shape = (self.cases["nof_grids"], self.cases["grid_nof_ports"], 14, self.cases["grid_nof_subc"])

    def cfg(self, b):
        comp = (b["type"], b["data_width"]) if b["static_compression"] else (ul.BFP, 9)
        return model.default_cfg(ignore_ecpri_payload_size=b["ignore_ecpri_payload_size"], static_compression=b["static_compression"],
                                 compression=comp, prach_compression=comp, ru_nof_prbs=b["ru_nof_prbs"], numerology=b["numerology"],
                                 nof_symbols=b["nof_symbols"], ul_eaxc=tuple(b["ul_eaxc"]), prach_eaxc=tuple(b["prach_eaxc"]))

    def ranges(self, b):
        return [(f["offset"], f["length"]) for f in b["frames"]]

    def words(self, f):
        w = f["write"]
        return self.values[w["values_offset"]:w["values_offset"] + w["nof_subc"]]

    def replay(self, b):
        """The grids after the reference took the batch's frames in order."""
        grid = np.full(self.shape, POISON, np.uint32)
        for f in b["frames"]:
            w = f["write"]
            if w is not None:
                grid[w["grid"], w["port"], w["symbol"], w["first_subc"]:w["first_subc"] + w["nof_subc"]] = self.words(f)
        return grid


@pytest.fixture(scope="module")
def recording():
    return Recording()


@pytest.fixture(scope="module")
def recorded_model_runs(recording):
    """Per batch: (records, grid) of the restatement, computed once."""
    out = []
    for b in recording.batches:
        grid = np.full(recording.shape, POISON, np.uint32)
        out.append((model.Receiver(recording.cfg(b)).run(recording.frames, recording.ranges(b), b["expects"], grid), grid))
    return out


def reference_view(r, frame_bytes):
    """What the recorder's wrappers would have noted for a frame that the restatement gives record r."""
    s = r["status"]
    eth = 0 if s == 1 else 1 if s == 2 else 2
    if s in (1, 2):
        ecpri = -1
    elif s in (3, 4):
        ecpri = 0
    elif s == 5:
        ecpri = 1 if frame_bytes[15] == 2 else 0   # real-time control decodes and is filtered; any other type does not decode
    else:
        ecpri = 1 if s == 6 else 2
    seq = None if 1 <= s <= 6 else r["seq_skipped"]
    flow = 0 if 1 <= s <= 9 else (2 if r["filter_index"] else 1)
    decoded = -1 if flow != 1 else (0 if 10 <= s <= 16 else 1)
    write = None
    if s == 0 and r["nof_prbs_written"]:
        write = dict(grid=r["grid_index"], port=r["port"], symbol=r["symbol"], first_subc=12 * r["start_prb"],
                     nof_subc=12 * r["nof_prbs_written"])
    return dict(eth=eth, ecpri=ecpri, seq=seq, flow=flow, decoded=decoded, write=write)


# ---- the mutation batch: one field of a valid frame changed at a time ----------------------------------------------------
MUTATION_EXPECTS = [model.expect(sfn8=7, subframe=3, slot=1, eaxc=4), model.expect(sfn8=7, subframe=3, slot=1, eaxc=5, start_symbol=2,
                                                                                   nof_symbols=5, prb_start=1, nof_prb=7),
                    model.expect(sfn8=7, subframe=3, slot=0, eaxc=4, grid_index=1, context_symbols=0x7F),
                    model.expect(sfn8=7, subframe=4, slot=1, eaxc=4, grid_index=1, filter_index=1)]


def records_of(seed, n, comp):
    rec = 3 * comp[1] + (1 if model.has_param(comp[0]) else 0)
    data = ul.seeded_bytes(seed, n * rec)
    if model.has_param(comp[0]):
        data[::rec] &= 0x0F
    return data


def mutation_batch(cfg, tci=None):
    """-> [(name, frame)]; sequence identifiers count up per eAxC unless the mutation is about them."""
    static = bool(cfg["static_compression"])
    next_seq, seed, out = {}, [5000], []

    def section(start_prb=2, nof_prbs=3, comp=(ul.BFP, 9), records=None, cut=0, route=0, **kw):
        if static:
            comp = cfg["prach_compression"] if route else cfg["compression"]
        n = (nof_prbs or cfg["ru_nof_prbs"]) if records is None else records
        seed[0] += 1000
        data = records_of(seed[0], n, comp)
        return model.section_bytes(start_prb, nof_prbs, data[:data.size - cut], None if static else comp, **kw)

    def add(name, seq=None, past=False, sections=None, cut_to=None, **kw):
        kw.setdefault("eaxc", 4)
        if seq is None:
            seq = next_seq.get(kw["eaxc"], 254)
        if not past:
            next_seq[kw["eaxc"]] = (seq + 1) & 0xFF
        base = dict(sfn8=7, subframe=3, slot=1, symbol=3, tci=tci)
        base.update(kw)
        f = model.build_frame(cfg, seq_id=seq << 8 | 0x80, sections=[section()] if sections is None else sections, **base)
        out.append((name, f if cut_to is None else f[:cut_to]))

    add("accepted")
    add("accepted, sequence 255", symbol=4)
    add("accepted, sequence wraps to 0", symbol=5)
    add("later frame over PRBs 3..5 of symbol 5", symbol=5, sections=[section(start_prb=3)])
    add("shorter than 64 bytes", cut_to=60)
    add("destination MAC", mac_dst=bytes(6))
    add("source MAC", mac_src=bytes([0x66, 0x77, 0x88, 0x99, 0xAA, 0xBA]))
    add("Ethernet type", eth_type=0x0800)
    add("eCPRI revision", revision=2)
    add("eCPRI concatenation", concatenation=1)
    add("payload size beyond the frame", payload_size=4000)
    add("payload size 3", payload_size=3)
    add("payload size 4", payload_size=4)
    add("payload size 6: a message of 2 bytes", payload_size=6)
    add("real-time control", msg_type=2)
    add("unknown eCPRI message type", msg_type=7)
    add("eAxC in neither list", eaxc=9)
    add("sequence from the past", seq=200, past=True)
    add("sequence skipped ahead", seq=40)
    add("in order again", seq=41, symbol=6)
    add("subframe 10", subframe=10)
    add("slot 2 at 30 kHz", slot=2)
    add("reserved filter index", filter_index=9)
    add("downlink", direction=1)
    add("payload version 2", version=2)
    add("symbol 14", symbol=14)
    add("reserved compression type", sections=[section(comp=(7, 9), records=0)])
    add("two complete sections", sections=[section(), section(start_prb=5, nof_prbs=1)])
    add("one complete section and an incomplete one", symbol=7, sections=[section(), section(start_prb=5, nof_prbs=1, cut=2)])
    add("records one byte short", sections=[section(cut=1)])
    add("header only", sections=[])
    add("mu-law", sections=[section(comp=(3, 8))])
    add("BFP with selective sending", sections=[section(comp=(5, 9), comp_len=84)])
    add("modulation compression", sections=[section(comp=(4, 4))])
    add("none with 1 bit", sections=[section(comp=(ul.NONE, 1))])
    add("accepted: none 16", symbol=8, sections=[section(comp=(ul.NONE, 16))])
    add("accepted: BFP 1", symbol=8, eaxc=5, sections=[section(comp=(ul.BFP, 1), start_prb=1)])
    add("no expectation for the frame number", sfn8=9)
    add("symbol outside the announced range", eaxc=5, symbol=8)
    add("announced with another filter index", subframe=4)
    add("PRACH-only eAxC with filter index 0", eaxc=0)
    add("every other RB", sections=[section(rb=1)])
    add("symbol increment", sections=[section(sym_inc=1)])
    add("starts below the announced PRBs", eaxc=5, sections=[section(start_prb=0)])
    add("ends beyond the announced PRBs", eaxc=5, sections=[section(start_prb=6)])
    add("no uplink context for the symbol", slot=0, symbol=9)
    add("accepted into the second grid", slot=0, symbol=6)
    add("nof_prbs 0: every PRB of the RU from 0, whatever start_prb says", symbol=11, sections=[section(start_prb=5, nof_prbs=0)])
    add("clipped at the grid", symbol=12, sections=[section(start_prb=4, nof_prbs=4)])
    add("wholly beyond the grid", symbol=12, sections=[section(start_prb=6, nof_prbs=2)])
    add("long PRACH", eaxc=0, filter_index=1, sections=[section(route=1)])
    add("short PRACH on a data eAxC", filter_index=3, sections=[section(route=1)])
    add("from the past and otherwise bad: the checker comes first", seq=30, past=True, direction=1)
    add("dropped after the checker: the state moves on", version=3)
    add("in order after a dropped frame", symbol=13)
    return out


MUTATION_CFGS = {
    "size+dynamic": dict(ignore_ecpri_payload_size=0, static_compression=0),
    "ignore+static+vlan": dict(ignore_ecpri_payload_size=1, static_compression=1, vlan_tag_present=1, compression=(ul.BFP, 14),
                               prach_compression=(ul.NONE, 12)),
}


def mutation_case(which):
    cfg = model.default_cfg(**MUTATION_CFGS[which])
    named = mutation_batch(cfg, tci=0x2005 if cfg["vlan_tag_present"] else None)
    buf, ranges = pack([f for _, f in named], gaps=[(3 * i) % 7 for i in range(len(named))])
    grid = np.full(GRID_SHAPE, POISON, np.uint32)
    records = model.Receiver(cfg).run(buf, ranges, MUTATION_EXPECTS, grid)
    return cfg, [n for n, _ in named], buf, ranges, records, grid


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_library_loads_without_a_device_and_the_pods_match_the_header():
    handle = lib.load()
    names = [s for s in abi.ABI_SYMBOLS if "_ofh_rx_" in s]
    assert len(names) == 6 and not [s for s in names if not hasattr(handle, s)]
    pods = [("nrphy_ofh_rx_cfg_t", abi.OfhRxCfg), ("nrphy_ofh_rx_frame_t", abi.OfhRxFrame), ("nrphy_ofh_rx_expect_t", abi.OfhRxExpect),
            ("nrphy_ofh_rx_record_t", abi.OfhRxRecord)]
    exprs, want = [], []
    for cname, cls in pods:
        exprs.append("sizeof(%s)" % cname)
        want.append(C.sizeof(cls))
        for f in cls._fields_:
            exprs.append("offsetof(%s, %s)" % (cname, f[0]))
            want.append(getattr(cls, f[0]).offset)
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){size_t v[] = {%s};
 for (size_t i = 0; i != sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]); return 0;}''' % ", ".join(exprs)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()]
    assert out == want
    assert C.sizeof(abi.OfhRxRecord) == 48 and C.sizeof(abi.OfhRxFrame) == 16 and C.sizeof(abi.OfhRxExpect) == 20


def test_restatement_equals_the_recording_for_every_frame(recording, recorded_model_runs):
    """How far each frame got in the reference, the checker's answer, which frames wrote, where, and every word."""
    assert len(recording.batches) == 4 and sum(len(b["frames"]) for b in recording.batches) > 200
    assert {(b["ignore_ecpri_payload_size"], b["static_compression"]) for b in recording.batches} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for b, (records, grid) in zip(recording.batches, recorded_model_runs):
        for f, r in zip(b["frames"], records):
            where = (b["name"], f["name"], r["status"])
            view = reference_view(r, recording.frames[f["offset"]:f["offset"] + f["length"]])
            got = {k: f[k] for k in ("eth", "ecpri", "seq", "flow", "decoded")}
            got["write"] = None if f["write"] is None else {k: f["write"][k] for k in ("grid", "port", "symbol", "first_subc", "nof_subc")}
            assert got == view, where
            if f["write"] is not None:
                rec = ul.record_bytes(r["type"], r["data_width"])
                data = recording.frames[r["payload_offset"]:r["payload_offset"] + r["nof_prbs_written"] * rec]
                assert same_bits(ul.words(ul.decompress(data, r["type"], r["data_width"])).reshape(-1), recording.words(f)), where
        assert same_bits(grid, recording.replay(b)), b["name"]


def test_recording_is_not_vacuous(recording, recorded_model_runs):
    statuses, by_name = set(), {}
    for b, (records, _) in zip(recording.batches, recorded_model_runs):
        for f, r in zip(b["frames"], records):
            statuses.add(r["status"])
            by_name.setdefault(f["name"], []).append((b, f, r))
    # every drop rule the reference can reach (4 only where the payload size counts, 13 only under dynamic compression; 16 and
    # 22's decode are the library's own), and the accepted frames
    assert statuses >= set(range(1, 4)) | set(range(5, 16)) | set(range(17, 22)) | {0, 4, 22}
    accepted = [(r["type"], r["data_width"]) for _, (records, _) in zip(recording.batches, recorded_model_runs) for r in records
                if r["status"] == 0 and r["nof_prbs_written"]]
    assert {t for t, _ in accepted} == {ul.NONE, ul.BFP} and {(ul.BFP, 1), (ul.NONE, 2), (ul.BFP, 9), (ul.NONE, 16)} <= set(accepted)
    # the reference wrote for exactly the accepted frames: the recording agrees on what "accepted" means
    for b, (records, _) in zip(recording.batches, recorded_model_runs):
        assert [f["write"] is not None for f in b["frames"]] == [r["status"] == 0 and r["nof_prbs_written"] > 0 for r in records]
    # the checker: from the past, skipped ahead, and 255 -> 0 in order
    seqs = [(f["seq"], r["seq_id"] >> 8) for _, f, r in by_name["checker stream"] if f["seq"] is not None]
    assert any(s < 0 for s, _ in seqs) and any(s > 0 for s, _ in seqs)
    stream = [(f["seq"], r["seq_id"] >> 8) for b, f, r in by_name["checker stream"] if b is recording.batches[0]]
    assert (0, 255) in stream and stream[stream.index((0, 255)) + 1] == (0, 0)
    for _, f, r in by_name["from the past and no expectation: the checker drops it first"]:
        assert f["seq"] < 0 and f["flow"] == 0 and r["status"] == 7
    for _, f, r in by_name["in order after a dropped frame"]:
        assert f["seq"] == 0 and r["status"] == 0
    # nof_prbs = 0, clipping, wholly beyond the grid, two sections, padding
    for _, f, r in by_name["nof_prbs 0: all 9 PRBs from 0, clipped to the grid's 6"]:
        assert (r["start_prb"], r["nof_prbs"], r["nof_prbs_written"]) == (0, 9, 6) and f["write"]["nof_subc"] == 72
    for _, f, r in by_name["clipped: PRBs 4..7 of a 6-PRB grid"]:
        assert (r["nof_prbs"], r["nof_prbs_written"]) == (4, 2) and (f["write"]["first_subc"], f["write"]["nof_subc"]) == (48, 24)
    for _, f, r in by_name["wholly beyond the grid: accepted, nothing written"]:
        assert r["status"] == 0 and r["nof_prbs_written"] == 0 and f["write"] is None and f["decoded"] == 1
    for _, f, r in by_name["two complete sections"]:
        assert r["status"] == 14 and f["decoded"] == 0
    for _, f, r in by_name["one complete section and an incomplete one: accepted"]:
        assert r["status"] == 0 and f["write"] is not None
    padded = [(b, f, r) for b, f, r in by_name["one PRB, padded to 64 bytes: accepted when the padding parses as an incomplete section"]
              if b["ignore_ecpri_payload_size"] and r["payload_offset"] + 28 < f["offset"] + f["length"] == f["offset"] + 64]
    assert padded and all(r["status"] == 0 and f["write"]["nof_subc"] == 12 for _, f, r in padded)
    # later message wins: two writes of one batch share resource elements
    b = recording.batches[2]
    writes = [f["write"] for f in b["frames"] if f["write"] is not None]
    cover = {}
    for w in writes:
        for k in range(w["first_subc"], w["first_subc"] + w["nof_subc"]):
            cover[(w["grid"], w["port"], w["symbol"], k)] = cover.get((w["grid"], w["port"], w["symbol"], k), 0) + 1
    assert max(cover.values()) >= 2


GOOD = dict(frames=[(0, 64), (64, 100), (200, 1)], expects=[model.expect(), model.expect(eaxc=5), model.expect(slot=1, grid_index=1)],
            frames_bytes=4096, nof_grids=2, grid_nof_ports=2, grid_nof_subc=72)


@pytest.mark.parametrize("name,cfg_change,change,want", [
    ("a good call", {}, {}, True),
    ("nothing to do", {}, dict(frames=[], expects=[]), True),
    ("numerology 5", dict(numerology=5), {}, False),
    ("numerology 4", dict(numerology=4), {}, True),
    ("13 symbols", dict(nof_symbols=13), {}, False),
    ("12 symbols", dict(nof_symbols=12), dict(expects=[model.expect(nof_symbols=12)]), True),
    ("no PRB", dict(ru_nof_prbs=0), {}, False),
    ("276 PRBs", dict(ru_nof_prbs=276), {}, False),
    ("275 PRBs", dict(ru_nof_prbs=275), {}, True),
    ("vlan flag 2", dict(vlan_tag_present=2), {}, False),
    ("payload size flag 2", dict(ignore_ecpri_payload_size=2), {}, False),
    ("checker flag 2", dict(seq_id_check=2), {}, False),
    ("static flag 2", dict(static_compression=2), {}, False),
    ("reserved bits of the configuration", dict(reserved_=1), {}, False),
    ("five eAxC", dict(n_ul_eaxc=5), {}, False),
    ("eAxC 32", dict(ul_eaxc=(4, 32)), {}, False),
    ("eAxC 31", dict(ul_eaxc=(4, 31)), dict(expects=[]), True),
    ("an eAxC twice in a list", dict(prach_eaxc=(1, 1)), {}, False),
    ("an eAxC in both lists", dict(prach_eaxc=(4, 1)), {}, True),
    ("static none with 1 bit", dict(compression=(0, 1)), {}, False),
    ("static BFP 17", dict(compression=(1, 17)), {}, False),
    ("static type 2", dict(prach_compression=(2, 9)), {}, False),
    ("the same under dynamic compression", dict(prach_compression=(2, 9), static_compression=0), {}, True),
    ("reserved bits of a frame", {}, dict(frames=[(0, 64, 1)]), False),
    ("a frame up to the last byte", {}, dict(frames=[(4000, 96)]), True),
    ("a frame one byte beyond", {}, dict(frames=[(4000, 97)]), False),
    ("a frame offset beyond the buffer", {}, dict(frames=[(1 << 40, 1)]), False),
    ("frames that overlap", {}, dict(frames=[(100, 64), (0, 101)]), False),
    ("frames that touch", {}, dict(frames=[(100, 64), (0, 100)]), True),
    ("a grid of 73 subcarriers", {}, dict(grid_nof_subc=73), False),
    ("more eAxC than grid ports", {}, dict(grid_nof_ports=1), False),
    ("expectation for a PRACH eAxC", {}, dict(expects=[model.expect(eaxc=0)]), False),
    ("grid index beyond the batch", {}, dict(expects=[model.expect(grid_index=2)]), False),
    ("subframe 10", {}, dict(expects=[model.expect(subframe=10)]), False),
    ("slot 2 at 30 kHz", {}, dict(expects=[model.expect(slot=2)]), False),
    ("filter index 8", {}, dict(expects=[model.expect(filter_index=8)]), False),
    ("filter index 7", {}, dict(expects=[model.expect(filter_index=7)]), True),
    ("symbols beyond the slot", {}, dict(expects=[model.expect(start_symbol=3, nof_symbols=12)]), False),
    ("symbols up to the slot's end", {}, dict(expects=[model.expect(start_symbol=3, nof_symbols=11)]), True),
    ("PRBs beyond 275", {}, dict(expects=[model.expect(prb_start=200, nof_prb=76)]), False),
    ("PRBs up to 275", {}, dict(expects=[model.expect(prb_start=200, nof_prb=75)]), True),
    ("frame number 256", {}, dict(expects=[model.expect(sfn8=256)]), False),
    ("reserved bits of an expectation", {}, dict(expects=[dict(model.expect(), reserved_=1)]), False),
    ("two expectations for one slot and eAxC", {}, dict(expects=[model.expect(), model.expect(prb_start=3)]), False),
    ("the same slot in another frame", {}, dict(expects=[model.expect(), model.expect(sfn8=1)]), True),
])
def test_validator(name, cfg_change, change, want):
    call = dict(GOOD, **change)
    frames = [abi.OfhRxFrame(*(list(f) + [0])[:3]) for f in call["frames"]]
    got = lib.ofh_rx_validate(make_cfg(model.default_cfg(), **cfg_change), frames, [make_expect(e) for e in call["expects"]],
                              call["frames_bytes"], call["nof_grids"], call["grid_nof_ports"], call["grid_nof_subc"])
    assert got == (abi.OK if want else abi.ERR_ARGUMENT), name


def test_mutation_batch_reaches_every_status():
    cfg, names, buf, ranges, records, grid = mutation_case("size+dynamic")
    by_status = {}
    for n, r in zip(names, records):
        by_status.setdefault(r["status"], []).append(n)
    assert sorted(by_status) == list(range(23)), by_status
    status = dict(zip(names, (r["status"] for r in records)))
    assert status["payload size 3"] == status["payload size 4"] == status["payload size beyond the frame"] == 4
    assert status["payload size 6: a message of 2 bytes"] == 8
    assert status["mu-law"] == status["BFP with selective sending"] == status["modulation compression"] == status["none with 1 bit"] == 16
    assert status["from the past and otherwise bad: the checker comes first"] == 7
    assert status["dropped after the checker: the state moves on"] == 11 and status["in order after a dropped frame"] == 0
    assert status["one complete section and an incomplete one"] == 0 and status["two complete sections"] == 14
    skipped = {n: r["seq_skipped"] for n, r in zip(names, records)}
    assert skipped["accepted, sequence wraps to 0"] == 0 and skipped["sequence skipped ahead"] > 0 and skipped["sequence from the past"] < 0
    assert (grid != POISON).any() and (grid[1] != POISON).any()
    # the other configuration takes the same frames another way
    other = mutation_case("ignore+static+vlan")
    assert {r["status"] for r in other[4]} >= {0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 17, 18, 19, 20, 21, 22}


# =======================================================================================================================
# GPU
# =======================================================================================================================
def poison_words(shape):
    import torch
    return torch.full(shape, int(np.uint32(POISON).view(np.int32)), dtype=torch.int32, device="cuda")


def host_words(t):
    return t.cpu().numpy().view(np.uint32)


def device_run(gpu_ctx, rx, buf, ranges, expects, d_grid, stream=None):
    """One nrphy_ofh_rx_run -> the records as dicts.  The frames' buffer is exactly buf: the last frame may end the allocation."""
    import torch
    d_frames = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    n = len(ranges)
    d_records = torch.full((max(n, 1) * C.sizeof(abi.OfhRxRecord),), 0xCD, dtype=torch.uint8, device="cuda")
    shape = d_grid.shape
    rc = rx.run(make_frames(ranges), [make_expect(e) for e in expects], d_frames, d_grid, shape[0], shape[1], shape[3], d_records,
                stream=stream)
    assert rc == abi.OK
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    raw = d_records.cpu().numpy().tobytes()
    recs = (abi.OfhRxRecord * n).from_buffer_copy(raw[:n * C.sizeof(abi.OfhRxRecord)])
    assert all(bytes(r.reserved_) == bytes(4) for r in recs)
    return [record_dict(r) for r in recs]


def assert_records(got, want, names=None):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, names[i] if names else None, {k: (g[k], w[k]) for k in g if g[k] != w[k]})


@pytest.mark.gpu
def test_recorded_batches_on_the_device(gpu_ctx, recording, recorded_model_runs):
    for b, (records, grid) in zip(recording.batches, recorded_model_runs):
        rx = lib.OfhRx(gpu_ctx, make_cfg(recording.cfg(b)))
        d_grid = poison_words(recording.shape)
        got = device_run(gpu_ctx, rx, recording.frames, recording.ranges(b), b["expects"], d_grid)
        rx.close()
        assert_records(got, records, [f["name"] for f in b["frames"]])
        out = host_words(d_grid)
        assert same_bits(out, grid) and same_bits(out, recording.replay(b)), b["name"]   # poison wherever no accepted section is


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(MUTATION_CFGS))
def test_mutation_batch_on_the_device(gpu_ctx, which):
    cfg, names, buf, ranges, records, grid = mutation_case(which)
    rx = lib.OfhRx(gpu_ctx, make_cfg(cfg))
    d_grid = poison_words(GRID_SHAPE)
    got = device_run(gpu_ctx, rx, buf, ranges, MUTATION_EXPECTS, d_grid)
    rx.close()
    assert_records(got, records, names)
    assert same_bits(host_words(d_grid), grid)


def checker_stream(cfg):
    """Frames of eAxC 4 and 5 interleaved: in order, a wrap, skips, frames from the past, drops after the checker."""
    seqs4 = [250, 251, 252, 253, 254, 255, 0, 1, 5, 4, 6, 7, 135, 134, 136]
    seqs5 = [10, 11, 9, 12, 13, 200, 201, 13, 202, 203, 204, 77, 205, 206, 207]
    frames = []
    for i, (a, b) in enumerate(zip(seqs4, seqs5)):
        frames.append(model.build_frame(cfg, eaxc=4, seq_id=a << 8, sfn8=7, subframe=3, slot=1, symbol=i % 14, direction=int(i == 10),
                                        sections=[model.section_bytes(i % 4, 2, records_of(100 + i, 2, cfg["compression"]))]))
        frames.append(model.build_frame(cfg, eaxc=5, seq_id=b << 8 | 0x80, sfn8=7, subframe=3, slot=1, symbol=2 + i % 5,
                                        sections=[model.section_bytes(1 + i % 5, 2, records_of(200 + i, 2, cfg["compression"]))]))
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("cut", [1, 13])
def test_checker_state_lives_across_calls_and_reset_clears_it(gpu_ctx, cut):
    cfg = model.default_cfg()
    buf, ranges = pack(checker_stream(cfg))
    grid = np.full(GRID_SHAPE, POISON, np.uint32)
    ref = model.Receiver(cfg)
    want = ref.run(buf, ranges, MUTATION_EXPECTS, grid)
    assert {r["status"] for r in want} == {0, 7, 10} and any(r["seq_skipped"] > 0 for r in want)
    rx = lib.OfhRx(gpu_ctx, make_cfg(cfg))
    d_grid = poison_words(GRID_SHAPE)
    got = device_run(gpu_ctx, rx, buf, ranges[:cut], MUTATION_EXPECTS, d_grid) + device_run(gpu_ctx, rx, buf, ranges[cut:], MUTATION_EXPECTS, d_grid)
    assert_records(got, want)
    assert same_bits(host_words(d_grid), grid)
    # the stream's last frame once more is from the past; after a reset it is the first packet, which is always valid
    again = ref.run(buf, ranges[-1:], MUTATION_EXPECTS, grid)
    assert want[-1]["status"] == 0 and again[0]["status"] == 7 and again[0]["seq_skipped"] == -1
    assert_records(device_run(gpu_ctx, rx, buf, ranges[-1:], MUTATION_EXPECTS, d_grid), again)
    rx.reset()
    assert_records(device_run(gpu_ctx, rx, buf, ranges[-1:], MUTATION_EXPECTS, d_grid), [want[-1]])
    rx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_later_message_wins(gpu_ctx, reverse):
    """PRBs 2-6, 4-8 and 4-5 of one symbol with different payloads, in one call."""
    cfg = model.default_cfg(seq_id_check=0)
    spans = [(2, 5), (4, 5), (4, 2)]
    frames = [model.build_frame(cfg, eaxc=4, sfn8=7, subframe=3, slot=1, symbol=6,
                                sections=[model.section_bytes(s, n, records_of(300 + i, n, cfg["compression"]))]) for i, (s, n) in enumerate(spans)]
    buf, ranges = pack(frames)
    if reverse:
        ranges = ranges[::-1]
    grid = np.full(GRID_SHAPE, POISON, np.uint32)
    want = model.Receiver(cfg).run(buf, ranges, MUTATION_EXPECTS, grid)
    assert [r["status"] for r in want] == [0, 0, 0] and sorted(r["nof_prbs_written"] for r in want) == [2, 2, 4]
    rx = lib.OfhRx(gpu_ctx, make_cfg(cfg))
    d_grid = poison_words(GRID_SHAPE)
    got = device_run(gpu_ctx, rx, buf, ranges, MUTATION_EXPECTS, d_grid)
    rx.close()
    assert_records(got, want)
    out = host_words(d_grid)
    assert same_bits(out, grid) and (out[0, 0, 6, 24:72] != POISON).all() and (np.delete(out[0, 0], 6, axis=0) == POISON).all()
    # the last frame of the batch owns what it covers
    last = want[-1]
    rec = ul.record_bytes(last["type"], last["data_width"])
    words = ul.words(ul.decompress(buf[last["payload_offset"]:last["payload_offset"] + last["nof_prbs_written"] * rec], last["type"], last["data_width"]))
    assert same_bits(out[0, 0, 6, 12 * last["start_prb"]:12 * (last["start_prb"] + last["nof_prbs_written"])], words.reshape(-1))


@pytest.mark.gpu
def test_every_alignment_and_the_end_of_the_allocation(gpu_ctx):
    """Frames back to back at every offset modulo 4 for none 16, BFP 1, BFP 9 and BFP 16; the last frame ends at the last byte of the
    allocation and its section header claims more PRBs than the frame holds: incomplete, nothing written, nothing read beyond."""
    rng = np.random.default_rng(41)
    cfg = model.default_cfg(static_compression=0, seq_id_check=0)
    frames, seen = [], {}
    pos = 0
    comps = [(ul.NONE, 16), (ul.BFP, 1), (ul.BFP, 9), (ul.BFP, 16)]
    for i in range(16):   # frame i is of compression i % 4 and starts at byte (i // 4) modulo 4
        comp = comps[i % 4]
        n = 1 + i % 3
        f = model.build_frame(cfg, eaxc=4 + i % 2, sfn8=7, subframe=3, slot=1, symbol=2 + i % 5,
                              sections=[model.section_bytes(1 + i % 4, n, records_of(400 + i, n, comp), comp)])
        # bytes beyond the eCPRI payload are never parsed: as many as put the next frame where it belongs
        f = np.concatenate([f, rng.integers(0, 256, ((i + 1) // 4 - pos - f.size) % 4, dtype=np.uint8)])
        seen.setdefault(comp, set()).add(pos % 4)
        frames.append(f)
        pos += f.size
    assert all(v == {0, 1, 2, 3} for v in seen.values()), seen
    last = model.build_frame(cfg, eaxc=4, sfn8=7, subframe=3, slot=1, symbol=0,
                             sections=[model.section_bytes(0, 6, records_of(999, 5, (ul.BFP, 9)), (ul.BFP, 9))])
    frames.append(last)
    buf, ranges = pack(frames)
    assert ranges[-1][0] + ranges[-1][1] == buf.size
    grid = np.full(GRID_SHAPE, POISON, np.uint32)
    want = model.Receiver(cfg).run(buf, ranges, MUTATION_EXPECTS, grid)
    assert [r["status"] for r in want] == [0] * 16 + [15]
    rx = lib.OfhRx(gpu_ctx, make_cfg(cfg))
    d_grid = poison_words(GRID_SHAPE)
    got = device_run(gpu_ctx, rx, buf, ranges, MUTATION_EXPECTS, d_grid)
    rx.close()
    assert_records(got, want)
    out = host_words(d_grid)
    assert same_bits(out, grid) and (out[0, :, 0] == POISON).all()


@pytest.mark.gpu
def test_sections_longer_than_one_workgroup_are_clipped_at_the_grid(gpu_ctx):
    """ru_nof_prbs = 40 on a grid of 25 PRBs: 16, 17 and 33 PRBs of BFP 9 cross the write pass's 16-PRB boundary."""
    cfg = model.default_cfg(ru_nof_prbs=40, seq_id_check=0)
    expects = [model.expect(sfn8=1, eaxc=4, nof_prb=40), model.expect(sfn8=1, eaxc=5, nof_prb=40, grid_index=1)]
    spans = [(0, 16, 4, 0), (5, 17, 4, 1), (0, 33, 4, 2), (10, 17, 5, 3), (9, 16, 5, 4), (24, 16, 5, 5), (25, 15, 4, 6)]
    frames = [model.build_frame(cfg, eaxc=e, sfn8=1, symbol=sym, sections=[model.section_bytes(s, n, records_of(500 + sym, n, (ul.BFP, 9)))])
              for s, n, e, sym in spans]
    buf, ranges = pack(frames, gaps=[1, 0, 2, 0, 3, 0, 1])
    grid = np.full((2, 2, 14, 300), POISON, np.uint32)
    want = model.Receiver(cfg).run(buf, ranges, expects, grid)
    assert [r["nof_prbs_written"] for r in want] == [16, 17, 25, 15, 16, 1, 0] and all(r["status"] == 0 for r in want)
    rx = lib.OfhRx(gpu_ctx, make_cfg(cfg))
    d_grid = poison_words(grid.shape)
    got = device_run(gpu_ctx, rx, buf, ranges, expects, d_grid)
    rx.close()
    assert_records(got, want)
    assert same_bits(host_words(d_grid), grid)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(MUTATION_CFGS))
def test_receiver_equals_the_section_path_on_its_own_records(gpu_ctx, which):
    """Every accepted record as an nrphy_ofh_ul_section_t through nrphy_ofh_ul_write_grid, one call per group without overlap."""
    import torch
    cfg, names, buf, ranges, records, grid = mutation_case(which)
    rx = lib.OfhRx(gpu_ctx, make_cfg(cfg))
    d_grid = poison_words(GRID_SHAPE)
    got = device_run(gpu_ctx, rx, buf, ranges, MUTATION_EXPECTS, d_grid)
    rx.close()
    groups, covered = [[]], set()
    for r in got:
        if r["status"] != 0:
            continue
        cells = {(r["grid_index"], r["port"], r["symbol"], p) for p in range(r["start_prb"], r["start_prb"] + r["nof_prbs_written"])}
        if cells & covered:
            groups.append([])
            covered = set()
        covered |= cells
        groups[-1].append(abi.OfhUlSection(r["payload_offset"], r["grid_index"], r["port"], r["symbol"], r["start_prb"], r["nof_prbs"],
                                           r["type"], r["data_width"], 0))
    assert len(groups) >= 2 and sum(len(g) for g in groups) == sum(r["status"] == 0 for r in records) >= 8
    d_payload = torch.from_numpy(buf).cuda()
    d_second = poison_words(GRID_SHAPE)
    for g in groups:
        assert gpu_ctx.ofh_ul_write_grid(g, d_payload, d_second, GRID_SHAPE[0], GRID_SHAPE[1], GRID_SHAPE[3]) == abi.OK
    gpu_ctx.synchronize()
    assert same_bits(host_words(d_second), host_words(d_grid)) and same_bits(host_words(d_second), grid)


@pytest.mark.gpu
@pytest.mark.parametrize("static,typ,width", [(1, ul.BFP, 9), (0, ul.NONE, 16), (0, ul.BFP, 12)])
def test_loop_back_from_the_transmit_side(gpu_ctx, static, typ, width):
    """nrphy_ofh_dl_write_frames of one symbol in three fragments, the direction bit of each frame flipped on the device, received
    with vlan_tag_present = 1: the received PRBs are nrphy_ofh_decompress of the transmitted records."""
    import torch
    rng = np.random.default_rng(width)
    nprb, eaxc, symbol = 25, 3, 5
    mac_dst, mac_src = (1, 2, 3, 4, 5, 6), (7, 8, 9, 10, 11, 12)
    rec = ul.record_bytes(typ, width)
    headers = 18 + 8 + (8 if static else 10)
    flow = abi.OfhDlFlow((C.c_uint8 * 6)(*mac_dst), (C.c_uint8 * 6)(*mac_src), 0x2003, 0xAEFE, headers + 10 * rec, nprb, static,
                         abi.OfhCompressionCfg(typ, width, 0.9))
    frags = lib.ofh_dl_fragments(flow)
    assert [f[:2] for f in frags] == [(0, 10), (10, 10), (20, 5)]
    stride = (headers + 10 * rec + 15) // 16 * 16
    tx_grid = ul.to_bf16((rng.standard_normal((1, 1, 14, 12 * nprb, 2)) * 0.2).astype(np.float32))
    d_tx = torch.from_numpy(tx_grid.view(np.int16).copy()).cuda()
    d_frames = torch.zeros(3 * stride, dtype=torch.uint8, device="cuda")
    sym = abi.OfhDlSymbol(0, 0, 0, 0, eaxc, 0x107, 3, 1, symbol, 254, (C.c_uint8 * 2)(0, 0))
    assert gpu_ctx.ofh_dl_write_frames([flow], [sym], d_tx, 1, 1, 12 * nprb, d_frames, stride) == abi.OK
    gpu_ctx.synchronize()
    d_frames.view(3, stride)[:, 26] &= 0x7F   # data direction: downlink -> uplink
    torch.cuda.synchronize()
    wire = d_frames.cpu().numpy()
    cfg = model.default_cfg(mac_dst=bytes(mac_dst), mac_src=bytes(mac_src), vlan_tag_present=1, static_compression=static,
                            compression=(typ, width), prach_compression=(typ, width), ru_nof_prbs=nprb, ul_eaxc=(eaxc,), prach_eaxc=())
    expects = [model.expect(sfn8=7, subframe=3, slot=1, eaxc=eaxc, nof_prb=nprb)]
    ranges = [(k * stride, f[2]) for k, f in enumerate(frags)]
    rx = lib.OfhRx(gpu_ctx, make_cfg(cfg))
    d_grid = poison_words((1, 1, 14, 12 * nprb))
    d_records = torch.zeros(3 * C.sizeof(abi.OfhRxRecord), dtype=torch.uint8, device="cuda")
    assert rx.run(make_frames(ranges), [make_expect(e) for e in expects], d_frames, d_grid, 1, 1, 12 * nprb, d_records) == abi.OK
    gpu_ctx.synchronize()
    rx.close()
    got = [record_dict(r) for r in (abi.OfhRxRecord * 3).from_buffer_copy(d_records.cpu().numpy().tobytes())]
    assert [(r["status"], r["seq_skipped"], r["start_prb"], r["nof_prbs_written"], r["seq_id"] >> 8) for r in got] == \
        [(0, 0, 0, 10, 254), (0, 0, 10, 10, 255), (0, 0, 20, 5, 0)]
    out = host_words(d_grid)
    want = np.full(out.shape, POISON, np.uint32)
    for (off, _), (start, n, _) in zip(ranges, frags):
        records = wire[off + headers:off + headers + n * rec]
        want[0, 0, symbol, 12 * start:12 * (start + n)] = ul.words(gpu_ctx.ofh_decompress_host(abi.OfhCompressionCfg(typ, width, 1.0), records)).reshape(-1)
    assert same_bits(out, want)
    model_grid = np.full(out.shape, POISON, np.uint32)
    assert_records(got, model.Receiver(cfg).run(wire, ranges, expects, model_grid))
    assert same_bits(out, model_grid)


@pytest.mark.gpu
def test_host_form_equals_the_batched_call(gpu_ctx):
    cfg, names, buf, ranges, records, grid = mutation_case("size+dynamic")
    expects = [e for e in MUTATION_EXPECTS if e["grid_index"] == 0]
    rx = lib.OfhRx(gpu_ctx, make_cfg(cfg))
    host_grid = np.full(GRID_SHAPE[1:], POISON, np.uint32)
    want_grid = np.full((1,) + GRID_SHAPE[1:], POISON, np.uint32)
    ref = model.Receiver(cfg)
    for name, (off, length) in list(zip(names, ranges))[:30]:
        frame = buf[off:off + length].copy()
        rc, rec = rx.host(frame, [make_expect(e) for e in expects], host_grid)
        assert rc == abi.OK, name
        assert record_dict(rec) == ref.frame(frame, 0, length, expects, want_grid), name
    rx.close()
    assert same_bits(host_grid, want_grid[0]) and (host_grid != POISON).any()
