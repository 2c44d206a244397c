"""Open Fronthaul downlink transmit (nrphy_ofh_dl_fragments, nrphy_ofh_dl_validate, nrphy_ofh_dl_write_frames,
nrphy_ofh_dl_frames_host): OFDM symbols of the device-resident downlink grid to complete Ethernet frames.

The reference's frames were recorded once by tests/golden/record_ofh_dl_reference.cpp, which drives srsRAN-5G-ER's real
data_flow_uplane_downlink_data_impl with the real VLAN Ethernet and eCPRI builders, both user-plane message builders, the AVX2
compressors and an eth_frame_pool of the case's MTU on seeded grids.  The grids are regenerated here from their seeds;
tests/golden/ofh_dl_reference_* hold the cases and the frames.  Everything is bytes, so every comparison is exact: the NumPy
restatement (tests/ofh_dl_model.py, records from the oracle's ofh_compress per fragment) against the recording on the CPU, the
device against the recording and the restatement on the GPU.

The grids hold integers and every case's iq_scaling makes the quantiser multiply by exactly 2.5, so odd values land on x.5 (the
reference's vector loop rounds them to even, the tail of a compress() call away from zero) and magnitudes from 16384 on leave the
int16 range (the vector loop saturates, the tail wraps): where a call ends shows in the bytes.

Two things differ from the wording of the change request, on purpose:
* It asks for the records of case a (the reference unit test's 186 + 87 PRBs) to differ from a whole-symbol row at the second
  fragment's tail.  They cannot: 186 * 24 values is a multiple of the 16-value vector, so the second fragment's vector loop starts
  where the whole row's does and both end with the same 8-value tail.  test_case_a_... pins that on the CPU, and the property
  itself -- a fragment is its own compress() call -- is checked where it shows: the fragments of cases c, f, h and j.
* It asks for one launch that mixes cases c, d, e and g "with two flows": those are four compressions, so four flows.  A launch
  has one grid width and case e's radio unit has 1 PRB, so that batch runs on a 12-subcarrier grid; a second batch (c, d, g, k)
  runs on a 240-subcarrier grid.
"""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import backends
import ofh_dl_model as model

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
SENTINEL = 0xA7


def iq_scaling_of(case):
    return float(np.uint32(case["iq_scaling_bits"]).view(np.float32))


class Recording:
    def __init__(self):
        self.cases = json.load(open(os.path.join(GOLDEN, "ofh_dl_reference_cases.json")))
        self.bytes = np.load(os.path.join(GOLDEN, "ofh_dl_reference_frames.npy"))
        self.by_name = {c["name"]: c for c in self.cases}
        self._grids = {}

    def grid(self, c):
        """uint16 [ports][14][nof_subc][2], computed once per case and never modified"""
        key = (c["seed"], c["grid_ports"], c["grid_nof_subc"])
        if key not in self._grids:
            self._grids[key] = model.seeded_grid(*key)
            self._grids[key].setflags(write=False)
        return self._grids[key]

    def frames(self, s):
        return [self.bytes[f["offset"]:f["offset"] + f["frame_bytes"]] for f in s["frames"]]


@pytest.fixture(scope="module")
def recording():
    return Recording()


@pytest.fixture(scope="module")
def compress(oracle):
    """One compress() call of the AVX2 compressors, from the oracle."""
    return lambda typ, width, iq_scaling, prbs: oracle.ofh_compress(abi.OfhCompressionCfg(typ, width, iq_scaling), prbs)


def flow_dict(c):
    return dict(mac_dst=c["mac_dst"], mac_src=c["mac_src"], tci=c["tci"], eth_type=c["eth_type"], mtu=c["mtu"], ru_nof_prbs=c["ru_nof_prbs"],
                static_compression=c["static_compression"], type=c["type"], data_width=c["data_width"], iq_scaling=iq_scaling_of(c))


def sym_dict(c, s, **kw):
    return dict(dict(port=s["port"], eaxc=s["eaxc"], sfn=c["sfn"], subframe=c["subframe"], slot=c["slot"], symbol=s["symbol"], seq_id=s["seq_id"],
                     flow=0, grid_index=0, frame_offset=0), **kw)


def make_flow(mac_dst=(1, 2, 3, 4, 5, 6), mac_src=(7, 8, 9, 10, 11, 12), tci=1, eth_type=0xAEFE, mtu=1500, ru_nof_prbs=25, static_compression=1,
              type=1, data_width=9, iq_scaling=1.0):
    return abi.OfhDlFlow((C.c_uint8 * 6)(*mac_dst), (C.c_uint8 * 6)(*mac_src), tci, eth_type, mtu, ru_nof_prbs, static_compression,
                         abi.OfhCompressionCfg(type, data_width, iq_scaling))


def make_symbol(frame_offset=0, flow=0, grid_index=0, port=0, eaxc=0, sfn=0, subframe=0, slot=0, symbol=0, seq_id=0, reserved_=(0, 0)):
    return abi.OfhDlSymbol(frame_offset, flow, grid_index, port, eaxc, sfn, subframe, slot, symbol, seq_id, (C.c_uint8 * 2)(*reserved_))


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_library_loads_without_a_device_and_the_pods_match_the_header():
    handle = lib.load()
    names = [s for s in abi.ABI_SYMBOLS if "_ofh_dl_" in s]
    assert len(names) == 4 and not [s for s in names if not hasattr(handle, s)]
    structs = [("nrphy_ofh_dl_flow_t", abi.OfhDlFlow), ("nrphy_ofh_dl_fragment_t", abi.OfhDlFragment), ("nrphy_ofh_dl_symbol_t", abi.OfhDlSymbol)]
    exprs, want = [], []
    for cname, S in structs:
        exprs.append("sizeof(%s)" % cname)
        want.append(C.sizeof(S))
        for f in S._fields_:
            exprs.append("offsetof(%s, %s)" % (cname, f[0]))
            want.append(getattr(S, f[0]).offset)
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


def test_recording_holds_the_cases_of_the_change_request(recording):
    frags = lambda name, i=0: [(f["start_prb"], f["nof_prbs"]) for f in recording.by_name[name]["symbols"][i]["frames"]]
    sizes = lambda name: [f["frame_bytes"] for f in recording.by_name[name]["symbols"][0]["frames"]]
    assert frags("a_unit_test_none16_two_fragments") == [(0, 186), (186, 87)]            # the reference unit test's segmented_prbs
    assert frags("b_bfp9_one_fragment_of_273") == [(0, 273)]
    assert recording.frames(recording.by_name["b_bfp9_one_fragment_of_273"]["symbols"][0])[0][33] == 0   # numPrbu of more than 255 PRBs
    for name in ("c_bfp12_dynamic_mtu1500_106", "c_bfp12_static_mtu1500_106", "h_sequence_wraps"):
        assert frags(name) == [(0, 39), (39, 39), (78, 28)]
    assert frags("d_none16_mtu1500_273") == [(30 * i, 30) for i in range(9)] + [(270, 3)]
    last = recording.frames(recording.by_name["d_none16_mtu1500_273"]["symbols"][0])[-1]
    assert (last[31], last[32]) == (1, 270 - 256)                                         # the 2 MSBs of startPrbu are used
    assert sizes("e_none8_static_one_prb") == [64] and sizes("e_none8_dynamic_one_prb") == [64]   # 58 and 60 bytes, padded
    e = recording.frames(recording.by_name["e_none8_static_one_prb"]["symbols"][0])[0]
    assert (e[58:] == 0).all() and e[34:58].any()
    f = recording.by_name["f_mtu_of_headers_and_one_record"]
    assert f["mtu"] == 34 + 48 and frags(f["name"]) == [(i, 1) for i in range(4)]
    g = recording.by_name["g_ru_25_prbs_over_a_240_subcarrier_grid"]
    body = recording.frames(g["symbols"][0])[0][34:].reshape(25, 28)
    assert (body[20:] == 0).all() and body[:20, 1:].any()                                 # five zero PRBs, exponent 0
    h = recording.frames(recording.by_name["h_sequence_wraps"]["symbols"][0])
    assert [int(x[24]) for x in h] == [254, 255, 0] and all(x[25] == 0x80 for x in h)
    j = recording.by_name["j_three_symbols_sfn_777"]
    assert (j["sfn"], j["subframe"], j["slot"]) == (777, 7, 5) and [s["symbol"] for s in j["symbols"]] == [0, 1, 2]
    for s in j["symbols"]:
        for k, x in enumerate(recording.frames(s)):
            assert (x[27], x[28], x[29]) == (777 & 0xFF, 7 << 4 | 5 >> 2, (5 & 3) << 6 | s["symbol"]) == (9, 0x71, 0x40 | s["symbol"])
            assert x[24] == s["seq_id"] + k
    assert {(c["static_compression"], c["name"][0]) for c in recording.cases} >= {(0, "c"), (1, "c"), (0, "e"), (1, "e")}
    assert recording.bytes.nbytes < 64 * 1024


def test_restatement_equals_every_recorded_frame(recording, compress):
    n = 0
    for c in recording.cases:
        grid = recording.grid(c)
        for s in c["symbols"]:
            got = model.symbol_frames(flow_dict(c), sym_dict(c, s), grid[s["port"], s["symbol"]], compress)
            want = recording.frames(s)
            assert len(got) == len(want), c["name"]
            for k, (a, b) in enumerate(zip(got, want)):
                assert same(a, b), (c["name"], s["symbol"], k)
                n += 1
    assert n == 37


def per_fragment_and_whole_row(c, s, grid, compress):
    """-> [(records of the fragment as its own call, the same PRBs sliced from one call for the whole symbol)]"""
    rec = model.record_bytes(c["type"], c["data_width"])
    full = np.zeros((12 * c["ru_nof_prbs"], 2), np.uint16)
    row = grid[s["port"], s["symbol"]]
    full[:len(row)] = row
    whole = compress(c["type"], c["data_width"], iq_scaling_of(c), full.reshape(-1, 12, 2))
    out = []
    for f in s["frames"]:
        prbs = full[12 * f["start_prb"]:12 * (f["start_prb"] + f["nof_prbs"])].reshape(-1, 12, 2)
        out.append((compress(c["type"], c["data_width"], iq_scaling_of(c), prbs), whole[rec * f["start_prb"]:rec * (f["start_prb"] + f["nof_prbs"])]))
    return out


# (case, fragment) whose records differ from the slice of a whole-symbol compress() call, all in the fragment's last PRB
DIFFERING = [("c_bfp12_dynamic_mtu1500_106", 0), ("c_bfp12_dynamic_mtu1500_106", 1), ("f_mtu_of_headers_and_one_record", 0),
             ("h_sequence_wraps", 0), ("j_three_symbols_sfn_777", 1)]


def test_a_fragment_is_its_own_compress_call_where_the_grids_make_it_show(recording, compress):
    """From the oracle, before the GPU test relies on it: the recorded frames hold the per-fragment records, and for the fragments
    of DIFFERING those are not the whole-symbol row's."""
    for name, k in DIFFERING:
        c = recording.by_name[name]
        s = c["symbols"][0]
        own, sliced = per_fragment_and_whole_row(c, s, recording.grid(c), compress)[k]
        hdr, rec = model.header_bytes(c["static_compression"]), model.record_bytes(c["type"], c["data_width"])
        assert same(recording.frames(s)[k][hdr:hdr + own.size], own), (name, k)
        differ = np.nonzero(own != sliced)[0]
        assert differ.size and (differ // rec == s["frames"][k]["nof_prbs"] - 1).all(), (name, k)


def test_case_a_cannot_differ_from_the_whole_symbol_row(recording, compress):
    """186 * 24 = 279 * 16: the second fragment's vector loop starts on the whole row's 16-value grid and 87 * 24 and 273 * 24 leave
    the same 8 values to the tail.  So for case a per-fragment and whole-symbol compression are the same bytes, whatever the grid."""
    c = recording.by_name["a_unit_test_none16_two_fragments"]
    assert (186 * 24) % 16 == 0 and (87 * 24) % 16 == (273 * 24) % 16 == 8
    for own, sliced in per_fragment_and_whole_row(c, c["symbols"][0], recording.grid(c), compress):
        assert same(own, sliced)
    # and the tail of that call is exercised all the same: with the tail's rule applied to all values the bytes change
    tail = recording.grid(c)[0, 13, -4:].astype(np.uint32) << 16
    assert (np.abs(tail.view(np.float32)) * 2.5 % 2 == 0.5).any() or (np.abs(tail.view(np.float32)) * 2.5 > 32767).any()


MTUS = [64, 65, 81, 82, 83, 100, 127, 128, 255, 256, 511, 1023, 1024, 1499, 1500, 1501, 4095, 4096, 8999, 9000, 9001, 9599, 9600]


def test_fragments_of_the_library_equal_the_restatement():
    n_refused = n = 0
    for typ in (0, 1):
        for width in range(8, 17):
            for static in (0, 1):
                for mtu in MTUS + [model.header_bytes(static) + model.record_bytes(typ, width) + d for d in (-1, 0, 1)]:
                    for ru in (1, 2, 25, 106, 273, 275):
                        want = model.fragments(mtu, ru, static, typ, width) if mtu >= 64 else None
                        got = lib.ofh_dl_fragments(make_flow(mtu=mtu, ru_nof_prbs=ru, static_compression=static, type=typ, data_width=width))
                        assert got == want, (typ, width, static, mtu, ru)
                        n += 1
                        n_refused += want is None
                        if want is not None:
                            assert sum(f[1] for f in want) == ru and all(f[2] <= max(mtu, 64) for f in want)
    assert n_refused > 50 and n - n_refused > 3000
    # the caller's array too short: refused, the count reported
    out, cnt = (abi.OfhDlFragment * 2)(), C.c_uint32(0)
    assert lib.load().nrphy_ofh_dl_fragments(C.byref(make_flow(mtu=128, ru_nof_prbs=25)), 2, out, C.byref(cnt)) == abi.ERR_ARGUMENT
    assert cnt.value == len(model.fragments(128, 25, 1, 1, 9)) == 9


GRID = dict(nof_grids=2, grid_nof_ports=2, grid_nof_subc=240, frames_bytes=1 << 16, frame_stride=1504)


@pytest.mark.parametrize("name,flows,symbols,change,want", [
    ("a good batch", [make_flow(), make_flow(type=0, data_width=16, mtu=200, ru_nof_prbs=20, static_compression=0)],
     [make_symbol(), make_symbol(frame_offset=1504, flow=1, grid_index=1, port=1, symbol=13, subframe=9, slot=15, sfn=1023, seq_id=255, eaxc=65535)],
     {}, True),
    ("no symbol", [make_flow()], [], {}, True),
    ("nothing at all", [], [], {}, True),
    ("unknown compression type", [make_flow(type=2)], [make_symbol()], {}, False),
    ("width 7", [make_flow(data_width=7)], [make_symbol()], {}, False),
    ("width 17", [make_flow(data_width=17)], [make_symbol()], {}, False),
    ("width 8", [make_flow(data_width=8)], [make_symbol()], {}, True),
    ("width 16", [make_flow(data_width=16)], [make_symbol()], {}, True),
    ("a scaling that is not finite", [make_flow(iq_scaling=float("inf"))], [make_symbol()], {}, False),
    ("no PRB", [make_flow(ru_nof_prbs=0)], [make_symbol()], dict(grid_nof_subc=0), False),
    ("276 PRBs", [make_flow(ru_nof_prbs=276)], [make_symbol()], {}, False),
    ("275 PRBs", [make_flow(ru_nof_prbs=275)], [make_symbol()], {}, True),
    ("static_compression 2", [make_flow(static_compression=2)], [make_symbol()], {}, False),
    ("mtu 9601", [make_flow(mtu=9601)], [make_symbol()], dict(frame_stride=9616), False),
    ("mtu 9600", [make_flow(mtu=9600)], [make_symbol()], dict(frame_stride=9600), True),
    ("mtu one byte short of headers and a record", [make_flow(mtu=34 + 48 - 1, type=0, data_width=16)], [make_symbol()], {}, False),
    ("mtu of headers and a record", [make_flow(mtu=34 + 48, type=0, data_width=16)], [make_symbol()], {}, True),
    ("the dynamic builder's two bytes more", [make_flow(mtu=34 + 48 + 1, type=0, data_width=16, static_compression=0)], [make_symbol()], {}, False),
    ("mtu below the shortest frame", [make_flow(mtu=63, data_width=8, type=0)], [make_symbol()], {}, False),
    ("a grid of 241 subcarriers", [make_flow()], [make_symbol()], dict(grid_nof_subc=241), False),
    ("a grid wider than the radio unit", [make_flow(ru_nof_prbs=19)], [make_symbol()], {}, False),
    ("a grid as wide as the radio unit", [make_flow(ru_nof_prbs=20)], [make_symbol()], {}, True),
    ("flow beyond the list", [make_flow()], [make_symbol(flow=1)], {}, False),
    ("grid index beyond the batch", [make_flow()], [make_symbol(grid_index=2)], {}, False),
    ("port beyond the grid", [make_flow()], [make_symbol(port=2)], {}, False),
    ("symbol 14", [make_flow()], [make_symbol(symbol=14)], {}, False),
    ("subframe 10", [make_flow()], [make_symbol(subframe=10)], {}, False),
    ("slot 16", [make_flow()], [make_symbol(slot=16)], {}, False),
    ("sfn 1024", [make_flow()], [make_symbol(sfn=1024)], {}, False),
    ("reserved byte 0", [make_flow()], [make_symbol(reserved_=(1, 0))], {}, False),
    ("reserved byte 1", [make_flow()], [make_symbol(reserved_=(0, 1))], {}, False),
    ("stride below the mtu", [make_flow()], [make_symbol()], dict(frame_stride=1488), False),
    ("stride no multiple of 16", [make_flow()], [make_symbol()], dict(frame_stride=1508), False),
    ("a frame up to the last byte", [make_flow()], [make_symbol(frame_offset=(1 << 16) - 734)], {}, True),
    ("a frame one byte beyond", [make_flow()], [make_symbol(frame_offset=(1 << 16) - 733)], {}, False),
    ("the second fragment beyond", [make_flow(mtu=400)], [make_symbol(frame_offset=(1 << 16) - 1504)], {}, False),
    ("an offset beyond everything", [make_flow()], [make_symbol(frame_offset=1 << 40)], {}, False),
    ("two symbols on one frame", [make_flow()], [make_symbol(), make_symbol(symbol=1, frame_offset=733)], {}, False),
    ("neighbours to the byte", [make_flow()], [make_symbol(), make_symbol(symbol=1, frame_offset=734)], {}, True),
    ("interleaved fragments of two symbols", [make_flow(mtu=400)], [make_symbol(), make_symbol(symbol=1, frame_offset=400)], {}, True),
    ("interleaved fragments that touch", [make_flow(mtu=400)], [make_symbol(), make_symbol(symbol=1, frame_offset=397)], {}, False),
])
def test_validator(name, flows, symbols, change, want):
    got = lib.ofh_dl_validate(flows, symbols, **dict(GRID, **change))
    assert got == (abi.OK if want else abi.ERR_ARGUMENT), name


# =======================================================================================================================
# GPU
# =======================================================================================================================
def device_grid(grid):
    import torch
    return torch.from_numpy(np.ascontiguousarray(grid).view(np.int16).copy()).cuda()


def run_batch(gpu_ctx, flows, symbols, grids, frames_bytes, frame_stride, base_skew=0, stream=None):
    """flows, symbols: dicts; grids uint16 [nof_grids][ports][14][nof_subc][2] -> (status, the whole frame buffer as uint8)"""
    import torch
    d_grid = device_grid(grids)
    d_frames = torch.full((frames_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    fl = [make_flow(**f) for f in flows]
    sy = [make_symbol(**s) for s in symbols]
    rc = gpu_ctx.ofh_dl_write_frames(fl, sy, d_grid, grids.shape[0], grids.shape[1], grids.shape[3], d_frames, frame_stride, stream=stream)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    return rc, d_frames.cpu().numpy()


def expected_buffer(flows, symbols, grids, frames_bytes, frame_stride, compress):
    want = np.full(frames_bytes, SENTINEL, np.uint8)
    for s in symbols:
        for k, fr in enumerate(model.symbol_frames(flows[s["flow"]], s, grids[s["grid_index"], s["port"], s["symbol"]], compress)):
            at = s["frame_offset"] + k * frame_stride
            assert (want[at:at + fr.size] == SENTINEL).all()
            want[at:at + fr.size] = fr
    return want


@pytest.mark.gpu
def test_device_reproduces_every_recorded_case_through_the_host_form(gpu_ctx, recording):
    for c in recording.cases:
        grid = recording.grid(c)
        stride = (c["mtu"] + 15) // 16 * 16
        for s in c["symbols"]:
            lead = 48 + 5  # the first frame at an odd byte of the host buffer
            frames = np.full(lead + stride * len(s["frames"]) + 7, SENTINEL, np.uint8)
            rc = gpu_ctx.ofh_dl_frames_host(make_flow(**flow_dict(c)), make_symbol(**sym_dict(c, s, port=0, frame_offset=lead)),
                                            grid[s["port"], s["symbol"]], frames, stride)
            assert rc == abi.OK, c["name"]
            untouched = np.ones(frames.size, bool)
            for k, want in enumerate(recording.frames(s)):
                at = lead + k * stride
                assert same(frames[at:at + want.size], want), (c["name"], s["symbol"], k)
                untouched[at:at + want.size] = False
            assert (frames[untouched] == SENTINEL).all(), c["name"]
    # refused: a port (the host form has one row), and what the validator refuses
    c = recording.cases[0]
    frames = np.full(1 << 15, SENTINEL, np.uint8)
    row = recording.grid(c)[0, 0]
    assert gpu_ctx.ofh_dl_frames_host(make_flow(**flow_dict(c)), make_symbol(port=1), row, frames, 9008) == abi.ERR_ARGUMENT
    assert gpu_ctx.ofh_dl_frames_host(make_flow(**flow_dict(c)), make_symbol(symbol=14), row, frames, 9008) == abi.ERR_ARGUMENT
    assert gpu_ctx.ofh_dl_frames_host(make_flow(**flow_dict(c)), make_symbol(), row, frames[:9008 + 4209], 9008) == abi.ERR_ARGUMENT
    assert (frames == SENTINEL).all()


@pytest.mark.gpu
def test_device_reproduces_every_recorded_case_in_place_with_sentinels(gpu_ctx, recording):
    """nrphy_ofh_dl_write_frames, one launch per case: the frames equal the recording, every other byte keeps the sentinel."""
    for c in recording.cases:
        grid = recording.grid(c)[None]
        stride = (c["mtu"] + 15) // 16 * 16 + 16
        nfr = len(c["symbols"][0]["frames"])
        symbols = [sym_dict(c, s, frame_offset=32 + i * nfr * stride) for i, s in enumerate(c["symbols"])]
        size = 32 + len(symbols) * nfr * stride + 16
        rc, got = run_batch(gpu_ctx, [flow_dict(c)], symbols, grid, size, stride)
        assert rc == abi.OK, c["name"]
        untouched = np.ones(size, bool)
        for s, d in zip(c["symbols"], symbols):
            for k, want in enumerate(recording.frames(s)):
                at = d["frame_offset"] + k * stride
                assert same(got[at:at + want.size], want), (c["name"], s["symbol"], k)
                untouched[at:at + want.size] = False
        assert (got[untouched] == SENTINEL).all(), c["name"]


@pytest.mark.gpu
@pytest.mark.parametrize("nof_subc,names", [
    (12, ["c_bfp12_dynamic_mtu1500_106", "d_none16_mtu1500_273", "e_none8_static_one_prb", "g_ru_25_prbs_over_a_240_subcarrier_grid"]),
    (240, ["c_bfp12_dynamic_mtu1500_106", "d_none16_mtu1500_273", "g_ru_25_prbs_over_a_240_subcarrier_grid", "k_none12_dynamic_two_fragments"]),
])
def test_one_launch_for_a_mixed_batch(gpu_ctx, recording, compress, nof_subc, names):
    """The flows of four recorded cases, two grids of two ports, descriptors in no particular order, frames at scattered offsets of
    every alignment modulo 16, on a stream of the caller's: equal to the restatement, sentinels elsewhere; then a refused batch and
    an empty one leave the buffer alone."""
    import torch
    flows = [flow_dict(recording.by_name[n]) for n in names]
    grids = model.seeded_grid(77 + nof_subc, 4, nof_subc).reshape(2, 2, 14, nof_subc, 2)
    stride = 1504
    rng = np.random.default_rng(nof_subc)
    symbols, at = [], 0
    for i in range(12):
        f = int(rng.integers(0, 4))
        nfr = len(model.fragments(flows[f]["mtu"], flows[f]["ru_nof_prbs"], flows[f]["static_compression"], flows[f]["type"], flows[f]["data_width"]))
        at += int(rng.integers(0, 40))                                  # a gap, so that offsets take every alignment
        symbols.append(dict(frame_offset=at, flow=f, grid_index=int(rng.integers(0, 2)), port=int(rng.integers(0, 2)), eaxc=int(rng.integers(0, 32)),
                            sfn=int(rng.integers(0, 1024)), subframe=int(rng.integers(0, 10)), slot=int(rng.integers(0, 16)),
                            symbol=int(rng.integers(0, 14)), seq_id=int(rng.integers(0, 256))))
        at += nfr * stride
    assert len({s["frame_offset"] % 16 for s in symbols}) >= 6 and len({s["flow"] for s in symbols}) == 4
    order = rng.permutation(len(symbols))
    symbols = [symbols[i] for i in order]
    size = at + 5
    stream = torch.cuda.Stream()
    rc, got = run_batch(gpu_ctx, flows, symbols, grids, size, stride, stream=C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    assert rc == abi.OK
    want = expected_buffer(flows, symbols, grids, size, stride, compress)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    # refused (two descriptors on one frame) and empty: nothing is written
    d_grid = device_grid(grids)
    d_frames = torch.full((size,), SENTINEL, dtype=torch.uint8, device="cuda")
    fl = [make_flow(**f) for f in flows]
    assert gpu_ctx.ofh_dl_write_frames(fl, [make_symbol(**symbols[0]), make_symbol(**dict(symbols[1], frame_offset=symbols[0]["frame_offset"] + 1))],
                                       d_grid, 2, 2, nof_subc, d_frames, stride) == abi.ERR_ARGUMENT
    assert gpu_ctx.ofh_dl_write_frames(fl, [], d_grid, 2, 2, nof_subc, d_frames, stride) == abi.OK
    gpu_ctx.synchronize()
    assert (d_frames.cpu().numpy() == SENTINEL).all()


@pytest.mark.gpu
def test_records_equal_the_existing_kernel_per_fragment_and_not_a_slice_of_a_whole_row(gpu_ctx, recording):
    """Each fragment's records = nrphy_ofh_compress on that fragment's PRBs as one row; for the fragments of DIFFERING they are not
    the slice of a whole-symbol row of the same kernel (the CPU test above shows the grids make these differ)."""
    differing = set(DIFFERING)
    seen = set()
    for c in recording.cases:
        cfg = abi.OfhCompressionCfg(c["type"], c["data_width"], iq_scaling_of(c))
        hdr, rec = model.header_bytes(c["static_compression"]), model.record_bytes(c["type"], c["data_width"])
        s = c["symbols"][0]
        full = np.zeros((12 * c["ru_nof_prbs"], 2), np.uint16)
        row = recording.grid(c)[s["port"], s["symbol"]]
        full[:len(row)] = row
        stride = (c["mtu"] + 15) // 16 * 16
        frames = np.full(stride * len(s["frames"]), SENTINEL, np.uint8)
        assert gpu_ctx.ofh_dl_frames_host(make_flow(**flow_dict(c)), make_symbol(**sym_dict(c, s, port=0)), row, frames, stride) == abi.OK
        whole = gpu_ctx.ofh_compress_host(cfg, full.reshape(-1, 12, 2))
        for k, f in enumerate(s["frames"]):
            got = frames[k * stride + hdr:k * stride + hdr + f["nof_prbs"] * rec]
            own = gpu_ctx.ofh_compress_host(cfg, full[12 * f["start_prb"]:12 * (f["start_prb"] + f["nof_prbs"])].reshape(-1, 12, 2))
            assert same(got, own), (c["name"], k)
            sliced = whole[rec * f["start_prb"]:rec * (f["start_prb"] + f["nof_prbs"])]
            if (c["name"], k) in differing:
                tail = slice((f["nof_prbs"] - 1) * rec, f["nof_prbs"] * rec)
                assert not same(got[tail], sliced[tail]) and same(got[:tail.start], sliced[:tail.start]), (c["name"], k)
                seen.add((c["name"], k))
    assert seen == differing


@pytest.mark.gpu
def test_seeded_random_sweep(gpu_ctx, compress):
    """30 launches of small random flows and descriptors: every type and width, both builders, MTUs from one record per frame to
    all PRBs in one, grids narrower than the radio unit, 1 to 4 descriptors per launch."""
    rng = np.random.default_rng(2024)
    widths = set()
    for trial in range(30):
        typ, width, static = trial % 2, 8 + (trial // 2) % 9, int(rng.integers(0, 2))
        widths.add((typ, width))
        rec, hdr = model.record_bytes(typ, width), model.header_bytes(static)
        ru = int(rng.integers(1, 61))
        fit = int(rng.integers(1, ru + 3))
        mtu = max(64, hdr + fit * rec + int(rng.integers(0, rec)))
        grid_prbs = ru if rng.integers(0, 2) else int(rng.integers(1, ru + 1))
        iq_scaling = float(np.float32(2.5 / ((1 << ((16 if typ else width) - 1)) - 1)))
        flow = dict(mac_dst=rng.integers(0, 256, 6).tolist(), mac_src=rng.integers(0, 256, 6).tolist(), tci=int(rng.integers(0, 65536)),
                    eth_type=int(rng.integers(0, 65536)), mtu=mtu, ru_nof_prbs=ru, static_compression=static, type=typ, data_width=width,
                    iq_scaling=iq_scaling)
        grids = model.seeded_grid(1000 + trial, 2, 12 * grid_prbs).reshape(1, 2, 14, 12 * grid_prbs, 2)
        stride = (mtu + 15) // 16 * 16
        nfr = len(model.fragments(mtu, ru, static, typ, width))
        symbols, at = [], int(rng.integers(0, 16))
        for i in range(int(rng.integers(1, 5))):
            symbols.append(dict(frame_offset=at, flow=0, grid_index=0, port=int(rng.integers(0, 2)), eaxc=int(rng.integers(0, 65536)),
                                sfn=int(rng.integers(0, 1024)), subframe=int(rng.integers(0, 10)), slot=int(rng.integers(0, 16)),
                                symbol=int(rng.integers(0, 14)), seq_id=int(rng.integers(0, 256))))
            at += nfr * stride + int(rng.integers(0, 16))
        size = at + 3
        rc, got = run_batch(gpu_ctx, [flow], symbols, grids, size, stride)
        assert rc == abi.OK, (trial, flow)
        want = expected_buffer([flow], symbols, grids, size, stride, compress)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (trial, flow, bad[:8], got[bad[:8]], want[bad[:8]])
    assert widths == {(t, w) for t in (0, 1) for w in range(8, 17)}
