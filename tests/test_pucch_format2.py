"""PUCCH format 2 receiver (nrphy_pf2_*).

CPU: the POD mirrors and the six names; the validator over each refused case, over the reference unit tests' configurations
(tests/golden/pf2_configs.json) and over the cases of the reference's validator test; the extractor that wrote the fixture; the
DM-RS seed's 64-bit product; the taps; a noiseless loop-back of the restatement (tests/pucch2_model.py) over every fixture
configuration; and the restatement alone on the grids of the GPU link test, which is what lets that test demand every message.
GPU, on a grid of 52 PRB x 4 ports: estimator parity with the restatement, the soft bits against the composition of
nrphy_channel_equalize, nrphy_demodulate_soft and nrphy_llr_descramble byte for byte, the hand-over to the UCI decoder, the link,
edge inputs, batches against per-PUCCH host calls, graph replay, sentinels, and a slot shared with PUSCH and PUCCH format 1.

The grids come from the restatement's own transmitter, not from the reference's test vectors (which are not available): they show
that transmitter and receiver agree.  Format 2 has no recording of the reference's own answers yet; formats 0 and 1 have one
(tests/golden/record_pucch_reference.cpp).  What is independent of the restatement's author: the UCI encoder and decoder (pinned to
recorded reference results by tests/test_uci_decoder.py), the QPSK demapper and the Gold sequence (the C oracle's, pinned to the
compiled reference), and the equaliser's restatement (shared with the PUSCH demodulator's tests).
"""
import ctypes as C
import functools
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import backends
import pucch2_model as model
import pucch_model
import uci_model
from pusch_chest_model import as_i32, dev

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
REFERENCE = "/root/reference/srsRAN-5G-ER"
CSI_DTYPE = model.CSI_DTYPE
MEAS_DTYPE = np.dtype([("noise_var", "<f4"), ("rsrp", "<f4"), ("epre", "<f4"), ("snr", "<f4"), ("ta_s", "<f4"), ("ta_bins", "<i4"),
                       ("cfo_hz", "<f4"), ("reserved_", "<u4")])
SENTINEL = 0x5A5AA5A5
GUARD = 16  # sentinel words on either side of every output
NOF_PORTS, NOF_PRB = 4, 52
NOF_SUBC = 12 * NOF_PRB
CE_STRIDE = NOF_PORTS * 14 * NOF_SUBC
LLR_STRIDE, MSG_STRIDE = 512, 400  # bytes per PUCCH in the batch buffers: E <= 512, A <= 398
# The link test's signal-to-noise ratio per receive port, which test_restatement_returns_every_message_of_the_link_test vouches
# for: the weakest case is the (32, 25) polar code of A = 19 on one port, which needs about 10 dB for a block error rate of 1e-2.
LINK_SNR_DB = 20.0
NAMES = ("nrphy_pf2_validate", "nrphy_pf2_sizes", "nrphy_pf2_plan_create", "nrphy_pf2_plan_destroy", "nrphy_pf2_run", "nrphy_pf2_host")


def fixtures():
    return json.load(open(os.path.join(GOLDEN, "pf2_configs.json")))


def to_abi(cfg):
    return model.to_abi(abi, cfg)


def make_cfg(*args, **kw):
    """model.make_cfg with the BWP of the tests' grid (52 PRBs from PRB 0) unless told otherwise."""
    kw.setdefault("bwp_size_rb", NOF_PRB - kw.get("bwp_start_rb", 0))
    return model.make_cfg(*args, **kw)


# The smallest shapes at which each branch can go wrong: 1, 2, 3 and 16 PRB (3, 7 and 11 taps; 4, 3 and 5 virtual pilots; a full wave
# of pilots and 256 data REs), 1 symbol (no CFO) and 2, symbols 13 and 12-13, 1 to 4 ports permuted, the last PRBs of a BWP that does
# not start at 0, numerology 0 and 1, and A = 3, 11 (largest short block), 12 (smallest polar, parity-check bits), 19 and 20 (CRC6 /
# CRC11) and 398 at 16 PRB x 2 symbols (the largest the code rate admits).  One case has the DM-RS seed's product beyond 32 bits.
SHAPES = [
    ("1 PRB, 1 symbol, 1 port, A 3, last PRB of a BWP from 3",
     dict(starting_prb=48, nof_prb=1, nof_symbols=1, start_symbol_index=13, bwp_start_rb=3, rx_ports=(2,), nof_harq_ack=3, rnti=4660,
          n_id=77, n_id_0=1001, slot_index=3)),
    ("1 PRB, 2 symbols, 2 ports, A 12, numerology 1, 64-bit seed",
     dict(starting_prb=7, nof_prb=1, nof_symbols=2, start_symbol_index=12, rx_ports=(3, 1), nof_harq_ack=2, nof_sr=1, nof_csi_part1=9,
          rnti=65535, n_id=1023, n_id_0=65535, numerology=1, slot_index=19)),
    ("2 PRB, 1 symbol, 3 ports, A 11", dict(starting_prb=20, nof_prb=2, nof_symbols=1, start_symbol_index=13, rx_ports=(2, 0, 3),
                                            nof_harq_ack=4, nof_csi_part1=7, rnti=17, n_id=5, n_id_0=9, slot_index=9)),
    ("2 PRB, 2 symbols, 4 ports, A 20, last PRBs of a BWP from 10",
     dict(starting_prb=40, nof_prb=2, nof_symbols=2, start_symbol_index=12, bwp_start_rb=10, rx_ports=(3, 1, 0, 2), nof_harq_ack=8,
          nof_sr=2, nof_csi_part1=10, rnti=999, n_id=300, n_id_0=40000, slot_index=5)),
    ("3 PRB, 1 symbol, 4 ports, A 19", dict(starting_prb=0, nof_prb=3, nof_symbols=1, start_symbol_index=5, rx_ports=(0, 1, 2, 3),
                                            nof_csi_part1=19, rnti=2, n_id=1, n_id_0=3)),
    ("3 PRB, 2 symbols, 2 ports, A 20, numerology 1", dict(starting_prb=30, nof_prb=3, nof_symbols=2, start_symbol_index=12,
                                                           rx_ports=(1, 2), nof_harq_ack=20, rnti=40000, n_id=512, n_id_0=123,
                                                           numerology=1, slot_index=7)),
    ("16 PRB, 1 symbol, 4 ports, A 12", dict(starting_prb=5, nof_prb=16, nof_symbols=1, start_symbol_index=13, rx_ports=(1, 0, 3, 2),
                                             nof_harq_ack=12, rnti=321, n_id=11, n_id_0=22, slot_index=1)),
    ("16 PRB, 2 symbols, 4 ports, A 398, last PRBs of a BWP from 4",
     dict(starting_prb=32, nof_prb=16, nof_symbols=2, start_symbol_index=12, bwp_start_rb=4, rx_ports=(2, 3, 0, 1), nof_harq_ack=200,
          nof_sr=4, nof_csi_part1=194, rnti=12345, n_id=678, n_id_0=54321, slot_index=8)),
    ("1 PRB, 2 symbols, 1 port, A 19", dict(starting_prb=51, nof_prb=1, nof_symbols=2, start_symbol_index=0, rx_ports=(0,),
                                            nof_harq_ack=19, rnti=7, n_id=8, n_id_0=9, slot_index=2)),
    ("1 PRB, 1 symbol, 4 ports, A 11", dict(starting_prb=13, nof_prb=1, nof_symbols=1, start_symbol_index=13, rx_ports=(0, 2, 1, 3),
                                            nof_harq_ack=11, rnti=100, n_id=200, n_id_0=300, slot_index=6)),
]


def shape_cfg(kw):
    kw = dict(kw)
    return make_cfg(kw.pop("starting_prb"), kw.pop("nof_prb"), kw.pop("nof_symbols"), **kw)


@functools.lru_cache(maxsize=None)
def link_cases():
    """(what, cfg, message, grid words) per shape: seeded two-path channels with a delay, a CFO and AWGN at LINK_SNR_DB.  Computed
    once and shared by the CPU test that vouches for the SNR and by the GPU tests."""
    rng = np.random.default_rng(20261017)
    out = []
    for i, (what, kw) in enumerate(SHAPES):
        cfg = shape_cfg(kw)
        assert model.validate(cfg, NOF_PORTS, NOF_SUBC), what
        message = rng.integers(0, 2, model.payload_bits(cfg)).astype(np.uint8)
        grid = model.received_grid(rng, cfg, message, NOF_PORTS, NOF_SUBC, snr_db=LINK_SNR_DB, delay=float(i % 5) - 2.0,
                                   cfo=0.002 * ((i % 7) - 3), taps=2)
        out.append((what, cfg, message, model.quantize(grid)))
    return out


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_pf2_pods_match_header():
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(nrphy_pf2_cfg_t),
 offsetof(nrphy_pf2_cfg_t, slot_index), offsetof(nrphy_pf2_cfg_t, bwp_start_rb), offsetof(nrphy_pf2_cfg_t, nof_prb),
 offsetof(nrphy_pf2_cfg_t, nof_symbols), offsetof(nrphy_pf2_cfg_t, rnti), offsetof(nrphy_pf2_cfg_t, n_id_0),
 offsetof(nrphy_pf2_cfg_t, nof_csi_part2), offsetof(nrphy_pf2_cfg_t, nof_rx_ports), offsetof(nrphy_pf2_cfg_t, rx_ports),
 sizeof(nrphy_pf2_csi_t), offsetof(nrphy_pf2_csi_t, time_alignment_s), offsetof(nrphy_pf2_csi_t, cfo_hz));return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()
    P, R = abi.Pf2Cfg, abi.Pf2Csi
    assert [int(x) for x in out] == [C.sizeof(P), P.slot_index.offset, P.bwp_start_rb.offset, P.nof_prb.offset, P.nof_symbols.offset,
                                     P.rnti.offset, P.n_id_0.offset, P.nof_csi_part2.offset, P.nof_rx_ports.offset, P.rx_ports.offset,
                                     C.sizeof(R), R.time_alignment_s.offset, R.cfo_hz.offset]
    assert C.sizeof(R) == CSI_DTYPE.itemsize and C.sizeof(R) % 16 == 0


def test_pf2_names_are_declared_listed_and_exported():
    header = open(os.path.join(backends.ROOT, "include", "mi355_nrphy.h")).read()
    for name in NAMES:
        assert "int %s(" % name in header, name
        assert name in abi.ABI_SYMBOLS and hasattr(lib.load(), name), name
    assert sorted(s for s in abi.ABI_SYMBOLS if "_pf2_" in s) == sorted(NAMES)
    assert not [s for s in NAMES if "pucch" in s or "_uci_" in s or "_ulsch_" in s]


def _pf2(**kw):
    args = dict(starting_prb=1, nof_prb=10, nof_symbols=1, start_symbol=12, bwp_size_rb=42, bwp_start_rb=10, slot_index=9, rnti=65535,
                nof_harq_ack=3, rx_ports=(0,))
    args.update(kw)
    return abi.make_pf2(**args)


@pytest.mark.parametrize("name,cfg,want", [
    ("the reference validator test's base", _pf2(), abi.OK),
    ("A 3", _pf2(nof_harq_ack=1, nof_sr=1, nof_csi_part1=1), abi.OK),
    ("A 2", _pf2(nof_harq_ack=2), abi.ERR_ARGUMENT),
    ("A 0", _pf2(nof_harq_ack=0), abi.ERR_ARGUMENT),
    ("code rate exactly at the limit: (53 + 11) / 80", _pf2(nof_prb=5, nof_harq_ack=53), abi.OK),
    ("code rate above the limit: (54 + 11) / 80", _pf2(nof_prb=5, nof_harq_ack=54), abi.ERR_ARGUMENT),
    ("A 11 on 1 PRB x 1 symbol", _pf2(nof_prb=1, nof_harq_ack=11), abi.OK),
    ("A 12 on 1 PRB x 1 symbol: (12 + 6) / 16", _pf2(nof_prb=1, nof_harq_ack=12), abi.ERR_ARGUMENT),
    ("A 398 on 16 PRB x 2 symbols", _pf2(nof_prb=16, nof_symbols=2, nof_csi_part1=395), abi.OK),
    ("A 399 on 16 PRB x 2 symbols", _pf2(nof_prb=16, nof_symbols=2, nof_csi_part1=396), abi.ERR_ARGUMENT),
    ("A 1706", _pf2(nof_harq_ack=1706), abi.ERR_ARGUMENT),
    ("A 1707", _pf2(nof_harq_ack=1706, nof_sr=1), abi.ERR_ARGUMENT),
    ("a count that wraps", _pf2(nof_harq_ack=0xFFFFFFFF, nof_sr=4), abi.ERR_ARGUMENT),
    ("16 PRB", _pf2(nof_prb=16), abi.OK),
    ("17 PRB", _pf2(nof_prb=17), abi.ERR_ARGUMENT),
    ("no PRB", _pf2(nof_prb=0), abi.ERR_ARGUMENT),
    ("2 symbols, the last of the slot", _pf2(nof_symbols=2), abi.OK),
    ("3 symbols", _pf2(nof_symbols=3, start_symbol=0), abi.ERR_ARGUMENT),
    ("no symbol", _pf2(nof_symbols=0), abi.ERR_ARGUMENT),
    ("symbols beyond the slot", _pf2(nof_symbols=2, start_symbol=13), abi.ERR_ARGUMENT),
    ("start symbol 14", _pf2(start_symbol=14), abi.ERR_ARGUMENT),
    ("CSI part 2", _pf2(nof_csi_part2=1), abi.ERR_ARGUMENT),
    ("the last PRBs of the BWP", _pf2(starting_prb=32), abi.OK),
    ("a PRB beyond the BWP", _pf2(starting_prb=33), abi.ERR_ARGUMENT),
    ("BWP beyond the grid", _pf2(bwp_size_rb=43), abi.ERR_ARGUMENT),
    ("BWP start beyond the grid", _pf2(bwp_start_rb=60, bwp_size_rb=10), abi.ERR_ARGUMENT),
    ("ports in another order", _pf2(rx_ports=(3, 1, 0, 2)), abi.OK),
    ("no port", _pf2(rx_ports=()), abi.ERR_ARGUMENT),
    ("port outside the grid", _pf2(rx_ports=(0, 4)), abi.ERR_ARGUMENT),
    ("repeated port", _pf2(rx_ports=(0, 1, 1)), abi.ERR_ARGUMENT),
    ("numerology 4, last slot", _pf2(numerology=4, slot_index=159), abi.OK),
    ("numerology 5", _pf2(numerology=5), abi.ERR_ARGUMENT),
    ("slot beyond the frame", _pf2(slot_index=10), abi.ERR_ARGUMENT),
    ("rnti 65536", _pf2(rnti=65536), abi.ERR_ARGUMENT),
    ("n_id 1023", _pf2(n_id=1023), abi.OK),
    ("n_id 1024", _pf2(n_id=1024), abi.ERR_ARGUMENT),
    ("n_id_0 65535", _pf2(n_id_0=65535), abi.OK),
    ("n_id_0 65536", _pf2(n_id_0=65536), abi.ERR_ARGUMENT),
])
def test_pf2_validator(name, cfg, want):
    assert lib.pf2_validate(cfg, NOF_PORTS, NOF_SUBC) == want, name
    sizes = lib.pf2_sizes(cfg)
    if want == abi.OK:
        assert sizes == (16 * cfg.nof_prb * cfg.nof_symbols, cfg.nof_harq_ack + cfg.nof_sr + cfg.nof_csi_part1), name
        assert uci_model.validate(sizes[1], sizes[0], model.QPSK), name


def test_pf2_validator_refuses_five_ports_and_null():
    cfg = _pf2()
    cfg.nof_rx_ports = 5
    assert lib.pf2_validate(cfg, 8, NOF_SUBC) == abi.ERR_ARGUMENT
    assert lib.load().nrphy_pf2_validate(None, NOF_PORTS, NOF_SUBC) == abi.ERR_ARGUMENT
    assert lib.load().nrphy_pf2_sizes(None, None, None) == abi.ERR_ARGUMENT


def fixture_cfgs():
    """Every fixture row as a receiver configuration with the grid it needs: (cfg, grid ports, grid PRBs).  The demodulator's and the
    DM-RS rows carry no payload sizes: they take 4 HARQ-ACK bits; the DM-RS rows that hop are left out (the validator refuses
    frequency hopping for format 2, and the configuration cannot say it)."""
    fx = fixtures()
    out = []
    for f in fx["processor"]:
        out.append((model.from_fixture(f), max(f["rx_ports"]) + 1, f["grid_nof_prb"]))
    for f in fx["demodulator"]:
        cfg = model.make_cfg(f["first_prb"], f["nof_prb"], f["nof_symbols"], f["start_symbol_index"], bwp_size_rb=f["grid_nof_prb"],
                             rnti=f["rnti"], n_id=f["n_id"], nof_harq_ack=4, rx_ports=f["rx_ports"])
        out.append((cfg, max(f["rx_ports"]) + 1, f["grid_nof_prb"]))
    for f in fx["dmrs"]:
        if not f["intra_slot_hopping"]:
            cfg = model.make_cfg(f["starting_prb"], f["nof_prb"], f["nof_symbols"], f["start_symbol_index"], numerology=f["numerology"],
                                 slot_index=f["slot_index"], n_id=f["n_id"], n_id_0=f["n_id_0"], nof_harq_ack=4, rx_ports=f["rx_ports"])
            out.append((cfg, max(f["rx_ports"]) + 1, 275))
    return out


def test_pf2_validator_over_the_reference_configurations():
    fx = fixtures()
    assert (len(fx["processor"]), len(fx["demodulator"]), len(fx["dmrs"]), len(fx["validator"]["cases"])) == (144, 48, 8, 11)
    cfgs = fixture_cfgs()
    assert len(cfgs) == 144 + 48 + 4
    for cfg, ports, prbs in cfgs:
        assert lib.pf2_validate(to_abi(cfg), ports, 12 * prbs) == abi.OK, cfg
        assert model.validate(cfg, ports, 12 * prbs), cfg
        assert lib.pf2_validate(to_abi(cfg), ports, 12 * (cfg["bwp_start_rb"] + cfg["bwp_size_rb"] - 1)) == abi.ERR_ARGUMENT, cfg
        assert lib.pf2_validate(to_abi(cfg), max(cfg["rx_ports"]), 12 * prbs) == abi.ERR_ARGUMENT, cfg
    # The cases of the reference's validator test.  Its processor is built for 13 symbols and 1 receive port, so two of its
    # refusals are limits of that instance, not of the format: here the slot has 14 symbols and the grid 4 ports.  Frequency
    # hopping has no field in nrphy_pf2_cfg_t: that case cannot be stated.
    base = fx["validator"]["base"]
    accepted_here = {"OFDM symbol allocation goes up to symbol": {13}, "The number of receive ports": {2}}
    seen = 0
    for case in fx["validator"]["cases"]:
        sets = dict(case["sets"])
        if "second_hop_prb" in sets:
            continue
        f = dict(base, **sets)
        cfg = model.from_fixture(f)
        want = abi.ERR_ARGUMENT
        if case["message"] in accepted_here and (f["start_symbol_index"] in accepted_here[case["message"]] or
                                                 len(f["rx_ports"]) in accepted_here[case["message"]]):
            want = abi.OK
        assert lib.pf2_validate(to_abi(cfg), NOF_PORTS, 12 * 275) == want, case
        assert model.validate(cfg, NOF_PORTS, 12 * 275) == (want == abi.OK), case
        seen += 1
    assert seen == 10
    assert lib.pf2_validate(to_abi(model.from_fixture(base)), NOF_PORTS, 12 * 275) == abi.OK


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_extractor_reproduces_the_committed_fixture():
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([os.environ.get("PYTHON", "python3"), os.path.join(GOLDEN, "extract_pf2_configs.py"), REFERENCE, d], check=True,
                       timeout=120)
        assert open(os.path.join(d, "pf2_configs.json")).read() == open(os.path.join(GOLDEN, "pf2_configs.json")).read()


def test_dmrs_seed_is_a_64_bit_product():
    """n_id_0 = 65535 in the last slot of numerology 4, last symbol: (14 x 159 + 14)(2 x 65535 + 1) 2^17 is 3.8e13.  The restatement
    (Python integers) against the same expression in 64-bit words, and against what the expression means: the seed's low 17 bits are
    2 n_id_0, its bits 17 to 30 the low 14 bits of (14 n_slot + l + 1)(2 n_id_0 + 1)."""
    for numerology, slot, symbol, n_id_0 in ((4, 159, 13, 65535), (1, 19, 13, 65535), (0, 3, 13, 1001), (0, 0, 0, 0)):
        cfg = model.make_cfg(0, 1, 1, symbol, numerology=numerology, slot_index=slot, n_id_0=n_id_0, nof_harq_ack=3)
        wide = (np.uint64(14 * slot + symbol + 1) * np.uint64(2 * n_id_0 + 1) * np.uint64(1 << 17) + np.uint64(2 * n_id_0)) % np.uint64(1 << 31)
        c = model.dmrs_c_init(cfg, symbol)
        assert c == int(wide) and c & 0x1FFFF == 2 * n_id_0 and c >> 17 == ((14 * slot + symbol + 1) * (2 * n_id_0 + 1)) & 0x3FFF
    assert (14 * 159 + 14) * (2 * 65535 + 1) * (1 << 17) > 1 << 32


def test_filter_taps_sum_to_one():
    """3, 7 and 11 taps for 1, 2 and 3 or more PRBs.  Each tap is a table entry times the rounded reciprocal of their float32 sum:
    the sum of T taps is within (T + 2) half-ulps of 1."""
    for nof_rb, ntaps, nof_v in ((1, 3, 4), (2, 7, 3), (3, 11, 5), (16, 11, 5)):
        taps = model.filter_taps(nof_rb)
        assert taps.dtype == np.float32 and taps.size == ntaps and model.nof_virtual_pilots(nof_rb, ntaps) == nof_v
        assert abs(float(np.sum(taps.astype(np.float64))) - 1.0) <= (ntaps + 2) * 2.0 ** -24, nof_rb
        assert (taps == taps[::-1]).all() and taps[ntaps // 2] == taps.max()


def test_restatement_loop_back_over_the_reference_configurations(oracle):
    """Every fixture configuration on a grid built from random bits, without noise: a gain and a phase per port and a delay of three
    samples of a 4096-point transform."""
    rng = np.random.default_rng(7)
    count = 0
    for cfg, ports, prbs in fixture_cfgs():
        message = rng.integers(0, 2, model.payload_bits(cfg)).astype(np.uint8)
        grid = np.zeros((ports, 14, 12 * prbs), complex)
        gains = [0.8 * np.exp(1j * (0.3 + 1.1 * p)) for p in range(ports)]
        model.add_to_grid(grid, model.transmit(cfg, message), gains, delay=3.0, numerology=cfg["numerology"])
        r = model.process(cfg, model.quantize(grid), oracle)
        assert r["status"] == model.VALID and (r["message"] == message).all(), cfg
        count += 1
    assert count == 196


def test_restatement_returns_every_message_of_the_link_test(oracle):
    """The condition that lets the GPU link test demand every message: at LINK_SNR_DB the restatement alone returns all of them."""
    for what, cfg, message, grid in link_cases():
        r = model.process(cfg, grid, oracle)
        assert r["status"] == model.VALID and (r["message"] == message).all(), what


# =======================================================================================================================
# GPU
# =======================================================================================================================
def guarded(nbytes, fill=SENTINEL):
    """A device buffer of `nbytes` (a multiple of 4) between two guards of sentinel words: (whole tensor, the view to hand over)."""
    import torch
    words = nbytes // 4
    whole = torch.full((words + 2 * GUARD,), int(np.uint32(SENTINEL).view(np.int32)), dtype=torch.int32, device="cuda")
    if fill != SENTINEL:
        whole[GUARD:GUARD + words] = int(np.uint32(fill).view(np.int32))
    return whole, whole[GUARD:GUARD + words]


def guards_intact(whole):
    a = whole.cpu().numpy().view(np.uint32)
    return bool((a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all())


def sentinel_bytes(lo, hi):
    """Bytes [lo, hi) of a buffer of sentinel words."""
    return np.frombuffer(np.uint32(SENTINEL).tobytes(), np.uint8)[np.arange(lo, hi) % 4]


def make_plan(ctx, cfgs, grid_indices, n_grids, with_ce=True):
    n = len(cfgs)
    return lib.Pf2Plan(ctx, [to_abi(c) for c in cfgs], grid_indices, n_grids, NOF_PORTS, NOF_SUBC, [i * LLR_STRIDE for i in range(n)],
                       [i * MSG_STRIDE for i in range(n)], [i * CE_STRIDE for i in range(n)] if with_ce else None)


def make_outputs(n, with_ce=True):
    return {"llr": guarded(n * LLR_STRIDE), "message": guarded(n * MSG_STRIDE), "status": guarded(4 * n),
            "csi": guarded(n * CSI_DTYPE.itemsize), "meas": guarded(n * NOF_PORTS * MEAS_DTYPE.itemsize),
            "ce": guarded(4 * n * CE_STRIDE) if with_ce else (None, None)}


def read_outputs(cfgs, outputs):
    """Per PUCCH a dict of llr [E], message [A], status, csi, meas [4], ce [4][14][subc] (sentinel words where nothing was written),
    after checking the guards around every output."""
    n = len(cfgs)
    for whole, _ in outputs.values():
        assert whole is None or guards_intact(whole)
    raw = {k: v.cpu().numpy() for k, (_, v) in outputs.items() if v is not None}
    out = []
    for i, cfg in enumerate(cfgs):
        E, A = model.nof_llr(cfg), model.payload_bits(cfg)
        llr = raw["llr"].view(np.int8)[i * LLR_STRIDE:(i + 1) * LLR_STRIDE]
        msg = raw["message"].view(np.uint8)[i * MSG_STRIDE:(i + 1) * MSG_STRIDE]
        assert (llr[E:].view(np.uint8) == sentinel_bytes(E, LLR_STRIDE)).all(), "soft bits beyond E"
        assert (msg[A:] == sentinel_bytes(A, MSG_STRIDE)).all(), "message bytes beyond A"
        out.append({"llr": llr[:E].copy(), "message": msg[:A].copy(), "status": int(raw["status"].view(np.uint32)[i]),
                    "csi": raw["csi"].view(CSI_DTYPE)[i].copy(), "meas": raw["meas"].view(MEAS_DTYPE).reshape(n, NOF_PORTS)[i].copy(),
                    "ce": raw["ce"].view(np.uint32).reshape(n, NOF_PORTS, 14, NOF_SUBC)[i].copy() if "ce" in raw else None})
    return out


def run_plan(ctx, cfgs, grid_indices, grids, with_ce=True, stream=None, plan=None, outputs=None):
    own = plan is None
    n_grids = len(grids) if not hasattr(grids, "data_ptr") else grids.shape[0]
    if own:
        plan = make_plan(ctx, cfgs, grid_indices, n_grids, with_ce)
    d_grid = dev(as_i32(np.asarray(grids))) if not hasattr(grids, "data_ptr") else grids
    if outputs is None:
        outputs = make_outputs(len(cfgs), with_ce)
    o = {k: v for k, (_, v) in outputs.items()}
    plan.run(d_grid, o["llr"], o["message"], o["status"], o["csi"], o["meas"], o["ce"], stream=stream)
    ctx.synchronize()
    out = read_outputs(cfgs, outputs)
    if own:
        plan.close()
    return out


_LINK_RUN = {}


def link_run(ctx):
    """One batch run over link_cases(), shared by the tests that read its outputs (nothing modifies them)."""
    if "out" not in _LINK_RUN:
        cases = link_cases()
        _LINK_RUN["out"] = run_plan(ctx, [c for _, c, _, _ in cases], list(range(len(cases))), np.stack([g for _, _, _, g in cases]))
    return _LINK_RUN["out"]


def bf16_ulps(a, b):
    """Largest distance in bf16 steps between the components of two arrays of cbf16 words (sign-magnitude order)."""
    def key(h):
        h = h.astype(np.int64)
        return np.where(h & 0x8000, -(h & 0x7FFF), h & 0x7FFF)
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    return np.maximum(np.abs(key(a & 0xFFFF) - key(b & 0xFFFF)), np.abs(key(a >> 16) - key(b >> 16)))


def region(cfg):
    """Mask [14][subc] of what a run writes of every receive port's estimate."""
    m = np.zeros((14, NOF_SUBC), bool)
    k0 = 12 * model.first_prb(cfg)
    m[cfg["start_symbol_index"]:cfg["start_symbol_index"] + cfg["nof_symbols"], k0:k0 + 12 * cfg["nof_prb"]] = True
    return m


def device_estimate(cfg, got):
    """The run's estimate in the restatement's layout [rx][nof_symbols][12 nof_prb], and its noise variances [rx]."""
    P, k0, s0 = len(cfg["rx_ports"]), 12 * model.first_prb(cfg), cfg["start_symbol_index"]
    est = got["ce"][:P, s0:s0 + cfg["nof_symbols"], k0:k0 + 12 * cfg["nof_prb"]]
    return est, got["meas"]["noise_var"][:P].copy()


@pytest.mark.gpu
def test_estimator_parity_with_the_restatement(gpu_ctx):
    """The tolerances of tests/test_pusch_channel_estimator.py::check_parity.  Time alignment: the device's bin must have, in the
    float64 restatement's spectrum, a magnitude within 1e-4 of the peak's (at 1 PRB neighbouring bins differ by about 2e-5 of the
    peak: an exact-bin check would compare rounding noise)."""
    worst = {"ulp": 0, "meas": 0.0, "cfo": 0.0, "ta": 0.0}
    for (what, cfg, _, grid), got in zip(link_cases(), link_run(gpu_ctx)):
        want_est, want_meas = model.estimate(cfg, grid)
        _, meas64 = model.estimate(cfg, grid, np.float64)
        P = len(cfg["rx_ports"])
        m = region(cfg)
        est, _ = device_estimate(cfg, got)
        scs = 15000 << cfg["numerology"]
        for p in range(NOF_PORTS):
            if p >= P:
                assert (got["ce"][p] == SENTINEL).all() and got["meas"][p].tobytes() == bytes(MEAS_DTYPE.itemsize), (what, p)
                continue
            u = bf16_ulps(est[p], want_est[p])
            worst["ulp"] = max(worst["ulp"], int(u.max()))
            assert u.max() <= 1, (what, p, int(u.max()), int((u > 1).sum()))
            assert (got["ce"][p][~m] == SENTINEL).all(), (what, "outside the region", p)
            g, w = got["meas"][p], want_meas[p]
            for key in ("rsrp", "epre", "snr", "noise_var"):
                worst["meas"] = max(worst["meas"], abs(float(g[key]) - float(w[key])) / abs(float(w[key])))
                assert float(g[key]) == pytest.approx(float(w[key]), rel=1e-4), (what, key, p)
            if np.isnan(w["cfo_hz"]):
                assert np.isnan(g["cfo_hz"]) and cfg["nof_symbols"] == 1, what
            else:
                worst["cfo"] = max(worst["cfo"], abs(float(g["cfo_hz"]) - float(w["cfo_hz"])))
                assert abs(float(g["cfo_hz"]) - float(w["cfo_hz"])) <= max(1e-4 * abs(float(w["cfo_hz"])), 1e-3 * scs), what
            mag = meas64[p]["ta_mag"]
            assert -model.TA_WINDOW <= int(g["ta_bins"]) < model.TA_WINDOW, what
            short = 1.0 - mag[model.ta_bin_index(int(g["ta_bins"]))] / mag.max()
            worst["ta"] = max(worst["ta"], float(short))
            assert short <= 1e-4, (what, p, int(g["ta_bins"]), want_meas[p]["ta_bins"], short)
            assert float(g["ta_s"]) == pytest.approx(int(g["ta_bins"]) / (4096.0 * scs), rel=1e-6)
        # channel state information: from the device's own per-port measurements exactly, and the best-SNR port's bin as above
        dev_meas = [{k: got["meas"][p][k] for k in ("noise_var", "rsrp", "epre", "snr", "ta_s", "cfo_hz")} for p in range(P)]
        csi, best = model.channel_state_information(dev_meas)
        assert got["csi"].tobytes() == csi.tobytes(), (what, got["csi"], csi)
        assert got["csi"]["time_alignment_s"] == got["meas"][best]["ta_s"]
    print("estimate: worst %d bf16 ulp; measurements: worst %.3g relative; CFO: worst %.3g Hz; time alignment: the device's bin at "
          "most %.3g of the peak below it" % (worst["ulp"], worst["meas"], worst["cfo"], worst["ta"]))


@pytest.mark.gpu
def test_soft_bits_equal_the_composed_calls_bit_for_bit(gpu_ctx, oracle):
    """From the estimate and noise variances the same run wrote: nrphy_channel_equalize over the gathered data REs ->
    nrphy_demodulate_soft (QPSK, one span) -> nrphy_llr_descramble equals d_llr byte for byte, and so does the restatement's
    equaliser + the oracle's demapper + descrambler fed with those estimates."""
    for (what, cfg, _, grid), got in zip(link_cases(), link_run(gpu_ctx)):
        est, nv = device_estimate(cfg, got)
        rx, ch = model.data_res(cfg, grid, est)
        eq, ev = gpu_ctx.channel_equalize_host(abi.EQ_ZF, rx, ch[None], nv, 1.0)
        soft = gpu_ctx.demodulate_soft_host(model.QPSK, eq[:, 0], ev[:, 0])
        composed = gpu_ctx.llr_descramble_host((cfg["rnti"] << 15) + cfg["n_id"], soft)
        assert composed.tobytes() == got["llr"].tobytes(), (what, int((composed != got["llr"]).sum()))
        assert model.demodulate(cfg, grid, est, nv, oracle).tobytes() == got["llr"].tobytes(), what
        assert np.abs(got["llr"].astype(int)).max() > 0, what


@pytest.mark.gpu
def test_decoder_hand_over(gpu_ctx):
    for (what, cfg, _, _), got in zip(link_cases(), link_run(gpu_ctx)):
        A, E = model.payload_bits(cfg), model.nof_llr(cfg)
        message, status = gpu_ctx.uci_decode_host(abi.make_uci_decoder(A, E, model.QPSK), got["llr"])
        assert (message.tobytes(), status) == (got["message"].tobytes(), got["status"]), what
        want, want_status = uci_model.decode(got["llr"], A, model.QPSK)
        assert (want.tobytes(), want_status) == (got["message"].tobytes(), got["status"]), what
    assert sorted({model.payload_bits(c) for _, c, _, _ in link_cases()}) == [3, 11, 12, 19, 20, 398]


@pytest.mark.gpu
def test_link_returns_every_message(gpu_ctx):
    for (what, cfg, message, _), got in zip(link_cases(), link_run(gpu_ctx)):
        assert got["status"] == abi.UCI_STATUS_VALID and got["message"].tobytes() == message.tobytes(), what


def same_result(got, want, what):
    """The device's outputs against model.process's: status, bits and the (possibly non-finite) dB values exactly."""
    assert got["status"] == want["status"] and got["message"].tobytes() == want["message"].tobytes(), what
    for key in ("sinr_dB", "rsrp_dB", "epre_dB", "time_alignment_s", "cfo_hz"):
        assert np.float32(got["csi"][key]).tobytes() == np.float32(want["csi"][key]).tobytes(), (what, key, got["csi"], want["csi"])


@pytest.mark.gpu
def test_edge_inputs(gpu_ctx, oracle):
    """A zero grid and noise-only grids give the restatement's status, bits and dB values; a wrong rnti, n_id or n_id_0 at A >= 12
    comes back invalid."""
    rng = np.random.default_rng(33)
    picks = [0, 1, 3, 4, 7]
    cfgs = [shape_cfg(SHAPES[i][1]) for i in picks]
    zero = np.zeros((NOF_PORTS, 14, NOF_SUBC), np.uint32)
    noise = [model.quantize(s * (rng.standard_normal((NOF_PORTS, 14, NOF_SUBC)) + 1j * rng.standard_normal((NOF_PORTS, 14, NOF_SUBC))))
             for s in (1.0, 1e-3)]
    grids = np.stack([zero] + noise)
    batch = [(c, g) for g in range(3) for c in cfgs]
    out = run_plan(gpu_ctx, [c for c, _ in batch], [g for _, g in batch], grids)
    valid = 0
    for (cfg, g), got in zip(batch, out):
        want = model.process(cfg, grids[g], oracle)
        same_result(got, want, (cfg, g))
        valid += got["status"] == abi.UCI_STATUS_VALID
        if g == 0:
            assert not got["llr"].any(), cfg
            assert np.isneginf(got["csi"]["epre_dB"]) and np.isneginf(got["csi"]["rsrp_dB"]) and got["csi"]["sinr_dB"] == 60.0, got["csi"]
            assert got["csi"]["time_alignment_s"] == 0.0 and (np.isnan(got["csi"]["cfo_hz"]) or cfg["nof_symbols"] == 2), got["csi"]
    print("noise-only and zero grids: %d of %d declared valid" % (valid, len(batch)))
    wrong = []
    for what, cfg, message, grid in link_cases():
        if model.payload_bits(cfg) >= 12:
            for key, value in (("rnti", cfg["rnti"] ^ 1), ("n_id", cfg["n_id"] ^ 1), ("n_id_0", cfg["n_id_0"] ^ 1)):
                wrong.append((dict(cfg, **{key: value}), grid, what + ", wrong " + key))
    assert len(wrong) == 3 * 7
    out = run_plan(gpu_ctx, [c for c, _, _ in wrong], list(range(len(wrong))), np.stack([g for _, g, _ in wrong]), with_ce=False)
    for (_, _, what), got in zip(wrong, out):
        assert got["status"] == abi.UCI_STATUS_INVALID, what


@pytest.mark.gpu
def test_batch_equals_per_pucch_host_calls(gpu_ctx):
    for (what, cfg, _, grid), got in zip(link_cases(), link_run(gpu_ctx)):
        n = len(cfg["rx_ports"])
        r = gpu_ctx.pf2_host(to_abi(cfg), grid, with_estimate=True, ch_est=np.full((n, 14, NOF_SUBC), SENTINEL, np.uint32))
        assert (r["status"], r["message"].tobytes(), r["llr"].tobytes()) == (got["status"], got["message"].tobytes(), got["llr"].tobytes()), what
        assert bytes(r["csi"]) == got["csi"].tobytes(), what
        assert b"".join(bytes(x) for x in r["meas"]) == got["meas"][:n].tobytes(), what
        assert r["ch_est"].tobytes() == got["ce"][:n].tobytes(), what
    plain = gpu_ctx.pf2_host(to_abi(link_cases()[3][1]), link_cases()[3][3])
    assert plain["ch_est"] is None and plain["message"].tobytes() == link_cases()[3][2].tobytes()


@pytest.mark.gpu
def test_graph_replay_and_two_runs_give_identical_bytes(gpu_ctx):
    import torch
    cases = link_cases()
    cfgs = [c for _, c, _, _ in cases]
    index = list(range(len(cases)))
    d_grid = dev(as_i32(np.stack([g for _, _, _, g in cases])))
    plan = make_plan(gpu_ctx, cfgs, index, len(cases))
    keys = ("llr", "message", "status", "csi", "meas", "ce")
    runs = []
    for _ in range(2):
        outputs = make_outputs(len(cfgs))
        run_plan(gpu_ctx, cfgs, index, d_grid, plan=plan, outputs=outputs)
        runs.append({k: outputs[k][1].cpu().numpy().tobytes() for k in keys})
    assert runs[0] == runs[1]
    outputs = make_outputs(len(cfgs))
    o = {k: v for k, (_, v) in outputs.items()}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.run(d_grid, o["llr"], o["message"], o["status"], o["csi"], o["meas"], o["ce"], stream=C.c_void_p(stream.cuda_stream))
    for _ in range(2):
        for k in keys:
            o[k].fill_(int(np.uint32(SENTINEL).view(np.int32)))
        graph.replay()
        torch.cuda.synchronize()
        for k in keys:
            assert o[k].cpu().numpy().tobytes() == runs[0][k], k
            assert guards_intact(outputs[k][0]), k
    plan.close()


@pytest.mark.gpu
def test_twiddles_are_built_on_first_use_and_outlive_a_plan(gpu_ctx):
    """The time-alignment twiddles are the context's: the first plan of a fresh context builds them, destroying that plan leaves
    them, and a second plan reads the same table.  Both runs give the bytes the session's context gives in link_run (whose
    parity tests vouch for them), so the table of a first use is the right one."""
    what, cfg, message, grid = link_cases()[0]
    ctx = lib.Context(0)
    try:
        runs = [run_plan(ctx, [cfg], [0], grid[None])[0] for _ in range(2)]  # each creates its plan, runs it and destroys it
    finally:
        ctx.close()
    for got in runs:
        for key in ("llr", "message", "csi", "meas", "ce"):
            assert got[key].tobytes() == link_run(gpu_ctx)[0][key].tobytes(), (what, key)
        assert got["status"] == abi.UCI_STATUS_VALID and got["message"].tobytes() == message.tobytes(), what


@pytest.mark.gpu
def test_unaligned_soft_bit_offsets_and_no_optional_outputs(gpu_ctx):
    """Soft bits at an offset that is no multiple of 16 take the byte path; d_meas and d_ch_est may be NULL."""
    cases = [link_cases()[i] for i in (1, 7)]
    cfgs = [c for _, c, _, _ in cases]
    plan = lib.Pf2Plan(gpu_ctx, [to_abi(c) for c in cfgs], [0, 1], 2, NOF_PORTS, NOF_SUBC, [3, 3 + LLR_STRIDE], [1, 1 + MSG_STRIDE])
    outputs = make_outputs(3, with_ce=False)
    o = {k: v for k, (_, v) in outputs.items()}
    plan.run(dev(as_i32(np.stack([g for _, _, _, g in cases]))), o["llr"], o["message"], o["status"], o["csi"], None, None)
    gpu_ctx.synchronize()
    plan.close()
    assert all(guards_intact(w) for w, _ in outputs.values() if w is not None)
    llr, msg = o["llr"].cpu().numpy().view(np.int8), o["message"].cpu().numpy().view(np.uint8)
    for i, (got, (what, cfg, message, _)) in enumerate(zip([link_run(gpu_ctx)[j] for j in (1, 7)], cases)):
        E, A = model.nof_llr(cfg), model.payload_bits(cfg)
        assert llr[3 + i * LLR_STRIDE:3 + i * LLR_STRIDE + E].tobytes() == got["llr"].tobytes(), what
        assert msg[1 + i * MSG_STRIDE:1 + i * MSG_STRIDE + A].tobytes() == message.tobytes(), what
    assert (o["meas"].cpu().numpy().view(np.uint32) == SENTINEL).all()
    # The receiver launch alone: the same soft bits, nothing decoded; one of the two decoder outputs alone is refused.
    plan = make_plan(gpu_ctx, cfgs, [0, 1], 2, with_ce=False)
    outputs = make_outputs(2, with_ce=False)
    o = {k: v for k, (_, v) in outputs.items()}
    d_grid = dev(as_i32(np.stack([g for _, _, _, g in cases])))
    plan.run(d_grid, o["llr"], None, None, o["csi"])
    gpu_ctx.synchronize()
    with pytest.raises(lib.NrphyError):
        plan.run(d_grid, o["llr"], o["message"], None, o["csi"])
    plan.close()
    assert all(guards_intact(w) for w, _ in outputs.values() if w is not None)
    llr = o["llr"].cpu().numpy().view(np.int8)
    for i, j in enumerate((1, 7)):
        assert llr[i * LLR_STRIDE:i * LLR_STRIDE + model.nof_llr(cfgs[i])].tobytes() == link_run(gpu_ctx)[j]["llr"].tobytes()
    assert (o["message"].cpu().numpy().view(np.uint32) == SENTINEL).all() and (o["status"].cpu().numpy().view(np.uint32) == SENTINEL).all()


@pytest.mark.gpu
def test_pusch_and_both_pucch_receivers_share_one_grid_buffer_and_stream(gpu_ctx):
    """A slot with a PUSCH on PRBs 10..29 (estimator + demodulator), a hopping format 1 PUCCH on PRBs 0 and 51 and a format 2 PUCCH on
    PRBs 40..42 of symbols 12-13: three plans read the same device grid on the same stream, and each gives what its host call gives."""
    import torch
    rng = np.random.default_rng(9)
    f1 = pucch_model.make_cfg(1, 0, 14, 0, second_hop_prb=51, bwp_size_rb=52, n_id=40, slot_index=6, initial_cyclic_shift=2,
                              nof_harq_ack=2, ports=(0, 1, 2, 3))
    f2 = make_cfg(40, 3, 2, 12, n_id=40, n_id_0=40, rnti=4097, slot_index=6, nof_harq_ack=4, nof_csi_part1=16, rx_ports=(0, 1, 2, 3))
    message = rng.integers(0, 2, 20).astype(np.uint8)
    gains = [1.0, 0.8j, -0.9, 0.7 - 0.2j]
    grid = 0.2 * (rng.standard_normal((NOF_PORTS, 14, NOF_SUBC)) + 1j * rng.standard_normal((NOF_PORTS, 14, NOF_SUBC)))
    pucch_model.add_to_grid(grid, pucch_model.transmit(f1, [0, 1]), gains, delay=2.0)
    model.add_to_grid(grid, model.transmit(f2, message), gains, delay=2.0)
    words = model.quantize(grid)
    pusch = abi.make_pusch_chest(prbs=range(10, 30), slot_index=6, scrambling_id=40, dmrs_symbols=(2, 11), rx_ports=(0, 1, 2, 3))
    demod = abi.make_pusch_demod(prbs=range(10, 30), qm=2, rnti=4097, n_id=40, dmrs_symbols=(2, 11), rx_ports=(0, 1, 2, 3))
    d_grid = dev(as_i32(words[None]))
    chest = lib.PuschChestPlan(gpu_ctx, [pusch], [0], 1, NOF_PORTS, NOF_SUBC, [0])
    pdemod = lib.PuschDemodPlan(gpu_ctx, [demod], [0], 1, NOF_PORTS, NOF_SUBC, [0])
    pucch = lib.PucchPlan(gpu_ctx, [pucch_model.to_abi(abi, f1)], [0], 1, NOF_PORTS, NOF_SUBC)
    pf2 = make_plan(gpu_ctx, [f2], [0], 1, with_ce=False)
    G = pdemod.codeword_bits(0)
    ce_w, ce = guarded(4 * CE_STRIDE, fill=0)
    nv_w, nv = guarded(4 * NOF_PORTS)
    cw_w, cw = guarded((G + 3) // 4 * 4)
    res_w, res = guarded(pucch_model.RESULT_DTYPE.itemsize)
    outputs = make_outputs(1, with_ce=False)
    o = {k: v for k, (_, v) in outputs.items()}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    handle = C.c_void_p(stream.cuda_stream)
    chest.run(d_grid, ce, nv, stream=handle)
    pdemod.run(d_grid, ce, nv, cw, G, stream=handle)
    pucch.run(d_grid, res, stream=handle)
    pf2.run(d_grid, o["llr"], o["message"], o["status"], o["csi"], o["meas"], None, stream=handle)
    stream.synchronize()
    assert guards_intact(ce_w) and guards_intact(nv_w) and guards_intact(cw_w) and guards_intact(res_w)
    want_ce, want_nv, _ = gpu_ctx.pusch_chest_host(pusch, words)
    assert ce.cpu().numpy().view(np.uint32).tobytes() == want_ce.tobytes()
    assert nv.cpu().numpy().view(np.float32).tobytes() == want_nv.tobytes()
    want_cw, _ = gpu_ctx.pusch_demodulate_host(demod, words, want_ce, want_nv)
    assert cw.cpu().numpy().view(np.int8)[:G].tobytes() == want_cw.tobytes()
    r1 = res.cpu().numpy().view(pucch_model.RESULT_DTYPE)[0]
    assert r1.tobytes() == bytes(gpu_ctx.pucch_host(pucch_model.to_abi(abi, f1), words)[0])
    assert r1["status"] == abi.PUCCH_STATUS_VALID and list(r1["harq_ack"]) == [0, 1]
    got = read_outputs([f2], outputs)[0]
    want = gpu_ctx.pf2_host(to_abi(f2), words)
    assert (got["status"], got["message"].tobytes(), got["llr"].tobytes()) == (want["status"], want["message"].tobytes(), want["llr"].tobytes())
    assert got["csi"].tobytes() == bytes(want["csi"])
    assert got["status"] == abi.UCI_STATUS_VALID and got["message"].tobytes() == message.tobytes()
    for plan in (chest, pdemod, pucch, pf2):
        plan.close()
