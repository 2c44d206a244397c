"""PUCCH format 0 and format 1 receivers (nrphy_pucch_*).

CPU: the POD mirrors, the validator over each refused case and over the reference unit tests' 186 configurations
(tests/golden/pucch_configs.json), the extractor that wrote the fixtures and the generator of csrc/pucch_tables.inc, the
restatement's sequences (tests/pucch_model.py) against their definitions, and a noiseless loop-back of the restatement over every
fixture configuration; the restatement in float32 and float64 against a recording of the reference's own answers
(tests/golden/record_pucch_reference.cpp and pucch_reference_*.npy: 271 cases on noisy two-tap channels), and that recording's
own consistency.
GPU: the fixture configurations on grids built here; the recording through one plan and through host calls; parity with the
restatement on seeded multipath + CFO + AWGN grids; physics (zero grid, noise only, CFO and gain measured back, wrong cyclic
shift and OCC); batches against per-PUCCH host calls, graph replay, sentinels, and a slot with PUSCH and PUCCH on one grid buffer.

The grids of the known-answer and loop-back tests come from the restatement's own transmitter, not from the reference's test
vectors (which are not available): they show that transmitter and receivers agree with each other.  What is independent of the
restatement's author is the recording -- the reference's detectors, estimator and equaliser, compiled and run on grids from the
recorder's transmitter, which takes its sequences from the reference --, the low-PAPR and cover-code definitions check, the
cyclic shift index against the C oracle's Gold generator, and the phi tables, which are extracted from the reference.
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
import pucch_model as model
from pusch_chest_model import as_i32, dev

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
REFERENCE = "/root/reference/srsRAN-5G-ER"
RESULT_DTYPE = model.RESULT_DTYPE
MEAS_DTYPE = np.dtype([("noise_var", "<f4"), ("rsrp", "<f4"), ("epre", "<f4"), ("snr", "<f4"), ("ta_s", "<f4"), ("ta_bins", "<i4"),
                       ("cfo_hz", "<f4"), ("reserved_", "<u4")])
SENTINEL = 0x5A5AA5A5
GUARD = 16  # sentinel words on either side of every output
NOF_PORTS, NOF_PRB = 4, 52
NOF_SUBC = 12 * NOF_PRB

# Largest |float32 restatement - float64 restatement| over the cases of test_parity_with_the_restatement (the test prints both
# again on every run), of the detection metric, the three dB values and the per-port measurements relative to max(|value|,
# FLOOR), and of the CFO in Hz relative to max(|cfo|, CFO_FLOOR_HZ).  The device may differ from the float64 restatement by 8 x
# that: it folds its double partial sums in another order than the restatement's pairwise sums, and its libm is not NumPy's.
# This is the float32-to-float64 spread of the parity cases and nothing more; the reference's own error is REF_SPREAD below.
MODEL_SPREAD = 2.85e-5  # measured 2.843e-05: format 0's metric, whose avg_pwr - corr cancels at the higher SNRs
CFO_SPREAD = 5.52e-5    # measured 5.517e-05
FLOOR = 1e-3        # metrics and linear powers
DB_FLOOR = 1.0      # dB values
CFO_FLOOR_HZ = 1.0

# The recording (tests/golden/record_pucch_reference.cpp).  Largest distance, in the terms of distance() below, between what the
# reference answered and the float64 restatement, over every recorded case that is not flagged; test_restatement_equals_the_recording
# measures and prints them again on every run.  The largest metric distance belongs to cases in which nothing was sent for the
# configuration (noise only, another cyclic shift or cover code): there the detected symbol is what is left of a sum that
# cancels, and the reference's float32 sums lose what cancelled.  REF_SIGNAL_SPREAD is the same over the cases whose UE was sent.
REF_SPREAD = 1.53e-3         # measured 1.521e-03: case 267, read with another cover code, detection_metric 0.0037
REF_SIGNAL_SPREAD = 9.3e-5   # measured 9.264e-05: case 208, format 1 on 14 symbols
REF_CFO_SPREAD = 4.37e-4     # measured 4.367e-04: case 96, two UEs on one PRB, Hz relative to max(|CFO|, 1 Hz)
REF_ESTIMATE_ULPS = 0        # float32 restatement's estimate against the recorded one, in bf16 steps: every word equal
# The recording admits no case whose decided metric lies in [T / 2, 2 T] and, where a UE was sent, none whose two best format 0
# candidates, two format 1 statistics or two best per-port SNRs are within this of the larger.
RECORDING_MARGIN = 0.02
NOF_RECORDED, NOF_FLAGGED = 271, 2


def make_cfg(*args, **kw):
    """model.make_cfg with the BWP of the tests' grid (52 PRBs from PRB 0) unless told otherwise."""
    kw.setdefault("bwp_size_rb", NOF_PRB - kw.get("bwp_start_rb", 0))
    return model.make_cfg(*args, **kw)


def fixtures():
    return json.load(open(os.path.join(GOLDEN, "pucch_configs.json")))


def to_abi(cfg):
    return model.to_abi(abi, cfg)


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_pucch_pods_match_header():
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u %u %u %u %u\n", sizeof(nrphy_pucch_cfg_t),
 offsetof(nrphy_pucch_cfg_t, slot_index), offsetof(nrphy_pucch_cfg_t, second_hop_prb), offsetof(nrphy_pucch_cfg_t, nof_symbols),
 offsetof(nrphy_pucch_cfg_t, time_domain_occ), offsetof(nrphy_pucch_cfg_t, n_id), offsetof(nrphy_pucch_cfg_t, sr_opportunity),
 offsetof(nrphy_pucch_cfg_t, rx_ports), sizeof(nrphy_pucch_result_t), offsetof(nrphy_pucch_result_t, harq_ack),
 offsetof(nrphy_pucch_result_t, detection_metric), offsetof(nrphy_pucch_result_t, time_alignment_s),
 offsetof(nrphy_pucch_result_t, cfo_hz), NRPHY_PUCCH_FORMAT_0, NRPHY_PUCCH_FORMAT_1, NRPHY_PUCCH_NO_HOP, NRPHY_PUCCH_STATUS_UNKNOWN,
 NRPHY_PUCCH_STATUS_VALID, NRPHY_PUCCH_STATUS_INVALID);return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()
    P, R = abi.PucchCfg, abi.PucchResult
    assert [int(x) for x in out] == [C.sizeof(P), P.slot_index.offset, P.second_hop_prb.offset, P.nof_symbols.offset,
                                     P.time_domain_occ.offset, P.n_id.offset, P.sr_opportunity.offset, P.rx_ports.offset, C.sizeof(R),
                                     R.harq_ack.offset, R.detection_metric.offset, R.time_alignment_s.offset, R.cfo_hz.offset,
                                     abi.PUCCH_FORMAT_0, abi.PUCCH_FORMAT_1, abi.PUCCH_NO_HOP, abi.PUCCH_STATUS_UNKNOWN,
                                     abi.PUCCH_STATUS_VALID, abi.PUCCH_STATUS_INVALID]
    assert C.sizeof(R) == RESULT_DTYPE.itemsize and C.sizeof(abi.PuschChestMeas) == MEAS_DTYPE.itemsize
    assert (abi.PUCCH_STATUS_UNKNOWN, abi.PUCCH_STATUS_VALID, abi.PUCCH_STATUS_INVALID) == (model.UNKNOWN, model.VALID, model.INVALID)
    missing = [s for s in abi.ABI_SYMBOLS if "pucch" in s and not hasattr(lib.load(), s)]
    assert not missing and sum("pucch" in s for s in abi.ABI_SYMBOLS) == 5


def _f0(**kw):
    args = dict(format=0, starting_prb=5, nof_symbols=2, start_symbol=12, bwp_size_rb=51, bwp_start_rb=1, slot_index=3,
                initial_cyclic_shift=4, n_id=500, nof_harq_ack=1, sr_opportunity=True, rx_ports=(0, 1))
    args.update(kw)
    return abi.make_pucch(**args)


def _f1(**kw):
    args = dict(format=1, starting_prb=5, nof_symbols=14, start_symbol=0, bwp_size_rb=51, bwp_start_rb=1, slot_index=3,
                initial_cyclic_shift=4, time_domain_occ=2, n_id=500, nof_harq_ack=2, rx_ports=(0, 1, 2, 3))
    args.update(kw)
    return abi.make_pucch(**args)


@pytest.mark.parametrize("name,cfg,want", [
    ("format 0", _f0(), abi.OK),
    ("format 0, one symbol, last of the slot", _f0(nof_symbols=1, start_symbol=13), abi.OK),
    ("format 0, hopping", _f0(second_hop_prb=50), abi.OK),
    ("format 0, SR only", _f0(nof_harq_ack=0), abi.OK),
    ("format 0, two bits without SR", _f0(nof_harq_ack=2, sr_opportunity=False), abi.OK),
    ("format 1", _f1(), abi.OK),
    ("format 1, hopping, last PRB of the BWP", _f1(second_hop_prb=50), abi.OK),
    ("format 1, SR only", _f1(nof_harq_ack=0), abi.OK),
    ("format 1, 4 symbols from symbol 10", _f1(nof_symbols=4, start_symbol=10, time_domain_occ=1), abi.OK),
    ("format 1, OCC 6 of 7", _f1(time_domain_occ=6), abi.OK),
    ("format 1, numerology 1, slot 19", _f1(numerology=1, slot_index=19), abi.OK),
    ("ports in another order", _f1(rx_ports=(3, 1, 0, 2)), abi.OK),
    ("unknown format", _f1(format=2), abi.ERR_ARGUMENT),
    ("BWP beyond the grid", _f1(bwp_size_rb=52), abi.ERR_ARGUMENT),
    ("BWP start beyond the grid", _f1(bwp_start_rb=60, bwp_size_rb=1, starting_prb=0), abi.ERR_ARGUMENT),
    ("PRB outside the BWP", _f1(starting_prb=51), abi.ERR_ARGUMENT),
    ("second hop outside the BWP", _f1(second_hop_prb=51), abi.ERR_ARGUMENT),
    ("format 0, PRB outside the BWP", _f0(starting_prb=51), abi.ERR_ARGUMENT),
    ("format 0, second hop outside the BWP", _f0(second_hop_prb=51), abi.ERR_ARGUMENT),
    ("format 0, symbols beyond the slot", _f0(start_symbol=13), abi.ERR_ARGUMENT),
    ("format 0, no symbol", _f0(nof_symbols=0), abi.ERR_ARGUMENT),
    ("format 0, three symbols", _f0(nof_symbols=3, start_symbol=0), abi.ERR_ARGUMENT),
    ("format 0, no payload", _f0(nof_harq_ack=0, sr_opportunity=False), abi.ERR_ARGUMENT),
    ("format 0, three ACK bits", _f0(nof_harq_ack=3), abi.ERR_ARGUMENT),
    ("format 0, cyclic shift 12", _f0(initial_cyclic_shift=12), abi.ERR_ARGUMENT),
    ("format 0, n_id 1024", _f0(n_id=1024), abi.ERR_ARGUMENT),
    ("format 0 with an OCC", _f0(time_domain_occ=1), abi.ERR_ARGUMENT),
    ("format 0, sr_opportunity 2", _f0(sr_opportunity=2), abi.ERR_ARGUMENT),
    ("format 1, start symbol 11", _f1(nof_symbols=3, start_symbol=11, time_domain_occ=0), abi.ERR_ARGUMENT),
    ("format 1, three symbols", _f1(nof_symbols=3, time_domain_occ=0), abi.ERR_ARGUMENT),
    ("format 1, symbols beyond the slot", _f1(start_symbol=1), abi.ERR_ARGUMENT),
    ("format 1, 15 symbols", _f1(nof_symbols=15), abi.ERR_ARGUMENT),
    ("format 1, OCC 7", _f1(time_domain_occ=7), abi.ERR_ARGUMENT),
    ("format 1, OCC 3 of 3 with hopping", _f1(second_hop_prb=9, time_domain_occ=3), abi.ERR_ARGUMENT),
    ("format 1, OCC 2 of 3 with hopping", _f1(second_hop_prb=9, time_domain_occ=2), abi.OK),
    ("format 1, OCC 2 of 2", _f1(nof_symbols=4, time_domain_occ=2), abi.ERR_ARGUMENT),
    ("format 1, OCC 1 of 1 with hopping", _f1(nof_symbols=5, second_hop_prb=9, time_domain_occ=1), abi.ERR_ARGUMENT),
    ("format 1, n_id 1024", _f1(n_id=1024), abi.ERR_ARGUMENT),
    ("format 1, three ACK bits", _f1(nof_harq_ack=3), abi.ERR_ARGUMENT),
    ("format 1, cyclic shift 12", _f1(initial_cyclic_shift=12), abi.ERR_ARGUMENT),
    ("format 1 with an SR opportunity", _f1(sr_opportunity=True), abi.ERR_ARGUMENT),
    ("no port", _f1(rx_ports=()), abi.ERR_ARGUMENT),
    ("port outside the grid", _f1(rx_ports=(0, 4)), abi.ERR_ARGUMENT),
    ("repeated port", _f1(rx_ports=(0, 1, 1)), abi.ERR_ARGUMENT),
    ("numerology 5", _f1(numerology=5), abi.ERR_ARGUMENT),
    ("slot beyond the frame", _f1(slot_index=10), abi.ERR_ARGUMENT),
])
def test_pucch_validator(name, cfg, want):
    assert lib.pucch_validate(cfg, NOF_PORTS, NOF_SUBC) == want, name


def test_pucch_validator_refuses_five_ports():
    cfg = _f1()
    cfg.nof_rx_ports = 5
    assert lib.pucch_validate(cfg, 8, NOF_SUBC) == abi.ERR_ARGUMENT
    assert lib.load().nrphy_pucch_validate(None, NOF_PORTS, NOF_SUBC) == abi.ERR_ARGUMENT


def test_pucch_validator_over_the_reference_configurations():
    fx = fixtures()
    assert (len(fx), sum(f["format"] == 0 for f in fx), len({f["case"] for f in fx if f["format"] == 1})) == (186, 90, 48)
    for f in fx:
        assert lib.pucch_validate(to_abi(model.from_fixture(f)), NOF_PORTS, NOF_SUBC) == abi.OK, f
        assert lib.pucch_validate(to_abi(model.from_fixture(f)), NOF_PORTS, 12 * 51) == abi.ERR_ARGUMENT, f  # the BWP ends at PRB 52


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_extractor_reproduces_the_committed_fixtures():
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([os.environ.get("PYTHON", "python3"), os.path.join(GOLDEN, "extract_pucch_configs.py"), REFERENCE, d], check=True,
                       timeout=120)
        for name in ("pucch_configs.json", "pucch_tables.json"):
            assert open(os.path.join(d, name)).read() == open(os.path.join(GOLDEN, name)).read(), name


def test_generator_script_reproduces_the_tables():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "pucch_tables.inc")
        subprocess.run([os.environ.get("PYTHON", "python3"), os.path.join(backends.ROOT, "profiles", "gen_pucch_tables.py"), out],
                       check=True, timeout=120)
        assert open(out).read() == open(os.path.join(backends.ROOT, "srsran-edgeric-5g_amd", "csrc", "pucch_tables.inc")).read()


def test_restatement_sequences_equal_their_definitions(oracle):
    """Bounds from the number format.  The phase of a table entry, float(2 pi) float(k) / float(size), carries three roundings at a
    magnitude below 2 pi (ulp 4.8e-7): 7.2e-7; two tables and their product (three more roundings below 1): 2e-6.  The cover
    code's phase TWOPI phi / N passes through TWOPI phi < 64 (ulp 3.8e-6): half an ulp, TWOPI's own error times 6 and the division:
    4e-6."""
    worst = 0.0
    for u in range(30):
        for alpha in range(12):
            re, im = model.low_papr(u, alpha)
            assert re.dtype == np.float32
            z = re.astype(np.float64) + 1j * im.astype(np.float64)
            worst = max(worst, float(np.abs(np.abs(z) - 1).max()), float(np.abs(z - model.low_papr_by_definition(u, alpha)).max()))
            r64 = model.low_papr(u, alpha, np.float64)
            assert np.abs(r64[0] + 1j * r64[1] - model.low_papr_by_definition(u, alpha)).max() < 1e-13  # the definition's phase reaches 66 rad: ulp 1.4e-14
    print("low-PAPR sequences: worst distance from the definition %.3g" % worst)
    assert worst < 2e-6
    # Orthogonality of the cover codes, and of the cyclic shifts of one base sequence.
    for n in range(1, 8):
        w = np.array([model.occ(n, i, np.float64)[0] + 1j * model.occ(n, i, np.float64)[1] for i in range(n)])
        assert np.abs(w @ w.conj().T - n * np.eye(n)).max() < 1e-12, n
        w32 = np.array([model.occ(n, i)[0].astype(np.float64) + 1j * model.occ(n, i)[1] for i in range(n)])
        assert np.abs(w32 - w).max() < 4e-6, n
    r = np.array([model.low_papr_by_definition(7, a) for a in range(12)])
    assert np.abs(r @ r.conj().T - 12 * np.eye(12)).max() < 1e-12
    # The cyclic shift index against the C oracle's pseudo-random generator, read the way pucch_helper reads it: byte 14 n_slot + l
    # of the packed sequence, bit-reversed.
    for n_id, slot, m0 in ((0, 0, 0), (821, 9, 7), (1023, 159, 11), (500, 19, 4)):
        packed = oracle.prg_xor(n_id, 0, np.zeros(14 * (slot + 1), np.uint8), 8 * 14 * (slot + 1))
        for l in range(14):
            byte = int(packed[14 * slot + l])
            n_cs = int("{:08b}".format(byte)[::-1], 2)
            cfg = model.make_cfg(1, 0, 14, slot_index=slot, n_id=n_id, initial_cyclic_shift=m0)
            assert model.alpha_index(cfg, l, 3) == (m0 + 3 + n_cs) % 12, (n_id, slot, l)


def known_answer_slots():
    """Every fixture configuration on a grid built from its bits, without noise: a gain and a phase per port and a delay of three
    samples of a 4096-point transform (a flat channel would leave format 0 nothing to estimate its noise from).  Format 1's
    entries come in pairs that share a PRB: both go into one grid."""
    slots = []
    by_case = {}
    for f in fixtures():
        if f["format"] == 0:
            slots.append([f])
        else:
            by_case.setdefault(f["case"], []).append(f)
    slots += list(by_case.values())
    out = []
    for entries in slots:
        grid = np.zeros((NOF_PORTS, 14, NOF_SUBC), complex)
        cfgs = []
        for k, f in enumerate(entries):
            cfg = model.from_fixture(f)
            gains = [(0.8 + 0.1 * k) * np.exp(1j * (0.3 + 1.1 * p + k)) for p in range(NOF_PORTS)]
            model.add_to_grid(grid, model.transmit(cfg, f["ack_bits"], f.get("sr")), gains, delay=3.0, numerology=cfg["numerology"])
            cfgs.append((cfg, f))
        out.append((model.quantize(grid), cfgs))
    return out


def test_restatement_loop_back_over_the_reference_configurations():
    count = 0
    for grid, cfgs in known_answer_slots():
        for cfg, f in cfgs:
            for dt in (np.float32, np.float64):
                r = model.process(cfg, grid, dt)
                assert r["status"] == model.VALID and r["harq_ack"] == f["ack_bits"], (f, dt)
                assert f.get("sr") is None or r["sr"] == f["sr"], (f, dt)
            count += 1
    assert count == 186


# =======================================================================================================================
# GPU
# =======================================================================================================================
def guarded(words, fill=SENTINEL):
    """A device buffer of `words` 32-bit words between two guards of sentinel words: (whole tensor, the view to hand over)."""
    import torch
    whole = torch.full((words + 2 * GUARD,), int(np.uint32(SENTINEL).view(np.int32)), dtype=torch.int32, device="cuda")
    if fill != SENTINEL:
        whole[GUARD:GUARD + words] = int(np.uint32(fill).view(np.int32))
    return whole, whole[GUARD:GUARD + words]


def guards_intact(whole):
    a = whole.cpu().numpy().view(np.uint32)
    return bool((a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all())


CE_STRIDE = NOF_PORTS * 14 * NOF_SUBC


def run_plan(ctx, cfgs, grid_indices, grids, with_ce=True, with_meas=True, stream=None, plan=None, outputs=None):
    """nrphy_pucch_run on a plan of cfgs over grids [n_grids][ports][14][subc] (words, or a device tensor); returns (results [n],
    meas [n][4] or None, ce [n][4][14][subc] words or None: sentinel words where nothing was written) after checking the guards
    around every output."""
    own = plan is None
    n = len(cfgs)
    n_grids = len(grids) if not hasattr(grids, "data_ptr") else grids.shape[0]
    if own:
        plan = lib.PucchPlan(ctx, [to_abi(c) for c in cfgs], grid_indices, n_grids, NOF_PORTS, NOF_SUBC,
                             [i * CE_STRIDE for i in range(n)] if with_ce else None)
    d_grid = dev(as_i32(np.asarray(grids))) if not hasattr(grids, "data_ptr") else grids
    if outputs is None:
        outputs = (guarded(n * RESULT_DTYPE.itemsize // 4), guarded(n * NOF_PORTS * MEAS_DTYPE.itemsize // 4) if with_meas else (None, None),
                   guarded(n * CE_STRIDE) if with_ce else (None, None))
    (res_w, res), (meas_w, meas), (ce_w, ce) = outputs
    plan.run(d_grid, res, meas, ce, stream=stream)
    ctx.synchronize()
    assert guards_intact(res_w) and (meas_w is None or guards_intact(meas_w)) and (ce_w is None or guards_intact(ce_w))
    out = (res.cpu().numpy().view(RESULT_DTYPE).copy(),
           meas.cpu().numpy().view(MEAS_DTYPE).reshape(n, NOF_PORTS).copy() if with_meas else None,
           ce.cpu().numpy().view(np.uint32).reshape(n, NOF_PORTS, 14, NOF_SUBC).copy() if with_ce else None)
    if own:
        plan.close()
    return out


def flatten(slots):
    """Slots of (grid, [(cfg, extra), ...]) -> (cfgs, grid index per cfg, grids, extras)."""
    cfgs, index, extras = [], [], []
    for g, (_, entries) in enumerate(slots):
        for cfg, extra in entries:
            cfgs.append(cfg)
            index.append(g)
            extras.append(extra)
    return cfgs, index, np.stack([grid for grid, _ in slots]), extras


@pytest.mark.gpu
def test_reference_configurations_return_their_bits(gpu_ctx):
    cfgs, index, grids, fx = flatten(known_answer_slots())
    assert len(cfgs) == 186
    res, _, _ = run_plan(gpu_ctx, cfgs, index, grids, with_ce=False, with_meas=False)
    for i, f in enumerate(fx):
        assert res[i]["status"] == abi.PUCCH_STATUS_VALID, (i, f, res[i])
        assert list(res[i]["harq_ack"][:f["nof_harq_ack"]]) == f["ack_bits"], (i, f, res[i])
        assert f.get("sr") is None or res[i]["sr"] == f["sr"], (i, f, res[i])
        assert res[i]["time_alignment_s"] == 0


def _channel(grid, res, rng, nof_ports, snr_db, numerology, cfo, fading=True):
    """One UE through a two-tap channel per port at `snr_db` per resource element and port (noise is added by the caller).  The
    first tap is Rayleigh, held above half its mean amplitude, or with fading off of that amplitude and a random phase."""
    amp = 10 ** (snr_db / 20)
    d0 = float(rng.uniform(0, 8))
    g0 = amp * (rng.standard_normal(nof_ports) + 1j * rng.standard_normal(nof_ports)) / np.sqrt(2)
    g0 = np.where(np.abs(g0) < 0.5 * amp, amp * np.exp(1j * np.angle(g0)) * 0.5, g0)  # no port in a deep fade
    if not fading:
        g0 = amp * np.exp(1j * np.angle(g0))
    g1 = 0.3 * amp * (rng.standard_normal(nof_ports) + 1j * rng.standard_normal(nof_ports)) / np.sqrt(2)
    model.add_to_grid(grid, res, g0, delay=d0, cfo=cfo, numerology=numerology)
    model.add_to_grid(grid, res, g1, delay=d0 + float(rng.uniform(5, 30)), cfo=cfo, numerology=numerology)


def _random_bits(rng, n):
    return [int(b) for b in rng.integers(0, 2, n)]


def parity_slots():
    """Seeded slots over both formats, 1 / 2 / 4 ports, with and without hopping, every symbol count, 0 / 1 / 2 ACK bits, with and
    without an SR opportunity; every third format 1 slot carries a second UE on the same PRBs (another cyclic shift).  Unit-variance
    noise on every port; the UEs arrive through two taps with a CFO of up to 1 % of the spacing."""
    rng = np.random.default_rng(20240611)
    slots = []
    k = 0
    for ns in range(4, 15):
        for hop in (False, True):
            for ports in ((2,), (1, 3), (3, 0, 2, 1)):
                for nack in (0, 1, 2):
                    numerology = int(rng.integers(0, 2))
                    start = int(rng.integers(0, min(10, 14 - ns) + 1))
                    limit = ns // 4 if hop else ns // 2
                    prb, prb2 = (int(x) for x in rng.choice(50, 2, replace=False))
                    base = dict(format=1, starting_prb=prb, nof_symbols=ns, start_symbol_index=start, second_hop_prb=prb2 if hop else None,
                                bwp_start_rb=1, bwp_size_rb=51, numerology=numerology, slot_index=int(rng.integers(0, 10 << numerology)),
                                time_domain_occ=int(rng.integers(0, limit)), n_id=int(rng.integers(0, 1024)), ports=ports)
                    shifts = [int(x) for x in rng.choice(12, 2, replace=False)]
                    grid = np.zeros((NOF_PORTS, 14, NOF_SUBC), complex)
                    entries = []
                    for ue in range(2 if k % 3 == 2 else 1):
                        cfg = make_cfg(**dict(base, initial_cyclic_shift=shifts[ue], nof_harq_ack=nack if ue == 0 else (nack + 1) % 3))
                        bits = _random_bits(rng, cfg["nof_harq_ack"])
                        full = np.zeros_like(grid)
                        # Detection gains 12 x data symbols x ports over the SNR of a resource element; no tap fades below a quarter
                        # of its power.  A metric of 40 or more in the mean keeps every case clear of [T / 2, 2 T].
                        # Two UEs on one PRB see each other as noise (the `mean` estimator does not separate cyclic shifts through a
                        # dispersive channel): they get like powers, 8 dB up, and do not fade.
                        floor_db = 10 * np.log10(160.0 / (12 * (ns // 2) * len(ports)))
                        snr_db = floor_db + (8 + float(rng.uniform(0, 3)) if k % 3 == 2 else float(rng.uniform(0, 8)))
                        _channel(full, model.transmit(cfg, bits), rng, NOF_PORTS, snr_db, numerology,
                                 float(rng.uniform(-0.01, 0.01)), fading=k % 3 != 2)
                        grid += full
                        entries.append((cfg, bits))
                    grid += (rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape)) / np.sqrt(2)
                    slots.append((model.quantize(grid), entries))
                    k += 1
    for rep in range(2):
        for ns, hop in ((1, False), (2, False), (2, True)):
            for ports in ((1,), (0, 2), (0, 1, 2, 3)):
                for nack, sr_opp in ((0, True), (1, False), (1, True), (2, False), (2, True)):
                    numerology = int(rng.integers(0, 2))
                    prb, prb2 = (int(x) for x in rng.choice(50, 2, replace=False))
                    cfg = make_cfg(format=0, starting_prb=prb, nof_symbols=ns, start_symbol_index=int(rng.integers(0, 15 - ns)),
                                         second_hop_prb=prb2 if hop else None, bwp_start_rb=1, bwp_size_rb=51, numerology=numerology,
                                         slot_index=int(rng.integers(0, 10 << numerology)), initial_cyclic_shift=int(rng.integers(0, 12)),
                                         n_id=int(rng.integers(0, 1024)), nof_harq_ack=nack, sr_opportunity=sr_opp, ports=ports)
                    bits = _random_bits(rng, nack)
                    sr = int(rng.integers(0, 2)) if sr_opp and nack else (1 if sr_opp else None)
                    grid = np.zeros((NOF_PORTS, 14, NOF_SUBC), complex)
                    # Format 0's metric is about (symbols x ports) x SNR: no coherent gain over the 12 subcarriers.
                    floor_db = 10 * np.log10(64.0 / (ns * len(ports)))
                    _channel(grid, model.transmit(cfg, bits, sr), rng, NOF_PORTS, floor_db + float(rng.uniform(0, 6)), numerology, 0.0)
                    grid += (rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape)) / np.sqrt(2)
                    slots.append((model.quantize(grid), [(cfg, (bits, sr))]))
    return slots


def rel(a, b, floor):
    if np.isnan(a) and np.isnan(b):
        return 0.0
    if np.isinf(b):
        return 0.0 if a == b else np.inf
    return abs(float(a) - float(b)) / max(abs(float(b)), floor)


FIELDS = (("metric", FLOOR), ("sinr_dB", DB_FLOOR), ("rsrp_dB", DB_FLOOR), ("epre_dB", DB_FLOOR))
MEAS_FIELDS = ("noise_var", "rsrp", "epre", "snr")


def distance(got, got_meas, want):
    """(largest relative distance of the metric, the dB values and the measurements; of the CFO) between a result and a
    restatement's."""
    d = max(rel(got[name], want[name], floor) for name, floor in FIELDS)
    c = rel(got["cfo_hz"], want["cfo_hz"], CFO_FLOOR_HZ)
    if want["meas"] is not None:
        for m_got, m_want in zip(got_meas, want["meas"]):
            d = max(d, max(rel(m_got[name], m_want[name], FLOOR) for name in MEAS_FIELDS))
            c = max(c, rel(m_got["cfo_hz"], m_want["cfo_hz"], CFO_FLOOR_HZ))
    return d, c


def assert_not_marginal(cfg, r64, tol, what):
    """The decision must not hang on the last bits: the float64 restatement's metric outside [T / 2, 2 T], the two detect_bits
    statistics of a two-bit format 1 apart, format 0's best candidate ahead of the runner-up."""
    T = model.THRESHOLD
    assert not (T / 2 <= r64["raw_metric"] <= 2 * T), (what, r64["raw_metric"])
    if cfg["format"] == 1 and cfg["nof_harq_ack"] == 2:
        m1, m2 = r64["statistics"]
        assert abs(m1 - m2) > tol * max(m1, m2, FLOOR), (what, m1, m2)
    if cfg["format"] == 0 and len(r64["candidates"]) > 1:
        top = sorted(r64["candidates"])[-2:]
        assert top[1] - top[0] > tol * max(top[1], FLOOR), (what, top)


def model_spread(slots):
    """The two restatements on every case: (metric spread, CFO spread, [(cfg, r32, r64)])."""
    spread = cfo_spread = 0.0
    rows = []
    for grid, entries in slots:
        for cfg, _ in entries:
            r32, r64 = model.process(cfg, grid, np.float32), model.process(cfg, grid, np.float64)
            got = dict(r32, metric=r32["metric"])
            d, c = distance(got, r32["meas"] or [], r64)
            spread, cfo_spread = max(spread, d), max(cfo_spread, c)
            rows.append((cfg, r32, r64))
    return spread, cfo_spread, rows


def bf16_key(words):
    """The two bf16 halves of cbf16 words as integers whose difference counts ulps."""
    w = np.asarray(words, np.uint32)
    out = []
    for half in (w & 0xFFFF, w >> 16):
        h = half.astype(np.int64)
        out.append(np.where(h & 0x8000, -(h & 0x7FFF), h))
    return out


@pytest.mark.gpu
def test_parity_with_the_restatement(gpu_ctx):
    slots = parity_slots()
    cfgs, index, grids, extras = flatten(slots)
    spread, cfo_spread, rows = model_spread(slots)
    tol, cfo_tol = 8 * MODEL_SPREAD, 8 * CFO_SPREAD
    assert len(cfgs) == len(rows) >= 350
    for i, (cfg, r32, r64) in enumerate(rows):
        assert_not_marginal(cfg, r64, tol, (i, cfg))
    worst = worst_cfo = 0.0
    ulps = 0
    for first in range(0, len(cfgs), 64):  # batches of mixed formats
        sl = slice(first, first + 64)
        used = sorted(set(index[sl]))
        res, meas, ce = run_plan(gpu_ctx, cfgs[sl], [used.index(g) for g in index[sl]], grids[used])
        for j, (cfg, r32, r64) in enumerate(rows[sl]):
            what = (first + j, cfg)
            got = res[j]
            assert got["status"] == r32["status"] and list(got["harq_ack"][:cfg["nof_harq_ack"]]) == r32["harq_ack"], (what, got, r32)
            assert got["sr"] == r32["sr"] and not got["harq_ack"][cfg["nof_harq_ack"]:].any(), (what, got, r32)
            d, c = distance(dict(metric=got["detection_metric"], sinr_dB=got["sinr_dB"], rsrp_dB=got["rsrp_dB"], epre_dB=got["epre_dB"],
                                 cfo_hz=got["cfo_hz"]), meas[j], r64)
            worst, worst_cfo = max(worst, d), max(worst_cfo, c)
            assert d <= tol and c <= cfo_tol, (what, d, c, got, r64)
            assert got["time_alignment_s"] == 0
            if cfg["format"] == 1:
                region = r32["region"]
                full = np.zeros((NOF_PORTS, 14, NOF_SUBC), bool)
                full[:len(cfg["ports"])] = region
                assert (ce[j][~full] == SENTINEL).all(), what
                for a, b in zip(bf16_key(ce[j][:len(cfg["ports"])][region]), bf16_key(r32["ce"][region])):
                    ulps = max(ulps, int(np.abs(a - b).max()))
                assert ulps <= 1, what
                assert not meas[j][len(cfg["ports"]):].tobytes().strip(b"\0"), what
            else:
                assert (ce[j] == SENTINEL).all() and not meas[j].tobytes().strip(b"\0"), what
    print("float32 - float64 restatement spread %.3g (constant %.3g), CFO %.3g (constant %.3g); device - float64 worst %.3g (allowed "
          "%.3g), CFO %.3g (allowed %.3g); estimate within %d bf16 ulp; %d PUCCHs" %
          (spread, MODEL_SPREAD, cfo_spread, CFO_SPREAD, worst, tol, worst_cfo, cfo_tol, ulps, len(cfgs)))
    assert spread <= MODEL_SPREAD * 1.0001 and cfo_spread <= CFO_SPREAD * 1.0001, "the constants no longer describe the cases"


@pytest.mark.gpu
def test_zero_grid_is_invalid(gpu_ctx):
    grid = np.zeros((NOF_PORTS, 14, NOF_SUBC), np.uint32)
    for cfg in (make_cfg(0, 3, 2, 5, nof_harq_ack=2, sr_opportunity=True, ports=(0, 1)),
                make_cfg(1, 3, 14, 0, second_hop_prb=20, nof_harq_ack=2, ports=(0, 1, 2, 3)),
                make_cfg(1, 3, 7, 2, nof_harq_ack=0, ports=(1,))):
        r, meas, _ = gpu_ctx.pucch_host(to_abi(cfg), grid)
        want = model.process(cfg, grid, np.float32)
        assert want["status"] == model.INVALID and float(want["metric"]) == 0
        # The bits are what the reference leaves behind (detect_bits reads a zero statistic as "not positive": ones), never NaN.
        assert r.status == abi.PUCCH_STATUS_INVALID and r.detection_metric == 0 and r.sr == 0, cfg
        assert list(r.harq_ack) == (want["harq_ack"] + [0, 0])[:2] and all(b in (0, 1) for b in r.harq_ack), cfg
        assert r.epre_dB == -np.inf and r.time_alignment_s == 0


@pytest.mark.gpu
def test_noise_only_grids_agree_with_the_restatement(gpu_ctx):
    """400 seeded PUCCHs on noise alone.  The share declared valid is the algorithm's false alarm rate and is reported; what is
    asserted is that the device declares exactly the PUCCHs the float32 restatement declares."""
    rng = np.random.default_rng(77)
    slots = []
    for k in range(400):
        ports = [(0,), (1, 2), (0, 1, 2, 3)][k % 3]
        if k % 2:
            ns = int(rng.integers(4, 15))
            hop = bool(rng.integers(0, 2))
            cfg = make_cfg(1, int(rng.integers(0, 52)), ns, int(rng.integers(0, min(10, 14 - ns) + 1)),
                                 second_hop_prb=int(rng.integers(0, 52)) if hop else None, bwp_size_rb=52, n_id=int(rng.integers(0, 1024)),
                                 slot_index=int(rng.integers(0, 10)), initial_cyclic_shift=int(rng.integers(0, 12)),
                                 nof_harq_ack=int(rng.integers(0, 3)), ports=ports)
        else:
            nack = int(rng.integers(0, 3))
            cfg = make_cfg(0, int(rng.integers(0, 52)), int(rng.integers(1, 3)), int(rng.integers(0, 13)), bwp_size_rb=52,
                                 n_id=int(rng.integers(0, 1024)), slot_index=int(rng.integers(0, 10)),
                                 initial_cyclic_shift=int(rng.integers(0, 12)), nof_harq_ack=nack,
                                 sr_opportunity=bool(rng.integers(0, 2)) or nack == 0, ports=ports)
        sigma = float(rng.uniform(0.1, 10.0))
        grid = sigma * (rng.standard_normal((NOF_PORTS, 14, NOF_SUBC)) + 1j * rng.standard_normal((NOF_PORTS, 14, NOF_SUBC)))
        slots.append((model.quantize(grid), [(cfg, None)]))
    cfgs, index, grids, _ = flatten(slots)
    res, _, _ = run_plan(gpu_ctx, cfgs, index, grids, with_ce=False, with_meas=False)
    want = [model.process(cfg, slots[i][0], np.float32)["status"] for i, cfg in enumerate(cfgs)]
    got = [int(s) for s in res["status"]]
    for fmt in (0, 1):
        sel = [i for i, c in enumerate(cfgs) if c["format"] == fmt]
        print("format %d: %d of %d noise-only PUCCHs declared valid (restatement: %d)" %
              (fmt, sum(got[i] == abi.PUCCH_STATUS_VALID for i in sel), len(sel), sum(want[i] == model.VALID for i in sel)))
    assert got == want


@pytest.mark.gpu
def test_format1_measures_gain_and_cfo_back(gpu_ctx):
    """A flat gain of 0.5 on two ports, no noise.  bf16 keeps 8 significant bits: a component of the grid is within 2^-8 of its
    value, a power within 2^-7 (0.034 dB), so RSRP and EPRE are 20 log10(0.5) = -6.02 dB within 0.05 dB.  A CFO of 0.5 % of a 15 kHz
    spacing (75 Hz) between DM-RS symbols 2.14 symbols apart: every sample's phase is within 2^-8 rad of the one sent, the phase
    between the two symbols within 2^-7 rad whatever the averaging does, which is 2^-7 / (2 pi 2.14) x 15 kHz = 8.7 Hz; bound 9 Hz."""
    cfg = make_cfg(1, 7, 14, 0, n_id=77, slot_index=4, initial_cyclic_shift=5, time_domain_occ=3, nof_harq_ack=2, ports=(0, 1))
    for cfo in (0.0, 0.005, -0.005):
        grid = np.zeros((NOF_PORTS, 14, NOF_SUBC), complex)
        model.add_to_grid(grid, model.transmit(cfg, [1, 0]), [0.5, 0.5j], cfo=cfo)
        r, meas, _ = gpu_ctx.pucch_host(to_abi(cfg), model.quantize(grid))
        assert r.status == abi.PUCCH_STATUS_VALID and list(r.harq_ack) == [1, 0]
        assert abs(r.cfo_hz - cfo * 15000) < 9.0, (cfo, r.cfo_hz)
        assert abs(r.epre_dB - 20 * np.log10(0.5)) < 0.05, r.epre_dB
        if cfo == 0.0:
            assert abs(r.rsrp_dB - 20 * np.log10(0.5)) < 0.05, r.rsrp_dB
            assert all(abs(m.rsrp - 0.25) < 0.25 * 0.012 for m in meas)  # 2^-7 and the estimate's own rounding


@pytest.mark.gpu
def test_wrong_cyclic_shift_or_cover_code_is_invalid(gpu_ctx):
    rng = np.random.default_rng(5)
    cfg = make_cfg(1, 9, 14, 0, n_id=301, slot_index=2, initial_cyclic_shift=3, time_domain_occ=1, nof_harq_ack=1, ports=(0, 1))
    grid = np.zeros((NOF_PORTS, 14, NOF_SUBC), complex)
    model.add_to_grid(grid, model.transmit(cfg, [1]), [1.0, 1.0j])
    grid += 0.05 * (rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape))
    words = model.quantize(grid)
    assert gpu_ctx.pucch_host(to_abi(cfg), words)[0].status == abi.PUCCH_STATUS_VALID
    for other in (dict(cfg, initial_cyclic_shift=4), dict(cfg, initial_cyclic_shift=9), dict(cfg, time_domain_occ=0),
                  dict(cfg, time_domain_occ=5)):
        r = gpu_ctx.pucch_host(to_abi(other), words)[0]
        assert r.status == abi.PUCCH_STATUS_INVALID, (other, r.detection_metric)
    f0 = make_cfg(0, 9, 2, 12, n_id=301, slot_index=2, initial_cyclic_shift=3, nof_harq_ack=1, ports=(0, 1))
    grid = np.zeros((NOF_PORTS, 14, NOF_SUBC), complex)
    model.add_to_grid(grid, model.transmit(f0, [1]), [1.0, 1.0j])
    grid += 0.05 * (rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape))
    words = model.quantize(grid)
    r = gpu_ctx.pucch_host(to_abi(f0), words)[0]
    assert r.status == abi.PUCCH_STATUS_VALID and r.harq_ack[0] == 1
    assert gpu_ctx.pucch_host(to_abi(dict(f0, initial_cyclic_shift=4)), words)[0].status == abi.PUCCH_STATUS_INVALID


def mixed_batch():
    slots = parity_slots()
    picks = [0, 17, 40, 75, 110, 150, 197, 200, 214, 230, 260, 287]
    return flatten([slots[i] for i in picks])


@pytest.mark.gpu
def test_mixed_batch_equals_per_pucch_host_calls(gpu_ctx):
    cfgs, index, grids, _ = mixed_batch()
    assert {c["format"] for c in cfgs} == {0, 1}
    res, meas, ce = run_plan(gpu_ctx, cfgs, index, grids)
    for i, cfg in enumerate(cfgs):
        n = len(cfg["ports"])
        r, m, e = gpu_ctx.pucch_host(to_abi(cfg), grids[index[i]], with_estimate=True,
                                     ch_est=np.full((n, 14, NOF_SUBC), SENTINEL, np.uint32))
        assert bytes(r) == res[i].tobytes(), (i, cfg)
        assert b"".join(bytes(x) for x in m) == meas[i][:n].tobytes(), (i, cfg)
        assert e.tobytes() == ce[i][:n].tobytes(), (i, cfg)


@pytest.mark.gpu
def test_graph_replay_and_two_runs_give_identical_bytes(gpu_ctx):
    import torch
    cfgs, index, grids, _ = mixed_batch()
    n = len(cfgs)
    plan = lib.PucchPlan(gpu_ctx, [to_abi(c) for c in cfgs], index, len(grids), NOF_PORTS, NOF_SUBC, [i * CE_STRIDE for i in range(n)])
    d_grid = dev(as_i32(grids))
    first = run_plan(gpu_ctx, cfgs, index, d_grid, plan=plan)
    second = run_plan(gpu_ctx, cfgs, index, d_grid, plan=plan)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    outputs = (guarded(n * RESULT_DTYPE.itemsize // 4), guarded(n * NOF_PORTS * MEAS_DTYPE.itemsize // 4), guarded(n * CE_STRIDE))
    (res_w, res), (meas_w, meas), (ce_w, ce) = outputs
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.run(d_grid, res, meas, ce, stream=C.c_void_p(stream.cuda_stream))
    for _ in range(2):
        res.zero_()
        meas.zero_()
        ce.fill_(int(np.uint32(SENTINEL).view(np.int32)))
        graph.replay()
        torch.cuda.synchronize()
        assert res.cpu().numpy().tobytes() == first[0].tobytes()
        assert meas.cpu().numpy().tobytes() == first[1].tobytes()
        assert ce.cpu().numpy().tobytes() == first[2].tobytes()
        assert guards_intact(res_w) and guards_intact(meas_w) and guards_intact(ce_w)
    plan.close()


@pytest.mark.gpu
def test_pusch_and_pucch_share_one_grid_buffer_and_stream(gpu_ctx):
    """A slot with a PUSCH on PRBs 10..29, a hopping format 1 PUCCH on PRBs 0 and 51 and a format 0 PUCCH on PRB 50: the PUSCH estimator's plan and the PUCCH plan read the
    same device grid on the same stream, and each gives what its host call gives on that grid."""
    import torch
    rng = np.random.default_rng(9)
    f1 = make_cfg(1, 0, 14, 0, second_hop_prb=51, bwp_size_rb=52, n_id=40, slot_index=6, initial_cyclic_shift=2, nof_harq_ack=2,
                        ports=(0, 1, 2, 3))
    f0 = make_cfg(0, 50, 2, 12, bwp_size_rb=52, n_id=40, slot_index=6, initial_cyclic_shift=7, nof_harq_ack=1, sr_opportunity=True,
                        ports=(0, 1, 2, 3))
    grid = 0.2 * (rng.standard_normal((NOF_PORTS, 14, NOF_SUBC)) + 1j * rng.standard_normal((NOF_PORTS, 14, NOF_SUBC)))
    model.add_to_grid(grid, model.transmit(f1, [0, 1]), [1.0, 0.8j, -0.9, 0.7 - 0.2j], delay=2.0)
    model.add_to_grid(grid, model.transmit(f0, [1], 1), [1.0, 0.8j, -0.9, 0.7 - 0.2j], delay=2.0)
    words = model.quantize(grid)
    pusch = abi.make_pusch_chest(prbs=range(10, 30), slot_index=6, scrambling_id=40, dmrs_symbols=(2, 11), rx_ports=(0, 1, 2, 3))
    d_grid = dev(as_i32(words[None]))
    chest = lib.PuschChestPlan(gpu_ctx, [pusch], [0], 1, NOF_PORTS, NOF_SUBC, [0])
    pucch = lib.PucchPlan(gpu_ctx, [to_abi(f1), to_abi(f0)], [0, 0], 1, NOF_PORTS, NOF_SUBC)
    ce_w, ce = guarded(CE_STRIDE, fill=0)
    nv_w, nv = guarded(NOF_PORTS)
    res_w, res = guarded(2 * RESULT_DTYPE.itemsize // 4)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    handle = C.c_void_p(stream.cuda_stream)
    chest.run(d_grid, ce, nv, stream=handle)
    pucch.run(d_grid, res, stream=handle)
    stream.synchronize()
    assert guards_intact(ce_w) and guards_intact(nv_w) and guards_intact(res_w)
    want_ce, want_nv, _ = gpu_ctx.pusch_chest_host(pusch, words)
    assert ce.cpu().numpy().view(np.uint32).tobytes() == want_ce.tobytes()
    assert nv.cpu().numpy().view(np.float32).tobytes() == want_nv.tobytes()
    got = res.cpu().numpy().view(RESULT_DTYPE)
    for i, (cfg, bits) in enumerate(((f1, [0, 1]), (f0, [1]))):
        assert got[i].tobytes() == bytes(gpu_ctx.pucch_host(to_abi(cfg), words)[0]), cfg
        assert got[i]["status"] == abi.PUCCH_STATUS_VALID and list(got[i]["harq_ack"][:len(bits)]) == bits, got[i]
    assert got[1]["sr"] == 1
    chest.close()
    pucch.close()


# =======================================================================================================================
# The recording of the reference (tests/golden/record_pucch_reference.cpp states every layout)
# =======================================================================================================================
def recorded_prb(cfg, off):
    """The grid PRB of the symbol at offset `off` of the allocation, as the recorder's header states the layout (not through the
    restatement, which is under test here)."""
    hop = cfg["second_hop_prb"] is not None and (off != 0 if cfg["format"] == 0 else off >= cfg["nof_symbols"] // 2)
    return cfg["bwp_start_rb"] + (cfg["second_hop_prb"] if hop else cfg["starting_prb"])


@functools.lru_cache(maxsize=None)
def recording():
    """The recorded cases: dicts of cfg, row (the case table's), grid (index into the second value), want (the reference's answer in
    the form distance() reads, with status, harq_ack, sr, time_alignment_s, ta [ports][3], estimate [ports][symbols] and top, the
    recorder's two margin numbers), flagged,
    sent; and the distinct grids [n_grids][4][14][624] rebuilt from the stored elements."""
    load = lambda name: np.load(os.path.join(GOLDEN, "pucch_reference_%s.npy" % name))
    rows, words, results, estimates = load("cases"), load("grids"), load("results"), load("estimates")
    cases, grids, grid_of = [], [], {}
    for row, r in zip(rows, results):
        row = [int(v) for v in row]
        P = row[14]
        cfg = model.make_cfg(format=row[0], numerology=row[1], slot_index=row[2], bwp_start_rb=row[3], bwp_size_rb=row[4], starting_prb=row[5],
                             second_hop_prb=None if row[6] < 0 else row[6], start_symbol_index=row[7], nof_symbols=row[8],
                             initial_cyclic_shift=row[9], time_domain_occ=row[10], n_id=row[11], nof_harq_ack=row[12],
                             sr_opportunity=row[13], ports=row[15:15 + P])
        ns, s0 = cfg["nof_symbols"], cfg["start_symbol_index"]
        if row[19] not in grid_of:
            stored = words[row[19]:row[19] + P * ns * 12].reshape(P, ns, 12)
            grid = np.zeros((NOF_PORTS, 14, NOF_SUBC), np.uint32)
            for off in range(ns):
                k = 12 * recorded_prb(cfg, off)
                grid[cfg["ports"], s0 + off, k:k + 12] = stored[:, off]
            grid_of[row[19]] = len(grids)
            grids.append(grid)
        per_port = r[10:42].reshape(4, 8)[:P]
        want = dict(status=int(r[0]), harq_ack=None if np.isnan(r[1]) else [int(b) for b in r[1:1 + cfg["nof_harq_ack"]]],
                    sr=None if np.isnan(r[3]) else int(r[3]), metric=r[4], sinr_dB=r[5], rsrp_dB=r[6], epre_dB=r[7], time_alignment_s=r[8],
                    cfo_hz=r[9], meas=None, ta=None, estimate=None, top=(r[42], r[43]))
        if cfg["format"] == 1:
            want["meas"] = [dict(noise_var=m[0], rsrp=m[1], epre=m[2], snr=m[3], cfo_hz=m[4]) for m in per_port]
            want["ta"] = per_port[:, 5:8]
            want["estimate"] = estimates[row[20]:row[20] + P * ns].reshape(P, ns)
        cases.append(dict(cfg=cfg, row=row, grid=grid_of[row[19]], want=want, flagged=bool(row[21]), sent=row[24] >= 0))
    return cases, np.stack(grids)


def recorded_distance(cfg, got, got_meas, want, what):
    """distance() against a recorded answer.  The reference's format 0 detector returns no metric (its SINR is 10 log10 of it).
    rel() and max() let a NaN on one side only pass unseen, so first: every compared field is NaN exactly where the recorded one
    is (a CFO where the reference has none, a measurement that is no number), as many measurements as ports, and what comes out
    is a number."""
    if cfg["format"] == 0:
        got = dict(got, metric=np.nan)
    pairs = [(name, got[name], want[name]) for name, _ in FIELDS] + [("cfo_hz", got["cfo_hz"], want["cfo_hz"])]
    assert want["meas"] is None or len(got_meas) == len(want["meas"]), (what, len(got_meas))  # format 0 has none
    for p, (m_got, m_want) in enumerate(zip(got_meas, want["meas"] or [])):
        pairs += [("%s of port %d" % (name, p), m_got[name], m_want[name]) for name in MEAS_FIELDS + ("cfo_hz",)]
    for name, a, b in pairs:
        assert bool(np.isnan(a)) == bool(np.isnan(b)), (what, name, a, b)
    d, c = distance(got, got_meas, want)
    assert np.isfinite(d) and np.isfinite(c), (what, d, c)
    return d, c


def same_exact_fields(cfg, got, want, what):
    """Status, bits and SR (where the reference wrote any: a zero grid leaves format 0's message unwritten) and the time alignment."""
    assert got["status"] == want["status"], (what, got, want)
    if want["harq_ack"] is not None:
        assert list(got["harq_ack"][:cfg["nof_harq_ack"]]) == want["harq_ack"] and got["sr"] == want["sr"], (what, got, want)
    assert got["time_alignment_s"] == want["time_alignment_s"], (what, got, want)


def same_special_values(cfg, got, got_meas, want, what):
    """Every recorded infinity, NaN and zero of a flagged case, exactly (format 0's metric is not recorded: recorded_distance)."""
    pairs = [(got[name], want[name]) for name, _ in FIELDS[cfg["format"] == 0:]] + [(got["cfo_hz"], want["cfo_hz"])]
    for m_got, m_want in zip(got_meas, want["meas"] or []):
        pairs += [(m_got[name], m_want[name]) for name in MEAS_FIELDS + ("cfo_hz",)]
    for a, b in pairs:
        if np.isnan(b):
            assert np.isnan(a), (what, a, b)
        elif np.isinf(b) or b == 0:
            assert a == b, (what, a, b)


def estimate_of(cfg, ce):
    """[ports][symbols] words of an estimate [ports][14][subc]: the first subcarrier of every symbol's PRB."""
    ns, s0 = cfg["nof_symbols"], cfg["start_symbol_index"]
    return np.array([[ce[p, s0 + off, 12 * recorded_prb(cfg, off)] for off in range(ns)] for p in range(len(cfg["ports"]))])


def estimate_steps(cfg, ce, want, what):
    """Largest distance in bf16 steps between an estimate [ports][14][subc] and the recorded one, which holds one value on the 12
    subcarriers of every symbol's PRB; the 12 must be equal in `ce` too."""
    ns, s0 = cfg["nof_symbols"], cfg["start_symbol_index"]
    for off in range(ns):
        k = 12 * recorded_prb(cfg, off)
        block = ce[:len(cfg["ports"]), s0 + off, k:k + 12]
        assert (block == block[:, :1]).all(), what
    return max(int(np.abs(a - b).max()) for a, b in zip(bf16_key(estimate_of(cfg, ce)), bf16_key(want["estimate"])))


def test_recording_is_consistent():
    cases, grids = recording()
    rows = np.load(os.path.join(GOLDEN, "pucch_reference_cases.npy"))
    words = np.load(os.path.join(GOLDEN, "pucch_reference_grids.npy"))
    results = np.load(os.path.join(GOLDEN, "pucch_reference_results.npy"))
    estimates = np.load(os.path.join(GOLDEN, "pucch_reference_estimates.npy"))
    assert rows.dtype == np.int32 and rows.shape == (NOF_RECORDED, 28) and results.dtype == np.float64 and results.shape == (NOF_RECORDED, 44)
    assert words.dtype == np.uint32 and words.ndim == 1 and estimates.dtype == np.uint32 and estimates.ndim == 1
    assert sum(os.path.getsize(os.path.join(GOLDEN, "pucch_reference_%s.npy" % n)) for n in ("cases", "grids", "results", "estimates")) < 400000
    # The first 186 are the reference's configurations, in the fixtures' order, with the fixtures' bits.
    fx = fixtures()
    for f, k in zip(fx, cases):
        assert k["cfg"] == model.from_fixture(f) and k["row"][22] == 0 and k["sent"], f
        assert k["row"][24] == sum(b << i for i, b in enumerate(f["ack_bits"])) and k["row"][25] == (-1 if f.get("sr") is None else f["sr"]), f
    assert [k["row"][22] for k in cases[len(fx):]] == sorted(k["row"][22] for k in cases[len(fx):]) and {k["row"][22] for k in cases} == {0, 1, 2, 3, 4}
    # Offsets: the grids and the estimates are stored back to back in the order of the cases; cases of one grid share its region.
    next_grid = next_estimate = 0
    regions = {}
    for i, k in enumerate(cases):
        cfg, row = k["cfg"], k["row"]
        assert lib.pucch_validate(to_abi(cfg), NOF_PORTS, NOF_SUBC) == abi.OK, (i, cfg)
        size = len(cfg["ports"]) * cfg["nof_symbols"] * 12
        region = (cfg["ports"], cfg["start_symbol_index"], [recorded_prb(cfg, off) for off in range(cfg["nof_symbols"])])
        if row[19] in regions:
            assert regions[row[19]] == region, i
        else:
            assert row[19] == next_grid, i
            regions[row[19]] = region
            next_grid += size
        # Every element the receiver reads is a stored one: the rebuilt grid is zero outside the region and the region is the
        # configured ports x the PUCCH's symbols x the 12 subcarriers of each symbol's PRB.
        mask = np.zeros((NOF_PORTS, 14, NOF_SUBC), bool)
        for off, prb in enumerate(region[2]):
            mask[cfg["ports"], region[1] + off, 12 * prb:12 * prb + 12] = True
        assert mask.sum() == size and not grids[k["grid"]][~mask].any(), i
        if cfg["format"] == 1:
            assert row[20] == next_estimate, i
            next_estimate += size // 12
        else:
            assert row[20] == -1 and k["want"]["meas"] is None and np.isnan(results[i][10:42]).all(), i
    assert next_grid == len(words) and next_estimate == len(estimates) and len(grids) == len(regions)
    # The flagged cases are the two zero grids; every other grid holds noise on every stored element.
    flagged = [i for i, k in enumerate(cases) if k["flagged"]]
    assert len(flagged) == NOF_FLAGGED <= 12 and [cases[i]["cfg"]["format"] for i in flagged] == [0, 1]
    for i, k in enumerate(cases):
        assert k["flagged"] == (not grids[k["grid"]].any()) == (k["row"][22] == 2), i
    noise_only = [k for k in cases if k["row"][22] == 3]
    assert sorted(k["cfg"]["format"] for k in noise_only) == [0] * 13 + [1] * 13 and not any(k["sent"] for k in noise_only)
    # Every candidate of each of format 0's five tables was sent at least once.
    for (nack, sr_opp), table in model.FORMAT0_TABLES.items():
        sent = {(k["row"][24], k["row"][25]) for k in cases if k["sent"] and k["cfg"]["format"] == 0 and k["cfg"]["nof_harq_ack"] == nack and
                k["cfg"]["sr_opportunity"] == sr_opp}
        assert sent >= {(sum(b << i for i, b in enumerate(ack)), -1 if sr is None else sr) for _, sr, ack in table}, (nack, sr_opp)
    # The margins, on recorded numbers alone: the decided metric, the per-port SNRs, and what the recorder evaluated in double for
    # format 0's two best candidates and format 1's two statistics.
    T = model.THRESHOLD
    for i, k in enumerate(cases):
        cfg, want = k["cfg"], k["want"]
        if k["flagged"]:
            continue
        decided = want["metric"] * T if cfg["format"] == 1 else 10 ** (want["sinr_dB"] / 10)
        assert not (T / 2 <= decided <= 2 * T), (i, decided)
        assert (want["status"] != model.INVALID) == (decided > T), (i, decided)
        if k["row"][22] == 3:
            continue
        top = sorted(want["top"])
        if len(model.FORMAT0_TABLES[(cfg["nof_harq_ack"], cfg["sr_opportunity"])]) > 1 if cfg["format"] == 0 else cfg["nof_harq_ack"] == 2:
            assert top[1] - top[0] >= RECORDING_MARGIN * top[1] > 0, (i, top)
        if cfg["format"] == 1 and len(cfg["ports"]) > 1:
            snr = sorted(m["snr"] for m in want["meas"])
            assert snr[-1] - snr[-2] >= RECORDING_MARGIN * snr[-1], (i, snr)
    # Whatever the grid held, the reference's time alignment estimator returned 0 for every port and hop.
    ta = np.concatenate([k["want"]["ta"].ravel() for k in cases if k["cfg"]["format"] == 1])
    assert len(ta) == 3 * sum(len(k["cfg"]["ports"]) for k in cases if k["cfg"]["format"] == 1) and not ta[~np.isnan(ta)].any()
    assert not results[:, 8].any()
    # Each status is on record; `unknown` is the SR-only format 1 that carries the symbol of a 1 bit.
    assert {k["want"]["status"] for k in cases} == {model.UNKNOWN, model.VALID, model.INVALID}
    assert [(k["cfg"]["format"], k["cfg"]["nof_harq_ack"], k["row"][24]) for k in cases if k["want"]["status"] == model.UNKNOWN] == [(1, 0, 1)]


def test_restatement_equals_the_recording():
    """model.process in float32 and float64 on every recorded case: the reference's decisions exactly, its numbers within the
    spreads above (measured here, printed and held against the constants)."""
    cases, grids = recording()
    spread = signal_spread = cfo_spread = 0.0
    where = [None, None, None]
    steps = 0
    for i, k in enumerate(cases):
        cfg, want = k["cfg"], k["want"]
        r32, r64 = (model.process(cfg, grids[k["grid"]], dt) for dt in (np.float32, np.float64))
        for r in (r32, r64):
            same_exact_fields(cfg, r, want, (i, cfg))
            assert all(m["ta_s"] == 0 and m["ta_bins"] == 0 for m in r["meas"] or [])
            if k["flagged"]:
                same_special_values(cfg, r, r["meas"] or [], want, (i, cfg))
        if cfg["format"] == 1:
            steps = max(steps, estimate_steps(cfg, r32["ce"], want, (i, cfg)))
        if k["flagged"]:
            continue
        d, c = recorded_distance(cfg, r64, r64["meas"] or [], want, (i, cfg))
        if d > spread:
            spread, where[0] = d, i
        if k["sent"] and d > signal_spread:
            signal_spread, where[1] = d, i
        if c > cfo_spread:
            cfo_spread, where[2] = c, i
    print("recording - float64 restatement: spread %.4g at case %s (constant %.3g), with a UE sent %.4g at case %s (constant %.3g), CFO "
          "%.4g at case %s (constant %.3g); float32 restatement's estimate within %d bf16 step(s) (constant %d); %d cases" %
          (spread, where[0], REF_SPREAD, signal_spread, where[1], REF_SIGNAL_SPREAD, cfo_spread, where[2], REF_CFO_SPREAD, steps,
           REF_ESTIMATE_ULPS, len(cases)))
    assert len(cases) == NOF_RECORDED and sum(k["flagged"] for k in cases) == NOF_FLAGGED
    assert steps <= REF_ESTIMATE_ULPS
    assert spread <= REF_SPREAD * 1.0001 and signal_spread <= REF_SIGNAL_SPREAD * 1.0001 and cfo_spread <= REF_CFO_SPREAD * 1.0001, \
        "the constants no longer describe the cases"
    # What the device is granted against the recording stays inside the margin the recording keeps around every decision.
    assert 8 * REF_SPREAD < RECORDING_MARGIN


def device_against_recording(i, k, res, meas, ce):
    """One device result (a RESULT_DTYPE record, MEAS_DTYPE records of the PUCCH's ports, the estimate [ports][14][subc] with
    sentinel words where nothing is written) against recorded case i: -> (distance, CFO distance, bf16 steps of the estimate)."""
    cfg, want = k["cfg"], k["want"]
    what = (i, cfg)
    P = len(cfg["ports"])
    same_exact_fields(cfg, res, want, what)
    assert not res["harq_ack"][cfg["nof_harq_ack"]:].any() and (cfg["sr_opportunity"] or res["sr"] == 0), (what, res)
    got = dict(metric=res["detection_metric"], sinr_dB=res["sinr_dB"], rsrp_dB=res["rsrp_dB"], epre_dB=res["epre_dB"], cfo_hz=res["cfo_hz"])
    steps = 0
    if cfg["format"] == 1:
        region = np.zeros(ce.shape, bool)
        for off in range(cfg["nof_symbols"]):
            prb = recorded_prb(cfg, off)
            region[:, cfg["start_symbol_index"] + off, 12 * prb:12 * prb + 12] = True
        assert (ce[~region] == SENTINEL).all(), what
        steps = estimate_steps(cfg, ce, want, what)
        assert steps <= 1, (what, steps)
        assert (meas["ta_s"] == want["ta"][:, 2]).all() and not meas["ta_bins"].any(), (what, meas)
    else:
        assert (ce == SENTINEL).all() and not meas.tobytes().strip(b"\0"), what
    if k["flagged"]:
        same_special_values(cfg, got, meas, want, what)
        return 0.0, 0.0, steps
    d, c = recorded_distance(cfg, got, meas, want, what)
    assert d <= 8 * (REF_SIGNAL_SPREAD if k["sent"] else REF_SPREAD) and c <= 8 * REF_CFO_SPREAD, (what, d, c, res, meas, want)
    return d, c, steps


@pytest.mark.gpu
def test_device_equals_the_recording(gpu_ctx):
    """Every recorded case through nrphy_pucch_run as one plan of mixed formats and one launch.  Decisions, exact fields and the
    time alignment equal; the estimate within 1 bf16 step (the bound test_parity_with_the_restatement holds the device to);
    metric, dB values, per-port measurements and CFO within 8 x the reference's own distance from the float64 restatement -- the
    allowance of the parity test and of the PRACH pin, for the same reason: per-lane double partial sums folded in another order
    than the reference's float32 vector sums, and another libm."""
    cases, grids = recording()
    assert len(cases) == NOF_RECORDED and {k["cfg"]["format"] for k in cases} == {0, 1}
    res, meas, ce = run_plan(gpu_ctx, [k["cfg"] for k in cases], [k["grid"] for k in cases], grids)
    worst = worst_signal = worst_cfo = 0.0
    steps = 0
    for i, k in enumerate(cases):
        P = len(k["cfg"]["ports"])
        assert not meas[i][P:].tobytes().strip(b"\0") and (ce[i][P:] == SENTINEL).all(), i
        d, c, s = device_against_recording(i, k, res[i], meas[i][:P], ce[i][:P])
        worst, worst_cfo, steps = max(worst, d), max(worst_cfo, c), max(steps, s)
        if k["sent"]:
            worst_signal = max(worst_signal, d)
    print("device - recording: worst %.3g (allowed %.3g), with a UE sent %.3g (allowed %.3g), CFO %.3g (allowed %.3g); estimate within "
          "%d bf16 step(s); %d PUCCHs in one launch" % (worst, 8 * REF_SPREAD, worst_signal, 8 * REF_SIGNAL_SPREAD, worst_cfo,
                                                         8 * REF_CFO_SPREAD, steps, len(cases)))


@pytest.mark.gpu
def test_host_call_equals_the_recording(gpu_ctx):
    """Three recorded cases of each format through nrphy_pucch_host: the zero grid, the first of the reference's configurations
    and a small shape on four permuted ports."""
    cases, grids = recording()
    picks = []
    for fmt in (0, 1):
        of = [i for i, k in enumerate(cases) if k["cfg"]["format"] == fmt]
        picks += [next(i for i in of if cases[i]["flagged"]), next(i for i in of if cases[i]["row"][22] == 0),
                  next(i for i in of if cases[i]["row"][22] == 1 and cases[i]["cfg"]["ports"] == [3, 1, 0, 2])]
    assert len(set(picks)) == 6
    for i in picks:
        k = cases[i]
        P = len(k["cfg"]["ports"])
        r, m, e = gpu_ctx.pucch_host(to_abi(k["cfg"]), grids[k["grid"]], with_estimate=True, ch_est=np.full((P, 14, NOF_SUBC), SENTINEL, np.uint32))
        device_against_recording(i, k, np.frombuffer(bytes(r), RESULT_DTYPE)[0], np.frombuffer(b"".join(bytes(x) for x in m), MEAS_DTYPE), e)
