"""PUSCH DM-RS channel estimator (nrphy_pusch_chest_*).

CPU: the POD mirrors, the validator over the reference unit test's 96 configurations (tests/golden/pusch_chest_configs.json) and
over each refused case, the extractor that wrote them, the restatement's pilots against the oracle's Gold sequence, and the
restatement against a recording of the reference's estimator (tests/golden/record_pusch_chest_reference.cpp: 24 grids of 1 to 273
PRB; smoothed pilots in float32, estimate, per-path measurements, time alignment bin).
GPU: the reference's DM-RS known answer, the device against that recording through the plan and the host call, the DC step against
the run without it, parity with the NumPy restatement (tests/pusch_chest_model.py) on seeded synthetic grids, physics (flat channel,
delay, CFO, noise), batches against per-PUSCH calls, graph replay, and a link from PDSCH-written grids through estimator,
demodulator and decoder to transport blocks.

The reference's distance from the restatement over the recording, measured by the CPU tests on every run (the device's allowance
is + 1 step and 8 x the spreads):
  REF_PILOT_SPREAD 5.3e-7 (measured 5.30e-07)   smoothed pilots, of the case's RMS pilot magnitude
  REF_CE_STEPS 63, REF_CE_WORD_STEPS 1.0        estimate: bf16 steps per component; in steps of the word's larger component
  REF_CE_SHARE 1.4e-3 (1.34e-03)                largest share of a case's components that differ at all
  REF_NOISE_SPREAD 4.8e-7 (4.74e-07), REF_RSRP_SPREAD 3.3e-7 (3.24e-07), REF_EPRE_SPREAD 3.2e-7 (3.11e-07),
  REF_SNR_SPREAD 4.7e-7 (4.64e-07), REF_CFO_SPREAD 3.1e-7 (3.04e-07)
  REF_ROW_STEPS 3, REF_ROW_SHARE 8.1e-4 (8.01e-04)  the estimate the restatement makes of the recorded smoothed pilots
The time alignment bin is the reference's in every recorded path.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import backends
import pusch_chest_model as model

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "pusch_chest_configs.json")
REFERENCE = "/root/reference/srsRAN-5G-ER"
MEAS_DTYPE = np.dtype([("noise_var", "<f4"), ("rsrp", "<f4"), ("epre", "<f4"), ("snr", "<f4"), ("ta_s", "<f4"),
                       ("ta_bins", "<i4"), ("cfo_hz", "<f4"), ("reserved_", "<u4")])
SENTINEL = 0x5A5AA5A5


def fixture_configs():
    return json.load(open(FIXTURE))


def cfg_from_fixture(f, **kw):
    args = dict(prbs=f["rb_mask"], numerology=f["numerology"], slot_index=f["slot_index"], scrambling_id=f["scrambling_id"],
                n_scid=f["n_scid"], scaling=f["scaling"], dmrs_type=f["dmrs_type"], dmrs_symbols=f["dmrs_symbols"],
                start_symbol=f["first_symbol"], nof_symbols=f["nof_symbols"], nof_layers=f["nof_tx_layers"],
                rx_ports=f["rx_ports"])
    args.update(kw)
    return abi.make_pusch_chest(**args)


def fixture_subc(f):
    return 12 * f["nof_rb"]


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_pusch_chest_pods_match_header():
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(nrphy_pusch_chest_cfg_t),
 offsetof(nrphy_pusch_chest_cfg_t, scaling), offsetof(nrphy_pusch_chest_cfg_t, rx_ports),
 offsetof(nrphy_pusch_chest_cfg_t, dc_position), offsetof(nrphy_pusch_chest_cfg_t, prb_mask),
 sizeof(nrphy_pusch_chest_meas_t), offsetof(nrphy_pusch_chest_meas_t, ta_bins), offsetof(nrphy_pusch_chest_meas_t, cfo_hz),
 (size_t)NRPHY_PUSCH_CHEST_NO_DC);return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()
    P, M = abi.PuschChestCfg, abi.PuschChestMeas
    assert [int(x) for x in out] == [C.sizeof(P), P.scaling.offset, P.rx_ports.offset, P.dc_position.offset, P.prb_mask.offset,
                                     C.sizeof(M), M.ta_bins.offset, M.cfo_hz.offset, abi.PUSCH_CHEST_NO_DC]
    assert C.sizeof(M) == MEAS_DTYPE.itemsize


def _base(**kw):
    args = dict(prbs=range(10, 30), numerology=1, slot_index=7, scrambling_id=500, n_scid=1, scaling=1.4125, dmrs_symbols=(2, 11),
                start_symbol=0, nof_symbols=14, nof_layers=2, rx_ports=(0, 1, 2, 3), dc_position=300)
    args.update(kw)
    return abi.make_pusch_chest(**args)


@pytest.mark.parametrize("name,cfg,ports,subc,want", [
    ("base", _base(), 4, 624, abi.OK),
    ("dc none", _base(dc_position=None), 4, 624, abi.OK),
    ("dc last", _base(dc_position=623), 4, 624, abi.OK),
    ("numerology 4, last slot", _base(numerology=4, slot_index=159), 4, 624, abi.OK),
    ("type 2", _base(dmrs_type=2), 4, 624, abi.ERR_ARGUMENT),
    ("3 layers", _base(nof_layers=3), 4, 624, abi.ERR_ARGUMENT),
    ("0 layers", _base(nof_layers=0), 4, 624, abi.ERR_ARGUMENT),
    ("repeated port", _base(rx_ports=(0, 1, 1)), 4, 624, abi.ERR_ARGUMENT),
    ("port outside the grid", _base(rx_ports=(0, 2)), 2, 624, abi.ERR_ARGUMENT),
    ("no port", _base(rx_ports=()), 4, 624, abi.ERR_ARGUMENT),
    ("PRB beyond the grid", _base(prbs=range(40, 53)), 4, 624, abi.ERR_ARGUMENT),
    ("empty PRB mask", _base(prbs=()), 4, 624, abi.ERR_ARGUMENT),
    ("no DM-RS symbol", _base(dmrs_symbols=()), 4, 624, abi.ERR_ARGUMENT),
    ("no DM-RS inside", _base(dmrs_symbols=(2,), start_symbol=4, nof_symbols=10), 4, 624, abi.ERR_ARGUMENT),
    ("DM-RS bit outside", _base(dmrs_symbols=(2, 11), start_symbol=0, nof_symbols=10), 4, 624, abi.ERR_ARGUMENT),
    ("symbols beyond the slot", _base(start_symbol=2, nof_symbols=13), 4, 624, abi.ERR_ARGUMENT),
    ("no symbol", _base(start_symbol=2, nof_symbols=0), 4, 624, abi.ERR_ARGUMENT),
    ("numerology 5", _base(numerology=5), 4, 624, abi.ERR_ARGUMENT),
    ("slot index", _base(numerology=1, slot_index=20), 4, 624, abi.ERR_ARGUMENT),
    ("scrambling id", _base(scrambling_id=65536), 4, 624, abi.ERR_ARGUMENT),
    ("n_scid", _base(n_scid=2), 4, 624, abi.ERR_ARGUMENT),
    ("zero scaling", _base(scaling=0.0), 4, 624, abi.ERR_ARGUMENT),
    ("negative scaling", _base(scaling=-1.0), 4, 624, abi.ERR_ARGUMENT),
    ("infinite scaling", _base(scaling=float("inf")), 4, 624, abi.ERR_ARGUMENT),
    ("NaN scaling", _base(scaling=float("nan")), 4, 624, abi.ERR_ARGUMENT),
    ("dc outside the grid", _base(dc_position=624), 4, 624, abi.ERR_ARGUMENT),
    ("grid not whole PRBs", _base(), 4, 620, abi.ERR_ARGUMENT),
])
def test_pusch_chest_validator(name, cfg, ports, subc, want):
    assert lib.pusch_chest_validate(cfg, ports, subc) == want, name


def test_pusch_chest_validator_over_the_reference_configurations():
    cfgs = fixture_configs()
    assert len(cfgs) == 96
    t1 = [f for f in cfgs if f["dmrs_type"] == 1]
    assert len(t1) == 48 and sum(f["label"] == "dmrs_creation" for f in t1) == 24
    for f in cfgs:
        want = abi.OK if f["dmrs_type"] == 1 else abi.ERR_ARGUMENT
        assert lib.pusch_chest_validate(cfg_from_fixture(f), 1, fixture_subc(f)) == want, f


def test_extractor_reproduces_the_committed_configurations():
    if not os.path.isdir(REFERENCE):
        pytest.skip("reference sources not present")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "c.json")
        subprocess.run([sys.executable, os.path.join(GOLDEN, "extract_pusch_chest_configs.py"), REFERENCE, out], check=True,
                       capture_output=True, timeout=120)
        assert open(out, "rb").read() == open(FIXTURE, "rb").read()


def test_restatement_pilots_equal_the_oracle_gold_sequence(oracle):
    cfg = _base(prbs=[0, 3, 4, 17, 50, 51], nof_layers=1)
    for l in (2, 11):
        pr, pi, k = model.pilots(cfg, l, 0)
        ci = model.c_init(cfg.slot_index, l, cfg.scrambling_id, cfg.n_scid)
        for j, n in enumerate(model.prbs_of(cfg)):
            want = oracle.prg_float(ci, 12 * n, 1 / np.sqrt(2), 12)
            assert np.array_equal(pr[6 * j:6 * j + 6], want[0::2]) and np.array_equal(pi[6 * j:6 * j + 6], want[1::2])
            assert np.array_equal(k[6 * j:6 * j + 6], 12 * n + 2 * np.arange(6))
    pr1, pi1, _ = model.pilots(cfg, 2, 1)
    pr0, pi0, _ = model.pilots(cfg, 2, 0)
    sign = np.where(np.arange(pr0.size) % 2 == 1, -1, 1)
    assert np.array_equal(pr1, pr0 * sign) and np.array_equal(pi1, pi0 * sign)


# ---- the recording of the reference's estimator (tests/golden/record_pusch_chest_reference.cpp) ----------------------------------
RES = ("noise_var", "rsrp", "epre", "snr", "ta_s", "cfo_hz", "ta_answer_s", "ta_bin", "ta_best", "ta_second", "ta_asked", "zero")
SIZE_CAP = 1000000  # bytes, every file of the recording
TA_MARGIN = 0.02    # MARGIN of the recorder; its comment says why shapes below 27 PRB are asked for half their curvature instead
CFO_FLOOR_HZ = 1.0  # as tests/test_pusch_processor.py
# The largest distances, over the recorded cases, between the reference's answers and the restatement's;
# test_restatement_equals_the_recording measures and prints them on every run.
#  - REF_PILOT_SPREAD: the smoothed pilots, float32 before any bf16 rounding, relative to the case's RMS pilot magnitude.
#  - REF_CE_STEPS: the estimate, bf16 steps per component.  Large where a component nearly cancels: with a CFO the estimate is rounded
#    to cbf16, rotated and rounded again, so a first rounding that falls the other way (a float32-sized difference of the pilots)
#    moves the other component by up to sin(phase) of a step of the larger one, which is many steps of a component a thousand times
#    smaller.  REF_CE_WORD_STEPS is the same distance in steps of the larger component of the recorded word, where it stays within
#    one; test_restatement_rounds_and_rotates_the_recorded_pilots_as_the_reference shows the second stage alone is the reference's.
#  - REF_CE_SHARE: the largest share of a case's components that differ at all.
#  - the measurements: relative distances, the CFO relative to max(|CFO|, CFO_FLOOR_HZ).
# The device may be REF_CE_STEPS + 1 and REF_CE_WORD_STEPS + 1 steps from the recording (the + 1 is what
# test_parity_with_the_restatement grants between device and restatement), differ in 8 x REF_CE_SHARE of a case's components, and be
# 8 x the other spreads away: the factor this project uses between the reference's spread and the device's allowance.
REF_PILOT_SPREAD = 5.3e-7  # measured 5.30e-07: 43 PRB, 2 layers, 2 ports
REF_CE_STEPS = 63          # measured 63: configuration 17, 108 PRB, an imaginary part of 0.0019 beside a real part of 0.55
REF_CE_WORD_STEPS = 1.0    # measured 1: 43 PRB, 2 layers, 2 ports
REF_CE_SHARE = 1.4e-3      # measured 1.34e-03: configuration 17, 108 PRB
REF_NOISE_SPREAD = 4.8e-7  # measured 4.74e-07: 1 PRB, 1 DM-RS, 1 port
REF_RSRP_SPREAD = 3.3e-7   # measured 3.24e-07: PRBs 3-8, 15-39, 51
REF_EPRE_SPREAD = 3.2e-7   # measured 3.11e-07: configuration 29, 47 PRB
REF_SNR_SPREAD = 4.7e-7    # measured 4.64e-07: 2 PRB, 2 DM-RS
REF_CFO_SPREAD = 3.1e-7    # measured 3.04e-07: 43 PRB, 2 layers, 2 ports
# The estimate the restatement makes of the *recorded* smoothed pilots (interpolation, cbf16, rotation with its own CFO, cbf16):
REF_ROW_STEPS = 3          # measured 3: 4 PRB, 4 DM-RS, an imaginary part of 2.6e-6 beside a real part of 1.2
REF_ROW_SHARE = 8.1e-4     # measured 8.01e-04: 4 PRB, 4 DM-RS (1 component of 1248)
REF_SPREADS = {"noise_var": REF_NOISE_SPREAD, "rsrp": REF_RSRP_SPREAD, "epre": REF_EPRE_SPREAD, "snr": REF_SNR_SPREAD,
               "cfo_hz": REF_CFO_SPREAD}


@functools.lru_cache(maxsize=None)
def recording():
    """The recorded cases, each with its configuration and its slices of the four arrays (read-only)."""
    cases = json.load(open(os.path.join(GOLDEN, "pusch_chest_reference_cases.json")))
    data = {k: np.load(os.path.join(GOLDEN, "pusch_chest_reference_%s.npy" % k)) for k in ("grids", "pilots", "estimates", "results")}
    for a in data.values():
        a.setflags(write=False)
    out = []
    for c in cases:
        P, L, nprb, nd, ns = len(c["rx_ports"]), c["nof_tx_layers"], len(c["prbs"]), len(c["dmrs_symbols"]), c["nof_symbols"]
        c = dict(c)
        c["cfg"] = abi.make_pusch_chest(prbs=c["prbs"], numerology=c["numerology"], slot_index=c["slot_index"],
                                        scrambling_id=c["scrambling_id"], n_scid=c["n_scid"], scaling=c["scaling"],
                                        dmrs_symbols=c["dmrs_symbols"], start_symbol=c["first_symbol"], nof_symbols=ns, nof_layers=L,
                                        rx_ports=c["rx_ports"])
        c["subc"] = (12 * np.array(c["prbs"])[:, None] + np.arange(12)).ravel()
        c["rows"] = data["grids"][c["grid_off"]:c["grid_off"] + P * nd * 12 * nprb].reshape(P, nd, 12 * nprb)
        c["pilots"] = data["pilots"][c["pilot_off"]:c["pilot_off"] + P * L * 6 * nprb].reshape(P, L, 6 * nprb)
        c["est"] = data["estimates"][c["est_off"]:c["est_off"] + L * P * ns * 12 * nprb].reshape(L, P, ns, 12 * nprb)
        c["res"] = data["results"][c["res_row"]:c["res_row"] + P * L].reshape(P, L, len(RES))
        out.append(c)
    return out, {k: a.size for k, a in data.items()}


def recorded_grid(c, nports, nsubc):
    """The case's grid [nports][14][nsubc]: the recorded DM-RS symbols of the allocated PRBs, zero elsewhere."""
    grid = np.zeros((nports, 14, nsubc), np.uint32)
    for i, p in enumerate(c["rx_ports"]):
        for d, l in enumerate(sorted(c["dmrs_symbols"])):
            grid[p, l, c["subc"]] = c["rows"][i, d]
    return grid


def component_steps(a, b):
    """bf16 steps between cbf16 words, per component: [..., 2]."""
    out = []
    for sh in (0, 16):
        x = ((np.asarray(a, np.uint32) >> sh) & 0xFFFF).astype(np.int64)
        y = ((np.asarray(b, np.uint32) >> sh) & 0xFFFF).astype(np.int64)
        out.append(np.abs(np.where(x & 0x8000, -(x & 0x7FFF), x) - np.where(y & 0x8000, -(y & 0x7FFF), y)))
    return np.stack(out, -1)


def word_steps(a, b):
    """Distance between cbf16 words per component, in bf16 steps of the larger component of b: [..., 2]."""
    (ar, ai), (br, bi) = model.from_words(a), model.from_words(b)
    big = np.maximum(np.abs(br), np.abs(bi)).astype(np.float32)
    step = ((big.view(np.uint32) & 0x7F800000).view(np.float32) * np.float32(2.0 ** -7)).astype(np.float64)
    step = np.where(step > 0, step, np.inf)  # a zero word: equal or not, which component_steps counts
    return np.stack([np.abs(ar.astype(np.float64) - br) / step, np.abs(ai.astype(np.float64) - bi) / step], -1)


def rel(a, b, floor=0.0):
    return abs(float(a) - float(b)) / max(abs(float(b)), floor)


def distances_from_the_recording(c, ce, nv, meas):
    """ce [L][P][14][subc] words, nv [P] or None, meas[p][l] with the fields of MEAS_DTYPE -> the figures the tests bound: bf16 steps
    and differing components of the estimate, relative distances of the measurements.  The time alignment bin is asserted here."""
    first, ns = c["first_symbol"], c["nof_symbols"]
    got = ce[:, :, first:first + ns][..., c["subc"]]
    steps = component_steps(got, c["est"])
    fig = {"steps": int(steps.max()), "word_steps": float(word_steps(got, c["est"]).max()), "differ": int((steps > 0).sum()),
           "components": steps.size, "noise_var": 0.0, "rsrp": 0.0, "epre": 0.0, "snr": 0.0, "cfo_hz": 0.0}
    fig["share"] = fig["differ"] / fig["components"]
    for p in range(len(c["rx_ports"])):
        for l in range(c["nof_tx_layers"]):
            r, m = dict(zip(RES, c["res"][p, l])), meas[p][l]
            for k in ("noise_var", "rsrp", "epre", "snr"):
                fig[k] = max(fig[k], rel(m[k], r[k]))
            if np.isnan(r["cfo_hz"]):
                assert np.isnan(float(m["cfo_hz"])), (c["name"], p, l)
            else:
                fig["cfo_hz"] = max(fig["cfo_hz"], rel(m["cfo_hz"], r["cfo_hz"], CFO_FLOOR_HZ))
            assert int(m["ta_bins"]) == int(r["ta_bin"]), (c["name"], p, l, int(m["ta_bins"]), r["ta_bin"])
        if nv is not None:  # what pusch_demodulator_impl reads: the port's layer 0
            fig["noise_var"] = max(fig["noise_var"], rel(nv[p], c["res"][p, 0, 0]))
    return fig


def test_recording_is_consistent():
    cases, sizes = recording()
    for k in ("cases.json", "grids.npy", "pilots.npy", "estimates.npy", "results.npy"):
        assert os.path.getsize(os.path.join(GOLDEN, "pusch_chest_reference_" + k)) < SIZE_CAP, k
    at = {"grid_off": 0, "pilot_off": 0, "est_off": 0, "res_row": 0}
    for c in cases:
        P, L, nprb, nd, ns = len(c["rx_ports"]), c["nof_tx_layers"], len(c["prbs"]), len(c["dmrs_symbols"]), c["nof_symbols"]
        assert {k: c[k] for k in at} == at, c["name"]
        at = {"grid_off": at["grid_off"] + P * nd * 12 * nprb, "pilot_off": at["pilot_off"] + P * L * 6 * nprb,
              "est_off": at["est_off"] + L * P * ns * 12 * nprb, "res_row": at["res_row"] + P * L}
        assert lib.pusch_chest_validate(c["cfg"], max(c["rx_ports"]) + 1, 12 * c["grid_prb"]) == abi.OK, c["name"]
        assert c["prbs"] == sorted(set(c["prbs"])) and c["prbs"][-1] < c["grid_prb"] and c["draws"] >= 1
        assert all(c["first_symbol"] <= l < c["first_symbol"] + ns for l in c["dmrs_symbols"])
        # the lead the recorder asked for, and that every path has it: no time alignment of the recording is a near tie
        k = c["subc"][0::2].astype(np.float64)
        asked = min(TA_MARGIN, 0.5 * (2 * np.pi / 4096) ** 2 * k.var())
        scs = 15000 << c["numerology"]
        for r in c["res"].reshape(-1, len(RES)):
            r = dict(zip(RES, r))
            assert r["ta_asked"] == pytest.approx(asked, rel=1e-12) and r["ta_best"] - r["ta_second"] >= asked * r["ta_best"], c["name"]
            assert r["ta_bin"] == int(r["ta_bin"]) and abs(r["ta_bin"]) <= model.TA_WINDOW and r["zero"] == 0
            assert r["ta_answer_s"] == pytest.approx(r["ta_bin"] / (4096.0 * scs), rel=1e-12, abs=1e-18)
            assert r["ta_s"] == pytest.approx(r["ta_answer_s"], rel=1e-9, abs=1e-18)  # a phy_time_unit: whole T_c, as every bin is
            assert np.isnan(r["cfo_hz"]) == (nd == 1) and r["noise_var"] > 0 and r["epre"] > 0
    assert (at["grid_off"], at["pilot_off"], at["est_off"], at["res_row"] * len(RES)) == \
        (sizes["grids"], sizes["pilots"], sizes["estimates"], sizes["results"])
    # every regime of the kernel
    assert {model.filter_taps(len(c["prbs"])).size for c in cases} == {5, 11, 15}
    assert {len(c["dmrs_symbols"]) for c in cases} == {1, 2, 3, 4} and {c["nof_tx_layers"] for c in cases} == {1, 2}
    assert any(c["prbs"][-1] - c["prbs"][0] + 1 != len(c["prbs"]) for c in cases)                      # a non-contiguous mask
    assert any(c["rx_ports"] != list(range(len(c["rx_ports"]))) for c in cases)                       # a port list that is not 0 .. n - 1
    assert {256 < 6 * len(c["prbs"]) <= 512 for c in cases} == {False, True} and any(6 * len(c["prbs"]) > 512 for c in cases)
    assert any(len(c["prbs"]) == 273 for c in cases) and {c["numerology"] for c in cases} == {0, 1}
    assert any(c["first_symbol"] > 0 for c in cases) and any(c["nof_symbols"] == 3 for c in cases)
    bins = [r[RES.index("ta_bin")] for c in cases for r in c["res"].reshape(-1, len(RES))]
    assert min(bins) <= -30 and max(bins) >= 30 and any(-8 <= b < 0 for b in bins) and any(0 < b <= 8 for b in bins)
    assert any(not c["ue"] for c in cases) and {0.0, 40.0} <= {c["snr_db"] for c in cases}
    assert sum(c["source"] >= 0 for c in cases) == 6 and all(fixture_configs()[c["source"]]["label"] == "ch_estimation"
                                                             for c in cases if c["source"] >= 0)


@functools.lru_cache(maxsize=None)
def restatement(i):
    """model.estimate of recorded case i, computed once."""
    c = recording()[0][i]
    return model.estimate(c["cfg"], recorded_grid(c, max(c["rx_ports"]) + 1, 12 * c["grid_prb"]))


FIGURES = ("steps", "word_steps", "share", "noise_var", "rsrp", "epre", "snr", "cfo_hz")


def allowance_line(worst, where):
    return ", ".join("%s %.3g (%s)" % (k, worst[k], where.get(k, "-")) for k in worst)


def test_restatement_equals_the_recording():
    """The reference's own distance from the restatement: the smoothed pilots (float32, before any bf16 rounding) relative to the
    case's RMS pilot magnitude, the estimate in bf16 steps, the measurements; the time alignment bin equal in every case."""
    cases, _ = recording()
    worst, where = dict.fromkeys(("pilots",) + FIGURES, 0), {}
    for i, c in enumerate(cases):
        ce, nv, meas = restatement(i)
        fig = distances_from_the_recording(c, ce, nv, meas)
        rms = np.sqrt(np.mean(np.abs(c["pilots"].astype(np.complex128)) ** 2))
        fig["pilots"] = max(np.abs(meas[p][l]["smoothed"].astype(np.complex128) - c["pilots"][p, l]).max() / rms
                            for p in range(len(c["rx_ports"])) for l in range(c["nof_tx_layers"]))
        for k in worst:
            if fig[k] > worst[k]:
                worst[k], where[k] = fig[k], c["name"]
    print("recording - restatement: " + allowance_line(worst, where))
    print("constants: pilots %.3g, steps %d, word_steps %.3g, share %.3g, %s" %
          (REF_PILOT_SPREAD, REF_CE_STEPS, REF_CE_WORD_STEPS, REF_CE_SHARE, ", ".join("%s %.3g" % kv for kv in REF_SPREADS.items())))
    # beyond float32 rounding the two would read the reference differently: a finding, not a constant
    assert worst["pilots"] <= 1e-5 and worst["word_steps"] <= 2
    assert worst["pilots"] <= REF_PILOT_SPREAD and worst["steps"] <= REF_CE_STEPS and worst["word_steps"] <= REF_CE_WORD_STEPS
    assert worst["share"] <= REF_CE_SHARE
    for k, v in REF_SPREADS.items():
        assert worst[k] <= v, (k, worst[k], where[k])


def test_restatement_rounds_and_rotates_the_recorded_pilots_as_the_reference():
    """From the reference's own smoothed pilots on: interpolation with the last element repeated, cbf16, the rotation by the CFO at
    every symbol of the window (the restatement's CFO, within REF_CFO_SPREAD of the reference's), cbf16 again.  Per component."""
    cases, _ = recording()
    steps, share, where = 0, 0.0, None
    for i, c in enumerate(cases):
        meas, ep, differ = restatement(i)[2], model.epochs(c["numerology"]), 0
        for p in range(len(c["rx_ports"])):
            for l in range(c["nof_tx_layers"]):
                f = c["pilots"][p, l]
                row = model.interpolate(f.real.astype(np.float32), f.imag.astype(np.float32))
                for j in range(c["nof_symbols"]):
                    u = component_steps(model.rotate(row, meas[p][l]["cfo"], ep[c["first_symbol"] + j]), c["est"][l, p, j])
                    steps, differ = max(steps, int(u.max())), differ + int((u > 0).sum())
        if differ / (2 * c["est"].size) > share:
            share, where = differ / (2 * c["est"].size), c["name"]
    print("recording - restatement from the recorded pilots: %d steps (constant %d), share %.3g at %s (constant %.3g)" %
          (steps, REF_ROW_STEPS, share, where, REF_ROW_SHARE))
    assert steps <= REF_ROW_STEPS and share <= REF_ROW_SHARE


# =======================================================================================================================
# GPU
# =======================================================================================================================
dev, as_i32 = model.dev, model.as_i32


def run_plan(ctx, cfgs, grids, grid_index, nports, nsubc, stream=None):
    """One nrphy_pusch_chest_run: returns (estimates [i] of [L][P][14][nsubc] words, noise rows [n][4], meas [n][4][2]), the
    estimate buffer filled with SENTINEL first."""
    import torch
    sizes = [c.nof_tx_layers * c.nof_rx_ports * 14 * nsubc for c in cfgs]
    offs = [int(o) for o in np.cumsum([0] + sizes)[:-1]]
    plan = lib.PuschChestPlan(ctx, cfgs, grid_index, len(grids), nports, nsubc, offs)
    d_grid = dev(as_i32(np.stack(grids)))
    d_ce = torch.full((sum(sizes),), np.int32(np.uint32(SENTINEL).view(np.int32)), dtype=torch.int32, device="cuda")
    d_nv = torch.full((len(cfgs), 4), -1.0, dtype=torch.float32, device="cuda")
    d_meas = torch.zeros((len(cfgs), 4, 2, MEAS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    plan.run(d_grid, d_ce, d_nv, d_meas)
    ctx.synchronize()
    ce = d_ce.cpu().numpy().view(np.uint32)
    out = [ce[o:o + s].reshape(c.nof_tx_layers, c.nof_rx_ports, 14, nsubc) for c, o, s in zip(cfgs, offs, sizes)]
    meas = d_meas.cpu().numpy().reshape(-1).view(MEAS_DTYPE).reshape(len(cfgs), 4, 2)
    plan.close()
    return out, d_nv.cpu().numpy(), meas


def region(cfg, nsubc):
    """Boolean [14][nsubc]: what the estimator writes."""
    m = np.zeros((14, nsubc), bool)
    subc = (12 * np.array(model.prbs_of(cfg))[:, None] + np.arange(12)).ravel()
    for s in range(cfg.start_symbol_index, cfg.start_symbol_index + cfg.nof_symbols):
        m[s, subc] = True
    return m


def synthetic_grid(rng, cfg, nports, nsubc, snr_db=20.0, delay=3.0, cfo_hz=150.0, paths=2):
    """Grid of DM-RS (scaled by beta) and QPSK data through a per-(port, layer) multipath channel with delay and CFO, + AWGN."""
    L, P = cfg.nof_tx_layers, cfg.nof_rx_ports
    k = np.arange(nsubc)
    ep = np.array(model.epochs(cfg.numerology), np.float64)
    scs = 15000 << cfg.numerology
    x = np.zeros((L, 14, nsubc), np.complex128)
    for l in range(L):
        x[l] = (rng.choice([-1, 1], (14, nsubc)) + 1j * rng.choice([-1, 1], (14, nsubc))) / np.sqrt(2)
        for s in range(14):
            if (cfg.dmrs_symbol_mask >> s) & 1:
                pr, pi, kk = model.pilots(cfg, s, l)
                x[l, s, kk] = float(cfg.scaling) * (pr + 1j * pi)
                x[l, s, kk + 1] = 0
    grid = np.zeros((nports, 14, nsubc), np.complex128)
    nv = 10 ** (-snr_db / 10)
    for p in range(P):
        for l in range(L):
            H = np.zeros(nsubc, np.complex128)
            for q in range(paths):
                g = (0.5 ** q) * np.exp(1j * rng.uniform(0, 2 * np.pi))
                H += g * np.exp(-2j * np.pi * k * (delay + 4 * q) / 4096.0)
            grid[cfg.rx_ports[p]] += H[None, :] * x[l]
        grid[cfg.rx_ports[p]] *= np.exp(2j * np.pi * (cfo_hz / scs) * ep)[:, None]
        grid[cfg.rx_ports[p]] += (rng.standard_normal((14, nsubc)) + 1j * rng.standard_normal((14, nsubc))) * np.sqrt(nv / 2)
    return model.to_cbf16(grid.astype(np.complex64))


def bf16_ulps(a, b):
    worst = np.zeros(np.shape(a), np.int64)
    for sh in (0, 16):
        x = ((np.asarray(a, np.uint32) >> sh) & 0xFFFF).astype(np.int64)
        y = ((np.asarray(b, np.uint32) >> sh) & 0xFFFF).astype(np.int64)
        ox = np.where(x & 0x8000, -(x & 0x7FFF), x)
        oy = np.where(y & 0x8000, -(y & 0x7FFF), y)
        worst = np.maximum(worst, np.abs(ox - oy))
    return worst


def check_parity(cfg, grid, got_ce, got_nv, got_meas, nsubc, what):
    want_ce, want_nv, want_meas = model.estimate(cfg, grid)
    m = region(cfg, nsubc)
    for l in range(cfg.nof_tx_layers):
        for p in range(cfg.nof_rx_ports):
            u = bf16_ulps(got_ce[l, p][m], want_ce[l, p][m])
            assert u.max() <= 1, (what, l, p, int(u.max()), int((u > 1).sum()))
            assert (got_ce[l, p][~m] == SENTINEL).all(), (what, "outside the region", l, p)
    scs = 15000 << cfg.numerology
    for p in range(cfg.nof_rx_ports):
        assert got_nv[p] == pytest.approx(float(want_nv[p]), rel=1e-4), (what, p)
        for l in range(cfg.nof_tx_layers):
            g, w = got_meas[p, l], want_meas[p][l]
            for key in ("rsrp", "epre", "snr", "noise_var"):
                assert float(g[key]) == pytest.approx(float(w[key]), rel=1e-4), (what, key, p, l)
            if np.isnan(w["cfo_hz"]):
                assert np.isnan(g["cfo_hz"]), what
            else:
                assert abs(float(g["cfo_hz"]) - float(w["cfo_hz"])) <= max(1e-4 * abs(float(w["cfo_hz"])), 1e-3 * scs), what
            if not w["ta_near_tie"]:
                assert int(g["ta_bins"]) == w["ta_bins"], (what, p, l, int(g["ta_bins"]), w["ta_bins"])
            assert float(g["ta_s"]) == pytest.approx(int(g["ta_bins"]) / (4096.0 * scs), rel=1e-6)


@pytest.mark.gpu
def test_dmrs_known_answer_over_the_reference_configurations(gpu_ctx):
    """dmrs_pusch_estimator_test.cpp, test Creation: a grid holding only beta x DM-RS estimates 1 on every allocated RE."""
    for f in fixture_configs():
        if f["dmrs_type"] != 1:
            continue
        cfg = cfg_from_fixture(f)
        nsubc = fixture_subc(f)
        grid = np.zeros((1, 14, nsubc), np.complex64)
        for s in f["dmrs_symbols"]:
            pr, pi, k = model.pilots(cfg, s, 0)
            grid[0, s, k] = np.float32(cfg.scaling) * (pr + 1j * pi)
        (ce,), nv, meas = run_plan(gpu_ctx, [cfg], [model.to_cbf16(grid)], [0], 1, nsubc)
        m = region(cfg, nsubc)
        est = model.from_cbf16(ce[0, 0][m])
        assert np.abs(est - 1).max() < 0.01, (f["label"], f["slot"], np.abs(est - 1).max())
        assert (ce[0, 0][~m] == SENTINEL).all()


def parity_cases():
    cases = []
    for f in fixture_configs():
        if f["dmrs_type"] == 1 and f["label"] == "ch_estimation":
            cases.append(("ref slot %s rb %d" % (f["slot"], len(f["rb_mask"])), cfg_from_fixture(f), 1, fixture_subc(f)))
    b = abi.make_pusch_chest
    cases += [
        ("1 PRB, 1 DM-RS", b(prbs=[7], dmrs_symbols=(2,), rx_ports=(0,)), 1, 624),
        ("2 PRB, 2 ports, 2 layers", b(prbs=[10, 11], dmrs_symbols=(2, 11), nof_layers=2, rx_ports=(1, 0)), 2, 624),
        ("3 PRB, n_scid 1, mu 1", b(prbs=[20, 21, 22], numerology=1, slot_index=13, scrambling_id=77, n_scid=1,
                                    dmrs_symbols=(3, 8), start_symbol=1, nof_symbols=13, rx_ports=(0, 1, 2)), 3, 624),
        ("273 PRB, 4 ports, 2 layers, DC", b(prbs=range(273), scrambling_id=1001, slot_index=9, scaling=1.4125,
                                             dmrs_symbols=(2, 7, 11), nof_layers=2, rx_ports=(0, 1, 2, 3), dc_position=1638),
         4, 3276),
        ("non-contiguous, 4 DM-RS, DC", b(prbs=list(range(3, 9)) + list(range(15, 40)) + [51], dmrs_symbols=(2, 5, 8, 11),
                                          scaling=1.4125, rx_ports=(3, 1, 0, 2), nof_layers=2, dc_position=306), 4, 624),
        ("mu 1, 3 DM-RS, 1 layer", b(prbs=range(5, 60), numerology=1, slot_index=17, dmrs_symbols=(2, 7, 11),
                                     rx_ports=(0, 1), dc_position=400), 2, 1272),
        ("single symbol window", b(prbs=range(0, 24), dmrs_symbols=(5,), start_symbol=4, nof_symbols=3, rx_ports=(0,)), 1, 624),
    ]
    return cases


@pytest.mark.gpu
def test_parity_with_the_restatement(gpu_ctx):
    rng = np.random.default_rng(2024)
    for i, (what, cfg, nports, nsubc) in enumerate(parity_cases()):
        grid = synthetic_grid(rng, cfg, nports, nsubc, snr_db=15.0 + 5 * (i % 3), delay=float(i % 5) - 2.0,
                              cfo_hz=100.0 * ((i % 7) - 3))
        (ce,), nv, meas = run_plan(gpu_ctx, [cfg], [grid], [0], nports, nsubc)
        check_parity(cfg, grid, ce, nv[0], meas[0], nsubc, what)


def check_against_the_recording(c, ce, nv, meas, nsubc, worst, where):
    """One recorded case: the device within the allowances that REF_* give, nothing written outside the region."""
    fig = distances_from_the_recording(c, ce, nv, meas)
    assert (ce[:, :, ~region(c["cfg"], nsubc)] == SENTINEL).all(), (c["name"], "outside the region")
    for k in FIGURES:
        if fig[k] > worst[k]:
            worst[k], where[k] = fig[k], c["name"]
    assert fig["steps"] <= REF_CE_STEPS + 1 and fig["word_steps"] <= REF_CE_WORD_STEPS + 1, (c["name"], fig)
    assert fig["differ"] <= (8 * REF_CE_SHARE * fig["components"] if REF_CE_SHARE else 1), (c["name"], fig)
    for k, v in REF_SPREADS.items():
        assert fig[k] <= 8 * v, (c["name"], k, fig[k], 8 * v)


def device_allowances():
    return "steps %d, word_steps %.3g, share %.3g, %s" % (REF_CE_STEPS + 1, REF_CE_WORD_STEPS + 1, 8 * REF_CE_SHARE,
                                                          ", ".join("%s %.3g" % (k, 8 * v) for k, v in REF_SPREADS.items()))


@pytest.mark.gpu
def test_device_equals_the_recording(gpu_ctx):
    """Every recorded case in two plans: the grids of up to 52 PRB as 4 ports x 624 subcarriers, the wider ones as 1 x 3276."""
    cases, _ = recording()
    worst, where = dict.fromkeys(FIGURES, 0), {}
    for nports, nsubc, group in ((4, 624, [c for c in cases if c["grid_prb"] <= 52]), (1, 3276, [c for c in cases if c["grid_prb"] > 52])):
        assert all(max(c["rx_ports"]) < nports and 12 * (c["prbs"][-1] + 1) <= nsubc for c in group)
        ces, nv, meas = run_plan(gpu_ctx, [c["cfg"] for c in group], [recorded_grid(c, nports, nsubc) for c in group],
                                 list(range(len(group))), nports, nsubc)
        for i, c in enumerate(group):
            check_against_the_recording(c, ces[i], nv[i], meas[i], nsubc, worst, where)
            assert (nv[i, len(c["rx_ports"]):] == -1.0).all()
    print("device - recording: " + allowance_line(worst, where) + "; allowed: " + device_allowances())


@pytest.mark.gpu
def test_host_call_equals_the_recording(gpu_ctx):
    """The same through nrphy_pusch_chest_host, for the recorded shapes of up to 4 PRB."""
    cases, _ = recording()
    small = [c for c in cases if len(c["prbs"]) <= 4]
    assert len(small) >= 5
    worst, where = dict.fromkeys(FIGURES, 0), {}
    for c in small:
        nports, nsubc = max(c["rx_ports"]) + 1, 12 * c["grid_prb"]
        sentinel = np.full((c["nof_tx_layers"], len(c["rx_ports"]), 14, nsubc), SENTINEL, np.uint32)
        ce, nv, m = gpu_ctx.pusch_chest_host(c["cfg"], recorded_grid(c, nports, nsubc), sentinel)
        meas = [[np.frombuffer(bytes(m[p][l]), MEAS_DTYPE)[0] for l in range(c["nof_tx_layers"])] for p in range(len(c["rx_ports"]))]
        check_against_the_recording(c, ce, nv, meas, nsubc, worst, where)
    print("host call - recording: " + allowance_line(worst, where) + "; allowed: " + device_allowances())


@pytest.mark.gpu
def test_dc_step_zeroes_its_subcarrier_and_nothing_else(gpu_ctx):
    """pusch_processor_impl's DC step, which the recording leaves out: on a pilot subcarrier of an allocated PRB, on a subcarrier
    between pilots, and in an unallocated PRB between two allocated ranges.  Against the run without DC, byte for byte."""
    prbs = list(range(3, 9)) + list(range(15, 40)) + [51]
    base = dict(prbs=prbs, dmrs_symbols=(2, 7, 11), start_symbol=1, nof_symbols=13, scaling=1.4125, nof_layers=2, rx_ports=(2, 0),
                slot_index=6, scrambling_id=321)
    placements = [("pilot subcarrier", 12 * 5 + 4, True), ("between pilots", 12 * 20 + 7, True), ("unallocated PRB", 12 * 10 + 3, False)]
    cfgs = [abi.make_pusch_chest(**base)] + [abi.make_pusch_chest(dc_position=k, **base) for _, k, _ in placements]
    assert cfgs[0].dc_position == abi.PUSCH_CHEST_NO_DC and all(lib.pusch_chest_validate(c, 3, 624) == abi.OK for c in cfgs)
    grid = synthetic_grid(np.random.default_rng(31), cfgs[0], 3, 624)
    ces, nv, meas = run_plan(gpu_ctx, cfgs, [grid], [0] * len(cfgs), 3, 624)
    m = region(cfgs[0], 624)
    assert (ces[0][:, :, m] != 0).all() and (ces[0][:, :, ~m] == SENTINEL).all()  # (no estimate of this grid is exactly zero)
    for (what, k, allocated), ce, n, ms in zip(placements, ces[1:], nv[1:], meas[1:]):
        assert (k // 12 in prbs) == allocated and m[1:, k].all() == allocated, what
        other = np.ones(624, bool)
        other[k] = False
        assert np.array_equal(ce[..., other], ces[0][..., other]), what
        if allocated:
            assert (ce[:, :, 1:, k] == 0).all() and (ce[:, :, 0, k] == SENTINEL).all(), what
        else:
            assert (ce[..., k] == SENTINEL).all(), what
        assert n.tobytes() == nv[0].tobytes() and ms.tobytes() == meas[0].tobytes(), what


@pytest.mark.gpu
def test_twiddles_are_built_on_first_use_and_outlive_a_plan():
    """The time-alignment twiddles are the context's: the first plan of a fresh context builds them, destroying that plan leaves
    them, and a second plan reads the same table.  Same bytes both times, and the restatement's answer, time alignment included."""
    what, cfg, nports, nsubc = "1 PRB, 1 DM-RS", abi.make_pusch_chest(prbs=[7], dmrs_symbols=(2,), rx_ports=(0,)), 1, 624
    grid = synthetic_grid(np.random.default_rng(7), cfg, nports, nsubc)
    ctx = lib.Context(0)
    try:
        runs = [run_plan(ctx, [cfg], [grid], [0], nports, nsubc) for _ in range(2)]  # each creates, runs and destroys its plan
    finally:
        ctx.close()
    for (ce,), nv, meas in runs:
        assert (ce.tobytes(), nv.tobytes(), meas.tobytes()) == (runs[0][0][0].tobytes(), runs[0][1].tobytes(), runs[0][2].tobytes())
    (ce,), nv, meas = runs[0]
    check_parity(cfg, grid, ce, nv[0], meas[0], nsubc, what)


@pytest.mark.gpu
def test_flat_noiseless_channel_is_estimated_exactly(gpu_ctx):
    h = 0.8 * np.exp(0.6j)
    cfg = abi.make_pusch_chest(prbs=range(4, 40), dmrs_symbols=(2, 11), rx_ports=(0,))
    grid = np.zeros((1, 14, 624), np.complex64)
    for s in (2, 11):
        pr, pi, k = model.pilots(cfg, s, 0)
        grid[0, s, k] = h * (pr + 1j * pi)
    (ce,), nv, meas = run_plan(gpu_ctx, [cfg], [model.to_cbf16(grid)], [0], 1, 624)
    est = model.from_cbf16(ce[0, 0][region(cfg, 624)])
    assert np.abs(est - h).max() < 2 * 2 ** -8 * abs(h)
    assert abs(float(meas[0, 0, 0]["cfo_hz"])) < 1.0 and int(meas[0, 0, 0]["ta_bins"]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("d", [0, 3, -3, 40, -40])
def test_pure_delay_gives_its_bin(gpu_ctx, d):
    cfg = abi.make_pusch_chest(prbs=range(0, 106), dmrs_symbols=(2,), rx_ports=(0,))
    grid = np.zeros((1, 14, 1272), np.complex64)
    pr, pi, k = model.pilots(cfg, 2, 0)
    grid[0, 2, k] = np.exp(-2j * np.pi * k * d / 4096.0) * (pr + 1j * pi)
    (ce,), nv, meas = run_plan(gpu_ctx, [cfg], [model.to_cbf16(grid)], [0], 1, 1272)
    assert int(meas[0, 0, 0]["ta_bins"]) == d
    assert float(meas[0, 0, 0]["ta_s"]) == pytest.approx(d / (4096 * 15000.0), abs=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("cfo", [300.0, -300.0])
def test_cfo_is_measured(gpu_ctx, cfo):
    rng = np.random.default_rng(int(cfo) & 0xFFFF)
    cfg = abi.make_pusch_chest(prbs=range(0, 52), dmrs_symbols=(2, 7, 11), rx_ports=(0,))
    grid = synthetic_grid(rng, cfg, 1, 624, snr_db=30.0, delay=0.0, cfo_hz=cfo, paths=1)
    (ce,), nv, meas = run_plan(gpu_ctx, [cfg], [grid], [0], 1, 624)
    assert float(meas[0, 0, 0]["cfo_hz"]) == pytest.approx(cfo, rel=0.01)


@pytest.mark.gpu
def test_noise_variance_on_a_flat_channel(gpu_ctx):
    rng = np.random.default_rng(10)
    cfg = abi.make_pusch_chest(prbs=range(0, 106), dmrs_symbols=(2, 5, 8, 11), rx_ports=(0,))
    grid = np.zeros((1, 14, 1272), np.complex128)
    sigma2 = 0.1  # 10 dB below the unit-power pilots
    for s in (2, 5, 8, 11):
        pr, pi, k = model.pilots(cfg, s, 0)
        grid[0, s, k] = 0.9 * np.exp(0.3j) * (pr + 1j * pi)
    grid += (rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape)) * np.sqrt(sigma2 / 2)
    (ce,), nv, meas = run_plan(gpu_ctx, [cfg], [model.to_cbf16(grid.astype(np.complex64))], [0], 1, 1272)
    assert 0.85 <= nv[0, 0] / sigma2 <= 1.05, nv[0, 0]


def batch_cases():
    b = abi.make_pusch_chest
    return [b(prbs=range(0, 20), dmrs_symbols=(2, 11), rx_ports=(0, 1), nof_layers=2, slot_index=3, dc_position=120),
            b(prbs=range(30, 52), dmrs_symbols=(2,), rx_ports=(1,), scrambling_id=9),
            b(prbs=[0, 2, 4, 6, 8], dmrs_symbols=(3, 7, 10), start_symbol=2, nof_symbols=12, rx_ports=(1, 0), n_scid=1),
            b(prbs=range(10, 45), dmrs_symbols=(2, 5, 8, 11), rx_ports=(0,), scaling=1.4125, dc_position=300)]


@pytest.mark.gpu
def test_mixed_batch_equals_per_pusch_host_calls(gpu_ctx):
    rng = np.random.default_rng(77)
    cfgs = batch_cases()
    grids = [synthetic_grid(rng, c, 2, 624, snr_db=18.0) for c in cfgs[:2]]
    gidx = [0, 1, 1, 0]
    ces, nv, meas = run_plan(gpu_ctx, cfgs, grids, gidx, 2, 624)
    for i, c in enumerate(cfgs):
        sentinel = np.full((c.nof_tx_layers, c.nof_rx_ports, 14, 624), SENTINEL, np.uint32)
        ce1, nv1, m1 = gpu_ctx.pusch_chest_host(c, grids[gidx[i]], sentinel)
        assert np.array_equal(ces[i], ce1), i
        assert np.array_equal(nv[i, :c.nof_rx_ports].view(np.uint32), nv1.view(np.uint32)), i
        assert (nv[i, c.nof_rx_ports:] == -1.0).all()  # entries of absent ports are left alone
        for p in range(c.nof_rx_ports):
            for l in range(c.nof_tx_layers):
                assert bytes(m1[p][l]) == meas[i, p, l].tobytes(), (i, p, l)
        check_parity(c, grids[gidx[i]], ces[i], nv[i], meas[i], 624, "batch %d" % i)


@pytest.mark.gpu
def test_graph_replay_and_two_runs_give_identical_bits(gpu_ctx):
    import torch
    rng = np.random.default_rng(5)
    cfgs = batch_cases()
    grid = synthetic_grid(rng, cfgs[0], 2, 624)
    sizes = [c.nof_tx_layers * c.nof_rx_ports * 14 * 624 for c in cfgs]
    offs = [int(o) for o in np.cumsum([0] + sizes)[:-1]]
    plan = lib.PuschChestPlan(gpu_ctx, cfgs, [0] * len(cfgs), 1, 2, 624, offs)
    d_grid = dev(as_i32(grid))
    outs = []
    for _ in range(2):
        d_ce = torch.zeros(sum(sizes), dtype=torch.int32, device="cuda")
        d_nv = torch.zeros((len(cfgs), 4), dtype=torch.float32, device="cuda")
        d_meas = torch.zeros((len(cfgs), 4, 2, 32), dtype=torch.uint8, device="cuda")
        plan.run(d_grid, d_ce, d_nv, d_meas)
        gpu_ctx.synchronize()
        outs.append((d_ce.cpu().numpy(), d_nv.cpu().numpy().view(np.uint32), d_meas.cpu().numpy()))
    for a, b_ in zip(*outs):
        assert np.array_equal(a, b_)
    g_ce = torch.zeros(sum(sizes), dtype=torch.int32, device="cuda")
    g_nv = torch.zeros((len(cfgs), 4), dtype=torch.float32, device="cuda")
    g_meas = torch.zeros((len(cfgs), 4, 2, 32), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.run(d_grid, g_ce, g_nv, g_meas, stream=C.c_void_p(stream.cuda_stream))
    for _ in range(2):
        g_ce.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(g_ce.cpu().numpy(), outs[0][0])
        assert np.array_equal(g_nv.cpu().numpy().view(np.uint32), outs[0][1])
        assert np.array_equal(g_meas.cpu().numpy(), outs[0][2])
    plan.close()


# ---- link: transport blocks -> device PDSCH chain -> multipath channel with delay and CFO + noise -> nrphy_pusch_chest_run ->
# nrphy_pusch_demod_run (with the estimator's noise variances) -> nrphy_pusch_decode_batch ------------------------------------
LINK_CASES = [  # qm, code rate x 1024, SNR dB of one port, equaliser, layers, rx ports
    (2, 449, 8.0, abi.EQ_ZF, 1, 1),
    (4, 616, 16.0, abi.EQ_MMSE, 1, 2),
    (6, 719, 22.0, abi.EQ_ZF, 1, 4),
    (8, 797, 30.0, abi.EQ_MMSE, 1, 4),
    (2, 449, 10.0, abi.EQ_ZF, 2, 2),
    (4, 616, 20.0, abi.EQ_ZF, 2, 4),
    (4, 616, 20.0, abi.EQ_ZF, 2, 2),
]
# Two layers stop at 16-QAM: ports 1000 and 1001 share their RE, and the reference's per-layer noise estimate (estimate_noise)
# counts the other layer's DM-RS as noise, so a port's layer-0 variance is about |h_other|^2 beta^2; the 2-layer ZF demodulator
# takes the ports' maximum, which scales the soft bits down by some 30 dB here.  64-QAM did not decode at 27 dB for that reason.
BETA = float(np.float32(10 ** (3 / 20)))  # convert_dB_to_amplitude(-get_sch_to_dmrs_ratio_dB(2))
# The PDSCH writer scales by 10^(-ratio / 20) (pdsch_processor_impl.cpp:154,177): DM-RS at -3 dB, data at 0 dB put the DM-RS
# 3 dB above the data, as a PUSCH with two CDM groups without data carries them.


def link_chain(ctx, oracle, qm, rate, layers, ports, equalizer, slots=2, nprb=52):
    """Transmit grids, channel and the three plans of a link (shared by the test below and the graph test)."""
    import torch
    nsubc = 12 * nprb
    dmrs = (2, 11)
    tb_bits = oracle.tbs(14, 12 * len(dmrs), 0, qm, float(rate), layers, nprb)
    bg = 2 if (rate <= 256 or tb_bits <= 292 or (tb_bits <= 3824 and rate <= 686)) else 1
    prec = np.eye(layers, dtype=np.complex64)[None]
    pdus = [abi.make_pdu(slot_index=3 + i, rnti=0x4321, n_id=11 + i, bwp_size_rb=nprb, qm=qm, dmrs_symbols=dmrs, prb_start=0,
                         prb_count=nprb, nof_symbols=14, base_graph=bg, tb_size_bytes=tb_bits // 8, scrambling_id=100 + i,
                         n_scid=i % 2, nof_cdm_groups_without_data=2, ratio_dmrs_dB=-3.0, ratio_data_dB=0.0, precoding=prec)
            for i in range(slots)]
    d = lib.derive(pdus[0])
    G, tb_size = d["codeword_bits"], pdus[0].tb_size_bytes
    tb_stride = (tb_size + 3) & ~3
    rng = np.random.default_rng(1000 * qm + 10 * layers + ports)
    d_tb = dev(rng.integers(0, 256, (slots, tb_stride), dtype=np.uint8))
    plan = lib.PdschPlan(ctx, pdus, [i * tb_stride for i in range(slots)], list(range(slots)), slots, layers, nsubc)
    d_txgrid = torch.zeros((slots, layers, 14, nsubc), dtype=torch.int32, device="cuda")
    plan.run(d_tb.reshape(-1), d_txgrid)
    ctx.synchronize()
    plan.close()
    tx = model.from_cbf16(d_txgrid.cpu().numpy().view(np.uint32)).astype(np.complex128)  # [slot][layer][14][subc]
    # two paths per (port, layer), a common delay of a few samples at 4096 x SCS, a CFO of a few hundred Hz
    k = np.arange(nsubc)
    H = np.zeros((ports, layers, nsubc), np.complex128)
    for p in range(ports):
        for l in range(layers):
            g = (1.0 if (p % layers) == l else 0.35) * np.exp(1j * rng.uniform(0, 2 * np.pi))
            H[p, l] = g * np.exp(-2j * np.pi * k * 3 / 4096.0) * (1 + 0.3 * np.exp(-2j * np.pi * k * rng.uniform(1, 8) / 4096.0))
    ep = np.array(model.epochs(0), np.float64)
    rot = np.exp(2j * np.pi * (250.0 / 15000.0) * ep)
    clean = np.einsum("plk,slmk->spmk", H, tx) * rot[None, None, :, None]
    chest = [abi.make_pusch_chest(prbs=range(nprb), slot_index=p.slot_index, scrambling_id=p.scrambling_id, n_scid=p.n_scid,
                                  scaling=BETA, dmrs_symbols=dmrs, nof_layers=layers, rx_ports=tuple(range(ports)),
                                  dc_position=nsubc // 2) for p in pdus]
    demod = [abi.make_pusch_demod(prbs=range(nprb), qm=qm, rnti=p.rnti, n_id=p.n_id, dmrs_symbols=dmrs, nof_cdm_groups_without_data=2,
                                  nof_layers=layers, rx_ports=tuple(range(ports)), equalizer=equalizer) for p in pdus]
    assert lib.pusch_demod_codeword_bits(demod[0]) == G
    ce_size = layers * ports * 14 * nsubc
    cplan = lib.PuschChestPlan(ctx, chest, list(range(slots)), slots, ports, nsubc, [i * ce_size for i in range(slots)])
    dplan = lib.PuschDemodPlan(ctx, demod, list(range(slots)), slots, ports, nsubc, [i * ce_size for i in range(slots)])
    cfg_dec = abi.PuschDecoderCfg(bg, qm, 0, layers, d["n_ref"], tb_size, G // qm, 10, 1, 1)
    return dict(clean=clean, G=G, tb_size=tb_size, tb_stride=tb_stride, d_tb=d_tb, cplan=cplan, dplan=dplan, cfg_dec=cfg_dec,
                ce_size=ce_size, slots=slots, rng=rng)


def link_buffers(ctx, L):
    import torch
    soft_bytes, state_bytes, _ = ctx.pusch_decoder_sizes(L["cfg_dec"], L["slots"])
    s = L["slots"]
    return dict(ce=torch.zeros(s * L["ce_size"], dtype=torch.int32, device="cuda"),
                nv=torch.zeros((s, 4), dtype=torch.float32, device="cuda"),
                llr=torch.zeros((s, L["G"]), dtype=torch.int8, device="cuda"),
                soft=torch.zeros((s, soft_bytes), dtype=torch.int8, device="cuda"),
                state=torch.zeros((state_bytes,), dtype=torch.uint8, device="cuda"),
                out=torch.zeros((s, L["tb_stride"]), dtype=torch.uint8, device="cuda"),
                res=torch.zeros((s, 4), dtype=torch.int32, device="cuda"))


def link_run(ctx, L, d_grid, B, stream=None):
    L["cplan"].run(d_grid, B["ce"], B["nv"], None, stream=stream)
    L["dplan"].run(d_grid, B["ce"], B["nv"], B["llr"], L["G"], None, stream=stream)
    ctx.pusch_decode_batch(L["cfg_dec"], L["slots"], B["llr"], L["G"], B["soft"], B["state"], B["out"], L["tb_stride"], B["res"],
                           stream=stream)


def noisy_grid(L, snr_db):
    clean = L["clean"]
    nv = 10.0 ** (-snr_db / 10.0)
    noise = (L["rng"].standard_normal(clean.shape) + 1j * L["rng"].standard_normal(clean.shape)) * np.sqrt(nv / 2)
    return model.to_cbf16((clean + noise).astype(np.complex64))


@pytest.mark.gpu
@pytest.mark.parametrize("qm,rate,snr_db,equalizer,layers,ports", LINK_CASES)
def test_link_from_the_grid_to_transport_blocks(gpu_ctx, oracle, qm, rate, snr_db, equalizer, layers, ports):
    import torch
    L = link_chain(gpu_ctx, oracle, qm, rate, layers, ports, equalizer)
    for good in (True, False):
        d_grid = dev(as_i32(noisy_grid(L, snr_db if good else -12.0)))
        B = link_buffers(gpu_ctx, L)
        link_run(gpu_ctx, L, d_grid, B)
        gpu_ctx.synchronize()
        torch.cuda.synchronize()
        ok = B["res"].cpu().numpy()[:, 0]
        if good:
            assert ok.all(), (ok, B["nv"].cpu().numpy())
            assert torch.equal(B["out"][:, :L["tb_size"]], L["d_tb"][:, :L["tb_size"]])
        else:
            assert not ok.any(), ok
    L["cplan"].close()
    L["dplan"].close()


@pytest.mark.gpu
def test_link_chain_captured_in_one_graph_replays_to_the_same_blocks(gpu_ctx, oracle):
    import torch
    L = link_chain(gpu_ctx, oracle, 4, 616, 2, 4, abi.EQ_ZF)
    d_grid = dev(as_i32(noisy_grid(L, 20.0)))
    B = link_buffers(gpu_ctx, L)
    link_run(gpu_ctx, L, d_grid, B)
    gpu_ctx.synchronize()
    want = B["out"].cpu().numpy().copy()
    assert B["res"].cpu().numpy()[:, 0].all()
    G = link_buffers(gpu_ctx, L)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            link_run(gpu_ctx, L, d_grid, G, stream=C.c_void_p(stream.cuda_stream))
    for _ in range(2):
        G["out"].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(G["out"].cpu().numpy(), want)
        assert G["res"].cpu().numpy()[:, 0].all()
    L["cplan"].close()
    L["dplan"].close()
