"""The low-PAPR DM-RS of a transform-precoded PUSCH in the channel estimator: nrphy_pusch_chest_validate_ex / _plan_create_ex /
_host_ex and nrphy_pusch_lowpapr_sequence_host.

The recording (tests/golden/pusch_lowpapr_reference_*, written by tests/golden/record_pusch_lowpapr_reference.cpp) holds what the
reference's low_papr_sequence_generator_impl generates for every valid number of PRBs but 5, and what its
port_channel_estimator_average_impl answers when it is handed those pilots, laid out as dmrs_pusch_estimator_impl lays out the
Gold ones.

CPU: the PODs, the names, the validator; the generated table file; tests/pusch_lowpapr_model.py (the restatement of
tests/pusch_chest_model.py with the pilot swapped) against every recorded sequence bit for bit and against the recorded estimates.
GPU: the kernel's sequence against the model and the recording, bit for bit; the estimator through a plan and through the host
form against the recording, within the project's device allowances, and against the model (5 PRB included: only the model pins
that size); Gold PUSCHs through the _ex forms and inside a mixed plan, byte for byte what they were; two runs and a graph replay.

The recorded exponential tables hold the C library's single-precision sine and cosine, which are not correctly rounded: with cos and
sin evaluated in double and rounded once, 1478 of the 117,768 recorded components (1.26 %) would be one float32 step away.  The model
and the kernel restate the library's routine instead (pusch_lowpapr_model.libm_sincosf, unit_circle_libm of low_papr_device.h).
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
import pusch_chest_model as chest_model
import pusch_lowpapr_model as model
import test_pusch_channel_estimator as gold

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
CSRC = os.path.join(os.path.dirname(os.path.abspath(backends.pkg.__file__)), "csrc")
RES, MEAS_DTYPE, SENTINEL, FIGURES = gold.RES, gold.MEAS_DTYPE, gold.SENTINEL, gold.FIGURES
NEW_SYMBOLS = ["nrphy_pusch_chest_validate_ex", "nrphy_pusch_chest_plan_create_ex", "nrphy_pusch_chest_host_ex",
               "nrphy_pusch_lowpapr_sequence_host"]
BETA = gold.BETA  # what the processor hands down: two CDM groups without data


def lp(n_rs_id, enabled=1):
    return abi.PuschChestLowpapr(enabled, n_rs_id)


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_pod_and_names():
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu\n", sizeof(nrphy_pusch_chest_lowpapr_t), offsetof(nrphy_pusch_chest_lowpapr_t, enabled),
 offsetof(nrphy_pusch_chest_lowpapr_t, n_rs_id));return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()
    P = abi.PuschChestLowpapr
    assert [int(x) for x in out] == [C.sizeof(P), P.enabled.offset, P.n_rs_id.offset] == [8, 0, 4]
    header = open(os.path.join(backends.ROOT, "include", "mi355_nrphy.h")).read()
    handle = lib.load()
    for name in NEW_SYMBOLS:
        assert name in abi.ABI_SYMBOLS and name + "(" in header and hasattr(handle, name), name
        assert not [s for s in ("_pusch_proc_", "_pusch_csi2_", "_ul_slot", "_srs_", "_uci_", "_ulsch_", "_pf2_", "pucch") if s in name]
    assert "comes from the caller" not in header and "M_zc = 30 (5 PRB) is ours and not the reference's" in header


def _base(**kw):
    args = dict(prbs=range(10, 30), numerology=1, slot_index=7, scrambling_id=500, n_scid=0, scaling=1.4125, dmrs_symbols=(2, 11),
                start_symbol=0, nof_symbols=14, nof_layers=1, rx_ports=(0, 1, 2, 3), dc_position=300)
    args.update(kw)
    return abi.make_pusch_chest(**args)


@pytest.mark.parametrize("name,cfg,desc,want", [
    ("base", _base(), lp(1007), abi.OK),
    ("no description", _base(), None, abi.OK),
    ("disabled", _base(nof_layers=2, n_scid=1, prbs=range(10, 17)), lp(5000, 0), abi.OK),  # then nothing of it is read
    ("270 PRB", _base(prbs=range(270), dc_position=None), lp(0), abi.OK),
    ("scrambling_id is ignored", _base(scrambling_id=65535), lp(3), abi.OK),
    ("two layers", _base(nof_layers=2), lp(3), abi.ERR_ARGUMENT),
    ("n_scid 1", _base(n_scid=1), lp(3), abi.ERR_ARGUMENT),
    ("n_rs_id 1008", _base(), lp(1008), abi.ERR_ARGUMENT),
    ("7 PRB", _base(prbs=range(10, 17)), lp(3), abi.ERR_ARGUMENT),
    ("273 PRB", _base(prbs=range(273), dc_position=None), lp(3), abi.ERR_ARGUMENT),
    ("enabled 2", _base(), lp(3, 2), abi.ERR_ARGUMENT),
    ("what the plain validator refuses", _base(dmrs_type=2), lp(3), abi.ERR_ARGUMENT),
])
def test_validator(name, cfg, desc, want):
    assert lib.pusch_chest_validate_ex(cfg, desc, 4, 3276) == want, name
    if desc is None or desc.enabled == 0:
        assert lib.pusch_chest_validate(cfg, 4, 3276) == want, name


def test_generated_tables_are_the_generator_s_output():
    sys.path.insert(0, os.path.join(backends.ROOT, "profiles"))
    try:
        import gen_pusch_lowpapr_tables as gen
    finally:
        sys.path.pop(0)
    assert open(os.path.join(CSRC, "pusch_lowpapr_tables.inc")).read() == gen.render()
    t = json.load(open(os.path.join(GOLDEN, "pusch_lowpapr_tables.json")))
    for key, length in (("phi_6", 6), ("phi_18", 18)):
        assert len(t[key]) == 30 and all(len(r) == length and set(r) <= {-3, -1, 1, 3} for r in t[key])


# ---- the recording ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recorded_sequences():
    """{(nof_prb, u): complex64 [6 nof_prb]} for u = 0, 29 of every valid size but 5, and {(nof_prb, u)} for u < 30 of 1 .. 4 PRB."""
    s = np.load(os.path.join(GOLDEN, "pusch_lowpapr_reference_sequences.npy"))
    s.setflags(write=False)
    pair, table, at = {}, {}, 0
    for n in model.VALID_NOF_PRB:
        if n == 5:
            continue
        for u in (0, 29):
            pair[n, u], at = s[at:at + 6 * n], at + 6 * n
    for n in (1, 2, 3, 4):
        for u in range(30):
            table[n, u], at = s[at:at + 6 * n], at + 6 * n
    assert at == s.size
    return pair, table


@functools.lru_cache(maxsize=None)
def recording():
    """The recorded cases in the layout of test_pusch_channel_estimator.recording(), one layer each."""
    cases = json.load(open(os.path.join(GOLDEN, "pusch_lowpapr_reference_cases.json")))
    data = {k: np.load(os.path.join(GOLDEN, "pusch_lowpapr_reference_%s.npy" % k)) for k in ("grids", "pilots", "estimates", "results")}
    for a in data.values():
        a.setflags(write=False)
    out = []
    for c in cases:
        P, nprb, nd, ns = len(c["rx_ports"]), len(c["prbs"]), len(c["dmrs_symbols"]), c["nof_symbols"]
        c = dict(c, nof_tx_layers=1)
        c["cfg"] = abi.make_pusch_chest(prbs=c["prbs"], numerology=c["numerology"], scaling=c["scaling"], dmrs_symbols=c["dmrs_symbols"],
                                        start_symbol=c["first_symbol"], nof_symbols=ns, rx_ports=c["rx_ports"],
                                        dc_position=None if c["dc"] < 0 else c["dc"])
        c["lp"] = lp(c["n_rs_id"])
        c["subc"] = (12 * np.array(c["prbs"])[:, None] + np.arange(12)).ravel()
        c["rows"] = data["grids"][c["grid_off"]:c["grid_off"] + P * nd * 12 * nprb].reshape(P, nd, 12 * nprb)
        c["pilots"] = data["pilots"][c["pilot_off"]:c["pilot_off"] + P * 6 * nprb].reshape(P, 1, 6 * nprb)
        c["est"] = data["estimates"][c["est_off"]:c["est_off"] + P * ns * 12 * nprb].reshape(1, P, ns, 12 * nprb)
        c["res"] = data["results"][c["res_row"]:c["res_row"] + P].reshape(P, 1, len(RES))
        out.append(c)
    return out, {k: a.size for k, a in data.items()}


def test_recording_is_consistent():
    cases, sizes = recording()
    for k in ("cases.json", "grids.npy", "pilots.npy", "estimates.npy", "results.npy", "sequences.npy"):
        assert os.path.getsize(os.path.join(GOLDEN, "pusch_lowpapr_reference_" + k)) < gold.SIZE_CAP, k
    at = {"grid_off": 0, "pilot_off": 0, "est_off": 0, "res_row": 0}
    for c in cases:
        P, nprb, nd, ns = len(c["rx_ports"]), len(c["prbs"]), len(c["dmrs_symbols"]), c["nof_symbols"]
        assert {k: c[k] for k in at} == at, c["name"]
        at = {"grid_off": at["grid_off"] + P * nd * 12 * nprb, "pilot_off": at["pilot_off"] + P * 6 * nprb,
              "est_off": at["est_off"] + P * ns * 12 * nprb, "res_row": at["res_row"] + P}
        assert lib.pusch_chest_validate_ex(c["cfg"], c["lp"], max(c["rx_ports"]) + 1, 12 * c["grid_prb"]) == abi.OK, c["name"]
        # the lead the recorder asked for (TA_MARGIN's rule), and that every port has it: no recorded time alignment is a near tie
        k = c["subc"][0::2].astype(np.float64)
        asked = min(gold.TA_MARGIN, 0.5 * (2 * np.pi / 4096) ** 2 * k.var())
        for r in c["res"].reshape(-1, len(RES)):
            r = dict(zip(RES, r))
            assert r["ta_asked"] == pytest.approx(asked, rel=1e-12) and r["ta_best"] - r["ta_second"] >= asked * r["ta_best"], c["name"]
            assert np.isnan(r["cfo_hz"]) == (nd == 1) and r["noise_var"] > 0 and r["epre"] > 0
    assert (at["grid_off"], at["pilot_off"], at["est_off"], at["res_row"] * len(RES)) == \
        (sizes["grids"], sizes["pilots"], sizes["estimates"], sizes["results"])
    # the cases the sequence and the kernel branch on
    assert {1, 2, 3, 4, 6, 8, 25, 270} <= {len(c["prbs"]) for c in cases}
    assert {0, 29, 30, 1007} <= {c["n_rs_id"] for c in cases}
    assert {len(c["dmrs_symbols"]) for c in cases} == {1, 2, 3, 4} and {len(c["rx_ports"]) for c in cases} == {1, 2, 3, 4}
    assert any(c["prbs"][-1] - c["prbs"][0] + 1 != len(c["prbs"]) for c in cases)
    assert any(c["dc"] >= 0 and c["dc"] // 12 in c["prbs"] for c in cases)
    pair, table = recorded_sequences()
    assert len(pair) == 2 * 52 and len(table) == 120


def ulps(a, b):
    """Distance in float32 steps per component between complex64 arrays of equal signs."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_model_gives_every_recorded_sequence_bit_for_bit():
    pair, table = recorded_sequences()
    for (n, u), want in list(pair.items()) + list(table.items()):
        assert np.array_equal(model.sequence(u, n).view(np.uint32), want.view(np.uint32)), (n, u)
    assert np.array_equal(model.sequence(30 + 29, 6), model.sequence(29, 6)) and np.array_equal(model.sequence(1007, 6), model.sequence(17, 6))


def test_recorded_tables_are_not_correctly_rounded():
    """Why the model restates the C library's sincosf: cos and sin in float64 rounded once (the SRS model's circle) are within one
    float32 step of every recorded component and differ from 1478 of them."""
    pair, table = recorded_sequences()
    differ = total = 0
    for (n, u), want in list(pair.items()) + list(table.items()):
        idx, size = model.indices(u, n)
        d = ulps(model.srs_model.unit_circle(size)[idx], want)
        assert d.max() <= 1, (n, u)
        differ, total = differ + int((d > 0).sum()), total + d.size
    print("components one step from the double-rounded circle: %d of %d" % (differ, total))
    assert (differ, total) == (1478, 117768)


def test_phi_tables_are_what_the_recorded_sequences_imply():
    """phi(n) = the recorded element's angle in units of pi / 4, for the two new tables and for the two the library had."""
    _, table = recorded_sequences()
    for n in (1, 2, 3, 4):
        for u in range(30):
            k = np.rint(np.angle(table[n, u].astype(np.complex128)) / (np.pi / 4)).astype(int)
            assert np.abs(table[n, u] - np.exp(1j * np.pi * k / 4)).max() < 1e-6
            assert list(k) == model.phi_tables()[6 * n][u], (n, u)


def test_length_30_closed_form():
    """The size that is ours (the reference's generator terminates on it): unit modulus, the index law
    (62 - ((u + 1)(n + 1)(n + 2) mod 62)) mod 62 on the 62-point circle, and the closed form exp(-j pi (u + 1)(n + 1)(n + 2) / 31)."""
    for u in (0, 17, 29):
        idx, size = model.indices(u, 5)
        n = np.arange(30)
        assert size == 62 and np.array_equal(idx, (62 - ((u + 1) * (n + 1) * (n + 2)) % 62) % 62)
        s = model.sequence(u, 5).astype(np.complex128)
        assert np.abs(np.abs(s) - 1).max() < 2e-7
        assert np.abs(s - np.exp(-1j * np.pi * (u + 1) * (n + 1) * (n + 2) / 31)).max() < 1e-6


# The largest distances, over the recorded cases, between the reference's answers and the restatement's (the figures of
# tests/test_pusch_channel_estimator.py, which says what each is); test_restatement_equals_the_recording measures and prints them
# on every run.  The device may be REF_CE_STEPS + 1 and REF_CE_WORD_STEPS + 1 steps from the recording, differ in 8 x REF_CE_SHARE
# of a case's components and be 8 x the other spreads away: the project's rule.
REF_PILOT_SPREAD = 3.8e-7  # measured 3.72e-07: 3 PRB (length 18), 3 DM-RS, n_rs_id 30, 3 ports
REF_CE_STEPS = 1           # measured 1: 25 PRB, DC in the middle, n_rs_id 1007, 2 ports
REF_CE_WORD_STEPS = 4.9e-4 # measured 4.88e-04: 270 PRB, 2 DM-RS, n_rs_id 29
REF_CE_SHARE = 6.0e-5      # measured 5.95e-05: 25 PRB, DC in the middle, n_rs_id 1007, 2 ports (1 component of 16800)
REF_NOISE_SPREAD = 3.4e-7  # measured 3.36e-07: 3 PRB (length 18), 3 DM-RS, n_rs_id 30, 3 ports
REF_RSRP_SPREAD = 1.6e-7   # measured 1.54e-07: 4 PRB (length 24), 4 DM-RS, mu 1, n_rs_id 1007
REF_EPRE_SPREAD = 3.7e-7   # measured 3.67e-07: 270 PRB, 2 DM-RS, n_rs_id 29
REF_SNR_SPREAD = 4.1e-7    # measured 4.04e-07: 3 PRB (length 18), 3 DM-RS, n_rs_id 30, 3 ports
REF_CFO_SPREAD = 1.9e-7    # measured 1.84e-07: 3 PRB (length 18), 3 DM-RS, n_rs_id 30, 3 ports
REF_SPREADS = {"noise_var": REF_NOISE_SPREAD, "rsrp": REF_RSRP_SPREAD, "epre": REF_EPRE_SPREAD, "snr": REF_SNR_SPREAD,
               "cfo_hz": REF_CFO_SPREAD}


def recorded_grid(c, nports, nsubc):
    return gold.recorded_grid(c, nports, nsubc)


@functools.lru_cache(maxsize=None)
def restatement(i):
    c = recording()[0][i]
    return model.estimate(c["cfg"], c["n_rs_id"], recorded_grid(c, max(c["rx_ports"]) + 1, 12 * c["grid_prb"]))


def test_restatement_equals_the_recording():
    cases, _ = recording()
    worst, where = dict.fromkeys(("pilots",) + FIGURES, 0), {}
    for i, c in enumerate(cases):
        ce, nv, meas = restatement(i)
        fig = gold.distances_from_the_recording(c, ce, nv, meas)
        rms = np.sqrt(np.mean(np.abs(c["pilots"].astype(np.complex128)) ** 2))
        fig["pilots"] = max(np.abs(meas[p][0]["smoothed"].astype(np.complex128) - c["pilots"][p, 0]).max() / rms
                            for p in range(len(c["rx_ports"])))
        for k in worst:
            if fig[k] > worst[k]:
                worst[k], where[k] = fig[k], c["name"]
    print("recording - restatement: " + gold.allowance_line(worst, where))
    print("constants: pilots %.3g, steps %d, word_steps %.3g, share %.3g, %s" %
          (REF_PILOT_SPREAD, REF_CE_STEPS, REF_CE_WORD_STEPS, REF_CE_SHARE, ", ".join("%s %.3g" % kv for kv in REF_SPREADS.items())))
    assert worst["pilots"] <= 1e-5 and worst["word_steps"] <= 2  # beyond float32 rounding: a finding, not a constant
    assert worst["pilots"] <= REF_PILOT_SPREAD and worst["steps"] <= REF_CE_STEPS and worst["word_steps"] <= REF_CE_WORD_STEPS
    assert worst["share"] <= REF_CE_SHARE
    for k, v in REF_SPREADS.items():
        assert worst[k] <= v, (k, worst[k], where[k])


# =======================================================================================================================
# GPU
# =======================================================================================================================
dev, as_i32 = chest_model.dev, chest_model.as_i32


def run_plan(ctx, cfgs, lps, grids, grid_index, nports, nsubc, ex=True):
    """test_pusch_channel_estimator.run_plan through nrphy_pusch_chest_plan_create_ex (ex = False: the plain creation call)."""
    import torch
    sizes = [c.nof_tx_layers * c.nof_rx_ports * 14 * nsubc for c in cfgs]
    offs = [int(o) for o in np.cumsum([0] + sizes)[:-1]]
    plan = lib.PuschChestPlan(ctx, cfgs, grid_index, len(grids), nports, nsubc, offs, lowpapr=lps, ex=ex)
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


@functools.lru_cache(maxsize=None)
def device_sequences(ctx):
    return {(n, u): ctx.pusch_lowpapr_sequence_host(u + (30 if u == 17 else 0), n) for n in model.VALID_NOF_PRB for u in (0, 17, 29)}


@pytest.mark.gpu
def test_sequence_equals_the_model(gpu_ctx):
    """All 53 sizes, u = 0, 17 (as n_rs_id 47) and 29, bit for bit."""
    for (n, u), got in device_sequences(gpu_ctx).items():
        assert np.array_equal(got.view(np.uint32), model.sequence(u, n).view(np.uint32)), (n, u)
    assert len(model.VALID_NOF_PRB) == 53


@pytest.mark.gpu
def test_sequence_equals_the_recording_bit_for_bit(gpu_ctx):
    pair, _ = recorded_sequences()
    dev_seq = device_sequences(gpu_ctx)
    for key, want in pair.items():
        assert np.array_equal(dev_seq[key].view(np.uint32), want.view(np.uint32)), key


@pytest.mark.gpu
def test_sequence_host_refusals(gpu_ctx):
    h = lib.load().nrphy_pusch_lowpapr_sequence_host
    out = np.zeros(12 * 7, np.float32)
    assert int(h(gpu_ctx.handle, 0, 7, out.ctypes.data)) == abi.ERR_ARGUMENT and int(h(gpu_ctx.handle, 1008, 6, out.ctypes.data)) == abi.ERR_ARGUMENT


def check_against_the_recording(c, ce, nv, meas, nsubc, worst, where):
    """test_pusch_channel_estimator.check_against_the_recording with this file's constants."""
    fig = gold.distances_from_the_recording(c, ce, nv, meas)
    assert (ce[:, :, ~gold.region(c["cfg"], nsubc)] == SENTINEL).all(), (c["name"], "outside the region")
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
    """Every recorded case in two plans: the grids of up to 52 PRB as 4 ports x 624 subcarriers, the wide one as 1 x 3276."""
    cases, _ = recording()
    worst, where = dict.fromkeys(FIGURES, 0), {}
    for nports, nsubc, group in ((4, 624, [c for c in cases if c["grid_prb"] <= 52]), (1, 3276, [c for c in cases if c["grid_prb"] > 52])):
        ces, nv, meas = run_plan(gpu_ctx, [c["cfg"] for c in group], [c["lp"] for c in group],
                                 [recorded_grid(c, nports, nsubc) for c in group], list(range(len(group))), nports, nsubc)
        for i, c in enumerate(group):
            check_against_the_recording(c, ces[i], nv[i], meas[i], nsubc, worst, where)
            assert (nv[i, len(c["rx_ports"]):] == -1.0).all()
    print("device - recording: " + gold.allowance_line(worst, where) + "; allowed: " + device_allowances())


@pytest.mark.gpu
def test_host_call_equals_the_recording(gpu_ctx):
    cases, _ = recording()
    worst, where = dict.fromkeys(FIGURES, 0), {}
    for c in cases:
        nports, nsubc = max(c["rx_ports"]) + 1, 12 * c["grid_prb"]
        sentinel = np.full((1, len(c["rx_ports"]), 14, nsubc), SENTINEL, np.uint32)
        ce, nv, m = gpu_ctx.pusch_chest_host(c["cfg"], recorded_grid(c, nports, nsubc), sentinel, lowpapr=c["lp"])
        meas = [[np.frombuffer(bytes(m[p][0]), MEAS_DTYPE)[0]] for p in range(len(c["rx_ports"]))]
        check_against_the_recording(c, ce, nv, meas, nsubc, worst, where)
    print("host call - recording: " + gold.allowance_line(worst, where) + "; allowed: " + device_allowances())


def parity_cases():
    b = abi.make_pusch_chest
    return [  # name, configuration, n_rs_id, grid ports, grid subcarriers
        ("1 PRB, 1 DM-RS", b(prbs=[7], dmrs_symbols=(2,), rx_ports=(0,)), 0, 1, 624),
        ("2 PRB, 2 ports", b(prbs=[10, 11], dmrs_symbols=(2, 11), rx_ports=(1, 0), scaling=BETA), 29, 2, 624),
        ("3 PRB, mu 1", b(prbs=[20, 21, 22], numerology=1, slot_index=13, dmrs_symbols=(3, 8), start_symbol=1, nof_symbols=13,
                          rx_ports=(0, 1, 2), scaling=BETA), 30, 3, 624),
        ("4 PRB, 4 DM-RS", b(prbs=range(30, 34), dmrs_symbols=(2, 5, 8, 11), rx_ports=(3, 1, 0, 2), scaling=BETA), 1007, 4, 624),
        ("5 PRB: the size that is ours", b(prbs=range(8, 13), dmrs_symbols=(2, 11), rx_ports=(0, 1), scaling=BETA, dc_position=125),
         777, 2, 624),
        ("6 PRB", b(prbs=range(3, 9), dmrs_symbols=(2, 7, 11), rx_ports=(0,), scaling=BETA), 17, 1, 624),
        ("non-contiguous 45 PRB, DC", b(prbs=list(range(3, 23)) + list(range(25, 50)), dmrs_symbols=(2, 11), scaling=BETA,
                                        rx_ports=(1, 0), dc_position=306), 400, 2, 624),
        ("270 PRB, 2 ports, DC", b(prbs=range(3, 273), dmrs_symbols=(2, 7, 11), scaling=BETA, rx_ports=(0, 1), dc_position=1638),
         1006, 2, 3276),
    ]


@pytest.mark.gpu
def test_parity_with_the_restatement(gpu_ctx):
    rng = np.random.default_rng(2026)
    for i, (what, cfg, n_rs_id, nports, nsubc) in enumerate(parity_cases()):
        with model.pilot_swapped(n_rs_id):  # the transmitter and the check read the pilots through pusch_chest_model
            grid = gold.synthetic_grid(rng, cfg, nports, nsubc, snr_db=15.0 + 5 * (i % 3), delay=float(i % 5) - 2.0,
                                       cfo_hz=100.0 * ((i % 7) - 3))
            (ce,), nv, meas = run_plan(gpu_ctx, [cfg], [lp(n_rs_id)], [grid], [0], nports, nsubc)
            gold.check_parity(cfg, grid, ce, nv[0], meas[0], nsubc, what)


@pytest.mark.gpu
def test_gold_puschs_keep_their_bytes(gpu_ctx):
    """The _ex creation call without descriptions and with every one disabled, and a mixed plan: the Gold PUSCHs give the bytes of
    nrphy_pusch_chest_plan_create on the same grids; the low-PAPR PUSCHs of the mixed plan give the bytes of a plan of their own."""
    rng = np.random.default_rng(77)
    cfgs = gold.batch_cases()
    grids = [gold.synthetic_grid(rng, c, 2, 624, snr_db=18.0) for c in cfgs[:2]]
    gidx = [0, 1, 1, 0]
    want = gold.run_plan(gpu_ctx, cfgs, grids, gidx, 2, 624)
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1].tobytes() == b[1].tobytes() and \
        a[2].tobytes() == b[2].tobytes()
    assert same(run_plan(gpu_ctx, cfgs, None, grids, gidx, 2, 624), want)
    assert same(run_plan(gpu_ctx, cfgs, [lp(900 + i, 0) for i in range(4)], grids, gidx, 2, 624), want)
    # mixed: low-PAPR PUSCHs between the Gold ones, so that the plan's job order is not the PUSCHs' order
    tp = [abi.make_pusch_chest(prbs=range(4, 10), dmrs_symbols=(2, 11), rx_ports=(1, 0), scaling=BETA),
          abi.make_pusch_chest(prbs=range(20, 45), dmrs_symbols=(2, 7, 11), rx_ports=(0,), scaling=BETA, dc_position=300)]
    mixed = [cfgs[0], tp[0], cfgs[1], cfgs[2], tp[1], cfgs[3]]
    lps = [lp(0, 0), lp(33), lp(0, 0), lp(0, 0), lp(1007), lp(0, 0)]
    midx = [0, 1, 1, 1, 0, 0]
    ces, nv, meas = run_plan(gpu_ctx, mixed, lps, grids, midx, 2, 624)
    for j, i in enumerate((0, 2, 3, 5)):
        assert np.array_equal(ces[i], want[0][j]) and nv[i].tobytes() == want[1][j].tobytes() and meas[i].tobytes() == want[2][j].tobytes(), i
    alone = run_plan(gpu_ctx, tp, [lps[1], lps[4]], grids, [1, 0], 2, 624)
    for j, i in enumerate((1, 4)):
        assert np.array_equal(ces[i], alone[0][j]) and nv[i].tobytes() == alone[1][j].tobytes() and meas[i].tobytes() == alone[2][j].tobytes(), i
    # the host form without a description
    c = cfgs[0]
    sentinel = np.full((c.nof_tx_layers, c.nof_rx_ports, 14, 624), SENTINEL, np.uint32)
    a, b = gpu_ctx.pusch_chest_host(c, grids[0], sentinel), gpu_ctx.pusch_chest_host(c, grids[0], sentinel, ex=True)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and all(bytes(x) == bytes(y) for r, s in zip(a[2], b[2]) for x, y in zip(r, s))


@pytest.mark.gpu
def test_two_runs_and_a_graph_replay_give_identical_bits(gpu_ctx):
    import torch
    rng = np.random.default_rng(5)
    cfgs = [abi.make_pusch_chest(prbs=range(4, 10), dmrs_symbols=(2, 11), rx_ports=(1, 0), scaling=BETA),
            gold.batch_cases()[0],
            abi.make_pusch_chest(prbs=range(20, 45), dmrs_symbols=(2, 7, 11), rx_ports=(0,), scaling=BETA, dc_position=300)]
    lps = [lp(33), lp(0, 0), lp(1007)]
    with model.pilot_swapped(33):
        grid = gold.synthetic_grid(rng, cfgs[0], 2, 624)
    sizes = [c.nof_tx_layers * c.nof_rx_ports * 14 * 624 for c in cfgs]
    offs = [int(o) for o in np.cumsum([0] + sizes)[:-1]]
    plan = lib.PuschChestPlan(gpu_ctx, cfgs, [0] * len(cfgs), 1, 2, 624, offs, lowpapr=lps)
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
    assert outs[0][0].any()
    g_ce = torch.zeros(sum(sizes), dtype=torch.int32, device="cuda")
    g_nv = torch.zeros((len(cfgs), 4), dtype=torch.float32, device="cuda")
    g_meas = torch.zeros((len(cfgs), 4, 2, 32), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.run(d_grid, g_ce, g_nv, g_meas, stream=C.c_void_p(stream.cuda_stream))
    g_ce.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(g_ce.cpu().numpy(), outs[0][0])
    assert np.array_equal(g_nv.cpu().numpy().view(np.uint32), outs[0][1])
    assert np.array_equal(g_meas.cpu().numpy(), outs[0][2])
    plan.close()
