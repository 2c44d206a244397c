"""PUSCH demodulator with transform precoding and pi/2-BPSK (the _ex forms of nrphy_pusch_demod_*).

CPU: the validator with a feature mask over the reference unit test's 50 configurations and its refusals, the ABI's layout, and
the condition the recording (tests/golden/pusch_tp_reference_*, written by tests/golden/record_pusch_tp_reference.cpp from the
reference's pusch_demodulator_impl) has to meet for the comparison below to mean something.
GPU: the fused kernel against the composed path (RE in NumPy -> nrphy_channel_equalize -> nrphy_transform_deprecode ->
nrphy_demodulate_soft per OFDM symbol -> nrphy_llr_descramble) byte for byte, and against the recording: the equaliser's output
as the existing equaliser test compares it, the deprecoded symbols within 4 x the single-precision bound of their size
(tests/golden/pusch_tp_dft_bounds.json) x the symbol's input RMS, and the soft bits -- equal where the pinned demapper gives one
value all around the recorded symbol ("firm"), inside the span of those values (+-1) elsewhere; a launch that mixes the small
shapes and two plain PUSCHs; repeatability and graph replay.
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
import pusch_tp_model as model
from pusch_chest_model import as_i32, dev, gold

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
QM = {"PI_2_BPSK": 1, "QPSK": 2, "QAM16": 4, "QAM64": 6, "QAM256": 8}
BOTH = abi.PUSCH_DEMOD_TRANSFORM_PRECODING | abi.PUSCH_DEMOD_PI2_BPSK
MAX_NOT_FIRM = 0.05


def reference_configs():
    return json.load(open(os.path.join(GOLDEN, "pusch_demodulator_configs.json")))


def cfg_from_fixture(f, equalizer=abi.EQ_ZF):
    return abi.make_pusch_demod(prbs=f["rb_mask"], qm=QM[f["modulation"]], rnti=f["rnti"], n_id=f["n_id"],
                                start_symbol=f["start_symbol_index"], nof_symbols=f["nof_symbols"], dmrs_symbols=f["dmrs_symbols"],
                                dmrs_type=f["dmrs_type"], nof_cdm_groups_without_data=f["nof_cdm_groups_without_data"],
                                nof_layers=f["nof_tx_layers"], rx_ports=f["rx_ports"], equalizer=equalizer,
                                transform_precoding=int(f["transform_precoding"]))


# ---- the recording --------------------------------------------------------------------------------------------------------
class Recorded:
    """One case of the recording: its configuration, its inputs laid out as the library reads them, and what the reference's
    equaliser, deprecoder and demodulator gave per OFDM symbol with data."""

    def __init__(self, row, blobs, nports=None, nsubc=None):
        self.row = row
        self.cfg = abi.make_pusch_demod(prbs=row["prbs"], qm=row["qm"], rnti=row["rnti"], n_id=row["n_id"],
                                        start_symbol=row["start_symbol_index"], nof_symbols=row["nof_symbols"],
                                        dmrs_symbols=row["dmrs_symbols"], dmrs_type=row["dmrs_type"],
                                        nof_cdm_groups_without_data=row["nof_cdm_groups_without_data"],
                                        nof_layers=row["nof_tx_layers"], rx_ports=row["rx_ports"], equalizer=row["equalizer"],
                                        transform_precoding=row["transform_precoding"])
        self.tp = bool(row["transform_precoding"])
        self.nports = nports or max(row["rx_ports"]) + 1
        self.nsubc = nsubc or 12 * (max(row["prbs"]) + 1)
        P, L, nsym, nsc = len(row["rx_ports"]), row["nof_tx_layers"], row["nof_symbols"], 12 * len(row["prbs"])
        subc = np.array([12 * p + k for p in row["prbs"] for k in range(12)])
        syms = np.arange(row["start_symbol_index"], row["start_symbol_index"] + nsym)
        g = blobs["grids"][row["grid_off"]: row["grid_off"] + P * nsym * nsc].reshape(P, nsym, nsc)
        c = blobs["ce"][row["ce_off"]: row["ce_off"] + L * P * nsc].reshape(L, P, nsc)
        self.grid = np.zeros((self.nports, 14, self.nsubc), np.uint32)
        self.ce = np.zeros((L, P, 14, self.nsubc), np.uint32)
        for i, port in enumerate(row["rx_ports"]):
            self.grid[port][np.ix_(syms, subc)] = g[i]
        self.ce[:, :, syms[:, None], subc[None, :]] = c[:, :, None, :]
        self.noise_vars = np.zeros(abi.MAX_PORTS, np.float32)
        self.noise_vars[:P] = row["noise_vars"]
        self.llr = blobs["llr"][row["llr_off"]: row["llr_off"] + row["nof_bits"]]
        self.sinr = float(row["sinr_db"])
        self.eq, self.nvar, self.z = [], [], []  # per OFDM symbol with data
        at, zat = row["eq_off"], row["z_off"]
        for l in range(14):
            n = model.data_subcarriers(self.cfg, l).size * L
            if n == 0:
                continue
            self.eq.append(blobs["eq"][at: at + n])
            self.nvar.append(blobs["nvar"][at: at + n])
            self.z.append(blobs["z"][zat: zat + n] if self.tp else self.eq[-1])
            at, zat = at + n, zat + n
        assert sum(e.size for e in self.eq) * row["qm"] == row["nof_bits"]


@functools.lru_cache(maxsize=None)
def recording():
    load = lambda name: np.load(os.path.join(GOLDEN, "pusch_tp_reference_%s.npy" % name))
    blobs = {k: load(k) for k in ("grids", "ce", "nvar", "llr")}
    blobs["eq"] = load("eq").view(np.complex64).reshape(-1)
    blobs["z"] = load("z").view(np.complex64).reshape(-1)
    rows = json.load(open(os.path.join(GOLDEN, "pusch_tp_reference_cases.json")))
    return rows, blobs


SMALL_PORTS, SMALL_SUBC = 4, 273 * 12


def recorded_cases(group):
    rows, blobs = recording()
    dims = dict(nports=SMALL_PORTS, nsubc=SMALL_SUBC) if group == 1 else {}
    return [Recorded(r, blobs, **dims) for r in rows if r["group"] == group]


@functools.lru_cache(maxsize=None)
def dft_bounds():
    return {int(k): v for k, v in json.load(open(os.path.join(GOLDEN, "pusch_tp_dft_bounds.json"))).items()}


def soft_bit_spans(case, demodulate_soft):
    """Per soft bit of a transform-precoded case: the smallest and largest value the pinned demapper gives at the recorded
    deprecoded symbol z and at the four corners z +- d +- jd, descrambled; d = 4 x the size's bound x the RMS of the symbol's
    recorded input.  A bit is firm where the two agree."""
    modulation = 0 if case.cfg.qm == 1 else case.cfg.qm
    bound = dft_bounds()[len(case.row["prbs"])]
    lo, hi = [], []
    for eq, nvar, z in zip(case.eq, case.nvar, case.z):
        d = np.float32(4 * bound * np.sqrt(np.mean(np.abs(eq.astype(np.complex128)) ** 2)))
        five = [demodulate_soft(modulation, (z + np.complex64(complex(a * d, b * d))).astype(np.complex64), nvar).astype(np.int16)
                for a, b in ((0, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))]
        lo.append(np.min(five, axis=0))
        hi.append(np.max(five, axis=0))
    lo, hi = np.concatenate(lo), np.concatenate(hi)
    flip = gold(case.cfg.rnti * 2 ** 15 + case.cfg.n_id, lo.size).astype(bool)
    return np.where(flip, -hi, lo), np.where(flip, -lo, hi)


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_validate_ex_accepts_all_the_reference_configurations():
    configs = reference_configs()
    assert len(configs) == 50
    for f in configs:
        nports, nsubc = max(f["rx_ports"]) + 1, f["nof_rb"] * 12
        for equalizer in (abi.EQ_ZF,) + ((abi.EQ_MMSE,) if f["nof_tx_layers"] == 1 else ()):
            cfg = cfg_from_fixture(f, equalizer)
            assert lib.pusch_demod_validate_ex(cfg, nports, nsubc, BOTH) == abi.OK, f
            assert lib.pusch_demod_validate_ex(cfg, nports, nsubc, 0) == lib.pusch_demod_validate(cfg, nports, nsubc), f
            plain_ok = not f["transform_precoding"] and f["modulation"] != "PI_2_BPSK"
            assert (lib.pusch_demod_validate(cfg, nports, nsubc) == abi.OK) == plain_ok, f


def _tp(**kw):
    args = dict(prbs=range(10, 30), qm=4, dmrs_symbols=(2, 11), dmrs_type=1, nof_cdm_groups_without_data=2, nof_layers=1,
                rx_ports=(0, 1), transform_precoding=1)
    args.update(kw)
    return abi.make_pusch_demod(**args)


@pytest.mark.parametrize("name,kw,features,want", [
    ("transform precoding", {}, BOTH, abi.OK),
    ("the transform bit alone", {}, abi.PUSCH_DEMOD_TRANSFORM_PRECODING, abi.OK),
    ("non-contiguous PRBs", dict(prbs=[3, 4, 9, 40, 41, 51]), BOTH, abi.OK),
    ("270 PRBs", dict(prbs=range(270)), BOTH, abi.OK),
    ("pi/2-BPSK with it", dict(qm=1), BOTH, abi.OK),
    ("pi/2-BPSK without it", dict(qm=1, transform_precoding=0, nof_layers=2, nof_cdm_groups_without_data=1), BOTH, abi.OK),
    ("pi/2-BPSK, the bit alone", dict(qm=1, transform_precoding=0), abi.PUSCH_DEMOD_PI2_BPSK, abi.OK),
    ("2 layers", dict(nof_layers=2), BOTH, abi.ERR_ARGUMENT),
    ("DM-RS type 2", dict(dmrs_type=2), BOTH, abi.ERR_ARGUMENT),
    ("1 CDM group without data", dict(nof_cdm_groups_without_data=1), BOTH, abi.ERR_ARGUMENT),
    ("7 PRBs", dict(prbs=range(7)), BOTH, abi.ERR_ARGUMENT),
    ("11 PRBs", dict(prbs=range(11)), BOTH, abi.ERR_ARGUMENT),
    ("271 PRBs", dict(prbs=range(271)), BOTH, abi.ERR_ARGUMENT),
    ("the transform bit missing", {}, abi.PUSCH_DEMOD_PI2_BPSK, abi.ERR_ARGUMENT),
    ("no bit", {}, 0, abi.ERR_ARGUMENT),
    ("the pi/2-BPSK bit missing", dict(qm=1), abi.PUSCH_DEMOD_TRANSFORM_PRECODING, abi.ERR_ARGUMENT),
    ("transform_precoding = 2", dict(transform_precoding=2), BOTH, abi.ERR_ARGUMENT),
    ("an unknown bit", {}, BOTH | 4, abi.ERR_ARGUMENT),
    ("MMSE with it", dict(equalizer=abi.EQ_MMSE), BOTH, abi.OK),
])
def test_validate_ex(name, kw, features, want):
    assert lib.pusch_demod_validate_ex(_tp(**kw), 4, 273 * 12, features) == want, name


def test_abi_additions_and_the_unmoved_structure():
    protos = r'''#include "mi355_nrphy.h"
int (*a)(const nrphy_pusch_demod_cfg_t*, uint32_t, uint32_t, uint32_t) = nrphy_pusch_demod_validate_ex;
int (*b)(nrphy_ctx_t*, uint32_t, const nrphy_pusch_demod_cfg_t*, const uint32_t*, uint32_t, uint32_t, uint32_t, const uint64_t*,
         uint32_t, nrphy_pusch_demod_plan_t**) = nrphy_pusch_demod_plan_create_ex;
int (*c)(nrphy_ctx_t*, const nrphy_pusch_demod_cfg_t*, const void*, uint32_t, uint32_t, const void*, const float*, uint32_t,
         int8_t*, float*) = nrphy_pusch_demodulate_host_ex;
int (*d)(nrphy_ctx_t*, uint32_t, uint32_t, const float*, float*, void*) = nrphy_transform_deprecode;
int (*e)(nrphy_ctx_t*, uint32_t, const float*, float*) = nrphy_transform_deprecode_host;
int (*f)(uint32_t) = nrphy_transform_precoding_nof_prb_valid;
'''
    sizes = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %u %u\n", sizeof(nrphy_pusch_demod_cfg_t), offsetof(nrphy_pusch_demod_cfg_t, qm),
 offsetof(nrphy_pusch_demod_cfg_t, nof_rx_ports), offsetof(nrphy_pusch_demod_cfg_t, rx_ports),
 offsetof(nrphy_pusch_demod_cfg_t, equalizer), offsetof(nrphy_pusch_demod_cfg_t, transform_precoding),
 offsetof(nrphy_pusch_demod_cfg_t, prb_mask), NRPHY_PUSCH_DEMOD_TRANSFORM_PRECODING, NRPHY_PUSCH_DEMOD_PI2_BPSK);
 return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        include = ["-I", os.path.join(backends.ROOT, "include")]
        open(os.path.join(d, "p.c"), "w").write(protos)  # compiled, not linked: the prototypes are the ones stated here
        subprocess.run(["gcc", "-Werror", "-c", os.path.join(d, "p.c"), "-o", os.path.join(d, "p.o")] + include, check=True, timeout=120)
        open(os.path.join(d, "t.c"), "w").write(sizes)
        subprocess.run(["gcc", os.path.join(d, "t.c"), "-o", os.path.join(d, "t")] + include, check=True, timeout=120)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()
    assert set(abi.ABI_SYMBOLS) >= {"nrphy_pusch_demod_validate_ex", "nrphy_pusch_demod_plan_create_ex", "nrphy_pusch_demodulate_host_ex",
                                    "nrphy_transform_deprecode", "nrphy_transform_deprecode_host",
                                    "nrphy_transform_precoding_nof_prb_valid"}
    # the structure as it was before the _ex forms: 112 bytes, these offsets
    assert [int(x) for x in out] == [112, 8, 36, 40, 56, 60, 72, 1, 2]
    P = abi.PuschDemodCfg
    assert [C.sizeof(P), P.qm.offset, P.nof_rx_ports.offset, P.rx_ports.offset, P.equalizer.offset, P.transform_precoding.offset,
            P.prb_mask.offset] == [112, 8, 36, 40, 56, 60, 72]
    assert (abi.PUSCH_DEMOD_TRANSFORM_PRECODING, abi.PUSCH_DEMOD_PI2_BPSK) == (1, 2)


def test_recording_covers_the_reference_configurations_and_the_small_shapes():
    rows, _ = recording()
    configs = [f for f in reference_configs() if f["transform_precoding"] or f["modulation"] == "PI_2_BPSK"]
    want = [(f["rnti"], f["n_id"], eq) for f in configs for eq in ((0, 1) if f["nof_tx_layers"] == 1 else (0,))]
    assert [(r["rnti"], r["n_id"], r["equalizer"]) for r in rows if r["group"] == 0] == want
    assert sum(1 for r in rows if r["group"] == 0 and r["transform_precoding"]) == 28
    small = [r for r in rows if r["group"] == 1]
    assert {len(r["prbs"]) for r in small if r["transform_precoding"]} >= {1, 5, 25, 27, 270, 6}
    assert {r["qm"] for r in small} >= {1, 8} and {len(r["rx_ports"]) for r in small} == {1, 2, 3, 4}
    assert any(r["rx_ports"] == [2, 0] for r in small) and any(min(r["noise_vars"]) < 0 for r in small)
    assert sum(1 for r in small if not r["transform_precoding"]) == 2
    for r in rows:
        assert lib.pusch_demod_validate_ex(Recorded(r, recording()[1]).cfg, 4, 273 * 12, BOTH) == abi.OK


def test_recording_has_few_soft_bits_that_are_not_firm(oracle):
    """The comparison with the recording is exact on firm soft bits only; at most 5 % of a case's may be anything else."""
    worst = 0.0
    for group in (0, 1):
        for n, case in enumerate(recorded_cases(group)):
            if not case.tp:
                continue
            lo, hi = soft_bit_spans(case, oracle.demodulate_soft)
            assert ((lo <= case.llr) & (case.llr <= hi)).all(), (group, n)  # the pinned demapper at z is the recording
            share = float(np.mean(lo != hi))
            worst = max(worst, share)
            assert share <= MAX_NOT_FIRM, (group, n, share)
    print("largest share of soft bits that are not firm: %.4f" % worst)


# =======================================================================================================================
# GPU
# =======================================================================================================================
def run_plan(ctx, cases, nports, nsubc, features, stream=None, plan=None, buffers=None):
    """One nrphy_pusch_demod_run over the cases, each on a grid of its own: ([soft bits], SINR); 77 fills what nobody writes."""
    import torch
    cfgs = [c.cfg for c in cases]
    ces = [c.ce for c in cases]
    ce_offsets = np.cumsum([0] + [c.size for c in ces])[:-1]
    own = plan is None
    if own:
        plan = lib.PuschDemodPlan(ctx, cfgs, list(range(len(cases))), len(cases), nports, nsubc, [int(o) for o in ce_offsets],
                                  features=features)
    G = [plan.codeword_bits(i) for i in range(len(cfgs))]
    stride = max(G) + 13  # odd stride: rows start at every byte phase
    d_llr = torch.full((len(cfgs) * stride + 64,), 77, dtype=torch.int8, device="cuda")
    d_sinr = torch.zeros(len(cfgs), dtype=torch.float32, device="cuda")
    d_grids = dev(as_i32(np.stack([c.grid for c in cases])))
    d_ces = dev(as_i32(np.concatenate([c.reshape(-1) for c in ces])))
    d_nv = dev(np.stack([c.noise_vars for c in cases]))
    plan.run(d_grids, d_ces, d_nv, d_llr, stride, d_sinr, stream=stream)
    ctx.synchronize()
    out = d_llr.cpu().numpy()
    llrs = [out[i * stride: i * stride + G[i]] for i in range(len(cfgs))]
    for i in range(len(cfgs)):  # nothing outside the codewords is written
        assert (out[i * stride + G[i]: (i + 1) * stride] == 77).all(), i
    assert (out[len(cfgs) * stride:] == 77).all()
    if own:
        plan.close()
    return llrs, d_sinr.cpu().numpy()


def check_against_composed_and_recording(ctx, oracle, case, got, sinr, tag):
    want, want_sinr, eqs, nvs, zs = model.composed(ctx, case.cfg, case.grid, case.ce, case.noise_vars)
    assert np.array_equal(got, want), (tag, int((got != want).sum()))
    assert abs(float(sinr) - want_sinr) < 1e-4 or (np.isinf(sinr) and np.isinf(want_sinr)), (tag, sinr, want_sinr)
    # The reference adds the variances one by one in float32 (pusch_demodulator_impl.cpp:207-217), the device in double: a sum
    # of n positive terms is off by at most n x 2^-24 relative (1.2e-3 dB for the largest case, n = 4800); 1e-5 dB for the
    # division, the logarithm and the rounding of the result to float.
    sinr_tol = 10 * np.log10(1 + sum(e.size for e in case.eq) * 2.0 ** -24) + 1e-5
    assert abs(float(sinr) - case.sinr) <= sinr_tol or (np.isinf(sinr) and np.isinf(case.sinr)), (tag, sinr, case.sinr)
    # The equaliser's output, as test_channel_equalize_matches_the_scalar_loops compares it.
    for pair in (zip(eqs, case.eq), zip(nvs, case.nvar)):
        for ours, theirs in pair:
            special = (theirs == 0) | np.isinf(theirs) | np.isnan(theirs)
            assert np.array_equal(ours[special], theirs[special], equal_nan=True), tag
            err = np.abs(ours[~special] - theirs[~special]) / np.maximum(np.abs(theirs[~special]), 1e-30)
            assert err.size == 0 or err.max() <= 1e-6, (tag, err.max())
    if not case.tp:
        assert np.array_equal(got, case.llr), (tag, int((got != case.llr).sum()))
        return 0.0
    bound = dft_bounds()[len(case.row["prbs"])]
    for z, theirs, eq in zip(zs, case.z, case.eq):
        r = np.sqrt(np.mean(np.abs(eq.astype(np.complex128)) ** 2))
        err = np.abs(z.astype(np.complex128) - theirs.astype(np.complex128)).max()
        assert err <= bound * 4 * r, (tag, err, bound * 4 * r)
    lo, hi = soft_bit_spans(case, oracle.demodulate_soft)
    firm = lo == hi
    assert np.array_equal(got[firm], case.llr[firm]), (tag, int((got[firm] != case.llr[firm]).sum()))
    assert ((got >= lo - 1) & (got <= hi + 1)).all(), tag
    return float(np.mean(~firm))


@pytest.mark.gpu
def test_fused_equals_composed_and_the_recording_on_the_reference_configurations(gpu_ctx, oracle):
    for n, case in enumerate(recorded_cases(0)):
        (got,), sinr = run_plan(gpu_ctx, [case], case.nports, case.nsubc, BOTH)
        check_against_composed_and_recording(gpu_ctx, oracle, case, got, sinr[0], n)
        llr, s = gpu_ctx.pusch_demodulate_host_ex(case.cfg, case.grid, case.ce, case.noise_vars[:case.cfg.nof_rx_ports], BOTH)
        assert np.array_equal(llr, got) and np.float32(s).view(np.uint32) == sinr[0].view(np.uint32), n


@pytest.mark.gpu
def test_small_shapes_in_one_launch(gpu_ctx, oracle):
    cases = recorded_cases(1)
    got, sinr = run_plan(gpu_ctx, cases, SMALL_PORTS, SMALL_SUBC, BOTH)
    for n, case in enumerate(cases):
        check_against_composed_and_recording(gpu_ctx, oracle, case, got[n], sinr[n], n)
    # the plain PUSCHs of the mixed plan: the bytes of a plan of the first contract with the two alone
    plain = [n for n, c in enumerate(cases) if not c.tp and c.cfg.qm != 1]
    assert len(plain) == 2
    alone, alone_sinr = run_plan(gpu_ctx, [cases[n] for n in plain], SMALL_PORTS, SMALL_SUBC, 0)
    for k, n in enumerate(plain):
        assert np.array_equal(alone[k], got[n]), n
        assert alone_sinr[k].view(np.uint32) == sinr[n].view(np.uint32), n


@pytest.mark.gpu
def test_repeatability_and_graph_replay(gpu_ctx):
    import torch
    cases = [c for c in recorded_cases(1) if len(c.row["prbs"]) <= 27]
    ce_offsets = np.cumsum([0] + [c.ce.size for c in cases])[:-1]
    plan = lib.PuschDemodPlan(gpu_ctx, [c.cfg for c in cases], list(range(len(cases))), len(cases), SMALL_PORTS, SMALL_SUBC,
                              [int(o) for o in ce_offsets], features=BOTH)
    first = run_plan(gpu_ctx, cases, SMALL_PORTS, SMALL_SUBC, BOTH, plan=plan)
    second = run_plan(gpu_ctx, cases, SMALL_PORTS, SMALL_SUBC, BOTH, plan=plan)
    for a, b in zip(first[0], second[0]):
        assert np.array_equal(a, b)
    assert np.array_equal(first[1].view(np.uint32), second[1].view(np.uint32))
    G = [plan.codeword_bits(i) for i in range(len(cases))]
    stride = max(G)
    d_grids = dev(as_i32(np.stack([c.grid for c in cases])))
    d_ces = dev(as_i32(np.concatenate([c.ce.reshape(-1) for c in cases])))
    d_nv = dev(np.stack([c.noise_vars for c in cases]))
    g_llr = torch.zeros(len(cases) * stride, dtype=torch.int8, device="cuda")
    g_sinr = torch.zeros(len(cases), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.run(d_grids, d_ces, d_nv, g_llr, stride, g_sinr, stream=C.c_void_p(stream.cuda_stream))
    for _ in range(2):
        g_llr.zero_()
        g_sinr.zero_()
        graph.replay()
        torch.cuda.synchronize()
        out = g_llr.cpu().numpy()
        for i in range(len(cases)):
            assert np.array_equal(out[i * stride: i * stride + G[i]], first[0][i]), i
        assert np.array_equal(g_sinr.cpu().numpy().view(np.uint32), first[1].view(np.uint32))
    plan.close()
