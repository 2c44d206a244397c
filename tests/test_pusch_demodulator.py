"""PUSCH demodulator and channel equaliser (nrphy_pusch_demod_*, nrphy_channel_equalize).

CPU: the POD mirror, the validator, the codeword sizes over the reference unit test's 50 configurations
(tests/golden/pusch_demodulator_configs.json) and the extractor that wrote them.
GPU: the equaliser against a NumPy float32 restatement of the reference's scalar loops; the fused kernel against the composed path
(equalise -> nrphy_demodulate_soft per OFDM symbol -> nrphy_llr_descramble) bit for bit; a link from the grid to transport blocks;
graph capture, determinism and the host-span form.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import backends
from pusch_chest_model import as_i32, dev, from_cbf16, to_cbf16

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "pusch_demodulator_configs.json")
REFERENCE = "/root/reference/srsRAN-5G-ER"
QM = {"PI_2_BPSK": 1, "QPSK": 2, "QAM16": 4, "QAM64": 6, "QAM256": 8}


def fixture_configs():
    return json.load(open(FIXTURE))


def cfg_from_fixture(f, equalizer=abi.EQ_ZF):
    return abi.make_pusch_demod(prbs=f["rb_mask"], qm=QM[f["modulation"]], rnti=f["rnti"], n_id=f["n_id"],
                                start_symbol=f["start_symbol_index"], nof_symbols=f["nof_symbols"], dmrs_symbols=f["dmrs_symbols"],
                                dmrs_type=f["dmrs_type"], nof_cdm_groups_without_data=f["nof_cdm_groups_without_data"],
                                nof_layers=f["nof_tx_layers"], rx_ports=f["rx_ports"], equalizer=equalizer,
                                transform_precoding=int(f["transform_precoding"]))


def dmrs_data_subcarriers(dmrs_type, cdm):
    """Data subcarriers of a PRB on a DM-RS symbol (what dmrs_type::get_dmrs_prb_mask leaves)."""
    if dmrs_type == 1:
        removed = {k for k in range(12) if k % 2 == 0} if cdm == 1 else set(range(12))
    else:
        removed = {k for g in range(cdm) for k in (2 * g, 2 * g + 1, 2 * g + 6, 2 * g + 7)}
    return [k for k in range(12) if k not in removed]


def data_subcarriers(cfg, l):
    """Ascending grid subcarriers of the data RE of OFDM symbol l (empty outside the allocation)."""
    if not cfg.start_symbol_index <= l < cfg.start_symbol_index + cfg.nof_symbols:
        return np.zeros(0, np.int64)
    prbs = [b for b in range(abi.PRB_WORDS * 64) if (cfg.prb_mask[b // 64] >> (b % 64)) & 1]
    ks = dmrs_data_subcarriers(cfg.dmrs_type, cfg.nof_cdm_groups_without_data) if (cfg.dmrs_symbol_mask >> l) & 1 else range(12)
    return np.array([12 * p + k for p in prbs for k in ks], np.int64)


# ---- the reference's scalar equaliser loops, restated in float32 -----------------------------------------------------
def isnormal(x):
    a = np.abs(x)
    return (a >= np.finfo(np.float32).tiny) & (a <= np.finfo(np.float32).max)


def ref_equalize(algorithm, rx, ch, noise_vars, tx_scaling):
    """rx [port][re], ch [layer][port][re] (cbf16 words), noise_vars [port] -> (eq [re][layer] complex64, nv [re][layer] f32).
    equalize_zf_1xn.h:126-170 (after the port reduction of channel_equalizer_generic_impl.cpp), equalize_mmse_1xn.h,
    equalize_zf_2xn.h:182-252; every operation rounded to float32 as written."""
    f = np.float32
    s = f(tx_scaling)
    L, P, N = ch.shape
    y = from_cbf16(rx)
    h = from_cbf16(ch)
    nv = np.asarray(noise_vars, np.float32)
    eq = np.zeros((N, L), np.complex64)
    ev = np.full((N, L), np.inf, np.float32)
    with np.errstate(all="ignore"):
        if L == 1:
            mmse = algorithm == abi.EQ_MMSE
            msq = np.zeros(N, f)
            nacc = np.zeros(N, f)
            ar = np.zeros(N, f)
            ai = np.zeros(N, f)
            for i in range(P):
                a, b = y[i].real, y[i].imag
                c, d = h[0, i].real, h[0, i].imag
                if mmse:
                    c, d = c * s, d * s
                n = c * c + d * d
                ok = isnormal(n) & bool(isnormal(nv[i])) & bool(nv[i] > 0)
                msq = np.where(ok, msq + n, msq)
                nacc = np.where(ok, nacc + n * nv[i], nacc)
                ar = np.where(ok, ar + (a * c + b * d), ar)
                ai = np.where(ok, ai + (b * c - a * d), ai)
            if mmse:
                good = isnormal(msq) & isnormal(nacc)
                rcp = f(1) / (msq * msq + nacc)
                xr, xi_, v = (ar * msq) * rcp, (ai * msq) * rcp, nacc * rcp
            else:
                dp = s * msq
                good = isnormal(dp) & isnormal(nacc)
                rcp = f(1) / dp
                xr, xi_, v = ar * rcp, ai * rcp, (nacc * rcp) * rcp
            eq[good, 0] = (xr + 1j * xi_)[good]
            ev[good, 0] = v[good]
            return eq, ev
        nvm = nv[0]
        for i in range(1, P):
            if nvm < nv[i]:
                nvm = nv[i]
        z = np.zeros(N, f)
        n0, n1, xr, xim, m0r, m0i, m1r, m1i = (z.copy() for _ in range(8))
        for i in range(P):
            a, b = y[i].real, y[i].imag
            c0, d0, c1, d1 = h[0, i].real, h[0, i].imag, h[1, i].real, h[1, i].imag
            n0 = n0 + (c0 * c0 + d0 * d0)
            n1 = n1 + (c1 * c1 + d1 * d1)
            xr = xr + (c0 * c1 + d0 * d1)
            xim = xim + (c0 * d1 - d0 * c1)
            m0r = m0r + (c0 * a + d0 * b)
            m0i = m0i + (c0 * b - d0 * a)
            m1r = m1r + (c1 * a + d1 * b)
            m1i = m1i + (c1 * b - d1 * a)
        xsq = xr * xr + xim * xim
        dp = s * (n0 * n1 - xsq)
        dn = s * dp
        good = isnormal(dp)
        rcp, nrcp = f(1) / dp, f(1) / dn
        a0 = n1 * m0r - (xr * m1r - xim * m1i)
        b0 = n1 * m0i - (xr * m1i + xim * m1r)
        a1 = n0 * m1r - (xr * m0r + xim * m0i)
        b1 = n0 * m1i - (xr * m0i - xim * m0r)
        eq[good, 0] = (a0 * rcp + 1j * (b0 * rcp))[good]
        eq[good, 1] = (a1 * rcp + 1j * (b1 * rcp))[good]
        ev[good, 0] = ((nvm * n1) * nrcp)[good]
        ev[good, 1] = ((nvm * n0) * nrcp)[good]
    return eq, ev


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_pusch_demod_cfg_layout_matches_header():
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %zu\n", sizeof(nrphy_pusch_demod_cfg_t), offsetof(nrphy_pusch_demod_cfg_t, rx_ports),
 offsetof(nrphy_pusch_demod_cfg_t, equalizer), offsetof(nrphy_pusch_demod_cfg_t, prb_mask),
 offsetof(nrphy_pusch_demod_cfg_t, nof_rx_ports));return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()
    P = abi.PuschDemodCfg
    assert [int(x) for x in out] == [C.sizeof(P), P.rx_ports.offset, P.equalizer.offset, P.prb_mask.offset, P.nof_rx_ports.offset]


def _base(**kw):
    args = dict(prbs=range(10, 30), qm=4, dmrs_symbols=(2, 11), dmrs_type=1, nof_cdm_groups_without_data=2, nof_layers=1,
                rx_ports=(0, 1))
    args.update(kw)
    return abi.make_pusch_demod(**args)


@pytest.mark.parametrize("name,kw,ports,subc,want", [
    ("plain", {}, 4, 624, abi.OK),
    ("type 2 with CDM 3", dict(dmrs_type=2, nof_cdm_groups_without_data=3), 4, 624, abi.OK),
    ("2 layers on 4 ports", dict(nof_layers=2, rx_ports=(0, 1, 2, 3)), 4, 624, abi.OK),
    ("2 layers on 2 ports", dict(nof_layers=2, rx_ports=(1, 0)), 2, 624, abi.OK),
    ("non-identity rx ports", dict(rx_ports=(2, 0)), 3, 624, abi.OK),
    ("MMSE one layer", dict(equalizer=abi.EQ_MMSE, rx_ports=(0, 1, 2)), 4, 624, abi.OK),
    ("last PRB of the grid", dict(prbs=[51]), 2, 624, abi.OK),
    ("transform precoding", dict(transform_precoding=1), 4, 624, abi.ERR_ARGUMENT),
    ("3 layers", dict(nof_layers=3, rx_ports=(0, 1, 2, 3)), 4, 624, abi.ERR_ARGUMENT),
    ("MMSE with 2 layers", dict(nof_layers=2, equalizer=abi.EQ_MMSE), 4, 624, abi.ERR_ARGUMENT),
    ("2 layers on 1 port", dict(nof_layers=2, rx_ports=(0,)), 4, 624, abi.ERR_ARGUMENT),
    ("2 layers on 3 ports", dict(nof_layers=2, rx_ports=(0, 1, 2)), 4, 624, abi.ERR_ARGUMENT),
    ("type 1 with CDM 3", dict(nof_cdm_groups_without_data=3), 4, 624, abi.ERR_ARGUMENT),
    ("type 2 with CDM 4", dict(dmrs_type=2, nof_cdm_groups_without_data=4), 4, 624, abi.ERR_ARGUMENT),
    ("CDM 0", dict(nof_cdm_groups_without_data=0), 4, 624, abi.ERR_ARGUMENT),
    ("DM-RS type 3", dict(dmrs_type=3), 4, 624, abi.ERR_ARGUMENT),
    ("rx port outside the grid", dict(rx_ports=(0, 2)), 2, 624, abi.ERR_ARGUMENT),
    ("repeated rx port", dict(rx_ports=(1, 1)), 4, 624, abi.ERR_ARGUMENT),
    ("PRB beyond the grid", dict(prbs=[52]), 4, 624, abi.ERR_ARGUMENT),
    ("symbols beyond the slot", dict(start_symbol=4, nof_symbols=11), 4, 624, abi.ERR_ARGUMENT),
    ("no data RE: all DM-RS, CDM 2", dict(start_symbol=2, nof_symbols=1), 4, 624, abi.ERR_ARGUMENT),
    ("no data RE: no PRB", dict(prbs=[]), 4, 624, abi.ERR_ARGUMENT),
    ("no data RE: no symbol", dict(nof_symbols=0), 4, 624, abi.ERR_ARGUMENT),
    ("pi/2-BPSK", dict(qm=1), 4, 624, abi.ERR_ARGUMENT),
    ("qm 3", dict(qm=3), 4, 624, abi.ERR_ARGUMENT),
])
def test_pusch_demod_validator(name, kw, ports, subc, want):
    assert lib.pusch_demod_validate(_base(**kw), ports, subc) == want, name


def test_pusch_demod_validator_over_the_reference_configurations():
    """The reference unit test's 50 configurations: the 36 without transform precoding and with QPSK..256-QAM run, the 14 with
    transform precoding are refused, and so are the 6 that ask for pi/2-BPSK without it (a modulation this library does not
    demodulate on PUSCH)."""
    configs = fixture_configs()
    assert len(configs) == 50
    verdicts = {}
    for f in configs:
        nports = max(f["rx_ports"]) + 1
        rc = lib.pusch_demod_validate(cfg_from_fixture(f), nports, f["nof_rb"] * 12)
        key = ("tp" if f["transform_precoding"] else "plain", f["modulation"] == "PI_2_BPSK")
        verdicts.setdefault(key, set()).add(rc)
    counts = {k: sum(1 for f in configs if ("tp" if f["transform_precoding"] else "plain", f["modulation"] == "PI_2_BPSK") == k)
              for k in verdicts}
    assert sum(v for k, v in counts.items() if k[0] == "plain") == 36
    assert sum(v for k, v in counts.items() if k[0] == "tp") == 14
    assert verdicts[("plain", False)] == {abi.OK} and counts[("plain", False)] == 30
    assert verdicts[("plain", True)] == {abi.ERR_ARGUMENT}
    assert {rc for k, v in verdicts.items() if k[0] == "tp" for rc in v} == {abi.ERR_ARGUMENT}


def test_pusch_demod_codeword_bits_over_the_reference_configurations():
    for f in fixture_configs():
        cfg = cfg_from_fixture(f)
        cfg.transform_precoding = 0  # counted as if plain
        nre = sum(len(data_subcarriers(cfg, l)) for l in range(14))
        assert lib.pusch_demod_codeword_bits(cfg) == nre * f["nof_tx_layers"] * QM[f["modulation"]], f


def test_extractor_reproduces_the_committed_configurations():
    if not os.path.isdir(REFERENCE):
        pytest.skip("reference sources not present")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "c.json")
        subprocess.run([sys.executable, os.path.join(GOLDEN, "extract_pusch_demod_configs.py"), REFERENCE, out], check=True,
                       capture_output=True, timeout=120)
        assert open(out, "rb").read() == open(FIXTURE, "rb").read()


# =======================================================================================================================
# GPU
# =======================================================================================================================
def composed(ctx, cfg, grid, ce, noise_vars):
    """REs extracted in NumPy -> nrphy_channel_equalize -> nrphy_demodulate_soft (one span per OFDM symbol) ->
    nrphy_llr_descramble; also the float64 SINR of the equalised noise variances."""
    P, L = cfg.nof_rx_ports, cfg.nof_tx_layers
    ports = [cfg.rx_ports[i] for i in range(P)]
    llr, nvs = [], []
    for l in range(14):
        ks = data_subcarriers(cfg, l)
        if ks.size == 0:
            continue
        rx = grid[ports][:, l, ks]
        ch = ce[:, :, l, ks]
        eq, ev = ctx.channel_equalize_host(cfg.equalizer, rx, ch, noise_vars[:P], 1.0)
        llr.append(ctx.demodulate_soft_host(cfg.qm, eq.reshape(-1), ev.reshape(-1)))
        nvs.append(ev.reshape(-1))
    llr = ctx.llr_descramble_host(cfg.rnti * 2 ** 15 + cfg.n_id, np.concatenate(llr))
    v = np.concatenate(nvs).astype(np.float64)
    v = v[~np.isinf(v)]
    sinr = float(-10 * np.log10(v.sum() / v.size)) if v.size and v.sum() > 0 else float("inf")
    return llr, sinr


def synthetic(rng, cfg, nports, nsubc, noise_var, zero_subc=None):
    """Grid [nports][14][nsubc] and estimate [layers][rx][14][nsubc] (cbf16 words): y = H x + n on every RE."""
    L, P = cfg.nof_tx_layers, cfg.nof_rx_ports
    h = ((rng.standard_normal((L, P, 14, nsubc)) + 1j * rng.standard_normal((L, P, 14, nsubc))) / np.sqrt(2)).astype(np.complex64)
    x = ((rng.uniform(-1, 1, (L, 14, nsubc)) + 1j * rng.uniform(-1, 1, (L, 14, nsubc))) * 1.2).astype(np.complex64)
    grid = np.zeros((nports, 14, nsubc), np.complex64)
    for i in range(P):
        n = (rng.standard_normal((14, nsubc)) + 1j * rng.standard_normal((14, nsubc))) * np.sqrt(noise_var / 2)
        grid[cfg.rx_ports[i]] = (h[:, i] * x).sum(axis=0) + n
    if zero_subc is not None:
        h[:, :, :, zero_subc] = 0
    return to_cbf16(grid), to_cbf16(h)


def run_plan(ctx, cfgs, grids, ces, noise_vars, grid_index, nof_grids, nports, nsubc):
    """One nrphy_pusch_demod_run over all PUSCHs: returns ([llr_i], sinr)."""
    import torch
    ce_offsets = np.cumsum([0] + [c.size for c in ces])[:-1]
    plan = lib.PuschDemodPlan(ctx, cfgs, grid_index, nof_grids, nports, nsubc, [int(o) for o in ce_offsets])
    G = [plan.codeword_bits(i) for i in range(len(cfgs))]
    stride = max(G) + 13  # odd stride: rows start at every byte phase
    nv = np.zeros((len(cfgs), abi.MAX_PORTS), np.float32)
    nv[:, :noise_vars.shape[1]] = noise_vars
    d_llr = torch.full((len(cfgs) * stride + 64,), 77, dtype=torch.int8, device="cuda")
    d_sinr = torch.zeros(len(cfgs), dtype=torch.float32, device="cuda")
    d_grids, d_ces, d_nv = dev(as_i32(grids)), dev(as_i32(np.concatenate([c.reshape(-1) for c in ces]))), dev(nv)
    plan.run(d_grids, d_ces, d_nv, d_llr, stride, d_sinr)
    ctx.synchronize()
    out = d_llr.cpu().numpy()
    llrs = [out[i * stride: i * stride + G[i]] for i in range(len(cfgs))]
    for i in range(len(cfgs)):  # nothing outside the codewords is written
        assert (out[i * stride + G[i]: (i + 1) * stride] == 77).all() if i + 1 < len(cfgs) else True
    assert (out[(len(cfgs) - 1) * stride + G[-1]:] == 77).all()
    plan.close()
    return llrs, d_sinr.cpu().numpy()


EQ_SHAPES = [(abi.EQ_ZF, 1, p) for p in (1, 2, 3, 4)] + [(abi.EQ_MMSE, 1, p) for p in (1, 2, 3, 4)] + [(abi.EQ_ZF, 2, 2),
                                                                                                     (abi.EQ_ZF, 2, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("algorithm,layers,ports", EQ_SHAPES)
def test_channel_equalize_matches_the_scalar_loops(gpu_ctx, algorithm, layers, ports):
    import torch
    rng = np.random.default_rng(100 * algorithm + 10 * layers + ports)
    n_batch, N = 3, 517
    rx = to_cbf16((rng.standard_normal((n_batch, ports, N)) + 1j * rng.standard_normal((n_batch, ports, N))).astype(np.complex64))
    ch = to_cbf16((rng.standard_normal((n_batch, layers, ports, N)) + 1j * rng.standard_normal((n_batch, layers, ports, N)))
                  .astype(np.complex64))
    ch[:, :, :, 7] = 0                       # a zero channel coefficient (all ports)
    ch[:, 0, 0, 11] = 0                      # ... and on one port only
    nv = rng.uniform(0.01, 0.5, (n_batch, ports)).astype(np.float32)
    if layers == 1 and ports > 1:            # abnormal port variances: zero, negative, NaN, infinite
        nv[1, 0] = [0.0, -0.1, np.nan, np.inf][ports - 1 if ports <= 4 else 0]
        nv[2, :] = [0.0, -1.0, np.nan, np.inf][:ports]   # all ports invalid
    for s in (0.5, 1.0, float(np.float32(np.sqrt(2.0)))):
        d_eq = torch.zeros((n_batch, N, layers, 2), dtype=torch.float32, device="cuda")
        d_ev = torch.zeros((n_batch, N, layers), dtype=torch.float32, device="cuda")
        d_rx, d_ch, d_nv = dev(as_i32(rx)), dev(as_i32(ch)), dev(nv)
        gpu_ctx.channel_equalize(algorithm, n_batch, N, layers, ports, d_rx, d_ch, d_nv, s, d_eq, d_ev)
        gpu_ctx.synchronize()
        got_eq = d_eq.cpu().numpy().view(np.complex64)[..., 0]
        got_ev = d_ev.cpu().numpy()
        for b in range(n_batch):
            want_eq, want_ev = ref_equalize(algorithm, rx[b], ch[b], nv[b], s)
            for got, want in ((got_eq[b], want_eq), (got_ev[b], want_ev)):
                special = (want == 0) | np.isinf(want) | np.isnan(want)
                assert np.array_equal(got[special], want[special], equal_nan=True), (s, b)
                ok = ~special
                err = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-30)
                assert err.size == 0 or err.max() <= 1e-6, (s, b, err.max())
            if layers == 1 and ports > 1 and b == 2:
                assert (got_eq[b] == 0).all() and np.isinf(got_ev[b]).all()
        # the host form is the same call
        eq1, ev1 = gpu_ctx.channel_equalize_host(algorithm, rx[0], ch[0], nv[0], s)
        assert np.array_equal(eq1.view(np.uint64), got_eq[0].view(np.uint64)) and np.array_equal(ev1.view(np.uint32),
                                                                                                  got_ev[0].view(np.uint32))


def runnable_fixture_configs():
    return [f for f in fixture_configs() if not f["transform_precoding"] and f["modulation"] != "PI_2_BPSK"]


@pytest.mark.gpu
def test_fused_equals_composed_on_the_reference_configurations(gpu_ctx):
    rng = np.random.default_rng(4242)
    for n, f in enumerate(runnable_fixture_configs()):
        for equalizer in ((abi.EQ_ZF, abi.EQ_MMSE) if f["nof_tx_layers"] == 1 else (abi.EQ_ZF,)):
            cfg = cfg_from_fixture(f, equalizer)
            nports, nsubc = max(f["rx_ports"]) + 1, f["nof_rb"] * 12
            grid, ce = synthetic(rng, cfg, nports, nsubc, f["noise_var"], zero_subc=nsubc // 2)
            nv = np.full((1, cfg.nof_rx_ports), f["noise_var"], np.float32)
            (got,), sinr = run_plan(gpu_ctx, [cfg], grid[None], [ce], nv, [0], 1, nports, nsubc)
            want, want_sinr = composed(gpu_ctx, cfg, grid, ce, nv[0])
            assert np.array_equal(got, want), (n, f, equalizer, int((got != want).sum()))
            assert abs(float(sinr[0]) - want_sinr) < 1e-4, (n, sinr[0], want_sinr)


@pytest.mark.gpu
def test_fused_equals_composed_mixed_launch(gpu_ctx):
    """One launch: PUSCHs of every modulation and equaliser over three grids, rx_ports = {2, 0}, a non-contiguous PRB mask, a port
    with an invalid noise variance, DM-RS types 1 and 2."""
    rng = np.random.default_rng(777)
    nports, nsubc, nof_grids = 4, 106 * 12, 3
    cfgs = [
        abi.make_pusch_demod(prbs=list(range(3, 40)) + list(range(50, 51)) + list(range(70, 106, 2)), qm=8, rnti=0x4601, n_id=17,
                             dmrs_symbols=(2, 7, 11), nof_cdm_groups_without_data=1, rx_ports=(2, 0), equalizer=abi.EQ_ZF),
        abi.make_pusch_demod(prbs=range(0, 30), qm=2, rnti=7, n_id=1000, start_symbol=1, nof_symbols=13, dmrs_symbols=(3,),
                             dmrs_type=2, nof_cdm_groups_without_data=1, rx_ports=(3, 1, 0, 2), equalizer=abi.EQ_MMSE),
        abi.make_pusch_demod(prbs=range(30, 106), qm=6, rnti=0xFFF0, n_id=1007, dmrs_symbols=(2, 11), nof_cdm_groups_without_data=2,
                             nof_layers=2, rx_ports=(0, 1, 2, 3), equalizer=abi.EQ_ZF),
        abi.make_pusch_demod(prbs=[5, 9, 60, 61, 62, 100], qm=4, rnti=3, n_id=2, start_symbol=4, nof_symbols=8, dmrs_symbols=(4, 9),
                             dmrs_type=2, nof_cdm_groups_without_data=2, nof_layers=2, rx_ports=(1, 3), equalizer=abi.EQ_ZF),
        abi.make_pusch_demod(prbs=range(0, 106), qm=8, rnti=99, n_id=5, dmrs_symbols=(2,), dmrs_type=2,
                             nof_cdm_groups_without_data=3, rx_ports=(0, 1, 2), equalizer=abi.EQ_ZF),
    ]
    grid_index = [0, 1, 2, 0, 2]
    grids = np.zeros((nof_grids, nports, 14, nsubc), np.uint32)
    ces, nvs = [], np.zeros((len(cfgs), 4), np.float32)
    for i, cfg in enumerate(cfgs):
        g, ce = synthetic(rng, cfg, nports, nsubc, 0.05 * (i + 1), zero_subc=600)
        grids[grid_index[i]] = np.where(g != 0, g, grids[grid_index[i]])
        ces.append(ce)
        nvs[i, :cfg.nof_rx_ports] = 0.05 * (i + 1)
    nvs[4, 1] = -1.0  # an invalid port: left out by ZF
    got, sinr = run_plan(gpu_ctx, cfgs, grids, ces, nvs, grid_index, nof_grids, nports, nsubc)
    for i, cfg in enumerate(cfgs):
        want, want_sinr = composed(gpu_ctx, cfg, grids[grid_index[i]], ces[i], nvs[i])
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))
        assert abs(float(sinr[i]) - want_sinr) < 1e-4, (i, sinr[i], want_sinr)


def one_pusch(seed=5):
    rng = np.random.default_rng(seed)
    cfg = abi.make_pusch_demod(prbs=list(range(0, 20)) + list(range(25, 52)), qm=6, rnti=0x77, n_id=3, dmrs_symbols=(2, 11),
                               nof_cdm_groups_without_data=1, rx_ports=(1, 0), equalizer=abi.EQ_MMSE)
    grid, ce = synthetic(rng, cfg, 2, 624, 0.02, zero_subc=300)
    return cfg, grid, ce, np.array([0.02, 0.03], np.float32)


@pytest.mark.gpu
def test_pusch_demod_graph_replay_and_determinism(gpu_ctx):
    import torch
    cfg, grid, ce, nv = one_pusch()
    cfgs = [cfg, cfg]
    plan = lib.PuschDemodPlan(gpu_ctx, cfgs, [0, 0], 1, 2, 624, [0, 0])
    G = plan.codeword_bits(0)
    nvv = np.zeros((2, 4), np.float32)
    nvv[:, :2] = nv
    d_grid, d_ce, d_nv = dev(as_i32(grid)), dev(as_i32(ce)), dev(nvv)
    outs = []
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(2):
        d_llr = torch.zeros(2 * G, dtype=torch.int8, device="cuda")
        d_sinr = torch.zeros(2, dtype=torch.float32, device="cuda")
        plan.run(d_grid, d_ce, d_nv, d_llr, G, d_sinr)
        gpu_ctx.synchronize()
        outs.append((d_llr.cpu().numpy(), d_sinr.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
    g_llr = torch.zeros(2 * G, dtype=torch.int8, device="cuda")
    g_sinr = torch.zeros(2, dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.run(d_grid, d_ce, d_nv, g_llr, G, g_sinr, stream=C.c_void_p(stream.cuda_stream))
    for _ in range(2):
        g_llr.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(g_llr.cpu().numpy(), outs[0][0])
        assert np.array_equal(g_sinr.cpu().numpy().view(np.uint32), outs[0][1].view(np.uint32))
    plan.close()


@pytest.mark.gpu
def test_pusch_demodulate_host_equals_the_plan(gpu_ctx):
    cfg, grid, ce, nv = one_pusch(9)
    llr, sinr = gpu_ctx.pusch_demodulate_host(cfg, grid, ce, nv)
    (got,), s = run_plan(gpu_ctx, [cfg], grid[None], [ce], nv[None], [0], 1, 2, 624)
    assert np.array_equal(llr, got)
    assert np.float32(sinr).view(np.uint32) == s[0].view(np.uint32)
    assert np.isfinite(sinr) and sinr > 10


# ---- link: transport blocks -> device PDSCH chain (the transmitter) -> channel + noise in NumPy -> grid -> nrphy_pusch_demod_run
# -> nrphy_pusch_decode_batch --------------------------------------------------------------------------------------------
LINK_CASES = [  # qm, code rate x 1024, SNR dB after combining, equaliser, layers, rx ports, CDM groups without data
    (2, 449, 10.0, abi.EQ_ZF, 1, 2, 2),
    (4, 616, 18.0, abi.EQ_MMSE, 1, 2, 2),
    (6, 719, 25.0, abi.EQ_ZF, 1, 4, 2),
    (8, 797, 32.0, abi.EQ_MMSE, 1, 4, 2),
    (2, 449, 10.0, abi.EQ_MMSE, 1, 1, 2),
    (8, 797, 32.0, abi.EQ_ZF, 1, 1, 1),
    (2, 449, 11.0, abi.EQ_ZF, 2, 2, 1),
    (4, 616, 19.0, abi.EQ_ZF, 2, 4, 2),
    (6, 719, 26.0, abi.EQ_ZF, 2, 4, 1),
    (8, 797, 33.0, abi.EQ_ZF, 2, 4, 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("qm,rate,snr_db,equalizer,layers,ports,cdm", LINK_CASES)
def test_link_from_the_grid_to_transport_blocks(gpu_ctx, oracle, qm, rate, snr_db, equalizer, layers, ports, cdm):
    import torch
    nprb, slots, nsubc = 52, 2, 52 * 12
    dmrs = (2, 11)
    tb_bits = oracle.tbs(14, 12 * len(dmrs) if cdm == 2 else 6 * len(dmrs), 0, qm, float(rate), layers, nprb)  # the real rate
    bg = 2 if (rate <= 256 or tb_bits <= 292 or (tb_bits <= 3824 and rate <= 686)) else 1
    prec = np.eye(layers, dtype=np.complex64)[None]
    pdus = [abi.make_pdu(slot_index=i, rnti=0x4321, n_id=11 + i, bwp_size_rb=nprb, qm=qm, dmrs_symbols=dmrs, prb_start=0,
                         prb_count=nprb, nof_symbols=14, base_graph=bg, tb_size_bytes=tb_bits // 8,
                         nof_cdm_groups_without_data=cdm, precoding=prec) for i in range(slots)]
    d = lib.derive(pdus[0])
    G, tb_size = d["codeword_bits"], pdus[0].tb_size_bytes
    tb_stride = (tb_size + 3) & ~3
    rng = np.random.default_rng(1000 * qm + 10 * layers + ports)
    d_tb = dev(rng.integers(0, 256, (slots, tb_stride), dtype=np.uint8))
    plan = lib.PdschPlan(gpu_ctx, pdus, [i * tb_stride for i in range(slots)], list(range(slots)), slots, layers, nsubc)
    d_txgrid = torch.zeros((slots, layers, 14, nsubc), dtype=torch.int32, device="cuda")
    plan.run(d_tb.reshape(-1), d_txgrid)
    gpu_ctx.synchronize()
    plan.close()
    tx = from_cbf16(d_txgrid.cpu().numpy().view(np.uint32))  # [slot][layer][14][subc]
    cfgs = [abi.make_pusch_demod(prbs=range(nprb), qm=qm, rnti=p.rnti, n_id=p.n_id, dmrs_symbols=dmrs,
                                 nof_cdm_groups_without_data=cdm, nof_layers=layers, rx_ports=tuple(range(ports)),
                                 equalizer=equalizer) for p in pdus]
    assert lib.pusch_demod_codeword_bits(cfgs[0]) == G
    # data RE: unit mean power after normalisation (the grid carries the PDSCH amplitude)
    mask = np.zeros((14, nsubc), bool)
    for l in range(14):
        mask[l, data_subcarriers(cfgs[0], l)] = True
    tx = tx / np.sqrt(np.mean(np.abs(tx[:, :, mask]) ** 2))
    # frequency-selective channel per (rx port, layer): a direct path and a weaker delayed one; layers mixed but well conditioned
    k = np.arange(nsubc)
    H = np.zeros((ports, layers, nsubc), np.complex64)
    for p in range(ports):
        for l in range(layers):
            g = (1.0 if (p % layers) == l else 0.35) * np.exp(1j * rng.uniform(0, 2 * np.pi))
            H[p, l] = g * (1 + 0.3 * np.exp(-2j * np.pi * k * rng.uniform(1, 8) / nsubc + 1j * rng.uniform(0, 2 * np.pi)))
    ce = np.broadcast_to(H.transpose(1, 0, 2)[:, :, None, :], (layers, ports, 14, nsubc)).copy()
    ce[:, :, :, 301] = 0  # the DC subcarrier's estimate is zero: its RE give zero soft bits
    ce_w = to_cbf16(ce)
    clean = np.einsum("plk,slmk->spmk", H, tx)  # [slot][port][14][subc]
    cfg_dec = abi.PuschDecoderCfg(bg, qm, 0, layers, d["n_ref"], tb_size, G // qm, 10, 1, 1)
    soft_bytes, state_bytes, _ = gpu_ctx.pusch_decoder_sizes(cfg_dec, slots)
    dplan = lib.PuschDemodPlan(gpu_ctx, cfgs, list(range(slots)), slots, ports, nsubc, [0] * slots)
    d_ce = dev(as_i32(ce_w))
    for good in (True, False):
        # per-port noise: maximum-ratio combining over the ports brings the SNR to snr_db (layers of unit power each)
        nv = float(ports * 10.0 ** (-(snr_db if good else snr_db - 12.0) / 10.0))
        noise = (rng.standard_normal(clean.shape) + 1j * rng.standard_normal(clean.shape)) * np.sqrt(nv / 2)
        grid = to_cbf16((clean + noise).astype(np.complex64))
        nvs = np.zeros((slots, 4), np.float32)
        nvs[:, :ports] = nv
        d_llr = torch.zeros((slots, G), dtype=torch.int8, device="cuda")
        d_sinr = torch.zeros(slots, dtype=torch.float32, device="cuda")
        d_grid, d_nvs = dev(as_i32(grid)), dev(nvs)  # kept alive until the library's stream has read them
        dplan.run(d_grid, d_ce, d_nvs, d_llr, G, d_sinr)
        gpu_ctx.synchronize()
        d_soft = torch.zeros((slots, soft_bytes), dtype=torch.int8, device="cuda")
        d_state = torch.zeros((state_bytes,), dtype=torch.uint8, device="cuda")
        d_out = torch.zeros((slots, tb_stride), dtype=torch.uint8, device="cuda")
        d_res = torch.zeros((slots, 4), dtype=torch.int32, device="cuda")
        gpu_ctx.synchronize()
        gpu_ctx.pusch_decode_batch(cfg_dec, slots, d_llr, G, d_soft, d_state, d_out, tb_stride, d_res)
        gpu_ctx.synchronize()
        torch.cuda.synchronize()
        ok = d_res.cpu().numpy()[:, 0]
        if good:
            assert ok.all(), (ok, d_sinr.cpu().numpy())
            assert torch.equal(d_out[:, :tb_size], d_tb[:, :tb_size])
            assert (d_llr.cpu().numpy() == 0).sum() >= layers * qm  # the DC RE
        else:
            assert not ok.any(), ok
    dplan.close()
