"""Transform-precoded PUSCH through the processor, the blocking host form and the uplink slot pool: nrphy_pusch_tp_validate /
_derive / _harq_bytes / _plan_create / _host and nrphy_pusch_tp_slot.

CPU: the POD and the names; the validator, one row per refusal; the derived configurations against configurations built by hand,
for QPSK and pi/2-BPSK, with and without UCI.
GPU: the processor against the hand-driven chain (estimator _ex -> demodulator _ex -> demultiplexer -> UCI decoder -> decoder),
every result byte, the transport blocks and the UCI bits; a link from a DFT-s-OFDM transmitter of this file through the link
test's channel; without descriptors the bytes of nrphy_pusch_evm_plan_create; the slot pool against the blocking calls; two runs
and a graph replay.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import backends
import pusch_chest_model as chest_model
import pusch_lowpapr_model as lowpapr
import test_pusch_processor as T
import uci_model

abi = backends.abi
lib = backends.pkg.lib
dev, as_i32 = chest_model.dev, chest_model.as_i32

BOTH = abi.PUSCH_DEMOD_TRANSFORM_PRECODING | abi.PUSCH_DEMOD_PI2_BPSK
NPORTS, NSUBC, BETA = T.NPORTS, 12 * 30, T.BETA  # (the hand-driven chain of test_pusch_processor.py reads grids of T.NPORTS ports)
NEW_SYMBOLS = ["nrphy_pusch_tp_validate", "nrphy_pusch_tp_derive", "nrphy_pusch_tp_harq_bytes", "nrphy_pusch_tp_plan_create",
               "nrphy_pusch_tp_host", "nrphy_pusch_tp_slot"]
FIELDS = [f for f, _ in abi.PuschResult._fields_]
f32 = np.float32


def tp(n_rs_id, on=1):
    return abi.PuschTpDesc(on, n_rs_id)


def evm_opts(enable_evm=0, **kw):
    return abi.PuschEvmOptions(T._opts(**kw), enable_evm, 0)


def bits_of(modulation):
    return 1 if modulation == abi.MOD_PI2_BPSK else modulation


def pdu_kw(modulation, nprb, ports=(0,), uci=False, rate=308.0, first_prb=2, **kw):
    """Keyword arguments of abi.make_pusch_pdu for a one-layer PDU of nprb PRBs with a transport block of the size TS 38.214 gives."""
    a = dict(prbs=range(first_prb, first_prb + nprb), modulation=modulation, target_code_rate=rate, nof_layers=1, rx_ports=ports,
             alpha_scaling=1.0, beta_offset_harq_ack=10.0, beta_offset_csi_part1=6.25, beta_offset_csi_part2=6.25, rnti=0x4601,
             tbs_lbrm_bytes=3168, dmrs_symbols=(2, 11), slot_index=3 + nprb % 7, n_id=11 + nprb, scrambling_id=0, n_scid=0)
    if uci:
        a.update(nof_harq_ack=2, nof_csi_part1=5)
    a.update(kw)
    tb_bits = lib.tbs_calculate(14, 12 * len(a["dmrs_symbols"]), 6 if uci else 0, bits_of(modulation), a["target_code_rate"], 1, nprb)
    a.update(tb_size_bytes=tb_bits // 8, ldpc_base_graph=T.base_graph(tb_bits, a["target_code_rate"]))
    return a


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_pod_and_names():
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu\n", sizeof(nrphy_pusch_tp_desc_t), offsetof(nrphy_pusch_tp_desc_t, transform_precoding),
 offsetof(nrphy_pusch_tp_desc_t, n_rs_id));return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()
    P = abi.PuschTpDesc
    assert [int(x) for x in out] == [C.sizeof(P), P.transform_precoding.offset, P.n_rs_id.offset] == [8, 0, 4]
    header = open(os.path.join(backends.ROOT, "include", "mi355_nrphy.h")).read()
    handle = lib.load()
    for name in NEW_SYMBOLS:
        assert name in abi.ABI_SYMBOLS and name + "(" in header and hasattr(handle, name), name
        assert not [s for s in ("_pusch_proc_", "_pusch_csi2_", "_ul_slot", "_srs_", "_uci_", "_ulsch_", "_pf2_", "pucch") if s in name]


@pytest.mark.parametrize("name,kw,desc,opt,want", [
    ("QPSK", pdu_kw(2, 6), tp(5), {}, abi.OK),
    ("pi/2-BPSK", pdu_kw(0, 6), tp(1007), {}, abi.OK),
    ("pi/2-BPSK with UCI and the EVM-based SINR", pdu_kw(0, 25, uci=True), tp(0), dict(enable_evm=1, csi_sinr_calc_method=abi.PUSCH_SINR_EVM), abi.OK),
    ("5 PRB, MMSE, 2 ports", pdu_kw(4, 5, ports=(1, 0)), tp(29), dict(equalizer=abi.EQ_MMSE), abi.OK),
    ("no descriptor", pdu_kw(2, 7), None, {}, abi.OK),
    ("descriptor switched off: nothing else of it is read", pdu_kw(2, 7), tp(5000, 0), {}, abi.OK),
    ("pi/2-BPSK without transform precoding", pdu_kw(0, 6), tp(5, 0), {}, abi.ERR_ARGUMENT),
    ("pi/2-BPSK without a descriptor", pdu_kw(0, 6), None, {}, abi.ERR_ARGUMENT),
    ("two layers", pdu_kw(2, 6, ports=(0, 1), nof_layers=2), tp(5), {}, abi.ERR_ARGUMENT),
    ("7 PRB", pdu_kw(2, 7), tp(5), {}, abi.ERR_ARGUMENT),
    ("n_rs_id 1008", pdu_kw(2, 6), tp(1008), {}, abi.ERR_ARGUMENT),
    ("transform_precoding 2", pdu_kw(2, 6), tp(5, 2), {}, abi.ERR_ARGUMENT),
    ("n_scid 1 (the estimator's validator)", pdu_kw(2, 6, n_scid=1), tp(5), {}, abi.ERR_ARGUMENT),
    ("one CDM group without data (the demodulator's validator)", pdu_kw(2, 6, nof_cdm_groups_without_data=1), tp(5), {}, abi.ERR_ARGUMENT),
    ("a CSI part 2 description", pdu_kw(2, 6, uci=True, nof_csi_part2_entries=1), tp(5), {}, abi.ERR_ARGUMENT),
    ("the EVM-based SINR without the EVM", pdu_kw(2, 6), tp(5), dict(csi_sinr_calc_method=abi.PUSCH_SINR_EVM), abi.ERR_ARGUMENT),
])
def test_validator(name, kw, desc, opt, want):
    pdu = abi.make_pusch_pdu(**kw)
    assert lib.pusch_tp_validate(pdu, desc, evm_opts(**opt), NPORTS, NSUBC) == want, name
    assert (lib.pusch_tp_derive(pdu, desc, evm_opts(**opt), NPORTS, NSUBC) is not None) == (want == abi.OK), name
    if desc is None or desc.transform_precoding == 0:
        assert lib.pusch_evm_validate(pdu, evm_opts(**opt), NPORTS, NSUBC) == want, name


def test_csi2_interface_takes_no_descriptor():
    """nrphy_pusch_csi2_* keeps its signature: there is no way to hand it a transform-precoding descriptor, and it keeps
    refusing pi/2-BPSK."""
    header = open(os.path.join(backends.ROOT, "include", "mi355_nrphy.h")).read()
    for line in header.split(";"):
        if "nrphy_pusch_csi2_" in line and "(" in line:
            assert "nrphy_pusch_tp_desc_t" not in line
    desc = abi.PuschCsi2Desc()
    assert lib.pusch_csi2_validate(abi.make_pusch_pdu(**pdu_kw(0, 6, uci=True)), desc, T.OPTIONS, NPORTS, NSUBC) == abi.ERR_ARGUMENT


def by_hand(a, opts):
    """test_pusch_processor.by_hand for a transform-precoded PDU: the demodulator's configuration says so, and the bits per symbol
    are 1 where the modulation's code is 0 (the demultiplexer and the UCI decoder take the code)."""
    g = lambda k, default=0: a.get(k, default)
    prbs, mod, dmrs = list(a["prbs"]), a["modulation"], a["dmrs_symbols"]
    qm, mask, tb, dc = bits_of(mod), sum(1 << l for l in dmrs), a["tb_size_bytes"], g("dc_position", None)
    info = lib.ulsch_info(abi.make_ulsch_info_cfg(
        tbs_bits=8 * tb, modulation=mod, target_code_rate=a["target_code_rate"], nof_harq_ack_bits=g("nof_harq_ack"),
        nof_csi_part1_bits=g("nof_csi_part1"), nof_csi_part2_bits=0, alpha_scaling=a["alpha_scaling"],
        beta_offset_harq_ack=a["beta_offset_harq_ack"], beta_offset_csi_part1=a["beta_offset_csi_part1"],
        beta_offset_csi_part2=a["beta_offset_csi_part2"], nof_rb=len(prbs), start_symbol_index=0, nof_symbols=14, dmrs_type=1,
        dmrs_symbol_mask=mask, nof_cdm_groups_without_data=2, nof_layers=1, contains_dc=int(dc is not None and dc // 12 in prbs)))
    chest = abi.make_pusch_chest(prbs=prbs, slot_index=a["slot_index"], scrambling_id=a["scrambling_id"], n_scid=0, scaling=BETA,
                                 dmrs_symbols=dmrs, rx_ports=a["rx_ports"], dc_position=dc)
    demod = abi.make_pusch_demod(prbs=prbs, qm=qm, rnti=a["rnti"], n_id=a["n_id"], dmrs_symbols=dmrs, nof_cdm_groups_without_data=2,
                                 nof_layers=1, rx_ports=a["rx_ports"], equalizer=opts.equalizer, transform_precoding=1)
    demux = abi.make_ulsch_demux(modulation=mod, nof_layers=1, nof_prb=len(prbs), start_symbol_index=0, nof_symbols=14, dmrs_type=0,
                                 dmrs_symbol_mask=mask, nof_cdm_groups_without_data=2, nof_harq_ack_rvd=info.nof_harq_ack_rvd,
                                 nof_harq_ack_bits=g("nof_harq_ack"), nof_enc_harq_ack_bits=info.nof_harq_ack_bits,
                                 nof_csi_part1_bits=g("nof_csi_part1"), nof_enc_csi_part1_bits=info.nof_csi_part1_bits, rnti=a["rnti"],
                                 n_id=a["n_id"])
    uci = [abi.make_uci_decoder(bits, enc, mod) for bits, enc in ((g("nof_harq_ack"), info.nof_harq_ack_bits),
                                                                  (g("nof_csi_part1"), info.nof_csi_part1_bits)) if bits]
    codeword_bits = (14 - len(dmrs)) * 12 * len(prbs) * qm
    nof_sch_bits = lib.ulsch_demux_sizes(demux)[0] if uci else codeword_bits
    b = 8 * tb + (16 if 8 * tb <= 3824 else 24)
    kcb = 8448 if a["ldpc_base_graph"] == 1 else 3840
    assert b <= kcb and info.nof_ul_sch_bits == nof_sch_bits
    decoder = abi.PuschDecoderCfg(a["ldpc_base_graph"], qm, g("rv"), 1, min(a["tbs_lbrm_bytes"] * 8 * 3 // 2, 25344), tb,
                                  info.nof_ul_sch_bits // qm, opts.dec_nof_iterations, opts.dec_enable_early_stop, g("new_data", 1))
    return dict(info=info, chest=chest, demod=demod, demux=demux, uci=uci, decoder=decoder, codeword_bits=codeword_bits,
                nof_sch_bits=nof_sch_bits)


@pytest.mark.parametrize("modulation", [abi.MOD_QPSK, abi.MOD_PI2_BPSK])
@pytest.mark.parametrize("uci", [False, True])
def test_derive_equals_the_configurations_built_by_hand(modulation, uci):
    opts = T._opts(equalizer=abi.EQ_MMSE, dec_nof_iterations=6)
    for nprb, n_rs_id in ((3, 0), (25, 1007)):
        a = pdu_kw(modulation, nprb, ports=(1, 0), uci=uci, dc_position=12 * 3 + 5)
        got = lib.pusch_tp_derive(abi.make_pusch_pdu(**a), tp(n_rs_id), abi.PuschEvmOptions(opts, 0, 0), NPORTS, NSUBC)
        assert got is not None, (nprb, a)
        d, lp = got
        want = by_hand(a, opts)
        assert (lp.enabled, lp.n_rs_id) == (1, n_rs_id)
        for part in ("info", "chest", "demod"):
            assert bytes(getattr(d, part)) == bytes(want[part]), (nprb, part)
        assert (d.nof_uci, d.has_decoder, d.codeword_bits, d.nof_sch_bits) == (len(want["uci"]), 1, want["codeword_bits"], want["nof_sch_bits"])
        assert d.demod.transform_precoding == 1 and d.demod.qm == bits_of(modulation) and d.decoder.qm == bits_of(modulation)
        if uci:
            assert bytes(d.demux) == bytes(want["demux"]) and d.demux.modulation == modulation
            for k, u in enumerate(want["uci"]):
                assert bytes(d.uci[k]) == bytes(u) and d.uci[k].modulation == modulation, k
        assert bytes(d.decoder) == bytes(want["decoder"]), nprb
        # without transform precoding the same PDU derives as before, and tells the estimator nothing
        if modulation != abi.MOD_PI2_BPSK:
            plain, lp0 = lib.pusch_tp_derive(abi.make_pusch_pdu(**a), tp(n_rs_id, 0), abi.PuschEvmOptions(opts, 0, 0), NPORTS, NSUBC)
            assert bytes(plain) == bytes(lib.pusch_proc_derive(abi.make_pusch_pdu(**a), opts, NPORTS, NSUBC)) and lp0.enabled == 0
            assert plain.demod.transform_precoding == 0
    soft, state = lib.pusch_tp_harq_bytes(abi.make_pusch_pdu(**a), tp(3), abi.PuschEvmOptions(opts, 0, 0))
    assert soft > 0 and state > 0


# =======================================================================================================================
# GPU: the transmitter
# =======================================================================================================================
def modulate(bits, modulation):
    """TS 38.211 Section 5.1; pi/2-BPSK (5.1.1): e^{j (pi / 2)(i mod 2)} ((1 - 2 b) + j (1 - 2 b)) / sqrt(2), i counted within the
    OFDM symbol (every symbol holds an even number, so counting through is the same)."""
    if modulation != abi.MOD_PI2_BPSK:
        return T.modulate(bits, modulation)
    s = 1.0 - 2.0 * bits.astype(np.float64)
    return np.exp(0.5j * np.pi * (np.arange(bits.size) % 2)) * (s + 1j * s) / np.sqrt(2)


def transmit(oracle, pdu, desc, d, rng, nports=NPORTS, nsubc=NSUBC):
    """test_pusch_processor.transmit for a transform-precoded PDU: per data symbol fft(x) / sqrt(12 M_rb) onto the allocated
    subcarriers, the low-PAPR DM-RS at beta, the same channel (two taps, 3 samples of delay, 250 Hz)."""
    s, qm = T.Sent(), bits_of(pdu.modulation)
    demux = {f[0]: int(getattr(d.demux, f[0])) for f in abi.UlschDemuxCfg._fields_}
    s.tb = rng.integers(0, 256, pdu.tb_size_bytes, dtype=np.uint8)
    sch = np.unpackbits(oracle.pdsch_encode_cfg(pdu.ldpc_base_graph, pdu.rv, qm, d.decoder.nref, 1, d.nof_sch_bits // qm, s.tb))[:d.nof_sch_bits]
    s.harq = rng.integers(0, 2, pdu.nof_harq_ack, dtype=np.uint8)
    s.csi1 = rng.integers(0, 2, pdu.nof_csi_part1, dtype=np.uint8)
    if d.nof_uci:
        coded = [uci_model.encode(m, e, pdu.modulation) for m, e in ((s.harq, d.info.nof_harq_ack_bits), (s.csi1, d.info.nof_csi_part1_bits))]
        codeword = uci_model.ulsch_multiplex(demux, sch, coded[0], coded[1])
    else:
        codeword = sch
    assert codeword.size == d.codeword_bits
    symbols = modulate(T.scramble(codeword, pdu.rnti, pdu.n_id), pdu.modulation)
    prbs = chest_model.prbs_of(d.chest)
    subc = (12 * np.array(prbs)[:, None] + np.arange(12)).ravel()
    x = np.zeros((14, nsubc), np.complex128)
    pr, pi, kk = lowpapr.pilots(d.chest, desc.n_rs_id)
    at = 0
    for l in range(14):
        if (pdu.dmrs_symbol_mask >> l) & 1:
            x[l, kk] = BETA * (pr + 1j * pi)
        else:
            x[l, subc] = np.fft.fft(symbols[at:at + subc.size]) / np.sqrt(subc.size)
            at += subc.size
    assert at == symbols.size
    k = np.arange(nsubc)
    rot = np.exp(2j * np.pi * (250.0 / 15000.0) * np.array(chest_model.epochs(0), np.float64))
    s.clean = np.zeros((nports, 14, nsubc), np.complex128)
    for p in range(pdu.nof_rx_ports):
        g = np.exp(1j * rng.uniform(0, 2 * np.pi))
        H = g * np.exp(-2j * np.pi * k * 3 / 4096.0) * (1 + 0.3 * np.exp(-2j * np.pi * k * rng.uniform(1, 8) / 4096.0))
        s.clean[pdu.rx_ports[p]] = H[None, :] * x * rot[:, None]
    return s


def noisy(sent, snr_db, rng):
    return T.noisy(sent, snr_db, rng)


class Layout(T.Layout):
    """test_pusch_processor.Layout with the HARQ sizes of nrphy_pusch_tp_harq_bytes."""

    def __init__(self, pdus, tps, opts):
        self.soft, self.state, self.tb, self.uci, self.sizes = [], [], [], [], []
        harq = tb = uci = 0
        for p, t in zip(pdus, tps):
            soft_bytes, state_bytes = lib.pusch_tp_harq_bytes(p, t, opts)
            self.sizes.append((soft_bytes, state_bytes))
            self.soft.append(harq)
            self.state.append(harq + T.align(soft_bytes))
            harq = self.state[-1] + T.align(state_bytes)
            self.tb.append(tb)
            tb += T.align(p.tb_size_bytes, 4) + 4
            self.uci.append(uci)
            uci += p.nof_harq_ack + p.nof_csi_part1 + 3
        self.harq_bytes, self.tb_bytes, self.uci_bytes = max(harq, 256), max(tb, 4), max(uci, 4)


class HandChain(T.HandChain):
    """test_pusch_processor.HandChain whose estimator and demodulator plans are made by the _ex calls, and whose demodulator
    takes the EVM when asked to."""

    def __init__(self, ctx, pdus, lps, derived, layout, ngrids, gidx, with_evm):
        import torch
        chest_plan, demod_plan = lib.PuschChestPlan, lib.PuschDemodPlan
        lib.PuschChestPlan = lambda *a: chest_plan(*a, lowpapr=lps)
        lib.PuschDemodPlan = lambda *a: demod_plan(*a, features=BOTH)
        try:
            super().__init__(ctx, pdus, derived, layout, ngrids, gidx, NSUBC)
        finally:
            lib.PuschChestPlan, lib.PuschDemodPlan = chest_plan, demod_plan
        self.evm = torch.zeros(self.n, dtype=torch.float32, device="cuda") if with_evm else None
        run = self.dplan.run
        self.dplan.run = lambda *a, **kw: run(*a, d_evm=self.evm, **kw)


class Batch:
    """PDUs on a grid each (NPORTS x NSUBC), transmitted once under a fixed seed, with the processor's plan and the hand chain."""

    def __init__(self, oracle, kws, tps, opts, seed=2026):
        self.pdus, self.tps, self.opts = [abi.make_pusch_pdu(**a) for a in kws], tps, opts
        got = [lib.pusch_tp_derive(p, t, opts, NPORTS, NSUBC) for p, t in zip(self.pdus, tps)]
        assert None not in got
        self.derived, self.lps = [g[0] for g in got], [g[1] for g in got]
        rng = np.random.default_rng(seed)
        self.sent = [transmit(oracle, p, t, d, rng) if t.transform_precoding else None for p, t, d in zip(self.pdus, tps, self.derived)]
        self.layout = Layout(self.pdus, tps, opts)
        self.gidx = list(range(len(self.pdus)))

    def grids(self, snr_db, seed=77):
        rng = np.random.default_rng(seed)
        return np.stack([noisy(s, snr_db, rng) for s in self.sent])

    def plan(self, ctx, opts=None):
        L = self.layout
        return lib.PuschTpPlan(ctx, self.pdus, self.tps, opts or self.opts, self.gidx, len(self.pdus), NPORTS, NSUBC, L.soft, L.state, L.tb, L.uci)

    def processor(self, ctx, d_grid, opts=None):
        plan = self.plan(ctx, opts)
        B = T.Buffers(self.layout, len(self.pdus))
        plan.run(d_grid, B.harq, B.tb, B.uci, B.result)
        ctx.synchronize()
        got = B.read()
        plan.close()
        return got

    def chain(self, ctx, d_grid, with_evm):
        chain = HandChain(ctx, self.pdus, self.lps, self.derived, self.layout, len(self.pdus), self.gidx, with_evm)
        H = T.Buffers(self.layout, len(self.pdus))
        chain.run(d_grid, H)
        ctx.synchronize()
        want = chain.read()
        want["status_of"] = chain.status_of
        want["evm"] = chain.evm.cpu().numpy().copy() if with_evm else None
        want_buf = H.read()
        chain.close()
        return want_buf, want


def chain_cases(flip):
    """QPSK and pi/2-BPSK at 1, 3, 5, 6 and 25 PRB; receive ports and UCI alternate, the other way round with `flip`."""
    kws, tps = [], []
    for i, (modulation, nprb) in enumerate((m, n) for m in (abi.MOD_QPSK, abi.MOD_PI2_BPSK) for n in (1, 3, 5, 6, 25)):
        two, uci = (i + flip) % 2 == 1, ((i // 2) + flip) % 2 == 1 and nprb > 1
        kws.append(pdu_kw(modulation, nprb, ports=(1, 0) if two else (i % 2,), uci=uci, first_prb=1 + i % 4,
                          dc_position=12 * 3 + 7 if i % 3 == 0 else None))
        tps.append(tp((37 * i + 29) % 1008))
    return kws, tps


@pytest.mark.gpu
@pytest.mark.parametrize("equalizer,flip", [(abi.EQ_ZF, 0), (abi.EQ_MMSE, 1)])
def test_processor_equals_the_hand_driven_chain(gpu_ctx, oracle, equalizer, flip):
    """enable_evm = 0: every result byte, the transport blocks, the UCI bits and the HARQ blocks are the hand-driven chain's.
    enable_evm = 1: the same bytes but for has_evm and evm, and the EVM is the one nrphy_pusch_demod_run_evm gives the chain."""
    kws, tps = chain_cases(flip)
    opts = evm_opts(0, equalizer=equalizer, csi_sinr_calc_method=abi.PUSCH_SINR_POST_EQUALIZATION if flip else abi.PUSCH_SINR_CHANNEL_ESTIMATOR)
    b = Batch(oracle, kws, tps, opts)
    d_grid = dev(as_i32(b.grids(15.0)))
    got = b.processor(gpu_ctx, d_grid)
    want_buf, want = b.chain(gpu_ctx, d_grid, with_evm=True)
    names = ["%s %d PRB" % ("QPSK" if a["modulation"] else "pi/2-BPSK", len(a["prbs"])) for a in kws]
    T.assert_equal_to_the_hand_chain(names, b.pdus, b.derived, b.layout, got, want_buf, want, opts.proc.csi_sinr_calc_method)
    assert all(got["result"]["tb_crc_ok"] == 1), got["result"]["tb_crc_ok"]
    for i, (p, s) in enumerate(zip(b.pdus, b.sent)):
        assert got["tb"][b.layout.tb[i]:b.layout.tb[i] + p.tb_size_bytes].tobytes() == s.tb.tobytes(), names[i]
        at = b.layout.uci[i]
        assert got["uci"][at:at + p.nof_harq_ack + p.nof_csi_part1].tobytes() == np.concatenate([s.harq, s.csi1]).tobytes(), names[i]
    on = b.processor(gpu_ctx, d_grid, abi.PuschEvmOptions(opts.proc, 1, 0))
    for k in ("tb", "uci", "harq"):
        assert on[k].tobytes() == got[k].tobytes(), k
    for i, name in enumerate(names):
        for f in FIELDS:
            if f not in ("has_evm", "evm"):
                assert np.array(on["result"][i][f]).tobytes() == np.array(got["result"][i][f]).tobytes(), (name, f)
        assert on["result"][i]["has_evm"] == 1 and on["result"][i]["evm"] > 0, name
        assert np.array(on["result"][i]["evm"]).view(np.uint32) == want["evm"][i:i + 1].view(np.uint32)[0], name


LINK_MODULATIONS = [(abi.MOD_PI2_BPSK, 308.0), (abi.MOD_QPSK, 449.0), (abi.MOD_QAM16, 490.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("modulation,rate", LINK_MODULATIONS)
def test_link_from_the_transmitter_to_the_transport_block(gpu_ctx, oracle, modulation, rate):
    """The blocking host form at 30 dB behind the link test's channel: the CRC passes and the bytes and the UCI bits are the
    ones sent, at 1, 5, 6 and 25 PRB, with UCI from 5 PRB on.  Fixed seeds: a CRC failure is a failure."""
    rng = np.random.default_rng(1000 + modulation)
    o = evm_opts(1, csi_sinr_calc_method=abi.PUSCH_SINR_EVM)
    for nprb in (1, 5, 6, 25):
        a = pdu_kw(modulation, nprb, ports=(0, 1) if nprb % 2 else (1,), uci=nprb >= 5, rate=rate, first_prb=3)
        pdu, desc = abi.make_pusch_pdu(**a), tp((37 * nprb + modulation) % 1008)
        d, _ = lib.pusch_tp_derive(pdu, desc, o, NPORTS, NSUBC)
        sent = transmit(oracle, pdu, desc, d, rng)
        result, tb, uci = gpu_ctx.pusch_tp_host(pdu, desc, o, noisy(sent, 30.0, rng))
        assert result.tb_crc_ok == 1 and tb.tobytes() == sent.tb.tobytes(), (nprb, result.sinr_dB)
        assert uci.tobytes() == np.concatenate([sent.harq, sent.csi1]).tobytes(), nprb
        if nprb >= 5:
            assert result.harq_ack_status == abi.UCI_STATUS_VALID and result.csi_part1_status == abi.UCI_STATUS_VALID, nprb
        assert result.has_evm == 1 and result.evm > 0 and result.has_cfo == 1, (nprb, result.evm, result.cfo_hz)


def field_bytes(r, f):
    return np.array(getattr(r, f), T.RESULT_DTYPE[f]).tobytes()


@pytest.mark.gpu
def test_without_descriptors_it_is_the_old_call(gpu_ctx):
    """nrphy_pusch_tp_plan_create with tps = NULL, and with every descriptor switched off, on the mixed batch (a)-(f) of
    test_pusch_processor.py: the bytes of nrphy_pusch_evm_plan_create."""
    sc = T.Scenario.get(gpu_ctx, "abcdef", abi.EQ_ZF)
    d_grid = dev(as_i32(sc.grids(True)))
    L, n = sc.layout, len(sc.names)
    o = abi.PuschEvmOptions(sc.opts, 1, 0)
    outs = []
    for make in (lambda: lib.PuschProcPlan(gpu_ctx, sc.pdus, o, sc.gidx, n, T.NPORTS, T.NSUBC, L.soft, L.state, L.tb, L.uci),
                 lambda: lib.PuschTpPlan(gpu_ctx, sc.pdus, None, o, sc.gidx, n, T.NPORTS, T.NSUBC, L.soft, L.state, L.tb, L.uci),
                 lambda: lib.PuschTpPlan(gpu_ctx, sc.pdus, [tp(2000 + i, 0) for i in range(n)], o, sc.gidx, n, T.NPORTS, T.NSUBC, L.soft,
                                         L.state, L.tb, L.uci)):
        plan = make()
        B = T.Buffers(L, n)
        plan.run(d_grid, B.harq, B.tb, B.uci, B.result)
        gpu_ctx.synchronize()
        outs.append(B.read())
        plan.close()
    for other in outs[1:]:
        for k in outs[0]:
            assert other[k].tobytes() == outs[0][k].tobytes(), k
    assert all(outs[0]["result"]["tb_crc_ok"] == [p.has_codeword for p in sc.pdus])


@pytest.mark.gpu
def test_slot_pool_mixes_the_three_calls(gpu_ctx, oracle):
    import torch
    nports, nprb = 2, T.NSUBC // 12
    ofdm = abi.OfdmConfig(0, nprb, 384, 0, 1.0 / np.sqrt(384), 2.0e9)
    rng = np.random.default_rng(31)
    plain = T.make_pdus("a", rx_ports=(0,))[0]  # PRBs 0 to 5; the two transform-precoded PDUs beside it
    d0 = lib.pusch_proc_derive(plain, T.OPTIONS, nports, T.NSUBC)
    kws = [pdu_kw(abi.MOD_PI2_BPSK, 5, ports=(1, 0), uci=True, first_prb=8), pdu_kw(abi.MOD_QPSK, 6, ports=(1,), first_prb=16)]
    pdus, tps = [abi.make_pusch_pdu(**a) for a in kws], [tp(61), tp(1007)]
    o = evm_opts(1, csi_sinr_calc_method=abi.PUSCH_SINR_EVM)
    clean = T.transmit(gpu_ctx, plain, d0, rng).clean[:nports].copy()
    for p, t in zip(pdus, tps):
        d, _ = lib.pusch_tp_derive(p, t, o, nports, T.NSUBC)
        clean += transmit(oracle, p, t, d, rng, nports, T.NSUBC).clean
    noise = (rng.standard_normal(clean.shape) + 1j * rng.standard_normal(clean.shape)) * np.sqrt(0.5 * 10 ** -2.5)
    words = chest_model.to_cbf16((clean + noise).astype(np.complex64)).view(np.uint32).reshape(nports, 14, T.NSUBC)
    every, every_tp = [plain] + pdus, [tp(0, 0)] + tps
    layout = Layout(every, every_tp, o)
    d_harq = torch.zeros(layout.harq_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pool = lib.UlSlots(gpu_ctx, ofdm, nports, 1, d_harq=d_harq, max_pusch=3, max_uci_bits=64, max_tb_bytes=sum(p.tb_size_bytes for p in every))
    sid = pool.open(0)
    assert pool.load_grid(sid, words.view(np.uint16).reshape(nports, 14, T.NSUBC, 2)) == abi.OK
    assert pool.pusch_tp(sid, pdus[:1], [tp(1008)], o, layout.soft[1:2], layout.state[1:2]) == abi.ERR_ARGUMENT
    assert pool.pusch_evm(sid, pdus[:1], o, layout.soft[1:2], layout.state[1:2]) == abi.ERR_ARGUMENT  # pi/2-BPSK needs its descriptor
    assert pool.pusch_tp(sid, pdus[:1], tps[:1], o, layout.soft[1:2], layout.state[1:2]) == abi.OK
    assert pool.pusch(sid, [plain], T.OPTIONS, layout.soft[:1], layout.state[:1]) == abi.OK
    assert pool.pusch_tp(sid, pdus[1:], tps[1:], o, layout.soft[2:], layout.state[2:]) == abi.OK
    assert pool.finish(sid) == abi.OK and pool.wait(sid) == abi.OK
    got = pool.pusch_results(sid)
    want = [gpu_ctx.pusch_tp_host(pdus[0], tps[0], o, words), gpu_ctx.pusch_proc_host(plain, T.OPTIONS, words),
            gpu_ctx.pusch_tp_host(pdus[1], tps[1], o, words)]
    assert len(got) == 3
    for i, (w, tb, uci) in enumerate(want):
        assert bytes(got[i]) == bytes(w) and w.tb_crc_ok == 1, (i, w.tb_crc_ok)
        assert pool.tb(sid, i).tobytes() == tb.tobytes(), i
    assert pool.uci_bits(sid, 0).tobytes() == want[0][2].tobytes() and want[0][2].size == 7
    assert (got[0].has_evm, got[1].has_evm, got[2].has_evm) == (1, 0, 1)
    pool.close(sid)
    pool.destroy()


@pytest.mark.gpu
def test_two_runs_and_a_graph_replay_give_identical_bytes(gpu_ctx, oracle):
    import torch
    kws, tps = chain_cases(0)
    b = Batch(oracle, kws[3:8], tps[3:8], evm_opts(1, csi_sinr_calc_method=abi.PUSCH_SINR_EVM))
    d_grid = dev(as_i32(b.grids(12.0)))
    plan = b.plan(gpu_ctx)
    outs = []
    for _ in range(2):
        B = T.Buffers(b.layout, len(b.pdus))
        plan.run(d_grid, B.harq, B.tb, B.uci, B.result)
        gpu_ctx.synchronize()
        outs.append(B.read())
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    G = T.Buffers(b.layout, len(b.pdus))
    stream = torch.cuda.Stream()  # a single stream, as the other replay tests
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.run(d_grid, G.harq, G.tb, G.uci, G.result, stream=C.c_void_p(stream.cuda_stream))
    G.harq.zero_()
    G.tb.fill_(T.SENTINEL)
    G.uci.fill_(T.SENTINEL)
    G.result.zero_()
    graph.replay()
    torch.cuda.synchronize()
    replayed = G.read()
    for k in outs[0]:
        assert replayed[k].tobytes() == outs[0][k].tobytes(), k
    assert all(outs[0]["result"]["tb_crc_ok"] == 1)
    plan.close()
