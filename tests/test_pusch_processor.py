"""PUSCH processor (nrphy_pusch_proc_*): received grids to transport blocks, UCI payloads and the channel state information record.

CPU: the POD mirrors, the validator over each refusal, and nrphy_pusch_proc_derive against configurations built here by hand from
nrphy_ul_sch_info.
GPU: a transmitter assembled from the helpers of the other receive-side tests (UL-SCH bits from nrphy_pdsch_encode_host, UCI bits
from the restatement's encoder, multiplexed by the restatement, scrambled with the placeholders applied, a NumPy modulation mapper,
the restatement's DM-RS at +3 dB, the two-tap channel with a delay of 3 samples and a CFO of 250 Hz of the estimator's link test),
and the processor compared byte for byte with the same PDUs driven through the existing entry points by this test with the
configurations nrphy_pusch_proc_derive returned.  The record's channel state information is compared with a float32 restatement
of channel_estimate::get_channel_state_information applied to the measurements the hand-driven estimator returned.

Reference pin: tests/golden/record_pusch_processor_reference.cpp ran the reference's pusch_processor_impl on the grids of (a)-(f) at
both SNRs; verdicts, transport blocks, UCI payloads and statuses are pinned exactly, the channel state information within a measured
margin.

The equaliser is an option of the plan and MMSE takes one layer only, so the batch (a)-(f) runs on a ZF plan and the one-layer
PDUs of it, (c) among them, run again on an MMSE plan; both are compared with the hand-driven chain.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import backends
import pusch_chest_model as chest_model
import uci_model
from test_pusch_channel_estimator import BETA, LINK_CASES, MEAS_DTYPE

abi = backends.abi
lib = backends.pkg.lib
dev, as_i32 = chest_model.dev, chest_model.as_i32

NPORTS, NPRB_GRID = 4, 25
NSUBC = 12 * NPRB_GRID
GUARD, SENTINEL = 64, 0xA5
RESULT_DTYPE = np.dtype(abi.PuschResult)
f32 = np.float32
# per-port SNR at which every block decodes: the estimator's link cases, by (bits per symbol, layers)
GOOD_SNR = {(qm, layers): snr for qm, _, snr, _, layers, _ in LINK_CASES if (qm, layers) in ((2, 1), (4, 1), (6, 1), (4, 2))}
BAD_SNR = -12.0


def base_graph(tb_bits, rate):
    """get_ldpc_base_graph."""
    r = rate / 1024.0
    return 2 if (tb_bits <= 292 or r <= 0.25 or (tb_bits <= 3824 and r <= 0.67)) else 1


def nof_codeblocks(pdu):
    """ldpc::compute_nof_codeblocks for the PDU's base graph; 0 without codeword."""
    if not pdu.has_codeword:
        return 0
    b = 8 * pdu.tb_size_bytes + (16 if 8 * pdu.tb_size_bytes <= 3824 else 24)
    kcb = 8448 if pdu.ldpc_base_graph == 1 else 3840
    return 1 if b <= kcb else -(-b // (kcb - 24))


def pdu_args():
    """(a)-(f): name -> keyword arguments of abi.make_pusch_pdu."""
    common = dict(alpha_scaling=0.8, beta_offset_harq_ack=10.0, beta_offset_csi_part1=6.25, beta_offset_csi_part2=6.25, rnti=0x4601,
                  tbs_lbrm_bytes=3168, dmrs_symbols=(2, 11))
    shapes = {
        "a": dict(prbs=range(0, 6), modulation=2, target_code_rate=449.0, nof_layers=1, rx_ports=(2,)),
        "b": dict(prbs=range(10, 18), modulation=4, target_code_rate=616.0, nof_layers=1, rx_ports=(1, 3), nof_harq_ack=1,
                  dc_position=150),
        "c": dict(prbs=range(3, 15), modulation=6, target_code_rate=719.0, nof_layers=1, rx_ports=(0, 1, 2, 3), nof_harq_ack=4,
                  nof_csi_part1=7),
        "d": dict(prbs=range(0, 25), modulation=4, target_code_rate=616.0, nof_layers=2, rx_ports=(3, 2, 1, 0), nof_harq_ack=20,
                  nof_csi_part1=40, dc_position=299),
        "e": dict(prbs=range(19, 25), modulation=2, target_code_rate=449.0, nof_layers=1, rx_ports=(0, 1), nof_harq_ack=2,
                  nof_csi_part1=12, codeword=False),
        "f": dict(prbs=range(5, 18), modulation=2, target_code_rate=449.0, nof_layers=1, rx_ports=(2,), dmrs_symbols=(2, 7, 11)),
    }
    out = {}
    for i, (name, s) in enumerate(shapes.items()):
        a = dict(common, slot_index=3 + i, n_id=11 + i, scrambling_id=100 + i, n_scid=i % 2, **s)
        if a.pop("codeword", True):
            has_uci = a.get("nof_harq_ack", 0) + a.get("nof_csi_part1", 0) > 0
            tb_bits = lib.tbs_calculate(14, 12 * len(a["dmrs_symbols"]), 18 if has_uci else 0, a["modulation"], a["target_code_rate"],
                                        a["nof_layers"], len(a["prbs"]))
            a.update(tb_size_bytes=tb_bits // 8, ldpc_base_graph=base_graph(tb_bits, a["target_code_rate"]))
        out[name] = a
    return out


def make_pdus(names="abcdef", **override):
    args = pdu_args()
    return [abi.make_pusch_pdu(**dict(args[n], **override)) for n in names]


OPTIONS = abi.make_pusch_proc_options(10, 1, abi.PUSCH_SINR_CHANNEL_ESTIMATOR, abi.EQ_ZF)


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_pusch_proc_pods_match_header():
    pods = [("nrphy_pusch_pdu_t", abi.PuschPdu), ("nrphy_pusch_proc_options_t", abi.PuschProcOptions),
            ("nrphy_pusch_proc_derived_t", abi.PuschProcDerived), ("nrphy_pusch_result_t", abi.PuschResult)]
    exprs, want = [], []
    for cname, cls in pods:
        exprs.append("sizeof(%s)" % cname)
        want.append(C.sizeof(cls))
        for f in cls._fields_:
            exprs.append("offsetof(%s, %s)" % (cname, f[0]))
            want.append(getattr(cls, f[0]).offset)
    exprs += ["NRPHY_PUSCH_SINR_CHANNEL_ESTIMATOR", "NRPHY_PUSCH_SINR_POST_EQUALIZATION", "NRPHY_PUSCH_SINR_EVM"]
    want += [abi.PUSCH_SINR_CHANNEL_ESTIMATOR, abi.PUSCH_SINR_POST_EQUALIZATION, abi.PUSCH_SINR_EVM]
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){size_t v[] = {%s}; for (size_t i = 0; i != sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]); return 0;}''' % ", ".join(exprs)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()]
    assert out == want
    assert C.sizeof(abi.PuschResult) == RESULT_DTYPE.itemsize == 96
    names = [s for s in abi.ABI_SYMBOLS if "_pusch_proc_" in s]
    assert len(names) == 8 and not [s for s in names if not hasattr(lib.load(), s)]


def _opts(**kw):
    args = dict(dec_nof_iterations=10, dec_enable_early_stop=1, csi_sinr_calc_method=abi.PUSCH_SINR_CHANNEL_ESTIMATOR, equalizer=abi.EQ_ZF)
    args.update(kw)
    return abi.make_pusch_proc_options(**args)


@pytest.mark.parametrize("name,case,pdu_change,opt_change,want", [
    ("(a)", "a", {}, {}, True), ("(b)", "b", {}, {}, True), ("(c) with MMSE", "c", {}, dict(equalizer=abi.EQ_MMSE), True),
    ("(d)", "d", {}, {}, True), ("(e)", "e", {}, {}, True), ("(f)", "f", {}, {}, True),
    ("the post-equalisation SINR", "a", {}, dict(csi_sinr_calc_method=abi.PUSCH_SINR_POST_EQUALIZATION), True),
    # pusch_processor_validator_impl and assert_pdu
    ("DM-RS type 2", "a", dict(dmrs_type=2), {}, False),
    ("1 CDM group without data", "a", dict(nof_cdm_groups_without_data=1), {}, False),
    ("3 CDM groups without data", "a", dict(nof_cdm_groups_without_data=3), {}, False),
    ("no layer", "a", dict(nof_layers=0), {}, False), ("3 layers", "d", dict(nof_layers=3), {}, False),
    ("tbs_lbrm 0", "a", dict(tbs_lbrm_bytes=0), {}, False),
    ("DC outside the grid", "a", dict(dc_position=NSUBC), {}, False), ("DC on the last subcarrier", "a", dict(dc_position=NSUBC - 1), {}, True),
    ("a CSI part 2 description", "c", dict(nof_csi_part2_entries=1), {}, False),
    ("neither a codeword nor UCI", "e", dict(nof_harq_ack=0, nof_csi_part1=0), {}, False),
    # the stage validators
    ("no rx port", "a", dict(rx_ports=()), {}, False), ("5 rx ports", "a", dict(rx_ports=(0, 1, 2, 3, 0)), {}, False),
    ("an rx port outside the grid", "a", dict(rx_ports=(4,)), {}, False), ("a repeated rx port", "b", dict(rx_ports=(1, 1)), {}, False),
    ("2 layers on 3 ports", "d", dict(rx_ports=(0, 1, 2)), {}, False),
    ("a PRB beyond the grid", "a", dict(prbs=range(20, 26)), {}, False), ("no PRB", "a", dict(prbs=()), {}, False),
    ("symbols beyond the slot", "a", dict(start_symbol=1), {}, False),
    ("a DM-RS symbol outside the allocation", "a", dict(nof_symbols=11), {}, False), ("no DM-RS symbol", "a", dict(dmrs_symbols=()), {}, False),
    ("slot index beyond the frame", "a", dict(slot_index=10), {}, False), ("numerology 5", "a", dict(numerology=5), {}, False),
    ("scrambling_id above 65535", "a", dict(scrambling_id=65536), {}, False), ("n_scid 2", "a", dict(n_scid=2), {}, False),
    ("rnti above 65535", "a", dict(rnti=65536), {}, False), ("n_id above 1023", "a", dict(n_id=1024), {}, False),
    ("BPSK", "a", dict(modulation=1), {}, False), ("an unknown modulation", "a", dict(modulation=3), {}, False),
    ("rv 4", "a", dict(rv=4), {}, False), ("base graph 3", "a", dict(ldpc_base_graph=3), {}, False),
    ("a codeword without bytes", "a", dict(tb_size_bytes=0, has_codeword=1), {}, False),
    ("bytes without a codeword", "a", dict(has_codeword=0), {}, False),
    ("a code rate of 1", "a", dict(target_code_rate=1024.0), {}, False),
    ("1707 HARQ-ACK bits", "d", dict(nof_harq_ack=1707), {}, False),
    ("HARQ-ACK without a beta offset", "c", dict(beta_offset_harq_ack=0.0), {}, False),
    ("alpha 2 without UL-SCH: the reference's subtraction wraps", "e", dict(alpha_scaling=2.0, nof_harq_ack=100, beta_offset_harq_ack=20.0), {}, False),
    # the processor's configuration
    ("no decoder iteration", "a", {}, dict(dec_nof_iterations=0), False), ("early stop 2", "a", {}, dict(dec_enable_early_stop=2), False),
    ("the EVM-based SINR", "a", {}, dict(csi_sinr_calc_method=abi.PUSCH_SINR_EVM), False),
    ("an unknown SINR method", "a", {}, dict(csi_sinr_calc_method=3), False),
    ("an unknown equaliser", "a", {}, dict(equalizer=2), False), ("MMSE with two layers", "d", {}, dict(equalizer=abi.EQ_MMSE), False),
])
def test_pusch_proc_validator(name, case, pdu_change, opt_change, want):
    pdu = abi.make_pusch_pdu(**dict(pdu_args()[case], **pdu_change))
    opts = _opts(**opt_change)
    assert (lib.pusch_proc_validate(pdu, opts, NPORTS, NSUBC) == abi.OK) == want, name
    assert (lib.pusch_proc_derive(pdu, opts, NPORTS, NSUBC) is not None) == want, name


def test_pusch_proc_validator_against_the_grid():
    pdu = make_pdus("c")[0]
    assert lib.pusch_proc_validate(pdu, OPTIONS, 4, 12 * 15) == abi.OK
    assert lib.pusch_proc_validate(pdu, OPTIONS, 4, 12 * 14) == abi.ERR_ARGUMENT  # PRB 14 is beyond the grid
    assert lib.pusch_proc_validate(pdu, OPTIONS, 3, NSUBC) == abi.ERR_ARGUMENT    # port 3 is
    assert lib.pusch_proc_validate(pdu, OPTIONS, 4, 12 * 15 + 1) == abi.ERR_ARGUMENT


def by_hand(a, opts):
    """The stage configurations of one PDU (keyword arguments of make_pusch_pdu), written out as pusch_processor_impl::process
    derives them, the sizes from nrphy_ul_sch_info."""
    g = lambda k, default=0: a.get(k, default)
    prbs, qm, layers, dmrs = list(a["prbs"]), a["modulation"], a["nof_layers"], a["dmrs_symbols"]
    mask = sum(1 << l for l in dmrs)
    tb = g("tb_size_bytes")
    dc = g("dc_position", None)
    info = lib.ulsch_info(abi.make_ulsch_info_cfg(
        tbs_bits=8 * tb, modulation=qm, target_code_rate=a["target_code_rate"], nof_harq_ack_bits=g("nof_harq_ack"),
        nof_csi_part1_bits=g("nof_csi_part1"), nof_csi_part2_bits=0, alpha_scaling=a["alpha_scaling"],
        beta_offset_harq_ack=a["beta_offset_harq_ack"], beta_offset_csi_part1=a["beta_offset_csi_part1"],
        beta_offset_csi_part2=a["beta_offset_csi_part2"], nof_rb=len(prbs), start_symbol_index=0, nof_symbols=14, dmrs_type=1,
        dmrs_symbol_mask=mask, nof_cdm_groups_without_data=2, nof_layers=layers, contains_dc=int(dc is not None and dc // 12 in prbs)))
    chest = abi.make_pusch_chest(prbs=prbs, slot_index=a["slot_index"], scrambling_id=a["scrambling_id"], n_scid=a["n_scid"], scaling=BETA,
                                 dmrs_symbols=dmrs, nof_layers=layers, rx_ports=a["rx_ports"], dc_position=dc)
    demod = abi.make_pusch_demod(prbs=prbs, qm=qm, rnti=a["rnti"], n_id=a["n_id"], dmrs_symbols=dmrs, nof_cdm_groups_without_data=2,
                                 nof_layers=layers, rx_ports=a["rx_ports"], equalizer=opts.equalizer)
    demux = abi.make_ulsch_demux(modulation=qm, nof_layers=layers, nof_prb=len(prbs), start_symbol_index=0, nof_symbols=14, dmrs_type=0,
                                 dmrs_symbol_mask=mask, nof_cdm_groups_without_data=2, nof_harq_ack_rvd=info.nof_harq_ack_rvd,
                                 nof_harq_ack_bits=g("nof_harq_ack"), nof_enc_harq_ack_bits=info.nof_harq_ack_bits,
                                 nof_csi_part1_bits=g("nof_csi_part1"), nof_enc_csi_part1_bits=info.nof_csi_part1_bits, rnti=a["rnti"],
                                 n_id=a["n_id"])
    uci = [abi.make_uci_decoder(bits, enc, qm) for bits, enc in ((g("nof_harq_ack"), info.nof_harq_ack_bits),
                                                                 (g("nof_csi_part1"), info.nof_csi_part1_bits)) if bits]
    codeword_bits = (14 - len(dmrs)) * 12 * len(prbs) * layers * qm
    nof_sch_bits = lib.ulsch_demux_sizes(demux)[0] if uci else codeword_bits
    decoder = None
    if tb:
        b = 8 * tb + (16 if 8 * tb <= 3824 else 24)
        kcb = 8448 if a["ldpc_base_graph"] == 1 else 3840
        nof_cb = 1 if b <= kcb else -(-b // (kcb - 24))
        nref = min(a["tbs_lbrm_bytes"] * 8 * 3 // (2 * nof_cb), 25344)
        assert info.nof_ul_sch_bits == nof_sch_bits
        decoder = abi.PuschDecoderCfg(a["ldpc_base_graph"], qm, g("rv"), layers, nref, tb, info.nof_ul_sch_bits // qm,
                                      opts.dec_nof_iterations, opts.dec_enable_early_stop, g("new_data", 1))
    return dict(info=info, chest=chest, demod=demod, demux=demux, uci=uci, decoder=decoder, codeword_bits=codeword_bits,
                nof_sch_bits=nof_sch_bits)


def test_derive_equals_the_configurations_built_by_hand():
    for opts in (OPTIONS, _opts(equalizer=abi.EQ_MMSE, dec_nof_iterations=6, dec_enable_early_stop=0)):
        for name, a in pdu_args().items():
            if a["nof_layers"] == 2 and opts.equalizer == abi.EQ_MMSE:
                continue
            d = lib.pusch_proc_derive(abi.make_pusch_pdu(**a), opts, NPORTS, NSUBC)
            want = by_hand(a, opts)
            for part in ("info", "chest", "demod"):
                assert bytes(getattr(d, part)) == bytes(want[part]), (name, part)
            assert (d.nof_uci, d.has_decoder, d.codeword_bits, d.nof_sch_bits) == (len(want["uci"]), int(want["decoder"] is not None),
                                                                                 want["codeword_bits"], want["nof_sch_bits"]), name
            if want["uci"]:
                assert bytes(d.demux) == bytes(want["demux"]), name
            for k, u in enumerate(want["uci"]):
                assert bytes(d.uci[k]) == bytes(u), (name, k)
            if want["decoder"] is not None:
                assert bytes(d.decoder) == bytes(want["decoder"]), name
            assert lib.pusch_demod_codeword_bits(d.demod) == d.codeword_bits
    # the cases are what they claim to be
    d = {n: lib.pusch_proc_derive(abi.make_pusch_pdu(**a), OPTIONS, NPORTS, NSUBC) for n, a in pdu_args().items()}
    assert d["b"].info.nof_harq_ack_rvd > d["b"].info.nof_harq_ack_bits > 0 and d["b"].info.nof_dc_overlap_bits == 14 * 4
    assert d["a"].info.nof_dc_overlap_bits == 0 and d["d"].info.nof_dc_overlap_bits == 14 * 4
    assert d["c"].uci[0].message_length == 4 and d["c"].uci[1].message_length == 7
    assert d["d"].uci[0].message_length == 20 and d["d"].uci[1].message_length == 40 and d["d"].decoder.nof_layers == 2
    assert d["e"].has_decoder == 0 and d["e"].info.has_sch == 0 and d["e"].info.nof_csi_part1_bits > 0
    assert d["f"].chest.dmrs_symbol_mask == (1 << 2) | (1 << 7) | (1 << 11)


def test_harq_bytes_without_a_device():
    opts = OPTIONS
    for name, a in pdu_args().items():
        soft, state = lib.pusch_proc_harq_bytes(abi.make_pusch_pdu(**a), opts)
        assert (soft > 0) == (state > 0) == (name != "e"), name


# =======================================================================================================================
# GPU: the transmitter
# =======================================================================================================================
def modulate(bits, qm):
    """TS 38.211 Section 5.1: QPSK, 16-QAM, 64-QAM."""
    s = 1.0 - 2.0 * bits.reshape(-1, qm).astype(np.float64)
    if qm == 2:
        return (s[:, 0] + 1j * s[:, 1]) / np.sqrt(2)
    if qm == 4:
        return (s[:, 0] * (2 - s[:, 2]) + 1j * s[:, 1] * (2 - s[:, 3])) / np.sqrt(10)
    assert qm == 6
    return (s[:, 0] * (4 - s[:, 2] * (2 - s[:, 4])) + 1j * s[:, 1] * (4 - s[:, 3] * (2 - s[:, 5]))) / np.sqrt(42)


def scramble(codeword, rnti, n_id):
    """TS 38.211 Section 6.3.1.1 with the placeholders: x sends 1, y repeats the bit sent before it."""
    cw = np.asarray(codeword, np.int64)
    seq = uci_model.gold_bits((rnti << 15) + n_id, cw.size).astype(np.int64)
    sent = np.where(cw == uci_model.PLACEHOLDER_ONE, 1, (cw & 1) ^ seq)
    for i in np.flatnonzero(cw == uci_model.PLACEHOLDER_REPEAT):
        sent[i] = sent[i - 1]
    return sent.astype(np.uint8)


class Sent:
    """One PDU's transmission: the payloads and the noiseless received grid [NPORTS][14][nsubc]."""


def transmit(ctx, pdu, derived, rng, nsubc=NSUBC):
    d, s = derived, Sent()
    qm, layers = pdu.modulation, pdu.nof_tx_layers
    demux = {f[0]: int(getattr(d.demux, f[0])) for f in abi.UlschDemuxCfg._fields_}
    s.tb = rng.integers(0, 256, pdu.tb_size_bytes, dtype=np.uint8)
    sch = np.zeros(d.nof_sch_bits, np.uint8)
    if d.has_decoder:
        sch, _ = ctx.pdsch_encode_host(pdu.ldpc_base_graph, pdu.rv, qm, d.decoder.nref, layers, d.nof_sch_bits // qm, s.tb)
    s.harq = rng.integers(0, 2, pdu.nof_harq_ack, dtype=np.uint8)
    s.csi1 = rng.integers(0, 2, pdu.nof_csi_part1, dtype=np.uint8)
    if d.nof_uci:
        coded = [uci_model.encode(m, e, qm) if m.size else np.zeros(0, np.uint8)
                 for m, e in ((s.harq, d.info.nof_harq_ack_bits), (s.csi1, d.info.nof_csi_part1_bits))]
        codeword = uci_model.ulsch_multiplex(demux, sch, coded[0], coded[1])
    else:
        codeword = sch
    assert codeword.size == d.codeword_bits
    symbols = modulate(scramble(codeword, pdu.rnti, pdu.n_id), qm).reshape(-1, layers)  # [RE][layer]
    prbs = chest_model.prbs_of(d.chest)
    subc = (12 * np.array(prbs)[:, None] + np.arange(12)).ravel()
    x = np.zeros((layers, 14, nsubc), np.complex128)
    at = 0
    for l in range(14):
        if (pdu.dmrs_symbol_mask >> l) & 1:
            for layer in range(layers):
                pr, pi, kk = chest_model.pilots(d.chest, l, layer)
                x[layer, l, kk] = BETA * (pr + 1j * pi)
        else:
            x[:, l, subc] = symbols[at:at + subc.size].T
            at += subc.size
    assert at == symbols.shape[0]
    # the link test's channel: two taps per (port, layer), a common delay of 3 samples at 4096 x SCS, a CFO of 250 Hz
    k = np.arange(nsubc)
    ports = pdu.nof_rx_ports
    H = np.zeros((ports, layers, nsubc), np.complex128)
    for p in range(ports):
        for layer in range(layers):
            g = (1.0 if (p % layers) == layer else 0.35) * np.exp(1j * rng.uniform(0, 2 * np.pi))
            H[p, layer] = g * np.exp(-2j * np.pi * k * 3 / 4096.0) * (1 + 0.3 * np.exp(-2j * np.pi * k * rng.uniform(1, 8) / 4096.0))
    rot = np.exp(2j * np.pi * (250.0 / 15000.0) * np.array(chest_model.epochs(0), np.float64))
    s.clean = np.zeros((NPORTS, 14, nsubc), np.complex128)
    for p in range(ports):
        s.clean[pdu.rx_ports[p]] = np.einsum("lk,lmk->mk", H[p], x) * rot[:, None]
    return s


def noisy(sent, snr_db, rng):
    """Every port of the grid gets noise, the ones the PDU does not read too."""
    nv = 10.0 ** (-snr_db / 10.0)
    noise = (rng.standard_normal(sent.clean.shape) + 1j * rng.standard_normal(sent.clean.shape)) * np.sqrt(nv / 2)
    return chest_model.to_cbf16((sent.clean + noise).astype(np.complex64))


# =======================================================================================================================
# GPU: the two ways through the library
# =======================================================================================================================
def align(v, a=256):
    return (v + a - 1) // a * a


class Layout:
    """The caller's buffers of a batch: HARQ arena (soft block, then state block per PDU), transport blocks, UCI payloads."""

    def __init__(self, pdus, opts):
        self.soft, self.state, self.tb, self.uci, self.sizes = [], [], [], [], []
        harq = tb = uci = 0
        for p in pdus:
            soft_bytes, state_bytes = lib.pusch_proc_harq_bytes(p, opts)
            self.sizes.append((soft_bytes, state_bytes))
            self.soft.append(harq)
            self.state.append(harq + align(soft_bytes))
            harq = self.state[-1] + align(state_bytes)
            self.tb.append(tb)
            tb += align(p.tb_size_bytes, 4) + 4
            self.uci.append(uci)
            uci += p.nof_harq_ack + p.nof_csi_part1 + 3
        self.harq_bytes, self.tb_bytes, self.uci_bytes = max(harq, 256), max(tb, 4), max(uci, 4)


def guarded(nbytes):
    import torch
    whole = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes]


def guards_intact(whole):
    a = whole.cpu().numpy()
    return bool((a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all())


class Buffers:
    def __init__(self, layout, n, d_harq=None):
        import torch
        self.harq = torch.zeros(layout.harq_bytes, dtype=torch.uint8, device="cuda") if d_harq is None else d_harq
        self.tb_whole, self.tb = guarded(layout.tb_bytes)
        self.uci_whole, self.uci = guarded(layout.uci_bytes)
        self.result_whole, self.result = guarded(n * RESULT_DTYPE.itemsize)

    def read(self):
        assert guards_intact(self.tb_whole) and guards_intact(self.uci_whole) and guards_intact(self.result_whole)
        return dict(harq=self.harq.cpu().numpy().copy(), tb=self.tb.cpu().numpy().copy(), uci=self.uci.cpu().numpy().copy(),
                    result=self.result.cpu().numpy().copy().view(RESULT_DTYPE))


class HandChain:
    """The PDUs driven through the existing entry points with the configurations nrphy_pusch_proc_derive returned."""

    def __init__(self, ctx, pdus, derived, layout, ngrids, gidx, nsubc=NSUBC):
        import torch
        self.ctx, self.pdus, self.derived, self.layout, self.n = ctx, pdus, derived, layout, len(pdus)
        sizes = [d.chest.nof_tx_layers * d.chest.nof_rx_ports * 14 * nsubc for d in derived]
        offs = [int(o) for o in np.cumsum([0] + sizes)[:-1]]
        self.cplan = lib.PuschChestPlan(ctx, [d.chest for d in derived], gidx, ngrids, NPORTS, nsubc, offs)
        self.dplan = lib.PuschDemodPlan(ctx, [d.demod for d in derived], gidx, ngrids, NPORTS, nsubc, offs)
        self.stride = align(max(d.codeword_bits for d in derived), 16)
        self.with_uci = [i for i, d in enumerate(derived) if d.nof_uci]
        self.sch_off, self.uci_plan, self.demux = {}, None, None
        sch = llr = 0
        harq_off, csi1_off, cfgs, llr_offs, msg_offs, self.status_of = [], [], [], [], [], {}
        for i in self.with_uci:
            d, p = derived[i], pdus[i]
            self.sch_off[i] = sch
            sch += align(d.nof_sch_bits, 16)
            harq_off.append(0)
            csi1_off.append(0)
            msg = layout.uci[i]
            for k in range(d.nof_uci):
                is_harq = k == 0 and p.nof_harq_ack != 0
                (harq_off if is_harq else csi1_off)[-1] = llr
                self.status_of[(i, "harq" if is_harq else "csi1")] = len(cfgs)
                cfgs.append(d.uci[k])
                llr_offs.append(llr)
                msg_offs.append(msg)
                llr += align(d.uci[k].llr_length, 16)
                msg += d.uci[k].message_length
        if self.with_uci:
            self.demux = lib.UlschDemuxPlan(ctx, [derived[i].demux for i in self.with_uci], [i * self.stride for i in self.with_uci],
                                            [self.sch_off[i] for i in self.with_uci], harq_off, csi1_off, None)
            self.uci_plan = lib.UciDecoderPlan(ctx, cfgs, llr_offs, msg_offs)
        self.ce = torch.zeros(sum(sizes), dtype=torch.int32, device="cuda")
        self.nv = torch.zeros((self.n, 4), dtype=torch.float32, device="cuda")
        self.meas = torch.zeros((self.n, 4, 2, MEAS_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        self.llr = torch.zeros((self.n, self.stride), dtype=torch.int8, device="cuda")
        self.sinr = torch.zeros(self.n, dtype=torch.float32, device="cuda")
        self.sch = torch.zeros(max(sch, 16), dtype=torch.int8, device="cuda")
        self.uci_llr = torch.zeros(max(llr, 16), dtype=torch.int8, device="cuda")
        self.status = torch.zeros(max(len(cfgs), 1), dtype=torch.int32, device="cuda")
        self.res = torch.zeros((self.n, 4), dtype=torch.int32, device="cuda")

    def run(self, d_grid, B, stream=None):
        L = self.layout
        self.cplan.run(d_grid, self.ce, self.nv, self.meas, stream=stream)
        self.dplan.run(d_grid, self.ce, self.nv, self.llr, self.stride, self.sinr, stream=stream)
        if self.demux is not None:
            self.demux.run(self.llr, self.sch, self.uci_llr, self.uci_llr, None, stream=stream)
            self.uci_plan.run(self.uci_llr, B.uci, self.status, stream=stream)
        for i, d in enumerate(self.derived):
            if d.has_decoder:
                llr = self.sch[self.sch_off[i]:] if d.nof_uci else self.llr[i]
                self.ctx.pusch_decode_batch(d.decoder, 1, llr, d.nof_sch_bits, B.harq[L.soft[i]:].view(torch_int8()), B.harq[L.state[i]:],
                                            B.tb[L.tb[i]:], d.decoder.tb_size_bytes, self.res[i], stream=stream)

    def read(self):
        return dict(res=self.res.cpu().numpy().view(np.uint32).copy(), status=self.status.cpu().numpy().view(np.uint32).copy(),
                    sinr=self.sinr.cpu().numpy().copy(), meas=self.meas.cpu().numpy().reshape(-1).view(MEAS_DTYPE).reshape(self.n, 4, 2).copy())

    def close(self):
        for p in (self.cplan, self.dplan, self.demux, self.uci_plan):
            if p is not None:
                p.close()


def torch_int8():
    import torch
    return torch.int8


def to_db(x):
    """convert_power_to_dB as the library evaluates it: log10 in double, rounded once, times 10 in float."""
    return f32(f32(10) * f32(np.log10(np.float64(f32(x)))))


def csi_restatement(meas, nof_ports):
    """channel_estimate::get_channel_state_information and get_layer_average_snr(0) in float32, sums in port order."""
    epre = rsrp = noise = best_snr = f32(0)
    best = 0
    for p in range(nof_ports):
        m = meas[p, 0]
        epre, rsrp, noise = f32(epre + m["epre"]), f32(rsrp + m["rsrp"]), f32(noise + m["noise_var"])
        if m["snr"] > best_snr:
            best_snr, best = m["snr"], p
    snr = f32(rsrp / noise) if np.isfinite(noise) and abs(noise) >= np.finfo(np.float32).tiny else f32(1e6)
    cfo = meas[best, 0]["cfo_hz"]
    return dict(epre_dB=to_db(f32(epre / f32(nof_ports))), rsrp_dB=to_db(f32(rsrp / f32(nof_ports))), sinr_ch_estimator_dB=to_db(snr),
                time_alignment_s=meas[best, 0]["ta_s"], has_cfo=int(not np.isnan(cfo)), cfo_hz=f32(0) if np.isnan(cfo) else cfo)


def ulps(a, b):
    key = lambda v: int(np.array(v, np.float32).view(np.int32)) if v >= 0 else -int((np.array(-v, np.float32)).view(np.int32))
    return abs(key(f32(a)) - key(f32(b)))


def assert_equal_to_the_hand_chain(names, pdus, derived, layout, got, want_buf, want, sinr_method, has_cfo=1):
    """got: Buffers.read() of the processor; want_buf / want: Buffers.read() and HandChain.read() of the hand-driven chain."""
    assert got["tb"].tobytes() == want_buf["tb"].tobytes()
    assert got["uci"].tobytes() == want_buf["uci"].tobytes()
    assert got["harq"].tobytes() == want_buf["harq"].tobytes()
    hand_status = lambda i, part, chain_status_of: want["status"][chain_status_of[(i, part)]] if (i, part) in chain_status_of else abi.UCI_STATUS_UNKNOWN
    for i, (name, p, d) in enumerate(zip(names, pdus, derived)):
        r = got["result"][i]
        words = want["res"][i] if d.has_decoder else np.zeros(4, np.uint32)
        assert (r["has_sch"], r["tb_crc_ok"], r["nof_codeblocks_ok"], r["ldpc_iterations_sum"], r["ldpc_iterations_max"]) == \
            (d.has_decoder, words[0], words[1], words[2], words[3]), name
        assert r["nof_codeblocks"] == nof_codeblocks(p), name
        assert (r["nof_harq_ack"], r["nof_csi_part1"]) == (p.nof_harq_ack, p.nof_csi_part1), name
        assert r["harq_ack_status"] == hand_status(i, "harq", want["status_of"]), name
        assert r["csi_part1_status"] == hand_status(i, "csi1", want["status_of"]), name
        if p.nof_harq_ack:
            assert r["harq_ack_offset"] == layout.uci[i], name
        if p.nof_csi_part1:
            assert r["csi_part1_offset"] == layout.uci[i] + p.nof_harq_ack, name
        assert np.array(r["sinr_post_eq_dB"]).view(np.uint32) == want["sinr"][i:i + 1].view(np.uint32)[0], name
        csi = csi_restatement(want["meas"][i], p.nof_rx_ports)
        for field in ("epre_dB", "rsrp_dB", "sinr_ch_estimator_dB"):
            assert ulps(r[field], csi[field]) <= 1, (name, field, r[field], csi[field])
        for field in ("time_alignment_s", "cfo_hz"):
            assert np.array(r[field]).view(np.uint32) == np.array(csi[field], np.float32).view(np.uint32), (name, field)
        assert r["has_cfo"] == csi["has_cfo"] == has_cfo and (r["has_evm"], r["evm"]) == (0, 0.0), name
        selected = "sinr_post_eq_dB" if sinr_method == abi.PUSCH_SINR_POST_EQUALIZATION else "sinr_ch_estimator_dB"
        assert np.array(r["sinr_dB"]).view(np.uint32) == np.array(r[selected]).view(np.uint32), name


class Scenario:
    """PDUs `names` on a grid each, transmitted once under a fixed seed (shared by the tests of a session)."""
    cache = {}

    def __init__(self, ctx, names, opts, seed=2024, **override):
        self.names, self.opts = names, opts
        self.pdus = make_pdus(names, **override)
        self.derived = [lib.pusch_proc_derive(p, opts, NPORTS, NSUBC) for p in self.pdus]
        assert None not in self.derived
        self.rng = np.random.default_rng(seed)
        self.sent = [transmit(ctx, p, d, self.rng) for p, d in zip(self.pdus, self.derived)]
        self.layout = Layout(self.pdus, opts)
        self.gidx = list(range(len(names)))

    @classmethod
    def get(cls, ctx, names, equalizer):
        key = (names, equalizer)
        if key not in cls.cache:
            cls.cache[key] = cls(ctx, names, _opts(equalizer=equalizer, csi_sinr_calc_method=abi.PUSCH_SINR_POST_EQUALIZATION
                                                   if equalizer == abi.EQ_MMSE else abi.PUSCH_SINR_CHANNEL_ESTIMATOR))
        return cls.cache[key]

    def grids(self, good):
        rng = np.random.default_rng(77 if good else 78)
        return np.stack([noisy(s, GOOD_SNR[(p.modulation, p.nof_tx_layers)] if good else BAD_SNR, rng)
                         for s, p in zip(self.sent, self.pdus)])

    def plan(self, ctx):
        L = self.layout
        return lib.PuschProcPlan(ctx, self.pdus, self.opts, self.gidx, len(self.names), NPORTS, NSUBC, L.soft, L.state, L.tb, L.uci)

    def both(self, ctx, grids, d_harq_proc=None, d_harq_hand=None):
        """One run of the processor and one of the hand-driven chain over `grids`: (got, want_buf, want)."""
        d_grid = dev(as_i32(grids))
        plan = self.plan(ctx)
        B = Buffers(self.layout, len(self.names), d_harq_proc)
        plan.run(d_grid, B.harq, B.tb, B.uci, B.result)
        ctx.synchronize()
        got = B.read()
        plan.close()
        chain = HandChain(ctx, self.pdus, self.derived, self.layout, len(self.names), self.gidx)
        H = Buffers(self.layout, len(self.names), d_harq_hand)
        chain.run(d_grid, H)
        ctx.synchronize()
        want = chain.read()
        want["status_of"] = chain.status_of
        want_buf = H.read()
        chain.close()
        return got, want_buf, want, B, H


@pytest.mark.gpu
@pytest.mark.parametrize("names,equalizer", [("abcdef", abi.EQ_ZF), ("abcef", abi.EQ_MMSE)])
@pytest.mark.parametrize("good", [True, False])
def test_processor_equals_the_hand_driven_chain(gpu_ctx, names, equalizer, good):
    sc = Scenario.get(gpu_ctx, names, equalizer)
    got, want_buf, want, _, _ = sc.both(gpu_ctx, sc.grids(good))
    assert_equal_to_the_hand_chain(names, sc.pdus, sc.derived, sc.layout, got, want_buf, want, sc.opts.csi_sinr_calc_method)
    L = sc.layout
    for i, (name, p, s) in enumerate(zip(names, sc.pdus, sc.sent)):
        r = got["result"][i]
        if good:
            assert r["tb_crc_ok"] == p.has_codeword, (name, r)
            assert got["tb"][L.tb[i]:L.tb[i] + p.tb_size_bytes].tobytes() == s.tb.tobytes(), name
            assert r["nof_codeblocks_ok"] == r["nof_codeblocks"], name
            assert r["harq_ack_status"] == (abi.UCI_STATUS_VALID if p.nof_harq_ack else abi.UCI_STATUS_UNKNOWN), name
            assert r["csi_part1_status"] == (abi.UCI_STATUS_VALID if p.nof_csi_part1 else abi.UCI_STATUS_UNKNOWN), name
            at = L.uci[i]
            assert got["uci"][at:at + p.nof_harq_ack].tobytes() == s.harq.tobytes(), name
            assert got["uci"][at + p.nof_harq_ack:at + p.nof_harq_ack + p.nof_csi_part1].tobytes() == s.csi1.tobytes(), name
            assert -1e-6 < r["time_alignment_s"] < 1e-6 and 100.0 < r["cfo_hz"] < 400.0, (name, r)
            if p.nof_tx_layers == 1:  # with two layers a layer's noise estimate counts the other layer's DM-RS
                assert r["sinr_ch_estimator_dB"] > 3.0 and r["sinr_post_eq_dB"] > 3.0, (name, r)
        else:
            assert r["tb_crc_ok"] == 0, (name, r)


@pytest.mark.gpu
def test_harq_retransmission_equals_the_hand_driven_chain(gpu_ctx):
    """(a) sent twice to the same HARQ blocks: rv 0 with new_data 1 at an SNR where it fails, then rv 2 with new_data 0."""
    import torch
    opts = OPTIONS
    first = Scenario(gpu_ctx, "a", opts, seed=5, rv=0, new_data=1)
    second = Scenario(gpu_ctx, "a", opts, seed=5, rv=2, new_data=0)
    assert second.sent[0].tb.tobytes() == first.sent[0].tb.tobytes()
    h_proc = torch.full((first.layout.harq_bytes,), 0x11, dtype=torch.uint8, device="cuda")  # new_data needs no initialised blocks
    h_hand = h_proc.clone()
    rng = np.random.default_rng(9)
    oks = []
    for sc, snr in ((first, -4.0), (second, -4.0)):
        grids = np.stack([noisy(sc.sent[0], snr, rng)])
        got, want_buf, want, _, _ = sc.both(gpu_ctx, grids, h_proc, h_hand)
        assert_equal_to_the_hand_chain("a", sc.pdus, sc.derived, sc.layout, got, want_buf, want, opts.csi_sinr_calc_method)
        assert torch.equal(h_proc, h_hand)
        oks.append(int(got["result"][0]["tb_crc_ok"]))
        if oks[-1]:
            assert got["tb"][:sc.pdus[0].tb_size_bytes].tobytes() == sc.sent[0].tb.tobytes()
    print("tb_crc_ok of the two transmissions:", oks)
    assert oks == [0, 1]  # QPSK at R = 0.44 and -4 dB: the first transmission alone cannot decode, the two combined do
    soft, state = first.layout.sizes[0]
    assert (h_proc.cpu().numpy()[first.layout.state[0] + state:] == 0x11).all()  # nothing behind the state block was touched


@pytest.mark.gpu
def test_single_dmrs_symbol_reports_no_cfo(gpu_ctx):
    """With one DM-RS symbol the estimator has no CFO (NaN in its measurements): the record says has_cfo = 0 and cfo_hz = 0."""
    sc = Scenario(gpu_ctx, "ab", OPTIONS, seed=11, dmrs_symbols=(2,))
    got, want_buf, want, _, _ = sc.both(gpu_ctx, sc.grids(True))
    assert np.isnan(want["meas"][:, 0, 0]["cfo_hz"]).all()
    assert_equal_to_the_hand_chain("ab", sc.pdus, sc.derived, sc.layout, got, want_buf, want, OPTIONS.csi_sinr_calc_method, has_cfo=0)
    assert (got["result"]["has_cfo"] == 0).all() and (got["result"]["cfo_hz"].view(np.uint32) == 0).all()
    # (the channel's 250 Hz go uncompensated with one DM-RS symbol, so the blocks need not decode: no verdict is asked for)


@pytest.mark.gpu
def test_host_form_equals_its_row_of_the_batch(gpu_ctx):
    sc = Scenario.get(gpu_ctx, "abcef", abi.EQ_MMSE)
    grids = sc.grids(True)
    got, _, _, _, _ = sc.both(gpu_ctx, grids)
    i = sc.names.index("c")
    p, L = sc.pdus[i], sc.layout
    result, tb, uci = gpu_ctx.pusch_proc_host(p, sc.opts, grids[i])
    r = got["result"][i]
    for f, _ in abi.PuschResult._fields_:
        if f not in ("harq_ack_offset", "csi_part1_offset"):
            assert np.array(getattr(result, f), RESULT_DTYPE[f]).tobytes() == np.array(r[f]).tobytes(), f
    assert (result.harq_ack_offset, result.csi_part1_offset) == (0, p.nof_harq_ack)
    assert result.tb_crc_ok == 1 and tb.tobytes() == sc.sent[i].tb.tobytes() == got["tb"][L.tb[i]:L.tb[i] + p.tb_size_bytes].tobytes()
    assert uci.tobytes() == got["uci"][L.uci[i]:L.uci[i] + uci.size].tobytes() == np.concatenate([sc.sent[i].harq, sc.sent[i].csi1]).tobytes()


@pytest.mark.gpu
def test_two_runs_and_a_graph_replay_give_identical_bytes(gpu_ctx):
    import torch
    sc = Scenario.get(gpu_ctx, "abcdef", abi.EQ_ZF)
    d_grid = dev(as_i32(sc.grids(True)))
    plan = sc.plan(gpu_ctx)
    outs = []
    for _ in range(2):
        B = Buffers(sc.layout, len(sc.names))
        plan.run(d_grid, B.harq, B.tb, B.uci, B.result)
        gpu_ctx.synchronize()
        outs.append(B.read())
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    G = Buffers(sc.layout, len(sc.names))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.run(d_grid, G.harq, G.tb, G.uci, G.result, stream=C.c_void_p(stream.cuda_stream))
    for _ in range(2):
        G.harq.zero_()
        G.tb.fill_(SENTINEL)
        G.uci.fill_(SENTINEL)
        G.result.zero_()
        graph.replay()
        torch.cuda.synchronize()
        replayed = G.read()
        for k in outs[0]:
            assert replayed[k].tobytes() == outs[0][k].tobytes(), k
    assert all(outs[0]["result"]["tb_crc_ok"] == [p.has_codeword for p in sc.pdus])
    plan.close()


# =======================================================================================================================
# GPU, reference pin: tests/golden/record_pusch_processor_reference.cpp
# =======================================================================================================================
REC_CASES = [(n, good, abi.EQ_ZF) for good in (True, False) for n in "abcdef"] + [("c", True, abi.EQ_MMSE), ("c", False, abi.EQ_MMSE)]


def allocated(pdu, grid):
    """[rx port i][14][12 nof_prb]: what the PDU reads of a grid [NPORTS][14][NSUBC]."""
    prbs = [b for b in range(NPRB_GRID) if (pdu.prb_mask[0] >> b) & 1]
    return grid[[pdu.rx_ports[i] for i in range(pdu.nof_rx_ports)]][:, :, 12 * prbs[0]:12 * (prbs[-1] + 1)]


def write_recorder_inputs(ctx, directory):
    """The recorder's inputs: the grids of (a)-(f) at both SNRs as the composition test transmits them (inputs_grids.npy, uint32, per
    case the allocated region) and one line of numbers per case (inputs_cases.txt, the order of read_case() in the recorder)."""
    sc = Scenario.get(ctx, "abcdef", abi.EQ_ZF)
    grids = {True: sc.grids(True), False: sc.grids(False)}
    words, offs, lines = [], {}, []
    for name, good, eq in REC_CASES:
        i = sc.names.index(name)
        p = sc.pdus[i]
        if (name, good) not in offs:
            offs[(name, good)] = sum(w.size for w in words)
            words.append(allocated(p, grids[good][i]).ravel())
        prbs = [b for b in range(NPRB_GRID) if (p.prb_mask[0] >> b) & 1]
        snr = GOOD_SNR[(p.modulation, p.nof_tx_layers)] if good else BAD_SNR
        lines.append(" ".join(repr(v) for v in (
            i, int(good), snr, p.numerology, p.slot_index, p.rnti, p.n_id, p.scrambling_id, p.n_scid, p.modulation, p.target_code_rate,
            p.has_codeword, p.rv, p.ldpc_base_graph, p.new_data, p.tb_size_bytes, p.tbs_lbrm_bytes, p.nof_harq_ack, p.nof_csi_part1,
            p.alpha_scaling, p.beta_offset_harq_ack, p.beta_offset_csi_part1, p.beta_offset_csi_part2, p.start_symbol_index, p.nof_symbols,
            p.dmrs_symbol_mask, p.nof_tx_layers, p.nof_rx_ports, -1 if p.dc_position == abi.PUSCH_CHEST_NO_DC else p.dc_position, prbs[0],
            len(prbs), eq, offs[(name, good)])))
    np.save(os.path.join(directory, "inputs_grids.npy"), np.concatenate(words).astype(np.uint32))
    open(os.path.join(directory, "inputs_cases.txt"), "w").write("\n".join(lines) + "\n")


GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
RES = ("tb_crc_ok", "nof_codeblocks", "harq_ack_status", "csi_part1_status", "sinr_ch_estimator_dB", "sinr_post_eq_dB", "epre_dB",
       "rsrp_dB", "time_alignment_s", "has_cfo", "cfo_hz", "has_sch")
DB_FIELDS = ("epre_dB", "rsrp_dB", "sinr_ch_estimator_dB")
# The project's estimator and its restatement (tests/pusch_chest_model.py) are pinned to a recording of the reference's estimator
# in tests/test_pusch_channel_estimator.py (smoothed pilots, estimate, per-path measurements, time alignment bin); here the
# processor's aggregated channel state information is compared through that restatement.  REF_DB_SPREAD and
# REF_CFO_SPREAD are the largest distances, over the recorded cases, between what the reference's processor reported and the
# restatement's per-port measurements carried through get_channel_state_information in float64: dB values relative to
# max(|value|, DB_FLOOR), the CFO relative to max(|CFO|, CFO_FLOOR_HZ) -- the floors and the factor 8 are those of tests/test_pucch.py.
# test_restatement_csi_against_the_recording measures and prints them on every run.  The device may be 8 x that away from the
# recording, plus DB_ULPS float32 steps: the largest difference between 10 * (float)log10((double)x), the library's conversion, and
# the reference's convert_power_to_dB, 10.0F * std::log10(float), evaluated in NumPy over the recorded values.  The post-equalisation
# SINR has no restatement of its own: it is -10 log10 of the mean of nv / sum |h|^2, made of the same noise variances and channel
# powers as the estimator's SINR, so it gets that field's allowance.  The time alignment is an integer bin times a constant: 1e-6.
REF_DB_SPREAD = 2.9e-7   # measured 2.82e-07: (d) at its good SNR, sinr_ch_estimator_dB
REF_CFO_SPREAD = 1.6e-7  # measured 1.56e-07
DB_FLOOR, CFO_FLOOR_HZ, DB_ULPS = 1.0, 1.0, 1


def recording():
    import json
    cases = json.load(open(os.path.join(GOLDEN, "pusch_proc_reference_cases.json")))
    load = lambda name: np.load(os.path.join(GOLDEN, "pusch_proc_reference_%s.npy" % name))
    grids, results, tb, uci = load("grids"), load("results"), load("tb"), load("uci")
    pdus = make_pdus("abcdef")
    for c, row in zip(cases, results):
        p = pdus[c["pdu"]]
        assert (c["nof_rx_ports"], c["tb_size_bytes"], c["nof_harq_ack"], c["nof_csi_part1"]) == \
            (p.nof_rx_ports, p.tb_size_bytes, p.nof_harq_ack, p.nof_csi_part1), c  # the recording is of today's (a)-(f)
        c["ref"] = dict(zip(RES, row))
        c["tb"] = tb[c["tb_off"]:c["tb_off"] + c["tb_size_bytes"]]
        c["uci"] = uci[c["uci_off"]:c["uci_off"] + c["nof_harq_ack"] + c["nof_csi_part1"]]
        n = c["nof_rx_ports"] * 14 * 12 * c["prb_count"]
        grid = np.zeros((NPORTS, 14, NSUBC), np.uint32)
        region = grids[c["grid_off"]:c["grid_off"] + n].reshape(c["nof_rx_ports"], 14, 12 * c["prb_count"])
        grid[[p.rx_ports[i] for i in range(p.nof_rx_ports)], :, 12 * c["prb_start"]:12 * (c["prb_start"] + c["prb_count"])] = region
        c["grid"] = grid
    return cases, pdus


def rel(a, b, floor):
    return abs(float(a) - float(b)) / max(abs(float(b)), floor)


def test_recording_is_not_vacuous():
    cases, pdus = recording()
    assert len(cases) == len(REC_CASES) == 14
    assert [(c["pdu"], c["good"], c["equalizer"]) for c in cases] == [("abcdef".index(n), int(g), e) for n, g, e in REC_CASES]
    with_sch = [c for c in cases if c["ref"]["has_sch"]]
    assert {c["ref"]["tb_crc_ok"] for c in with_sch} == {0.0, 1.0}                       # both verdicts
    assert all(c["ref"]["tb_crc_ok"] == c["good"] for c in with_sch)                     # ... where they are expected
    sizes = {n for c in cases for n in (c["nof_harq_ack"], c["nof_csi_part1"]) if n}
    assert {1, 2} <= sizes and sizes & set(range(3, 12)) and [n for n in sizes if n >= 12]  # 1-2 bits, short block, polar
    assert any(not c["ref"]["has_sch"] and c["uci"].size for c in cases)                 # a PDU without codeword
    assert {c["ref"][k] for c in cases for k in ("harq_ack_status", "csi_part1_status")} == {0.0, 1.0, 2.0}
    assert {c["equalizer"] for c in cases} == {abi.EQ_ZF, abi.EQ_MMSE} and all(c["ref"]["has_cfo"] == 1 for c in cases)
    for c in cases:
        if c["good"]:  # the reference decodes what the transmitter of this test sent
            assert all(c["ref"][k] in (0.0, 1.0) for k in ("harq_ack_status", "csi_part1_status")), c["pdu"]


def test_restatement_csi_against_the_recording():
    """The reference's own distance from the restatement's measurements aggregated in float64, and the dB conversions' distance."""
    cases, pdus = recording()
    worst_db, worst_cfo, where, ulps_db, seen = 0.0, 0.0, None, 0, set()
    for c in cases:
        if (c["pdu"], c["good"]) in seen:
            continue
        seen.add((c["pdu"], c["good"]))
        p = pdus[c["pdu"]]
        cfg = lib.pusch_proc_derive(p, OPTIONS, NPORTS, NSUBC).chest
        m = [chest_model.estimate_port_layer(cfg, c["grid"], i, 0)[2] for i in range(p.nof_rx_ports)]
        f = lambda k: np.array([float(x[k]) for x in m])
        best = int(np.argmax(f("snr")))
        want = {"epre_dB": 10 * np.log10(f("epre").mean()), "rsrp_dB": 10 * np.log10(f("rsrp").mean()),
                "sinr_ch_estimator_dB": 10 * np.log10(f("rsrp").sum() / f("noise_var").sum())}
        for k in DB_FIELDS:
            d = rel(c["ref"][k], want[k], DB_FLOOR)
            if d > worst_db:
                worst_db, where = d, (c["pdu"], c["good"], k)
            x = f32(10.0 ** (c["ref"][k] / 10.0))
            ulps_db = max(ulps_db, ulps(to_db(x), f32(10) * np.log10(x, dtype=np.float32)))
        worst_cfo = max(worst_cfo, rel(c["ref"]["cfo_hz"], m[best]["cfo_hz"], CFO_FLOOR_HZ))
        assert abs(c["ref"]["time_alignment_s"] - float(m[best]["ta_s"])) <= 1e-6 * abs(float(m[best]["ta_s"])) + 1e-15, c["pdu"]
    print("recording - float64 aggregation of the restatement: dB %.3g at %s (constant %.3g), CFO %.3g (constant %.3g); dB conversions "
          "%d ulp apart (constant %d)" % (worst_db, where, REF_DB_SPREAD, worst_cfo, REF_CFO_SPREAD, ulps_db, DB_ULPS))
    assert worst_db <= REF_DB_SPREAD and worst_cfo <= REF_CFO_SPREAD and ulps_db <= DB_ULPS


@pytest.mark.gpu
def test_processor_against_the_recording_of_the_reference(gpu_ctx):
    """tb_crc_ok, the transport block where it is 1, the UCI payloads and statuses: exactly the reference's.  The channel state
    information within the allowance above.  LDPC iteration counts are not pinned."""
    cases, pdus = recording()
    worst_db = worst_cfo = 0.0
    for eq in (abi.EQ_ZF, abi.EQ_MMSE):
        mine = [c for c in cases if c["equalizer"] == eq]
        batch = [pdus[c["pdu"]] for c in mine]
        opts = _opts(equalizer=eq)
        layout = Layout(batch, opts)
        plan = lib.PuschProcPlan(gpu_ctx, batch, opts, list(range(len(mine))), len(mine), NPORTS, NSUBC, layout.soft, layout.state,
                                 layout.tb, layout.uci)
        B = Buffers(layout, len(mine))
        plan.run(dev(as_i32(np.stack([c["grid"] for c in mine]))), B.harq, B.tb, B.uci, B.result)
        gpu_ctx.synchronize()
        got = B.read()
        plan.close()
        for i, (c, p) in enumerate(zip(mine, batch)):
            r, ref, what = got["result"][i], c["ref"], ("abcdef"[c["pdu"]], c["good"], eq)
            assert (r["has_sch"], r["tb_crc_ok"], r["nof_codeblocks"]) == (ref["has_sch"], ref["tb_crc_ok"], ref["nof_codeblocks"]), what
            if r["tb_crc_ok"]:
                assert got["tb"][layout.tb[i]:layout.tb[i] + p.tb_size_bytes].tobytes() == c["tb"].tobytes(), what
            assert (r["harq_ack_status"], r["csi_part1_status"]) == (ref["harq_ack_status"], ref["csi_part1_status"]), what
            assert got["uci"][layout.uci[i]:layout.uci[i] + c["uci"].size].tobytes() == c["uci"].tobytes(), what
            for k in DB_FIELDS + ("sinr_post_eq_dB",):
                d = rel(r[k], ref[k], DB_FLOOR)
                worst_db = max(worst_db, d)
                assert abs(float(r[k]) - ref[k]) <= 8 * REF_DB_SPREAD * max(abs(ref[k]), DB_FLOOR) + DB_ULPS * np.spacing(f32(abs(ref[k]))), (what, k, r[k], ref[k])
            worst_cfo = max(worst_cfo, rel(r["cfo_hz"], ref["cfo_hz"], CFO_FLOOR_HZ))
            assert r["has_cfo"] == 1 and rel(r["cfo_hz"], ref["cfo_hz"], CFO_FLOOR_HZ) <= 8 * REF_CFO_SPREAD, (what, r["cfo_hz"], ref["cfo_hz"])
            assert abs(float(r["time_alignment_s"]) - ref["time_alignment_s"]) <= 1e-6 * abs(ref["time_alignment_s"]) + 1e-15, what
    print("device - recording: dB worst %.3g (allowed %.3g + %d ulp), CFO %.3g (allowed %.3g); %d cases" %
          (worst_db, 8 * REF_DB_SPREAD, DB_ULPS, worst_cfo, 8 * REF_CFO_SPREAD, len(cases)))


if __name__ == "__main__":  # python tests/test_pusch_processor.py DIRECTORY (on a GPU): the recorder's inputs
    import sys
    write_recorder_inputs(lib.Context(0), sys.argv[1])
