"""TEST INFRASTRUCTURE: PDU / OFDM configurations shared by the parity tests, the golden generator and bench.py.

BASELINE.json configs: all use normal CP, DM-RS type 1 on symbols {2, 7, 11} with 2 CDM groups
without data, PDSCH symbols 0-11, rnti 1, n_id 0, rv 0, CRB0, no reserved RE, 0 dB, tbs_lbrm = 159749 bytes.
"""
import os

import numpy as np

import backends

abi = backends.abi
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def codebook(name):
    """Precoding matrices of TS 38.214 the reference benchmark uses, stored from the reference
    (tests/golden/generate.py -> codebooks.npz): [1][ports][layers][2] float32."""
    return np.load(os.path.join(GOLDEN, "codebooks.npz"))[name]


def tbs(nof_symb, dmrs_re_per_prb, qm, rate_x1024, layers, n_prb):
    return backends.pkg.lib.tbs_calculate(nof_symb, dmrs_re_per_prb, 0, qm, rate_x1024, layers, n_prb)


def baseline_config(cfg, rnti=1, n_id=0, slot_index=0):
    """(pdu, nof_ports, nof_subc, ofdm_cfg) of BASELINE config 1, 2 or 3."""
    if cfg == 1:   # 10 MHz SISO QPSK R=120/1024, FFT 1024
        n_prb, bw, qm, rate, w, mu, n = 52, 52, 2, 120, codebook("single_port"), 0, 1024
        bg = 2
    elif cfg == 2:  # 20 MHz 2-layer 64-QAM R=873/1024, FFT 2048
        n_prb, bw, qm, rate, w, mu, n = 106, 106, 6, 873, codebook("two_layer_two_ports_0"), 0, 2048
        bg = 1
    elif cfg == 3:  # 100 MHz 4-layer 256-QAM R=948/1024, FFT 4096
        n_prb, bw, qm, rate, w, mu, n = 270, 273, 8, 948, codebook("four_layer_four_ports_0_0"), 1, 4096
        bg = 1
    else:
        raise ValueError(cfg)
    layers = w.shape[2]
    tb_bits = tbs(12, 36, qm, rate, layers, n_prb)
    pdu = abi.make_pdu(slot_index=slot_index, rnti=rnti, n_id=n_id, bwp_start_rb=0, bwp_size_rb=bw, qm=qm,
                       dmrs_symbols=(2, 7, 11), nof_cdm_groups_without_data=2, prb_start=0, prb_count=n_prb,
                       start_symbol=0, nof_symbols=12, base_graph=bg, precoding=w, tb_size_bytes=tb_bits // 8)
    ofdm = abi.OfdmConfig(mu, bw, n, 0, 1.0, 3.5e9 if cfg == 3 else 2.4e9)
    return pdu, w.shape[1], bw * 12, ofdm


def mixed_cell(cell_id, slot_index=0):
    """BASELINE config 4: one 100 MHz cell-slot with four 68-PRB PDUs (QPSK, 16/64/256-QAM), 4 layers each."""
    w = codebook("four_layer_four_ports_0_0")
    pdus = []
    for ue, (qm, rate) in enumerate(((2, 120), (4, 658), (6, 873), (8, 948))):
        tb_bits = tbs(12, 36, qm, rate, 4, 68)
        bg = 2 if (rate <= 256 or tb_bits <= 292 or (tb_bits <= 3824 and rate <= 686)) else 1
        pdus.append(abi.make_pdu(slot_index=slot_index, rnti=ue + 1, n_id=cell_id, bwp_size_rb=273, qm=qm,
                                 dmrs_symbols=(2, 7, 11), prb_start=68 * ue, prb_count=68, nof_symbols=12,
                                 base_graph=bg, precoding=w, tb_size_bytes=tb_bits // 8))
    return pdus, 4, 273 * 12


RESERVED_26 = [
    (range(1, 26, 1), [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1] + [0] * 10),
    (range(1, 26, 2), [0] * 11 + [1], [0, 0, 0, 0, 1] + [0] * 9),
    (range(2, 26, 2), [0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0], [0] * 12 + [1, 0]),
]


def unit_test_like_pdus(rng):
    """PDUs in the style of the reference's pdsch_processor_test_data.h (26-PRB grid, reserved RE patterns, identity
    precoding, 1-4 layers, all modulations, both base graphs, CRB0/PRB0, odd power ratios)."""
    out = []
    for layers in (1, 2, 3, 4):
        for qm in (2, 4, 6, 8):
            n_prb = int(rng.integers(1, 20))
            start = int(rng.integers(1, 26 - n_prb))
            tb_bits = tbs(12, 12 * 4, qm, int(rng.integers(100, 900)), layers, n_prb)
            out.append(abi.make_pdu(
                slot_index=int(rng.integers(0, 20)), rnti=int(rng.integers(1, 65535)), bwp_start_rb=1, bwp_size_rb=25,
                qm=qm, n_id=int(rng.integers(0, 1024)), dmrs_symbols=(2, 5, 8, 11),
                scrambling_id=int(rng.integers(0, 65536)), n_scid=layers & 1, nof_cdm_groups_without_data=2,
                prb_start=start, prb_count=n_prb, start_symbol=2, nof_symbols=12, base_graph=1 + (qm < 6),
                reserved=RESERVED_26, precoding=abi.identity_precoding(layers), tb_size_bytes=tb_bits // 8,
                ref_point=layers & 1, ratio_dmrs_dB=-3.0 if layers > 2 else 0.0, ratio_data_dB=1.5 * (layers - 1),
                rv=(layers + qm) % 4))
    return out


def random_tb(rng, pdu):
    return rng.integers(0, 256, pdu.tb_size_bytes, dtype=np.uint8)


# ---- LDPC decoder ("next" row) -------------------------------------------------------------------------
def make_ldpc_llrs(oracle, rng, bg, zc, nof_llr, crc_poly_id, nof_filler, amplitude, sigma):
    """A valid codeblock (random payload + CRC + filler zeros) encoded by the oracle, turned into noisy int8 LLRs."""
    kb = 22 if bg == 1 else 10
    K = kb * zc
    crc_len = 16 if crc_poly_id == 16 else 24
    payload = rng.integers(0, 2, K - nof_filler - crc_len, dtype=np.uint8)
    crc = oracle.crc_bits(crc_poly_id, payload)
    msg = np.concatenate([payload, [(crc >> (crc_len - 1 - i)) & 1 for i in range(crc_len)],
                          np.zeros(nof_filler, np.uint8)]).astype(np.uint8)
    cb = oracle.ldpc_encode(bg, zc, np.packbits(msg), nof_llr)
    bits = np.unpackbits(cb)[:nof_llr].astype(np.float64)
    llr = (1.0 - 2.0 * bits) * amplitude + rng.normal(0.0, sigma, nof_llr)
    return msg, np.clip(np.rint(llr), -120, 120).astype(np.int8)


LDPC_DECODE_CASES = [
    # bg, zc, nof_llr (in units of zc beyond K: total = K + extra * zc + tail), extra, tail, crc, filler, amp, sigma
    (1, 384, 4, 0, 0x24B, 72, 24, 0),      # config-3 codeblock, noiseless, high rate (four layers)
    (1, 384, 4, 120, 0x24B, 72, 20, 9),    # partial last node, noise
    (1, 384, 12, 0, 0x24B, 0, 16, 10),
    (1, 128, 44, 0, 0x24A, 40, 10, 7),     # full base graph 1, low rate
    (2, 352, 6, 33, 0x24B, 24, 14, 8),     # config-4 QPSK user: BG2
    (2, 144, 40, 0, 16, 104, 8, 6),        # config 1: BG2, CRC16, every layer
    (2, 6, 10, 3, 16, 2, 30, 12),          # tiny lifting size
    (1, 384, 6, 0, 0x24B, 72, 6, 9),       # too noisy: must fail the CRC after max_iterations
]


def ldpc_decode_nof_llr(case):
    bg, zc, extra, tail = case[:4]
    kb = 22 if bg == 1 else 10
    return max(kb * zc + extra * zc + tail - 2 * zc, kb * zc + 2 * zc)


# ---- LDPC rate dematcher ("next" row) ------------------------------------------------------------------
# (bg, zc, rm_length, rv, qm, nref, nof_filler).  The first 25 are the configurations of the reference's
# ldpc_rate_matcher_test_data.h (BG1, Zc = 14, N = 924, N_ref = 700 when limited-buffer rate matching is on); its
# ldpc_rm_test.cpp runs the dematcher on each of them.  The rest are the shapes of BASELINE configs 1-4 and corner
# cases: repetition (E > N), k0 beyond the systematic part, input ending inside the systematic part.
_REF_RM = [(277, 0, 1, 0, 0), (554, 1, 2, 700, 28), (924, 2, 4, 0, 28), (4620, 3, 6, 0, 0), (9240, 0, 8, 700, 0),
           (208, 1, 4, 700, 0), (420, 0, 6, 0, 12), (700, 3, 1, 700, 12), (3500, 2, 2, 700, 0), (7000, 1, 1, 0, 12),
           (924, 0, 2, 0, 0), (3500, 0, 4, 700, 12), (696, 1, 8, 0, 12), (3500, 1, 1, 700, 0), (276, 2, 6, 700, 28),
           (420, 2, 1, 700, 0), (9240, 2, 2, 0, 28), (210, 3, 2, 700, 0), (552, 3, 4, 0, 28), (7000, 3, 4, 700, 0),
           (924, 1, 6, 0, 28), (6996, 1, 6, 700, 0), (272, 2, 8, 0, 28), (416, 3, 8, 700, 0), (4616, 0, 8, 0, 28)]
LDPC_DEMATCH_CASES = [(1, 14, e, rv, qm, nref, nf) for e, rv, qm, nref, nf in _REF_RM] + [
    (1, 384, 8992, 0, 8, 18432, 72), (1, 384, 8960, 0, 8, 0, 72), (1, 384, 9804, 2, 6, 0, 80),
    (2, 144, 11232, 0, 2, 0, 104), (2, 352, 5000, 3, 4, 8000, 24), (1, 16, 2000, 1, 2, 0, 5),
    (2, 7, 2304, 3, 2, 0, 30), (1, 384, 60, 0, 6, 0, 72), (1, 384, 30000, 3, 8, 0, 0), (2, 384, 19200, 1, 4, 0, 0),
    (1, 384, 65536, 2, 8, 0, 16), (2, 30, 64000, 0, 4, 0, 0),
]


# ---- precoding shapes with exact zeros (signed-zero products in the layer sum) ----------------------------
def diagonal_precoding_variants():
    """[(name, weights [1][P][L] complex64)]: diagonal matrices with real / imaginary / complex entries, one off-diagonal
    entry, a permutation, a zero on the diagonal -- sums in which most products are signed zeros."""
    out = []
    d = np.zeros((1, 4, 4), np.complex64)
    for i, v in enumerate((0.5, -0.5, 0.5j, -0.5j)):
        d[0, i, i] = v
    out.append(("rotated", d))
    d = np.zeros((1, 4, 4), np.complex64)
    for i in range(4):
        d[0, i, i] = 0.70710678
    d[0, 2, 2] = (1 + 1j) * 0.5
    out.append(("complex_entry", d))
    d = np.eye(4, dtype=np.complex64)[None].copy()
    d[0, 1, 3] = 1e-3
    out.append(("off_diagonal", d))
    out.append(("permutation", np.eye(4, dtype=np.complex64)[[1, 0, 3, 2]][None].copy()))
    d = np.eye(4, dtype=np.complex64)[None].copy()
    d[0, 3, 3] = 0
    out.append(("zero_on_diagonal", d))
    d = -np.eye(2, dtype=np.complex64)[None].copy()
    out.append(("two_layers_negative", d))
    return out


LIFTING_SIZES = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 26, 28, 30, 32, 36, 40, 44, 48, 52,
                 56, 60, 64, 72, 80, 88, 96, 104, 112, 120, 128, 144, 160, 176, 192, 208, 224, 240, 256, 288, 320, 352,
                 384]


def ldpc_dec_test_lengths(bg, zc):
    """create_range(min_cb_length, max_cb_length, 3) of the reference's ldpc_enc_dec_test.cpp:237-252."""
    lo, hi = ((24, 66) if bg == 1 else (12, 50))
    lo, hi = lo * zc, hi * zc
    step = (hi - lo) // 3
    return list(range(lo, hi, step)) + [hi]


def noiseless_llrs(oracle, rng, bg, zc, nof_filler, length):
    """A random message (filler bits at the end of it), its codeblock as LLRs of amplitude 10, fillers +10 as the
    reference's LDPCDecTest maps them (ldpc_enc_dec_test.cpp:60-64).  Returns (message bits, llrs)."""
    kb = 22 if bg == 1 else 10
    msg = rng.integers(0, 2, kb * zc, dtype=np.uint8)
    if nof_filler:
        msg[-nof_filler:] = 0
    cb = np.unpackbits(oracle.ldpc_encode(bg, zc, np.packbits(msg), length))[:length]
    return msg, (10 * (1 - 2 * cb.astype(np.int8))).astype(np.int8)


# ---- extended cyclic prefix (12 symbols per slot; the reference's validator and processors accept it) ---------
def extended_cp_pdus(tbs):
    """[(pdu, nof_ports, nof_subc)] with cp = 1: every modulation, 1-4 layers, DM-RS on several of the 12 symbols,
    allocations ending on the last symbol.  tbs: a TBS calculator (oracle.tbs)."""
    out = []
    for layers, qm, dmrs, start, nsym, slot in ((1, 2, (2, 9), 1, 11, 3), (2, 6, (2,), 0, 12, 0), (4, 8, (3, 7, 11), 2, 10, 7),
                                                (3, 4, (0, 6), 0, 9, 19)):
        n_prb = 30
        dmrs_per_prb = 6 * len(dmrs) * 2
        tb_bits = tbs(nsym, dmrs_per_prb, 0, qm, 600.0, layers, n_prb)
        pdu = abi.make_pdu(bwp_size_rb=n_prb, qm=qm, dmrs_symbols=dmrs, prb_start=0, prb_count=n_prb, start_symbol=start,
                           nof_symbols=nsym, precoding=abi.identity_precoding(layers), tb_size_bytes=tb_bits // 8, cp=1,
                           slot_index=slot, scrambling_id=9 + layers, n_id=3, rnti=77, n_scid=layers & 1,
                           base_graph=1 if qm > 2 else 2)
        out.append((pdu, layers, n_prb * 12))
    return out


# ---- PUSCH decoder at transport-block level ("next" row) ------------------------------------------------
def pusch_decoder_shape(oracle, shape):
    """(pdu of the transmit side, nof_ports, nof_subc, LLR amplitude, noise sigma): the noise is set where the first
    transmission leaves codeblocks undecoded and the second (rv 2, combined) completes the transport block."""
    if shape == "cfg2":
        pdu, nof_ports, nof_subc, _ = baseline_config(2)
        return pdu, nof_ports, nof_subc, 10.0, 5.0
    if shape == "cfg1":
        pdu, nof_ports, nof_subc, _ = baseline_config(1)
        return pdu, nof_ports, nof_subc, 4.0, 7.0
    tb_bits = oracle.tbs(12, 12, 0, 2, 400.0, 2, 100)
    pdu = abi.make_pdu(bwp_size_rb=100, qm=2, dmrs_symbols=(2,), prb_start=0, prb_count=100, start_symbol=0, nof_symbols=14,
                       precoding=abi.identity_precoding(2), tb_size_bytes=tb_bits // 8, base_graph=2, rnti=9, n_id=1)
    return pdu, 2, 1200, 6.0, 6.0


def pusch_decode_expected(oracle, d, cfg, llr, soft, cb_ok, cb_msg):
    """pusch_decoder_impl restated on the oracle's codeblock functions (pusch_decoder_impl.cpp:318-497): updates soft /
    cb_ok / cb_msg in place, returns (tb_crc_ok, codeblocks ok, iteration sum, iteration max, transport block or None)."""
    bg, zc, C, n = cfg.base_graph, d["lifting_size"], d["nof_codeblocks"], d["full_length"]
    k, nf, info = d["segment_length"], d["nof_filler_bits"], d["cb_info_bits"]
    crc_id = 0x24B if C > 1 else (16 if d["nof_tb_crc_bits"] == 16 else 0x24A)
    if cfg.new_data:
        cb_ok[:] = 0
    offset, it_sum, it_max = 0, 0, 0
    for r in range(C):
        e = d["rm_length_short"] if r < d["nof_short_segments"] else d["rm_length_long"]
        soft[r] = oracle.ldpc_rate_dematch(bg, zc, cfg.rv, cfg.qm, d["n_ref"], nf, cfg.new_data, llr[offset: offset + e], soft[r])
        offset += e
        if cb_ok[r]:
            continue
        if cfg.use_early_stop:
            it, bits = oracle.ldpc_decode(bg, zc, nf, crc_id, cfg.max_iterations, 0.8, soft[r])
        else:  # pusch_codeblock_decoder.cpp:59-68: all iterations, then the CRC of the bits without the filler
            _, bits = oracle.ldpc_decode(bg, zc, nf, 0, cfg.max_iterations, 0.8, soft[r])
            it = cfg.max_iterations if oracle.crc_bits(crc_id, bits[: k - nf]) == 0 else 0
        cb_msg[r] = bits
        cb_ok[r] = 1 if it else 0
        it_sum += it if it else cfg.max_iterations
        it_max = max(it_max, it if it else cfg.max_iterations)
    n_ok = int(cb_ok.sum())
    tb, tb_ok = None, False
    tb_bits = 8 * cfg.tb_size_bytes
    if n_ok == C:
        if C == 1:
            tb_ok, tb = True, np.packbits(cb_msg[0][:tb_bits])
        else:
            stream = np.concatenate([cb_msg[r][:info] for r in range(C)])[: tb_bits + 24]
            tb = np.packbits(stream[:tb_bits])
            checksum = int("".join(map(str, stream[tb_bits:])), 2)
            tb_ok = oracle.crc(0x24A, tb) == checksum
            if not tb_ok:
                cb_ok[:] = 0
    return tb_ok, n_ok, it_sum, it_max, tb


# ---- NZP-CSI-RS ("next" row, section 8f-2) ---------------------------------------------------------------
def csi_rs_cases(rng):
    """[(name, cfg, nof_ports, nof_subc)]: rows 1-5 of TS 38.211 Table 7.4.1.5.3-1 with every density the row allows, odd
    and even first PRBs and PRB counts (the rounding rules of the 0.5 densities), identity and dense (wideband) precoding,
    both cyclic prefixes."""
    out = []

    def dense(ports, nof_prg):
        return ((rng.standard_normal((nof_prg, ports, ports)) + 1j * rng.standard_normal((nof_prg, ports, ports))) / 2).astype(np.complex64)

    for row, densities, k0s in ((1, ("three",), (0, 3)), (2, ("one", "dot5_even", "dot5_odd"), (0, 11)),
                                (3, ("one", "dot5_even", "dot5_odd"), (0, 10)), (4, ("one",), (0, 8)), (5, ("one",), (2, 10))):
        ports = abi.CSI_ROW_PORTS[row]
        for density in densities:
            for i, (start_rb, nof_rb) in enumerate(((0, 52), (3, 25), (4, 25), (7, 24), (1, 1), (0, 273))):
                k0 = k0s[i % 2]
                prg = None if i % 2 == 0 else dense(ports, 1)
                cfg = abi.make_csi_rs(row=row, start_rb=start_rb, nof_rb=nof_rb, k0=k0, l0=(3 + 2 * i) % 12, density=density,
                                      slot_index=(5 * i + row) % 20, cp=i % 2 if i != 5 else 0, scrambling_id=(97 * i + row) % 1024,
                                      amplitude=0.5 + 0.25 * i, precoding=prg,
                                      prg_size_rb=abi.MAX_RB)
                nof_subc = 12 * max(52, start_rb + nof_rb)
                out.append(("row%d_%s_%d" % (row, density, i), cfg, max(ports, 1 + i % 2 * 3), nof_subc))
    return out


# ---- randomised PDUs (fuzz) --------------------------------------------------------------------------------
def random_pdus(tbs, rng, count):
    """[(pdu, nof_ports, nof_subc)] drawn at random within what the validator accepts: allocation, layers and ports,
    dense wideband precoding, modulation and rate (TBS from the calculator, base graph by the TS 38.212 rule), symbol range,
    DM-RS symbols and CDM groups, reserved patterns off the DM-RS symbols, rv, LBRM size, power ratios, both cyclic
    prefixes.  tbs: a TBS calculator."""
    out = []
    while len(out) < count:
        cp = int(rng.integers(0, 5) == 0)
        nsymb = 12 if cp else 14
        bwp_start = int(rng.integers(0, 20))
        bwp_size = int(rng.integers(6, 120))
        n_prb = int(rng.integers(1, bwp_size + 1))
        prb_start = bwp_start + int(rng.integers(0, bwp_size - n_prb + 1))
        layers = int(rng.integers(1, 5))
        ports = int(rng.integers(layers, 5))
        qm = int(rng.choice([2, 4, 6, 8]))
        start = int(rng.integers(0, 4))
        nsym = int(rng.integers(3, nsymb - start + 1))
        n_dmrs = int(rng.integers(1, min(4, nsym) + 1))
        dmrs = sorted(int(x) for x in rng.choice(np.arange(start, start + nsym), n_dmrs, replace=False))
        groups = int(rng.integers((layers + 1) // 2, 3))
        # wideband precoding only: with more than one PRG the reference's DM-RS processor writes the per-group weights of
        # PRG 1, 2, ... past the end of a one-PRG configuration (dmrs_pdsch_processor_impl.cpp:179,216-221) -- undefined
        # behaviour that the fuzz hit as a crash; the per-PRG data path is covered by the fixed cases
        nof_prg, prg_size = 1, abi.MAX_RB
        w = ((rng.standard_normal((nof_prg, ports, layers)) + 1j * rng.standard_normal((nof_prg, ports, layers))) / 2).astype(np.complex64)
        reserved = []
        free_symbols = [l for l in range(nsymb) if l not in dmrs]
        for _ in range(int(rng.integers(0, 3))):
            if not free_symbols:
                break
            syms = rng.choice(free_symbols, int(rng.integers(1, min(3, len(free_symbols)) + 1)), replace=False)
            r_prbs = list(range(prb_start, prb_start + n_prb, int(rng.integers(1, 4))))
            reserved.append((r_prbs, [int(b) for b in rng.integers(0, 2, 12)], [1 if l in syms else 0 for l in range(14)]))
        rate = float(rng.uniform(60, 948))
        dmrs_re_prb = n_dmrs * (6 * groups)
        tb_bits = tbs(nsym, dmrs_re_prb, 0, qm, rate, layers, n_prb)
        if tb_bits < 24 or tb_bits > 1277992:
            continue
        r = rate / 1024
        bg = 2 if (tb_bits <= 292 or (tb_bits <= 3824 and r <= 0.67) or r <= 0.25) else 1
        pdu = abi.make_pdu(slot_index=int(rng.integers(0, 20)), rnti=int(rng.integers(1, 65520)), bwp_start_rb=bwp_start,
                           bwp_size_rb=bwp_size, qm=qm, rv=int(rng.integers(0, 4)), n_id=int(rng.integers(0, 1024)),
                           ref_point=int(rng.integers(0, 2)), dmrs_symbols=dmrs, scrambling_id=int(rng.integers(0, 65536)),
                           n_scid=int(rng.integers(0, 2)), nof_cdm_groups_without_data=groups, prb_start=prb_start,
                           prb_count=n_prb, start_symbol=start, nof_symbols=nsym, base_graph=bg,
                           tbs_lbrm_bytes=int(rng.choice([3168, 40000, abi.TBS_LBRM_DEFAULT])),
                           reserved=reserved, ratio_dmrs_dB=float(rng.choice([0.0, -3.0, 3.0])),
                           ratio_data_dB=float(rng.uniform(-3, 3)), precoding=w, prg_size_rb=prg_size,
                           tb_size_bytes=tb_bits // 8, cp=cp)
        out.append((pdu, ports, 12 * (bwp_start + bwp_size)))
    return out


def random_pdus_per_prg(tbs, rng, count):
    """[(pdu, nof_ports, nof_subc)]: PDUs of random_pdus (drawn from rng as it stands, so its own draws stay what they are)
    with the precoding replaced by 2-4 PRGs of random complex weights from a second generator.  prg_size_rb is drawn among the
    sizes at which the allocation spans all of the PRGs -- its first PRB in PRG 0, its last in the last PRG or, at the smaller
    sizes, beyond it, where the last PRG's weights hold (include/mi355_nrphy.h; the reference is undefined there and its DM-RS
    processor for any several PRGs, so the oracle is the yardstick for these).  Kept: allocations of two PRBs or more that
    the library accepts and that have data RE."""
    lib = backends.pkg.lib
    out, wrng = [], None
    while len(out) < count:
        batch = random_pdus(tbs, rng, count - len(out))
        if wrng is None:
            wrng = np.random.default_rng([int(rng.integers(0, 1 << 32)), 0x505247])
        for pdu, ports, nof_subc in batch:
            prbs = [p for p in range(nof_subc // 12) if (int(pdu.prb_mask[p // 64]) >> (p % 64)) & 1]
            first, last = prbs[0], prbs[-1]
            if last == first:
                continue
            nof_prg = int(wrng.integers(2, 5))
            while (nof_prg - 1) * (first + 1) > last:   # a size with PRB `first` in PRG 0 and PRB `last` in the last PRG
                nof_prg -= 1
            pdu.nof_prg = nof_prg
            pdu.prg_size_rb = int(wrng.integers(first + 1, last // (nof_prg - 1) + 1))
            layers = pdu.nof_layers
            w = ((wrng.standard_normal((nof_prg, ports, layers)) + 1j * wrng.standard_normal((nof_prg, ports, layers))) / 2)
            w = w.astype(np.complex64)
            attach_weights(pdu, np.stack([w.real, w.imag], axis=-1))
            if lib.validate(pdu) == 0 and lib.derive(pdu)["nof_re"] > 0:
                out.append((pdu, ports, nof_subc))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Downlink control side: random PDCCH and SS/PBCH PDUs within what the validators accept
# ---------------------------------------------------------------------------------------------------------------------
def random_pdcch(rng, nof_ports_max=4, nof_rb_grid=52):
    """One random PDCCH PDU (pdcch_processor::pdu_t) that fits a grid of nof_rb_grid PRBs."""
    while True:
        mapping = str(rng.choice(["coreset0", "non_interleaved", "interleaved"]))
        duration = int(rng.integers(1, 4))
        al = int(rng.choice([1, 2, 4, 8, 16]))
        kw = {}
        if mapping == "coreset0":
            size = int(rng.choice([24, 48]))
            if size > nof_rb_grid:
                continue
            start = int(rng.integers(0, nof_rb_grid - size + 1))
            kw.update(bwp_start_rb=start, bwp_size_rb=size, shift_index=int(rng.integers(0, 1008)))
            n_rb = size
        else:
            bwp_start = int(rng.integers(0, 5))
            n_groups_max = (nof_rb_grid - bwp_start) // 6
            groups = sorted(rng.choice(n_groups_max, size=int(rng.integers(1, n_groups_max + 1)), replace=False).tolist())
            kw.update(bwp_start_rb=bwp_start, bwp_size_rb=nof_rb_grid - bwp_start, frequency_resources=groups)
            n_rb = 6 * len(groups)
            if mapping == "interleaved":
                L = int(rng.choice([2, 6] if duration < 3 else [3, 6]))
                R = int(rng.choice([2, 3, 6]))
                if (n_rb * duration) % (L * R) != 0 or L % duration != 0:
                    continue
                kw.update(reg_bundle_size=L, interleaver_size=R, shift_index=int(rng.integers(0, 275)))
        n_cce = n_rb * duration // 6
        if n_cce < al:
            continue
        cce = al * int(rng.integers(0, n_cce // al))
        ports = int(rng.integers(1, nof_ports_max + 1))
        style = int(rng.integers(0, 3))
        if style == 0:
            w, prg = np.ones((1, 1), np.complex64), abi.MAX_RB   # make_wideband(make_single_port())
        elif style == 1:
            w = (rng.standard_normal((1, ports)) + 1j * rng.standard_normal((1, ports))).astype(np.complex64)
            prg = abi.MAX_RB
        else:
            w, prg = None, int(rng.choice([2, 4, 8, 16]))
        pdu = abi.make_pdcch(payload=rng.integers(0, 2, int(rng.integers(12, min(129, 108 * al - 24))), dtype=np.uint8),
                             rnti=int(rng.integers(0, 65536)),
                             cce_index=cce, aggregation_level=al, duration=duration, mapping=mapping,
                             start_symbol=int(rng.integers(0, 14 - duration + 1)), n_id_dmrs=int(rng.integers(0, 65536)),
                             n_id_data=int(rng.integers(0, 65536)), n_rnti=int(rng.integers(0, 65536)),
                             dmrs_dB=float(rng.choice([0.0, 3.0, -1.5])), data_dB=float(rng.choice([0.0, -3.0, 1.25])),
                             slot_index=int(rng.integers(0, 20)), precoding=w if w is not None else np.ones((1, 1), np.complex64),
                             prg_size_rb=prg if w is not None else abi.MAX_RB, **kw)
        if w is None:
            # per-PRG weights: as many PRGs as it takes to cover the highest allocated PRB exactly
            import backends
            o = backends.oracle()
            for nof_prg in range(1, nof_rb_grid // prg + 2):
                cand = (rng.standard_normal((nof_prg, ports)) + 1j * rng.standard_normal((nof_prg, ports))).astype(np.complex64)
                pdu2 = abi.make_pdcch(payload=np.frombuffer(bytes(pdu.payload)[: pdu.payload_size], np.uint8), rnti=pdu.rnti,
                                      cce_index=cce, aggregation_level=al, duration=duration, mapping=mapping,
                                      start_symbol=pdu.start_symbol_index, n_id_dmrs=pdu.n_id_pdcch_dmrs,
                                      n_id_data=pdu.n_id_pdcch_data, n_rnti=pdu.n_rnti, dmrs_dB=pdu.dmrs_power_offset_dB,
                                      data_dB=pdu.data_power_offset_dB, slot_index=pdu.slot_index, precoding=cand,
                                      prg_size_rb=prg, **kw)
                if o.pdcch_validate(pdu2) == 0:
                    return pdu2
            continue
        return pdu


def random_ssb(rng, nof_rb_grid=52, nof_ports=2):
    """One random SS/PBCH block PDU (cases A-C, FR1) that fits a grid of nof_rb_grid PRBs."""
    case = str(rng.choice(["A", "B", "C"]))
    mu = 0 if case == "A" else 1
    L_max = int(rng.choice([4, 8]))
    k_ssb, opa = int(rng.integers(0, 24)), int(rng.integers(0, (nof_rb_grid - 21) * (1 + mu)))
    if mu == 1:
        k_ssb, opa = k_ssb & ~1, opa & ~1
    ports = sorted(rng.choice(nof_ports, size=int(rng.integers(1, nof_ports + 1)), replace=False).tolist())
    pdu = abi.make_ssb(pattern_case=case, ssb_idx=int(rng.integers(0, L_max)), L_max=L_max, phys_cell_id=int(rng.integers(0, 1008)),
                       payload=rng.integers(0, 2, 32, dtype=np.uint8), sfn=int(rng.integers(0, 1024)), subcarrier_offset=k_ssb,
                       offset_to_pointA=opa, beta_pss_dB=float(rng.choice([0.0, 3.0, -3.0])), ports=ports)
    if rng.integers(0, 2):
        pdu.slot_index += (10 << mu) // 2   # the same candidate in the second half frame
    return pdu


def pdu_to_arrays(pdu, prefix):
    """A ctypes PDU (PdcchPdu / SsbPdu) as plain arrays for an .npz fixture: every scalar field, array fields as uint8
    arrays, the precoding weights (when the PDU has them) as complex64 [nof_prg][nof_ports]."""
    out = {}
    for name, ctype in pdu._fields_:
        v = getattr(pdu, name)
        if name == "precoding":
            w = np.ctypeslib.as_array(v, shape=(2 * pdu.nof_prg * pdu.nof_ports,)).copy()
            out[prefix + name] = w.view(np.complex64).reshape(pdu.nof_prg, pdu.nof_ports)
        elif hasattr(v, "__len__"):
            out[prefix + name] = np.array(list(v), dtype=np.uint8)
        else:
            out[prefix + name] = np.array(v)
    return out


def pdu_from_arrays(cls, g, prefix):
    """Inverse of pdu_to_arrays for abi.PdcchPdu / abi.SsbPdu."""
    import ctypes as C
    pdu = cls()
    for name, ctype in cls._fields_:
        v = g[prefix + name]
        if name == "precoding":
            f = np.ascontiguousarray(v, dtype=np.complex64).view(np.float32).reshape(-1)
            pdu._keepalive = f
            pdu.precoding = f.ctypes.data_as(C.POINTER(C.c_float))
        elif v.ndim == 1:
            arr = getattr(pdu, name)
            for i, x in enumerate(v):
                arr[i] = int(x)
        else:
            setattr(pdu, name, v.item())
    return pdu


def attach_weights(pdu, weights):
    """Points a PdschPdu's precoding at a float32 array [nof_prg][nof_ports][nof_layers][2] (kept alive on the struct)."""
    import ctypes as C
    f = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    assert f.size == 2 * pdu.nof_prg * pdu.nof_ports * pdu.nof_layers
    pdu._keepalive = f
    pdu.precoding = f.ctypes.data_as(C.POINTER(C.c_float))
    return pdu


def pdsch_pdu_from_fixture(g, key):
    """A PDSCH PDU stored by tests/golden/generate.py as the raw nrphy_pdsch_pdu_t bytes (`<key>_pod`) and its precoding
    weights (`<key>_weights`)."""
    from backends import abi
    import ctypes as C
    assert int(g["sizeof_pdu"]) == C.sizeof(abi.PdschPdu), "nrphy_pdsch_pdu_t changed: regenerate the fixture"
    pdu = abi.PdschPdu.from_buffer_copy(g[key + "_pod"].tobytes())
    return attach_weights(pdu, g[key + "_weights"])


def ref_test_config_grid(case_row, index):
    """The seeded grid tests/golden/generate.py fed the reference for case `index` of ofdm_modulator_test_data.h."""
    bw_rb, cp = int(case_row[1]), int(case_row[3])
    rng = np.random.default_rng([ord("o"), index])
    nsymb = 12 if cp else 14
    grid = np.zeros((1, 14, bw_rb * 12, 2), np.uint16)
    grid[:, :nsymb] = (rng.standard_normal((1, nsymb, bw_rb * 12, 2)).astype(np.float32).view(np.uint32) >> 16)
    return grid


def ref_test_config_tb(g, key, nbytes):
    return np.random.default_rng([int(x) for x in g[key + "_tb_seed"]]).integers(0, 256, nbytes, dtype=np.uint8)


def demod_inputs(rng, modulation, n, kind):
    """Equalised symbols and noise variances for the soft demodulator.  kind 0: uniform over a little more than the
    constellation; 1: values on the interval boundaries and decision thresholds (integer multiples of the constellation's unit
    amplitude), a tenth of them shrunk below the near-zero threshold; 2: like 0 with zero, negative and NaN variances."""
    amp = {0: 1.0, 1: 1.0, 2: 1.0, 4: 1.2, 6: 1.3, 8: 1.4}[modulation]
    unit = {0: 1.0, 1: 1.0, 2: 1.0, 4: 1 / np.sqrt(10), 6: 1 / np.sqrt(42), 8: 1 / np.sqrt(170)}[modulation]
    sym = rng.uniform(-amp, amp, (n, 2)).astype(np.float32)
    if kind == 1:
        sym = (rng.integers(-18, 19, (n, 2)) * np.float32(unit)).astype(np.float32)
        sym[rng.random((n, 2)) < 0.1] *= np.float32(1e-10)
    noise = rng.uniform(0.001, 2.0, n).astype(np.float32)
    if kind == 2:
        noise[rng.random(n) < 0.2] = 0
        noise[rng.random(n) < 0.1] = -1
        noise[rng.random(n) < 0.05] = np.nan
    return sym.view(np.complex64).reshape(n), noise


def struct_from_fixture(cls, g, key):
    """A ctypes POD stored by tests/golden/generate.py as raw bytes (`<key>_pod`), with its precoding weights (`<key>_weights`)
    re-attached when the struct has a `precoding` pointer."""
    import ctypes as C
    raw = g[key + "_pod"].tobytes()
    assert len(raw) == C.sizeof(cls), "%s changed: regenerate the fixture" % cls.__name__
    obj = cls.from_buffer_copy(raw)
    if key + "_weights" in g:
        f = np.ascontiguousarray(g[key + "_weights"], dtype=np.float32).reshape(-1)
        obj._keepalive = f
        obj.precoding = f.ctypes.data_as(C.POINTER(C.c_float))
    return obj


def seeded_grid(seed, *shape):
    """A grid of finite bf16 pairs for tests that map into a non-empty grid."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape + (2,)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def pdcch_encoder_payload_bits(index, E):
    """Payload length rule for the pdcch_encoder_test_data.h cases (their message files are absent): 12 + 5 (index mod 24) bits,
    at most 128 and at most E - 25 (the encoder needs K + 24 < E)."""
    return int(max(12, min(12 + 5 * (index % 24), 128, E - 25)))


def pbch_message_pdu(pod):
    """pbch_encoder_test_data.h draws ssb_idx up to 63 with L_max 4 or 8, which no SS/PBCH block has; the encoder does not read
    ssb_idx unless L_max = 64 (pbch_encoder_impl.cpp:62-75).  Returns the case-A block PDU this ABI accepts that produces the same
    PBCH message: ssb_idx reduced modulo L_max, the slot that holds that candidate in the half frame of the header's HRF bit."""
    pdu = type(pod).from_buffer_copy(bytes(pod))
    assert pdu.L_max in (4, 8) and pdu.numerology == 0 and pdu.pattern_case == 0
    hrf = pdu.slot_index >= 5
    pdu.ssb_idx = pod.ssb_idx % pdu.L_max
    l_first = (2, 8)[pdu.ssb_idx % 2] + 14 * (pdu.ssb_idx // 2)     # case A: {2, 8} + 14 n (ssb_mapping.h:46-52)
    pdu.slot_index = l_first // 14 + (5 if hrf else 0)
    return pdu


def ssb_grid_rb(pdu):
    """PRBs of a grid that holds the SS/PBCH block of `pdu`: its first subcarrier (ssb_get_k_first, ssb_mapping.h:116-167) plus
    the block's 20 PRBs, at least 24."""
    fr2 = pdu.pattern_case >= 3
    scs = (15, 30, 30, 120, 240)[pdu.pattern_case]
    k15 = (pdu.offset_to_pointA * 12 * (60 if fr2 else 15) + pdu.subcarrier_offset * ((15 << pdu.common_scs) if fr2 else 15)) // 15
    return max(24, (k15 * 15 // scs + 240 + 11) // 12)


def spec_rate_match(bg, zc, rv, qm, nref, nof_filler, codeblock_bits, e):
    """TS 38.212 Section 5.4.2.1 / 5.4.2.2 bit by bit: bit selection from the circular buffer of Ncb = min(N, Nref) bits starting at
    k0, NULL (filler) bits skipped, then the row-column interleaver.  codeblock_bits: the N = 66 Zc (50 Zc) bits after the two
    punctured columns, one per byte.  Slow; for the corner the reference leaves undefined (RM_CORNER_CASES)."""
    n = (66 if bg == 1 else 50) * zc
    k = (22 if bg == 1 else 10) * zc
    ncb = min(n, nref) if nref > 0 else n
    k0 = ({1: (0, 17, 33, 56), 2: (0, 13, 25, 43)}[bg][rv] * ncb // n) * zc
    fs, fe = k - 2 * zc - nof_filler, k - 2 * zc
    sel, j = [], 0
    while len(sel) < e:
        idx = (k0 + j) % ncb
        if not fs <= idx < fe:
            sel.append(codeblock_bits[idx])
        j += 1
    return np.array(sel, np.uint8).reshape(qm, e // qm).T.reshape(-1)


# (base graph, rv, Qm, Nref, transport block bytes, channel symbols): five BG1 / Zc 384 codeblocks whose limited circular buffer of
# 7603 bits ends INSIDE the filler range [7680 - F, 7680) -- a limited-buffer size below the transport block's own, which the
# reference's validator accepts and its rate matcher then reads out of bounds on (a crash in the compiled reference); the last
# two frame the window from outside (buffer beyond the filler bits, buffer before them).
RM_CORNER_CASES = [(1, 3, 4, 7603, 5122, 17328), (1, 2, 6, 7603, 4992, 8544), (1, 1, 2, 7603, 4867, 25272), (1, 0, 2, 7603, 4867, 40544),
                   (1, 2, 4, 7700, 5122, 17328), (1, 3, 4, 7000, 5122, 17328)]


def rm_corner_expected(oracle, case, tb):
    """The codeword TS 38.212 gives for one of RM_CORNER_CASES: the oracle's segmentation and LDPC encoding (pinned elsewhere),
    then spec_rate_match per codeblock."""
    bg, rv, qm, nref, _, nsym = case
    segs, meta, zc = oracle.segment(bg, rv, qm, nref, 1, nsym, tb)
    out = []
    for c in range(segs.shape[0]):
        full = np.unpackbits(oracle.ldpc_encode(bg, zc, segs[c], 66 * zc))[: 66 * zc]
        out.append(spec_rate_match(bg, zc, rv, qm, nref, int(meta[c][2]), full, int(meta[c][0])))
    return np.concatenate(out)


# ---------------------------------------------------------------------------------------------------------------------
# The scrambling-seed walk of the prologue (csrc/pdsch_kernels.hip, prologue_kernel): constructive corner cases
# ---------------------------------------------------------------------------------------------------------------------
SEED_BLOCK_WORDS = 31 * 64   # a block of 31 rows of the sequence wave (bits_device.h: GOLD_SEED_ROWS x WAVE)
RE_CHUNK = 512               # resource elements per codeblock work item (nrphy_internal.h)


def seed_walk_layout(d, lq, nof_pdus_in_plan=1):
    """Where the prologue's sequence wave meets the work items of a PDU: (items, boundaries).  items = [(first word of the
    item's scrambling bits, resource elements of the item)] in order; boundaries = the word indices at which a block of 31 rows
    or a part of the sequence ends (plan rule: csrc/pdsch_plan_build.cpp, "parts"; one part in a plan of 128 PDUs or more)."""
    G, C, n_short = d["codeword_bits"], d["nof_codeblocks"], d["nof_short_segments"]
    items, bit_cb = [], 0
    for cb in range(C):
        e = d["rm_length_short"] if cb < n_short else d["rm_length_long"]
        nre = e // lq
        for re_begin in range(0, nre, RE_CHUNK):
            items.append(((bit_cb + re_begin * lq) >> 5, min(RE_CHUNK, nre - re_begin)))
        bit_cb += e
    scr_words = (G + 31) // 32 + 1 + 31
    parts = min(1 if nof_pdus_in_plan >= 128 else 4, max(1, scr_words >> 11))
    chunk = -(-scr_words // parts)
    bounds = set()
    for first in range(0, scr_words, chunk):
        end = min(first + chunk, scr_words)
        bounds.add(end)
        bounds.update(range(first + SEED_BLOCK_WORDS, end, SEED_BLOCK_WORDS))
    return items, sorted(bounds)


def seed_walk_pdus(tbs, rng, count, max_draws=200000):
    """PDUs built so that a SHORT work item (the 1 ... 40 resource-element tail of a codeblock cut into RE_CHUNK pieces, whose
    31-word seed overlaps its neighbours') has its first scrambling word within -31 ... +1 words of the end of a 31-row block
    or of a sequence part -- the four interacting boundaries of the seed walk (the walk's one bug showed in 6
    of 64 sweep legs and in no fixed test).  Drawn at random over allocation, symbols, modulation x layers (2 ... 32 bits per
    resource element) and rate, kept when the layout computed from nrphy_pdsch_derive meets the condition; spread over the
    bits-per-RE values and both kinds of boundary.  [(pdu, nof_ports, nof_subc, (lq, tail RE, distance, kind))]."""
    lib = backends.pkg.lib
    out, seen = [], {}
    for _ in range(max_draws):
        if len(out) >= count:
            break
        layers = int(rng.integers(1, 5))
        qm = int(rng.choice([2, 4, 6, 8]))
        lq = qm * layers
        n_prb = int(rng.integers(24, 274))
        nsym = int(rng.integers(6, 15))
        dmrs = [2] if nsym < 10 else [2, 9]
        groups = int(rng.integers((layers + 1) // 2, 3))
        rate = float(rng.uniform(120, 948))
        tb_bits = tbs(nsym, len(dmrs) * 6 * groups, 0, qm, rate, layers, n_prb)
        if tb_bits < 3840 or tb_bits > 1277992:
            continue
        r = rate / 1024
        bg = 2 if (tb_bits <= 3824 and r <= 0.67) or r <= 0.25 else 1
        w = np.zeros((1, layers, layers), np.complex64)
        w[0] = np.eye(layers) / np.sqrt(layers)
        pdu = abi.make_pdu(slot_index=int(rng.integers(0, 20)), rnti=int(rng.integers(1, 65520)), bwp_start_rb=0, bwp_size_rb=273, qm=qm,
                           n_id=int(rng.integers(0, 1024)), dmrs_symbols=dmrs, scrambling_id=int(rng.integers(0, 65536)),
                           nof_cdm_groups_without_data=groups, prb_start=0, prb_count=n_prb, start_symbol=0, nof_symbols=nsym,
                           base_graph=bg, precoding=w, tb_size_bytes=tb_bits // 8)
        if lib.validate(pdu) != 0:
            continue
        d = lib.derive(pdu)
        if d["codeword_bits"] <= 32 * SEED_BLOCK_WORDS:
            continue   # a sequence of one block: no boundary inside
        items, bounds = seed_walk_layout(d, lq)
        part_ends = set(seed_walk_layout(d, lq)[1]) - {b for b in bounds if b % SEED_BLOCK_WORDS == 0 and b != bounds[-1]}
        hit = None
        for k, (w0, nre) in enumerate(items):
            if not 1 <= nre <= 40:
                continue
            for b in bounds:
                if -31 <= w0 - b <= 1:
                    kind = "part" if (b in part_ends and b % SEED_BLOCK_WORDS != 0) else "block"
                    hit = (lq, nre, w0 - b, kind)
                    break
            if hit:
                break
        if hit is None:
            continue
        key = (hit[0], hit[3], hit[2] // 8)
        if seen.get(key, 0) >= 2:   # spread: at most two per (bits per RE, boundary kind, distance octave)
            continue
        seen[key] = seen.get(key, 0) + 1
        out.append((pdu, layers, 273 * 12, hit))
    return out
