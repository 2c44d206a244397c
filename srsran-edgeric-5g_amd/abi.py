"""ctypes mirror of include/mi355_nrphy.h (the C ABI) plus PDU construction helpers.

The structures here are the POD mirror of the reference's ``pdsch_processor::pdu_t``
(srsRAN-5G-ER/include/srsran/phy/upper/channel_processors/pdsch_processor.h:58-155) and
``ofdm_modulator_configuration`` (include/srsran/phy/lower/modulation/ofdm_modulator.h:34-47).
Pure host-side plumbing: no compute happens in this module.
"""
import ctypes as C

import numpy as np

MAX_RB = 275
NRE = 12
NSYMB = 14
MAX_PORTS = 4
MAX_LAYERS = 4
PRB_WORDS = 5
MAX_RESERVED = 4
MAX_CODEBLOCKS = 162

OK = 0
ERR_INVALID_PDU = 1
ERR_ARGUMENT = 2
ERR_DEVICE = 3
ERR_CAPACITY = 4
ERR_NOT_READY = 5

TBS_LBRM_DEFAULT = 159749  # tbs_lbrm_default, include/srsran/ran/sch/sch_constants.h:47


class RePattern(C.Structure):
    _fields_ = [
        ("prb_mask", C.c_uint64 * PRB_WORDS),
        ("re_mask", C.c_uint16),
        ("symbol_mask", C.c_uint16),
        ("reserved_", C.c_uint32),
    ]


class PdschPdu(C.Structure):
    _fields_ = [
        ("slot_index", C.c_uint32),
        ("rnti", C.c_uint32),
        ("bwp_start_rb", C.c_uint32),
        ("bwp_size_rb", C.c_uint32),
        ("cp", C.c_uint32),
        ("qm", C.c_uint32),
        ("rv", C.c_uint32),
        ("nof_codewords", C.c_uint32),
        ("n_id", C.c_uint32),
        ("ref_point", C.c_uint32),
        ("dmrs_symbol_mask", C.c_uint32),
        ("dmrs_type", C.c_uint32),
        ("scrambling_id", C.c_uint32),
        ("n_scid", C.c_uint32),
        ("nof_cdm_groups_without_data", C.c_uint32),
        ("start_symbol_index", C.c_uint32),
        ("nof_symbols", C.c_uint32),
        ("ldpc_base_graph", C.c_uint32),
        ("tbs_lbrm_bytes", C.c_uint32),
        ("vrb_contiguous", C.c_uint32),
        ("prb_mask", C.c_uint64 * PRB_WORDS),
        ("nof_reserved", C.c_uint32),
        ("tb_size_bytes", C.c_uint32),
        ("reserved", RePattern * MAX_RESERVED),
        ("ratio_pdsch_dmrs_to_sss_dB", C.c_float),
        ("ratio_pdsch_data_to_sss_dB", C.c_float),
        ("nof_layers", C.c_uint32),
        ("nof_ports", C.c_uint32),
        ("prg_size_rb", C.c_uint32),
        ("nof_prg", C.c_uint32),
        ("precoding", C.POINTER(C.c_float)),
    ]


class PdschDerived(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "nof_re", "nof_codeblocks", "lifting_size", "segment_length", "cb_info_bits", "nof_filler_bits",
        "nof_tb_crc_bits", "nof_cb_crc_bits", "zero_pad", "full_length", "n_ref", "n_cb", "k0",
        "nof_short_segments", "rm_length_short", "rm_length_long", "codeword_bits")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PdschEncoderCfg(C.Structure):
    """nrphy_pdsch_encoder_cfg_t (pdsch_encoder::configuration + TB size)."""
    _fields_ = [("base_graph", C.c_uint32), ("rv", C.c_uint32), ("qm", C.c_uint32), ("nref", C.c_uint32),
                ("nof_layers", C.c_uint32), ("nof_ch_symbols", C.c_uint32), ("tb_size_bytes", C.c_uint32)]


class LdpcDecoderCfg(C.Structure):
    """nrphy_ldpc_decoder_cfg_t (ldpc_decoder::configuration + number of soft bits)."""
    _fields_ = [("base_graph", C.c_uint32), ("lifting_size", C.c_uint32), ("nof_filler_bits", C.c_uint32),
                ("crc_poly", C.c_uint32), ("nof_llr", C.c_uint32), ("max_iterations", C.c_uint32),
                ("scaling_factor", C.c_float)]


class LdpcRateDematcherCfg(C.Structure):
    """nrphy_ldpc_rate_dematcher_cfg_t (the codeblock_metadata fields the rate dematcher reads + input length)."""
    _fields_ = [("base_graph", C.c_uint32), ("lifting_size", C.c_uint32), ("rv", C.c_uint32), ("qm", C.c_uint32),
                ("nref", C.c_uint32), ("nof_filler_bits", C.c_uint32), ("rm_length", C.c_uint32)]


class PuschDecoderCfg(C.Structure):
    """nrphy_pusch_decoder_cfg_t (pusch_decoder::configuration + TB size + number of channel symbols)."""
    _fields_ = [("base_graph", C.c_uint32), ("qm", C.c_uint32), ("rv", C.c_uint32), ("nof_layers", C.c_uint32),
                ("nref", C.c_uint32), ("tb_size_bytes", C.c_uint32), ("nof_ch_symbols", C.c_uint32),
                ("max_iterations", C.c_uint32), ("use_early_stop", C.c_uint32), ("new_data", C.c_uint32)]


class PuschDemodCfg(C.Structure):
    """nrphy_pusch_demod_cfg_t (pusch_demodulator::configuration + the equaliser)."""
    _fields_ = [("rnti", C.c_uint32), ("n_id", C.c_uint32), ("qm", C.c_uint32), ("start_symbol_index", C.c_uint32),
                ("nof_symbols", C.c_uint32), ("dmrs_symbol_mask", C.c_uint32), ("dmrs_type", C.c_uint32),
                ("nof_cdm_groups_without_data", C.c_uint32), ("nof_tx_layers", C.c_uint32), ("nof_rx_ports", C.c_uint32),
                ("rx_ports", C.c_uint32 * MAX_PORTS), ("equalizer", C.c_uint32), ("transform_precoding", C.c_uint32),
                ("reserved_", C.c_uint32), ("prb_mask", C.c_uint64 * PRB_WORDS)]


EQ_ZF = 0
EQ_MMSE = 1
PUSCH_DEMOD_TRANSFORM_PRECODING = 1  # NRPHY_PUSCH_DEMOD_*: the feature mask of the _ex forms
PUSCH_DEMOD_PI2_BPSK = 2


def make_pusch_demod(*, prbs, qm=2, rnti=1, n_id=0, start_symbol=0, nof_symbols=14, dmrs_symbols=(), dmrs_type=1,
                     nof_cdm_groups_without_data=2, nof_layers=1, rx_ports=(0,), equalizer=EQ_ZF, transform_precoding=0):
    """A PuschDemodCfg from plain values (prbs: grid-indexed PRB numbers)."""
    c = PuschDemodCfg()
    c.rnti, c.n_id, c.qm = rnti, n_id, qm
    c.start_symbol_index, c.nof_symbols = start_symbol, nof_symbols
    c.dmrs_symbol_mask = sum(1 << l for l in set(dmrs_symbols))
    c.dmrs_type, c.nof_cdm_groups_without_data = dmrs_type, nof_cdm_groups_without_data
    c.nof_tx_layers, c.nof_rx_ports = nof_layers, len(rx_ports)
    for i, p in enumerate(rx_ports):
        c.rx_ports[i] = p
    c.equalizer, c.transform_precoding = equalizer, transform_precoding
    for i, w in enumerate(prb_mask_words(prbs)):
        c.prb_mask[i] = w
    return c


PUSCH_CHEST_NO_DC = 0xFFFFFFFF
PUSCH_CHEST_MAX_LAYERS = 2


class PuschChestCfg(C.Structure):
    """nrphy_pusch_chest_cfg_t (dmrs_pusch_estimator::configuration + the PUSCH processor's DC position)."""
    _fields_ = [("numerology", C.c_uint32), ("slot_index", C.c_uint32), ("scrambling_id", C.c_uint32), ("n_scid", C.c_uint32),
                ("scaling", C.c_float), ("dmrs_type", C.c_uint32), ("dmrs_symbol_mask", C.c_uint32),
                ("start_symbol_index", C.c_uint32), ("nof_symbols", C.c_uint32), ("nof_tx_layers", C.c_uint32),
                ("nof_rx_ports", C.c_uint32), ("rx_ports", C.c_uint32 * MAX_PORTS), ("dc_position", C.c_uint32),
                ("prb_mask", C.c_uint64 * PRB_WORDS)]


class PuschChestMeas(C.Structure):
    """nrphy_pusch_chest_meas_t: what channel_estimate holds per (PUSCH, receive port, layer)."""
    _fields_ = [("noise_var", C.c_float), ("rsrp", C.c_float), ("epre", C.c_float), ("snr", C.c_float), ("ta_s", C.c_float),
                ("ta_bins", C.c_int32), ("cfo_hz", C.c_float), ("reserved_", C.c_uint32)]


class PuschChestLowpapr(C.Structure):
    """nrphy_pusch_chest_lowpapr_t: the low-PAPR DM-RS of a transform-precoded PUSCH (enabled 0: Gold DM-RS)."""
    _fields_ = [("enabled", C.c_uint32), ("n_rs_id", C.c_uint32)]


def make_pusch_chest(*, prbs, numerology=0, slot_index=0, scrambling_id=0, n_scid=0, scaling=1.0, dmrs_type=1,
                     dmrs_symbols=(2,), start_symbol=0, nof_symbols=14, nof_layers=1, rx_ports=(0,), dc_position=None):
    """A PuschChestCfg from plain values (prbs: grid-indexed PRB numbers; dc_position None: no DC)."""
    c = PuschChestCfg()
    c.numerology, c.slot_index, c.scrambling_id, c.n_scid, c.scaling = numerology, slot_index, scrambling_id, n_scid, scaling
    c.dmrs_type, c.dmrs_symbol_mask = dmrs_type, sum(1 << l for l in set(dmrs_symbols))
    c.start_symbol_index, c.nof_symbols, c.nof_tx_layers, c.nof_rx_ports = start_symbol, nof_symbols, nof_layers, len(rx_ports)
    for i, p in enumerate(rx_ports):
        c.rx_ports[i] = p
    c.dc_position = PUSCH_CHEST_NO_DC if dc_position is None else dc_position
    for i, w in enumerate(prb_mask_words(prbs)):
        c.prb_mask[i] = w
    return c


PRACH_FORMATS = ("0", "1", "2", "3", "A1", "A2", "A3", "B1", "B4", "C0", "C2", "A1/B1", "A2/B2", "A3/B3")  # NRPHY_PRACH_FORMAT_*
PRACH_SPACINGS = ("15", "30", "60", "120", "1.25", "5")  # NRPHY_PRACH_SCS_*, kHz
PRACH_MAX_PREAMBLES = 64


class PrachCfg(C.Structure):
    """nrphy_prach_cfg_t (prach_detector::configuration + an optional threshold and window margin of the caller's)."""
    _fields_ = [("format", C.c_uint32), ("ra_scs", C.c_uint32), ("restricted_set", C.c_uint32), ("root_sequence_index", C.c_uint32),
                ("zero_correlation_zone", C.c_uint32), ("start_preamble_index", C.c_uint32), ("nof_preamble_indices", C.c_uint32),
                ("nof_rx_ports", C.c_uint32), ("threshold", C.c_float), ("win_margin", C.c_uint32)]


class PrachResult(C.Structure):
    """nrphy_prach_result_t: one per occasion."""
    _fields_ = [("rssi_dB", C.c_float), ("time_resolution_s", C.c_float), ("time_advance_max_s", C.c_float),
                ("nof_detected", C.c_uint32), ("detected_mask", C.c_uint64)]


class PrachPreamble(C.Structure):
    """nrphy_prach_preamble_t: one per (occasion, preamble index)."""
    _fields_ = [("detected", C.c_uint32), ("delay_samples", C.c_uint32), ("time_advance_s", C.c_float), ("peak", C.c_float),
                ("detection_metric", C.c_float)]


def make_prach(*, format, ra_scs=None, root_sequence_index=0, zero_correlation_zone=0, start_preamble_index=0,
               nof_preamble_indices=64, nof_rx_ports=1, restricted_set=0, threshold=0.0, win_margin=0):
    """A PrachCfg from plain values: format and ra_scs by name ("B4", "15") or number; ra_scs None: 1.25 / 5 kHz for the long
    formats, 15 kHz for the short ones."""
    c = PrachCfg()
    c.format = PRACH_FORMATS.index(format) if isinstance(format, str) else format
    if ra_scs is None:
        ra_scs = "5" if c.format == 3 else "1.25" if c.format < 3 else "15"
    c.ra_scs = PRACH_SPACINGS.index(ra_scs) if isinstance(ra_scs, str) else ra_scs
    c.restricted_set, c.root_sequence_index, c.zero_correlation_zone = restricted_set, root_sequence_index, zero_correlation_zone
    c.start_preamble_index, c.nof_preamble_indices, c.nof_rx_ports = start_preamble_index, nof_preamble_indices, nof_rx_ports
    c.threshold, c.win_margin = threshold, win_margin
    return c


class PrachDemodCfg(C.Structure):
    """nrphy_prach_demod_cfg_t (the sampling rate + ofdm_prach_demodulator::configuration, with ports in place of one port)."""
    _fields_ = [("srate_hz", C.c_uint32), ("format", C.c_uint32), ("nof_td_occasions", C.c_uint32), ("nof_fd_occasions", C.c_uint32),
                ("start_symbol", C.c_uint32), ("rb_offset", C.c_uint32), ("nof_prb_ul_grid", C.c_uint32),
                ("pusch_numerology", C.c_uint32), ("nof_rx_ports", C.c_uint32)]


class PrachDemodSizes(C.Structure):
    """nrphy_prach_demod_sizes_t."""
    _fields_ = [("dft_size", C.c_uint32), ("sequence_length", C.c_uint32), ("nof_symbols", C.c_uint32), ("window_samples", C.c_uint32)]


def make_prach_demod(*, srate_hz, format, nof_td_occasions=1, nof_fd_occasions=1, start_symbol=0, rb_offset=0, nof_prb_ul_grid,
                     pusch_numerology=0, nof_rx_ports=1):
    """A PrachDemodCfg from plain values: format by name ("B4") or number."""
    c = PrachDemodCfg()
    c.srate_hz = srate_hz
    c.format = PRACH_FORMATS.index(format) if isinstance(format, str) else format
    c.nof_td_occasions, c.nof_fd_occasions, c.start_symbol, c.rb_offset = nof_td_occasions, nof_fd_occasions, start_symbol, rb_offset
    c.nof_prb_ul_grid, c.pusch_numerology, c.nof_rx_ports = nof_prb_ul_grid, pusch_numerology, nof_rx_ports
    return c


PUCCH_FORMAT_0 = 0
PUCCH_FORMAT_1 = 1
PUCCH_NO_HOP = 0xFFFFFFFF
PUCCH_STATUS_UNKNOWN, PUCCH_STATUS_VALID, PUCCH_STATUS_INVALID = 0, 1, 2  # uci_status


class PucchCfg(C.Structure):
    """nrphy_pucch_cfg_t (pucch_processor::format0_configuration / format1_configuration)."""
    _fields_ = [("format", C.c_uint32), ("numerology", C.c_uint32), ("slot_index", C.c_uint32), ("bwp_size_rb", C.c_uint32),
                ("bwp_start_rb", C.c_uint32), ("starting_prb", C.c_uint32), ("second_hop_prb", C.c_uint32),
                ("start_symbol_index", C.c_uint32), ("nof_symbols", C.c_uint32), ("initial_cyclic_shift", C.c_uint32),
                ("time_domain_occ", C.c_uint32), ("n_id", C.c_uint32), ("nof_harq_ack", C.c_uint32), ("sr_opportunity", C.c_uint32),
                ("nof_rx_ports", C.c_uint32), ("rx_ports", C.c_uint32 * MAX_PORTS), ("reserved_", C.c_uint32)]


class PucchResult(C.Structure):
    """nrphy_pucch_result_t: one per PUCCH."""
    _fields_ = [("status", C.c_uint32), ("harq_ack", C.c_uint32 * 2), ("sr", C.c_uint32), ("detection_metric", C.c_float),
                ("sinr_dB", C.c_float), ("rsrp_dB", C.c_float), ("epre_dB", C.c_float), ("time_alignment_s", C.c_float),
                ("cfo_hz", C.c_float)]


def make_pucch(*, format, starting_prb, nof_symbols, start_symbol=0, second_hop_prb=None, bwp_size_rb=None, bwp_start_rb=0,
               numerology=0, slot_index=0, initial_cyclic_shift=0, time_domain_occ=0, n_id=0, nof_harq_ack=1, sr_opportunity=False,
               rx_ports=(0,)):
    """A PucchCfg from plain values (second_hop_prb None: no frequency hopping; bwp_size_rb None: the largest BWP, 275 PRBs less
    its start)."""
    c = PucchCfg()
    c.format, c.numerology, c.slot_index = format, numerology, slot_index
    c.bwp_size_rb = 275 - bwp_start_rb if bwp_size_rb is None else bwp_size_rb
    c.bwp_start_rb, c.starting_prb = bwp_start_rb, starting_prb
    c.second_hop_prb = PUCCH_NO_HOP if second_hop_prb is None else second_hop_prb
    c.start_symbol_index, c.nof_symbols = start_symbol, nof_symbols
    c.initial_cyclic_shift, c.time_domain_occ, c.n_id = initial_cyclic_shift, time_domain_occ, n_id
    c.nof_harq_ack, c.sr_opportunity, c.nof_rx_ports = nof_harq_ack, int(sr_opportunity), len(rx_ports)
    for i, q in enumerate(rx_ports):
        c.rx_ports[i] = q
    return c


class Pf2Cfg(C.Structure):
    """nrphy_pf2_cfg_t (pucch_processor::format2_configuration)."""
    _fields_ = [("numerology", C.c_uint32), ("slot_index", C.c_uint32), ("bwp_size_rb", C.c_uint32), ("bwp_start_rb", C.c_uint32),
                ("starting_prb", C.c_uint32), ("nof_prb", C.c_uint32), ("start_symbol_index", C.c_uint32), ("nof_symbols", C.c_uint32),
                ("rnti", C.c_uint32), ("n_id", C.c_uint32), ("n_id_0", C.c_uint32), ("nof_harq_ack", C.c_uint32), ("nof_sr", C.c_uint32),
                ("nof_csi_part1", C.c_uint32), ("nof_csi_part2", C.c_uint32), ("nof_rx_ports", C.c_uint32),
                ("rx_ports", C.c_uint32 * MAX_PORTS)]


class Pf2Csi(C.Structure):
    """nrphy_pf2_csi_t: one per PUCCH format 2."""
    _fields_ = [("sinr_dB", C.c_float), ("rsrp_dB", C.c_float), ("epre_dB", C.c_float), ("time_alignment_s", C.c_float),
                ("cfo_hz", C.c_float), ("reserved_", C.c_uint32 * 3)]


def make_pf2(*, starting_prb, nof_prb, nof_symbols, start_symbol=0, bwp_size_rb=None, bwp_start_rb=0, numerology=0, slot_index=0,
             rnti=1, n_id=0, n_id_0=0, nof_harq_ack=0, nof_sr=0, nof_csi_part1=0, nof_csi_part2=0, rx_ports=(0,)):
    """A Pf2Cfg from plain values (bwp_size_rb None: the largest BWP, 275 PRBs less its start)."""
    c = Pf2Cfg()
    c.numerology, c.slot_index = numerology, slot_index
    c.bwp_size_rb = 275 - bwp_start_rb if bwp_size_rb is None else bwp_size_rb
    c.bwp_start_rb, c.starting_prb, c.nof_prb = bwp_start_rb, starting_prb, nof_prb
    c.start_symbol_index, c.nof_symbols = start_symbol, nof_symbols
    c.rnti, c.n_id, c.n_id_0 = rnti, n_id, n_id_0
    c.nof_harq_ack, c.nof_sr, c.nof_csi_part1, c.nof_csi_part2 = nof_harq_ack, nof_sr, nof_csi_part1, nof_csi_part2
    c.nof_rx_ports = len(rx_ports)
    for i, q in enumerate(rx_ports):
        c.rx_ports[i] = q
    return c


class SrsCfg(C.Structure):
    """nrphy_srs_cfg_t (srs_estimator_configuration)."""
    _fields_ = [("numerology", C.c_uint32), ("nof_antenna_ports", C.c_uint32), ("nof_symbols", C.c_uint32), ("start_symbol", C.c_uint32),
                ("configuration_index", C.c_uint32), ("sequence_id", C.c_uint32), ("bandwidth_index", C.c_uint32),
                ("comb_size", C.c_uint32), ("comb_offset", C.c_uint32), ("cyclic_shift", C.c_uint32), ("freq_position", C.c_uint32),
                ("freq_shift", C.c_uint32), ("freq_hopping", C.c_uint32), ("hopping", C.c_uint32), ("nof_rx_ports", C.c_uint32),
                ("rx_ports", C.c_uint32 * MAX_PORTS)]


class SrsResult(C.Structure):
    """nrphy_srs_result_t: one per SRS; the matrices are [rx][tx]."""
    _fields_ = [("h_re", (C.c_float * 4) * 4), ("h_im", (C.c_float * 4) * 4), ("ta_bins", (C.c_int32 * 4) * 4),
                ("time_alignment_s", C.c_double), ("reserved_", C.c_uint32 * 2)]


def make_srs(*, configuration_index, bandwidth_index=0, comb_size=2, comb_offset=0, cyclic_shift=0, nof_antenna_ports=1, nof_symbols=1,
             start_symbol=13, sequence_id=0, freq_position=0, freq_shift=0, freq_hopping=None, hopping=0, numerology=0, rx_ports=(0,)):
    """An SrsCfg from plain values (freq_hopping None: b_hop = 3, no frequency hopping whatever the bandwidth index)."""
    c = SrsCfg()
    c.numerology, c.nof_antenna_ports, c.nof_symbols, c.start_symbol = numerology, nof_antenna_ports, nof_symbols, start_symbol
    c.configuration_index, c.sequence_id, c.bandwidth_index = configuration_index, sequence_id, bandwidth_index
    c.comb_size, c.comb_offset, c.cyclic_shift = comb_size, comb_offset, cyclic_shift
    c.freq_position, c.freq_shift = freq_position, freq_shift
    c.freq_hopping, c.hopping = 3 if freq_hopping is None else freq_hopping, hopping
    c.nof_rx_ports = len(rx_ports)
    for i, q in enumerate(rx_ports[:MAX_PORTS]):
        c.rx_ports[i] = q
    return c


UCI_STATUS_UNKNOWN, UCI_STATUS_VALID, UCI_STATUS_INVALID = 0, 1, 2  # uci_status


class UciDecoderCfg(C.Structure):
    """nrphy_uci_decoder_cfg_t (uci_decoder::decode's message and soft-bit lengths, uci_decoder::configuration's modulation)."""
    _fields_ = [("message_length", C.c_uint32), ("llr_length", C.c_uint32), ("modulation", C.c_uint32), ("reserved_", C.c_uint32)]


class UlschDemuxCfg(C.Structure):
    """nrphy_ulsch_demux_cfg_t (ulsch_demultiplex::configuration, set_csi_part2's sizes and the codeword's scrambling)."""
    _fields_ = [(n, C.c_uint32) for n in (
        "modulation", "nof_layers", "nof_prb", "start_symbol_index", "nof_symbols", "dmrs_type", "dmrs_symbol_mask",
        "nof_cdm_groups_without_data", "nof_harq_ack_rvd", "nof_harq_ack_bits", "nof_enc_harq_ack_bits", "nof_csi_part1_bits",
        "nof_enc_csi_part1_bits", "nof_csi_part2_bits", "nof_enc_csi_part2_bits", "rnti", "n_id")]


class UlschDemuxSizes(C.Structure):
    """nrphy_ulsch_demux_sizes_t."""
    _fields_ = [("nof_sch_bits", C.c_uint32), ("nof_codeword_bits", C.c_uint32)]


def make_ulsch_demux(**fields):
    """An UlschDemuxCfg from keyword fields (those not given are 0)."""
    c = UlschDemuxCfg()
    for k, v in fields.items():
        assert hasattr(c, k), k
        setattr(c, k, int(v))
    return c


def make_uci_decoder(message_length, llr_length, modulation=2):
    """A UciDecoderCfg; modulation is an NRPHY_MOD_* code (0 pi/2-BPSK, 1 BPSK, else the bits per symbol)."""
    c = UciDecoderCfg()
    c.message_length, c.llr_length, c.modulation = message_length, llr_length, modulation
    return c


class UlschInfoCfg(C.Structure):
    """nrphy_ulsch_info_cfg_t (ulsch_configuration)."""
    _fields_ = [("tbs_bits", C.c_uint32), ("modulation", C.c_uint32), ("target_code_rate", C.c_float),
                ("nof_harq_ack_bits", C.c_uint32), ("nof_csi_part1_bits", C.c_uint32), ("nof_csi_part2_bits", C.c_uint32),
                ("alpha_scaling", C.c_float), ("beta_offset_harq_ack", C.c_float), ("beta_offset_csi_part1", C.c_float),
                ("beta_offset_csi_part2", C.c_float), ("nof_rb", C.c_uint32), ("start_symbol_index", C.c_uint32),
                ("nof_symbols", C.c_uint32), ("dmrs_type", C.c_uint32), ("dmrs_symbol_mask", C.c_uint32),
                ("nof_cdm_groups_without_data", C.c_uint32), ("nof_layers", C.c_uint32), ("contains_dc", C.c_uint32)]


class UlschInfo(C.Structure):
    """nrphy_ulsch_info_t (ulsch_information)."""
    _fields_ = [(n, C.c_uint32) for n in (
        "has_sch", "tb_crc_bits", "base_graph", "nof_cb", "nof_filler_bits_per_cb", "lifting_size", "nof_bits_per_cb",
        "nof_ul_sch_bits", "nof_harq_ack_bits", "nof_harq_ack_rvd", "nof_csi_part1_bits", "nof_csi_part2_bits",
        "nof_harq_ack_re", "nof_csi_part1_re", "nof_csi_part2_re", "nof_dc_overlap_bits")]


def make_ulsch_info_cfg(**fields):
    """An UlschInfoCfg from keyword fields (those not given are 0)."""
    c = UlschInfoCfg()
    for k, v in fields.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    return c


PUSCH_SINR_CHANNEL_ESTIMATOR, PUSCH_SINR_POST_EQUALIZATION, PUSCH_SINR_EVM = 0, 1, 2  # NRPHY_PUSCH_SINR_*


class PuschPdu(C.Structure):
    """nrphy_pusch_pdu_t (pusch_processor::pdu_t)."""
    _fields_ = [("numerology", C.c_uint32), ("slot_index", C.c_uint32), ("rnti", C.c_uint32), ("n_id", C.c_uint32),
                ("scrambling_id", C.c_uint32), ("n_scid", C.c_uint32), ("modulation", C.c_uint32), ("target_code_rate", C.c_float),
                ("has_codeword", C.c_uint32), ("rv", C.c_uint32), ("ldpc_base_graph", C.c_uint32), ("new_data", C.c_uint32),
                ("tb_size_bytes", C.c_uint32), ("tbs_lbrm_bytes", C.c_uint32), ("nof_harq_ack", C.c_uint32),
                ("nof_csi_part1", C.c_uint32), ("nof_csi_part2_entries", C.c_uint32), ("alpha_scaling", C.c_float),
                ("beta_offset_harq_ack", C.c_float), ("beta_offset_csi_part1", C.c_float), ("beta_offset_csi_part2", C.c_float),
                ("start_symbol_index", C.c_uint32), ("nof_symbols", C.c_uint32), ("dmrs_type", C.c_uint32),
                ("dmrs_symbol_mask", C.c_uint32), ("nof_cdm_groups_without_data", C.c_uint32), ("nof_tx_layers", C.c_uint32),
                ("nof_rx_ports", C.c_uint32), ("rx_ports", C.c_uint32 * MAX_PORTS), ("dc_position", C.c_uint32),
                ("reserved_", C.c_uint32), ("prb_mask", C.c_uint64 * PRB_WORDS)]


class PuschProcOptions(C.Structure):
    """nrphy_pusch_proc_options_t (pusch_processor_impl::configuration and the factory's choices)."""
    _fields_ = [("dec_nof_iterations", C.c_uint32), ("dec_enable_early_stop", C.c_uint32), ("csi_sinr_calc_method", C.c_uint32),
                ("equalizer", C.c_uint32)]


class PuschEvmOptions(C.Structure):
    """nrphy_pusch_evm_options_t: the processor's options and whether the demodulator takes the EVM."""
    _fields_ = [("proc", PuschProcOptions), ("enable_evm", C.c_uint32), ("reserved_", C.c_uint32)]


class PuschProcDerived(C.Structure):
    """nrphy_pusch_proc_derived_t: the stage configurations of one PDU."""
    _fields_ = [("info", UlschInfo), ("chest", PuschChestCfg), ("demod", PuschDemodCfg), ("demux", UlschDemuxCfg),
                ("uci", UciDecoderCfg * 2), ("decoder", PuschDecoderCfg), ("nof_uci", C.c_uint32), ("has_decoder", C.c_uint32),
                ("codeword_bits", C.c_uint32), ("nof_sch_bits", C.c_uint32)]


class PuschResult(C.Structure):
    """nrphy_pusch_result_t: one per PDU."""
    _fields_ = [("has_sch", C.c_uint32), ("tb_crc_ok", C.c_uint32), ("nof_codeblocks", C.c_uint32), ("nof_codeblocks_ok", C.c_uint32),
                ("ldpc_iterations_sum", C.c_uint32), ("ldpc_iterations_max", C.c_uint32), ("harq_ack_status", C.c_uint32),
                ("csi_part1_status", C.c_uint32), ("nof_harq_ack", C.c_uint32), ("nof_csi_part1", C.c_uint32),
                ("harq_ack_offset", C.c_uint64), ("csi_part1_offset", C.c_uint64), ("sinr_dB", C.c_float),
                ("sinr_ch_estimator_dB", C.c_float), ("sinr_post_eq_dB", C.c_float), ("epre_dB", C.c_float), ("rsrp_dB", C.c_float),
                ("time_alignment_s", C.c_float), ("cfo_hz", C.c_float), ("has_cfo", C.c_uint32), ("has_evm", C.c_uint32),
                ("evm", C.c_float)]


def make_pusch_pdu(*, prbs, modulation=2, target_code_rate=449.0, numerology=0, slot_index=0, rnti=1, n_id=0, scrambling_id=0,
                   n_scid=0, tb_size_bytes=0, rv=0, ldpc_base_graph=1, new_data=1, tbs_lbrm_bytes=3168, nof_harq_ack=0,
                   nof_csi_part1=0, nof_csi_part2_entries=0, alpha_scaling=1.0, beta_offset_harq_ack=20.0, beta_offset_csi_part1=6.25,
                   beta_offset_csi_part2=6.25, start_symbol=0, nof_symbols=14, dmrs_type=1, dmrs_symbols=(2,),
                   nof_cdm_groups_without_data=2, nof_layers=1, rx_ports=(0,), dc_position=None, has_codeword=None):
    """A PuschPdu from plain values (prbs: grid-indexed PRB numbers; dc_position None: no DC; has_codeword None: by tb_size_bytes)."""
    p = PuschPdu()
    p.numerology, p.slot_index, p.rnti, p.n_id, p.scrambling_id, p.n_scid = numerology, slot_index, rnti, n_id, scrambling_id, n_scid
    p.modulation, p.target_code_rate = modulation, target_code_rate
    p.has_codeword = int(tb_size_bytes != 0) if has_codeword is None else int(has_codeword)
    p.rv, p.ldpc_base_graph, p.new_data, p.tb_size_bytes, p.tbs_lbrm_bytes = rv, ldpc_base_graph, new_data, tb_size_bytes, tbs_lbrm_bytes
    p.nof_harq_ack, p.nof_csi_part1, p.nof_csi_part2_entries = nof_harq_ack, nof_csi_part1, nof_csi_part2_entries
    p.alpha_scaling, p.beta_offset_harq_ack = alpha_scaling, beta_offset_harq_ack
    p.beta_offset_csi_part1, p.beta_offset_csi_part2 = beta_offset_csi_part1, beta_offset_csi_part2
    p.start_symbol_index, p.nof_symbols = start_symbol, nof_symbols
    p.dmrs_type, p.dmrs_symbol_mask = dmrs_type, sum(1 << l for l in set(dmrs_symbols))
    p.nof_cdm_groups_without_data, p.nof_tx_layers, p.nof_rx_ports = nof_cdm_groups_without_data, nof_layers, len(rx_ports)
    for i, port in enumerate(rx_ports[:MAX_PORTS]):
        p.rx_ports[i] = port
    p.dc_position = PUSCH_CHEST_NO_DC if dc_position is None else dc_position
    for i, w in enumerate(prb_mask_words(prbs)):
        p.prb_mask[i] = w
    return p


def make_pusch_proc_options(dec_nof_iterations=10, dec_enable_early_stop=1, csi_sinr_calc_method=PUSCH_SINR_CHANNEL_ESTIMATOR,
                            equalizer=EQ_ZF):
    """A PuschProcOptions."""
    return PuschProcOptions(dec_nof_iterations, dec_enable_early_stop, csi_sinr_calc_method, equalizer)


class PuschTpDesc(C.Structure):
    """nrphy_pusch_tp_desc_t: transform precoding of one PUSCH PDU and its DM-RS sequence identity."""
    _fields_ = [("transform_precoding", C.c_uint32), ("n_rs_id", C.c_uint32)]


def make_pusch_evm_options(enable_evm=1, reserved_=0, **proc):
    """A PuschEvmOptions; the keywords of make_pusch_proc_options fill its `proc`."""
    return PuschEvmOptions(make_pusch_proc_options(**proc), enable_evm, reserved_)


PUSCH_CSI2_MAX_ENTRIES, PUSCH_CSI2_MAX_PARAMETERS, PUSCH_CSI2_MAX_ENTRY_BITS = 2, 2, 4  # NRPHY_PUSCH_CSI2_*
PUSCH_CSI2_MAX_SIZES, PUSCH_CSI2_MAX_VARIANTS = 16, 17


class PuschCsi2Entry(C.Structure):
    """nrphy_pusch_csi2_entry_t (uci_part2_size_description::entry)."""
    _fields_ = [("nof_parameters", C.c_uint32), ("offset", C.c_uint32 * PUSCH_CSI2_MAX_PARAMETERS),
                ("width", C.c_uint32 * PUSCH_CSI2_MAX_PARAMETERS), ("map_size", C.c_uint32),
                ("map", C.c_uint32 * (1 << PUSCH_CSI2_MAX_ENTRY_BITS))]


class PuschCsi2Desc(C.Structure):
    """nrphy_pusch_csi2_desc_t (pusch_processor::pdu_t::uci.csi_part2_size)."""
    _fields_ = [("nof_entries", C.c_uint32), ("entries", PuschCsi2Entry * PUSCH_CSI2_MAX_ENTRIES)]


class PuschCsi2Result(C.Structure):
    """nrphy_pusch_csi2_result_t: one per PDU, next to its PuschResult."""
    _fields_ = [("status", C.c_uint32), ("nof_csi_part2", C.c_uint32), ("csi_part2_offset", C.c_uint64), ("nof_enc_bits", C.c_uint32),
                ("nof_ul_sch_bits", C.c_uint32), ("variant", C.c_uint32), ("reserved_", C.c_uint32)]


def make_pusch_csi2_desc(entries=()):
    """A PuschCsi2Desc from entries (parameters, map): parameters a sequence of (offset, width), map the sizes by index.  Nothing
    is checked here -- nof_entries and nof_parameters are the lengths given, what the arrays cannot hold is left out -- so that
    the validator can be shown what it refuses."""
    d = PuschCsi2Desc()
    d.nof_entries = len(entries)
    for e, (parameters, sizes) in zip(d.entries, entries):
        e.nof_parameters = len(parameters)
        for k, (offset, width) in enumerate(list(parameters)[:PUSCH_CSI2_MAX_PARAMETERS]):
            e.offset[k], e.width[k] = offset, width
        e.map_size = len(sizes)
        for k, v in enumerate(list(sizes)[:1 << PUSCH_CSI2_MAX_ENTRY_BITS]):
            e.map[k] = v
    return d


class GridRe(C.Structure):
    """nrphy_grid_re_t: one resource element written from the host into a device grid."""
    _fields_ = [("port", C.c_uint16), ("symbol", C.c_uint16), ("subc", C.c_uint32), ("value", C.c_uint32)]


class CsiRsCfg(C.Structure):
    """nrphy_csi_rs_cfg_t (nzp_csi_rs_generator::config_t)."""
    _fields_ = [("slot_index", C.c_uint32), ("cp", C.c_uint32), ("start_rb", C.c_uint32), ("nof_rb", C.c_uint32),
                ("row", C.c_uint32), ("nof_k_ref", C.c_uint32), ("k_ref", C.c_uint32 * 6), ("symbol_l0", C.c_uint32),
                ("symbol_l1", C.c_uint32), ("cdm", C.c_uint32), ("density", C.c_uint32), ("scrambling_id", C.c_uint32),
                ("amplitude", C.c_float), ("nof_ports", C.c_uint32), ("prg_size_rb", C.c_uint32), ("nof_prg", C.c_uint32),
                ("precoding", C.POINTER(C.c_float))]


PDSCH_DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_void_p)   # nrphy_pdsch_done_fn

CSI_DENSITY = {"dot5_even": 0, "dot5_odd": 1, "one": 2, "three": 3}
CSI_ROW_PORTS = {1: 1, 2: 1, 3: 2, 4: 4, 5: 4}


def make_csi_rs(*, row, start_rb, nof_rb, k0, l0, density, slot_index=0, cp=0, scrambling_id=0, amplitude=1.0,
                precoding=None, prg_size_rb=MAX_RB):
    """Builds a CsiRsCfg for rows 1-5; ``precoding`` [nof_prg][ports][ports] complex64 (default identity).  The weight
    array is attached to the struct (``_keepalive``)."""
    ports = CSI_ROW_PORTS[row]
    if precoding is None:
        precoding = np.eye(ports, dtype=np.complex64)[None]
    w = np.ascontiguousarray(np.asarray(precoding, dtype=np.complex64)).view(np.float32).reshape(-1)
    c = CsiRsCfg()
    c.slot_index, c.cp, c.start_rb, c.nof_rb, c.row = slot_index, cp, start_rb, nof_rb, row
    c.nof_k_ref, c.symbol_l0, c.symbol_l1 = 1, l0, 0
    c.k_ref[0] = k0
    c.cdm = 0 if row in (1, 2) else 1
    c.density = CSI_DENSITY[density]
    c.scrambling_id, c.amplitude, c.nof_ports = scrambling_id, amplitude, ports
    c.prg_size_rb, c.nof_prg = prg_size_rb, np.asarray(precoding).shape[0]
    c._keepalive = w
    c.precoding = w.ctypes.data_as(C.POINTER(C.c_float))
    return c


PDCCH_MAX_PAYLOAD = 128


class PdcchPdu(C.Structure):
    """nrphy_pdcch_pdu_t (pdcch_processor::pdu_t: coreset_description + dci_description)."""
    _fields_ = [("slot_index", C.c_uint32), ("cp", C.c_uint32), ("bwp_size_rb", C.c_uint32), ("bwp_start_rb", C.c_uint32),
                ("start_symbol_index", C.c_uint32), ("duration", C.c_uint32), ("frequency_resources", C.c_uint64),
                ("cce_to_reg_mapping", C.c_uint32), ("reg_bundle_size", C.c_uint32), ("interleaver_size", C.c_uint32),
                ("shift_index", C.c_uint32), ("rnti", C.c_uint32), ("n_id_pdcch_dmrs", C.c_uint32),
                ("n_id_pdcch_data", C.c_uint32), ("n_rnti", C.c_uint32), ("cce_index", C.c_uint32),
                ("aggregation_level", C.c_uint32), ("dmrs_power_offset_dB", C.c_float), ("data_power_offset_dB", C.c_float),
                ("payload_size", C.c_uint32), ("payload", C.c_uint8 * PDCCH_MAX_PAYLOAD), ("nof_ports", C.c_uint32),
                ("prg_size_rb", C.c_uint32), ("nof_prg", C.c_uint32), ("precoding", C.POINTER(C.c_float))]


CCE_TO_REG = {"coreset0": 0, "non_interleaved": 1, "interleaved": 2}


def make_pdcch(*, payload, rnti, cce_index, aggregation_level, duration, frequency_resources=(), mapping="non_interleaved",
               bwp_start_rb=0, bwp_size_rb=52, start_symbol=0, reg_bundle_size=6, interleaver_size=2, shift_index=0,
               n_id_dmrs=0, n_id_data=0, n_rnti=0, dmrs_dB=0.0, data_dB=0.0, slot_index=0, cp=0, precoding=None,
               prg_size_rb=MAX_RB):
    """Builds a PdcchPdu; ``payload`` = DCI bits, ``frequency_resources`` = indices of the 6-PRB groups of the CORESET,
    ``precoding`` [nof_prg][nof_ports] complex64 (default: one port, weight 1)."""
    p = PdcchPdu()
    p.slot_index, p.cp, p.bwp_size_rb, p.bwp_start_rb = slot_index, cp, bwp_size_rb, bwp_start_rb
    p.start_symbol_index, p.duration = start_symbol, duration
    p.frequency_resources = sum(1 << i for i in frequency_resources)
    p.cce_to_reg_mapping = CCE_TO_REG[mapping]
    p.reg_bundle_size, p.interleaver_size, p.shift_index = reg_bundle_size, interleaver_size, shift_index
    p.rnti, p.n_id_pdcch_dmrs, p.n_id_pdcch_data, p.n_rnti = rnti, n_id_dmrs, n_id_data, n_rnti
    p.cce_index, p.aggregation_level = cce_index, aggregation_level
    p.dmrs_power_offset_dB, p.data_power_offset_dB = dmrs_dB, data_dB
    payload = np.asarray(payload, dtype=np.uint8)
    p.payload_size = payload.size
    for i, b in enumerate(payload[:PDCCH_MAX_PAYLOAD]):
        p.payload[i] = int(b)
    if precoding is None:
        precoding = np.ones((1, 1), np.complex64)
    w = np.ascontiguousarray(np.asarray(precoding, dtype=np.complex64))
    assert w.ndim == 2
    p.nof_prg, p.nof_ports, p.prg_size_rb = w.shape[0], w.shape[1], prg_size_rb
    f = w.view(np.float32).reshape(-1)
    p._keepalive = f
    p.precoding = f.ctypes.data_as(C.POINTER(C.c_float))
    return p


class SsbPdu(C.Structure):
    """nrphy_ssb_pdu_t (ssb_processor::pdu_t)."""
    _fields_ = [("numerology", C.c_uint32), ("sfn", C.c_uint32), ("slot_index", C.c_uint32), ("phys_cell_id", C.c_uint32),
                ("beta_pss_dB", C.c_float), ("ssb_idx", C.c_uint32), ("L_max", C.c_uint32), ("common_scs", C.c_uint32),
                ("subcarrier_offset", C.c_uint32), ("offset_to_pointA", C.c_uint32), ("pattern_case", C.c_uint32),
                ("bch_payload", C.c_uint8 * 32), ("nof_ports", C.c_uint32), ("ports", C.c_uint8 * MAX_PORTS)]


SSB_CASE = {"A": 0, "B": 1, "C": 2, "D": 3, "E": 4}


def make_ssb(*, pattern_case, ssb_idx, L_max, phys_cell_id, payload, sfn=0, numerology=None, slot_index=None, common_scs=None,
             subcarrier_offset=0, offset_to_pointA=0, beta_pss_dB=0.0, ports=(0,)):
    """Builds an SsbPdu; the slot defaults to the one of the first half frame that carries candidate ``ssb_idx``."""
    case = SSB_CASE[pattern_case]
    mu = {0: 0, 1: 1, 2: 1, 3: 3, 4: 4}[case] if numerology is None else numerology
    first = {0: lambda i: (2, 8)[i % 2] + 14 * (i // 2), 1: lambda i: (4, 8, 16, 20)[i % 4] + 28 * (i // 4),
             2: lambda i: (2, 8)[i % 2] + 14 * (i // 2)}.get(case)
    p = SsbPdu()
    p.numerology, p.sfn = mu, sfn
    p.slot_index = (first(ssb_idx) // 14 if first else 0) if slot_index is None else slot_index
    p.phys_cell_id, p.beta_pss_dB, p.ssb_idx, p.L_max = phys_cell_id, beta_pss_dB, ssb_idx, L_max
    p.common_scs = (mu if mu < 4 else 3) if common_scs is None else common_scs
    p.subcarrier_offset, p.offset_to_pointA, p.pattern_case = subcarrier_offset, offset_to_pointA, case
    payload = np.asarray(payload, dtype=np.uint8)
    for i in range(32):
        p.bch_payload[i] = int(payload[i]) if i < payload.size else 0
    p.nof_ports = len(ports)
    for i, q in enumerate(ports):
        p.ports[i] = q
    return p


# NRPHY_MOD_*: bits per symbol, 0 for pi/2-BPSK
MOD_PI2_BPSK, MOD_BPSK, MOD_QPSK, MOD_QAM16, MOD_QAM64, MOD_QAM256 = 0, 1, 2, 4, 6, 8


class AmplitudeCfg(C.Structure):
    """nrphy_amplitude_cfg_t (the constructor arguments of amplitude_controller_{clipping,scaling}_impl)."""
    _fields_ = [("kind", C.c_uint32), ("enable_clipping", C.c_uint32), ("input_gain_dB", C.c_float),
                ("full_scale_lin", C.c_float), ("ceiling_dBFS", C.c_float)]


class AmplitudeStats(C.Structure):
    _fields_ = [("sum_power", C.c_float), ("peak_power", C.c_float), ("nof_clipped", C.c_uint32), ("nof_samples", C.c_uint32)]


class AmplitudeMetrics(C.Structure):
    """nrphy_amplitude_metrics_t (amplitude_controller_metrics)."""
    _fields_ = [("avg_power_fs", C.c_float), ("peak_power_fs", C.c_float), ("papr_lin", C.c_float), ("gain_dB", C.c_float),
                ("nof_processed_samples", C.c_uint64), ("nof_clipped_samples", C.c_uint64),
                ("clipping_probability", C.c_double), ("clipping_enabled", C.c_uint32), ("reserved_", C.c_uint32)]


class IqWireCfg(C.Structure):
    _fields_ = [("amplitude", AmplitudeCfg), ("ci16_scale", C.c_float)]


class DlSlotsCfg(C.Structure):
    """nrphy_dl_slots_cfg_t: the downlink slot pipeline (seams A and C on one device-resident grid)."""
    # (_fields_ set below OfdmConfig)


DL_SLOT_DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_uint32)   # nrphy_dl_slot_done_fn


class OfhCompressionCfg(C.Structure):
    """nrphy_ofh_compression_cfg_t (ru_compression_params + the compressor's iq_scaling)."""
    _fields_ = [("type", C.c_uint32), ("data_width", C.c_uint32), ("iq_scaling", C.c_float)]


class OfhUlSection(C.Structure):
    """nrphy_ofh_ul_section_t: one section of a decoded uplink user-plane message."""
    _fields_ = [("payload_offset", C.c_uint64), ("grid_index", C.c_uint32), ("port", C.c_uint16), ("symbol", C.c_uint16),
                ("start_prb", C.c_uint16), ("nof_prbs", C.c_uint16), ("type", C.c_uint8), ("data_width", C.c_uint8),
                ("reserved_", C.c_uint16)]


class OfhUlPrachSection(C.Structure):
    """nrphy_ofh_ul_prach_section_t: a section for the PRACH buffer with the two values of the reference's prach_context."""
    _fields_ = [("section", OfhUlSection), ("dst_offset", C.c_uint64), ("prach_nof_re", C.c_uint32), ("offset_to_first_re", C.c_uint32)]


class OfhDlFlow(C.Structure):
    """nrphy_ofh_dl_flow_t: one downlink user-plane data flow (addresses, MTU, RU bandwidth, builder, compression)."""
    _fields_ = [("mac_dst", C.c_uint8 * 6), ("mac_src", C.c_uint8 * 6), ("tci", C.c_uint16), ("eth_type", C.c_uint16),
                ("mtu", C.c_uint32), ("ru_nof_prbs", C.c_uint32), ("static_compression", C.c_uint32), ("compression", OfhCompressionCfg)]


class OfhDlFragment(C.Structure):
    """nrphy_ofh_dl_fragment_t: the PRBs and the length of one frame of a symbol."""
    _fields_ = [("start_prb", C.c_uint16), ("nof_prbs", C.c_uint16), ("frame_bytes", C.c_uint32)]


class OfhDlSymbol(C.Structure):
    """nrphy_ofh_dl_symbol_t: one OFDM symbol of one eAxC and where its frames go."""
    _fields_ = [("frame_offset", C.c_uint64), ("flow", C.c_uint32), ("grid_index", C.c_uint32), ("port", C.c_uint16),
                ("eaxc", C.c_uint16), ("sfn", C.c_uint16), ("subframe", C.c_uint8), ("slot", C.c_uint8), ("symbol", C.c_uint8),
                ("seq_id", C.c_uint8), ("reserved_", C.c_uint8 * 2)]


class OfhRxCfg(C.Structure):
    """nrphy_ofh_rx_cfg_t: what the reference's message receiver, its decoders and its user-plane decoders are constructed with."""
    _fields_ = [("mac_dst", C.c_uint8 * 6), ("mac_src", C.c_uint8 * 6), ("eth_type", C.c_uint16), ("reserved_", C.c_uint16),
                ("vlan_tag_present", C.c_uint32), ("ignore_ecpri_payload_size", C.c_uint32), ("seq_id_check", C.c_uint32),
                ("numerology", C.c_uint32), ("nof_symbols", C.c_uint32), ("ru_nof_prbs", C.c_uint32), ("static_compression", C.c_uint32),
                ("n_ul_eaxc", C.c_uint32), ("n_prach_eaxc", C.c_uint32), ("ul_eaxc", C.c_uint16 * 4), ("prach_eaxc", C.c_uint16 * 4),
                ("compression", OfhCompressionCfg), ("prach_compression", OfhCompressionCfg)]


class OfhRxFrame(C.Structure):
    """nrphy_ofh_rx_frame_t: the byte range of one received frame."""
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint32), ("reserved_", C.c_uint32)]


class OfhRxExpect(C.Structure):
    """nrphy_ofh_rx_expect_t: one (slot, eAxC) for which a control-plane message was sent."""
    _fields_ = [("grid_index", C.c_uint32), ("sfn8", C.c_uint16), ("eaxc", C.c_uint16), ("prb_start", C.c_uint16), ("nof_prb", C.c_uint16),
                ("context_symbols", C.c_uint16), ("subframe", C.c_uint8), ("slot", C.c_uint8), ("filter_index", C.c_uint8),
                ("start_symbol", C.c_uint8), ("nof_symbols", C.c_uint8), ("reserved_", C.c_uint8)]


class OfhRxRecord(C.Structure):
    """nrphy_ofh_rx_record_t: what became of one frame."""
    _fields_ = [("payload_offset", C.c_uint64), ("status", C.c_uint32), ("seq_skipped", C.c_int32), ("grid_index", C.c_uint32),
                ("expect_index", C.c_uint32), ("eaxc", C.c_uint16), ("seq_id", C.c_uint16), ("start_prb", C.c_uint16),
                ("nof_prbs", C.c_uint16), ("nof_prbs_written", C.c_uint16), ("port", C.c_uint16), ("sfn8", C.c_uint16),
                ("filter_index", C.c_uint8), ("subframe", C.c_uint8), ("slot", C.c_uint8), ("symbol", C.c_uint8), ("type", C.c_uint8),
                ("data_width", C.c_uint8), ("reserved_", C.c_uint8 * 4)]


class OfdmConfig(C.Structure):
    _fields_ = [
        ("numerology", C.c_uint32),
        ("bw_rb", C.c_uint32),
        ("dft_size", C.c_uint32),
        ("cp", C.c_uint32),
        ("scale", C.c_float),
        ("center_freq_hz", C.c_double),
    ]


DlSlotsCfg._fields_ = [("ofdm", OfdmConfig), ("nof_ports", C.c_uint32), ("depth", C.c_uint32), ("max_tb_bytes", C.c_uint32),
                       ("iq_format", C.c_uint32), ("wire", IqWireCfg)]

IQ_CF32, IQ_CI16 = 0, 1   # NRPHY_IQ_*: the sample format of nrphy_ofdm_demod_symbols and of an uplink slot pool


class UlSlotsCfg(C.Structure):
    """nrphy_ul_slots_cfg_t: the uplink slot pipeline (baseband samples to PUSCH, PUCCH and SRS results on one device-resident grid)."""
    _fields_ = [("ofdm", OfdmConfig), ("nof_ports", C.c_uint32), ("depth", C.c_uint32), ("iq_format", C.c_uint32),
                ("iq_scale", C.c_float), ("window_offset", C.c_uint32), ("max_pusch", C.c_uint32), ("max_pucch", C.c_uint32),
                ("max_pf2", C.c_uint32), ("max_srs", C.c_uint32), ("max_tb_bytes", C.c_uint32), ("max_uci_bits", C.c_uint32)]


UL_SLOT_DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_uint32)   # nrphy_ul_slot_done_fn


class PrachWindowsCfg(C.Structure):
    """nrphy_prach_windows_cfg_t: the PRACH window pipeline (baseband samples to detected preambles, the prach_buffer on the device)."""
    _fields_ = [("srate_hz", C.c_uint32), ("nof_radio_ports", C.c_uint32), ("depth", C.c_uint32), ("iq_format", C.c_uint32),
                ("max_window_samples", C.c_uint32), ("iq_scale", C.c_float), ("max_ports", C.c_uint32),
                ("max_td_occasions", C.c_uint32), ("max_fd_occasions", C.c_uint32)]


PRACH_WINDOW_DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_uint32)   # nrphy_prach_window_done_fn


def prb_mask_words(prbs):
    """Bit mask words (5 x uint64) with the given PRB indices set."""
    words = [0] * PRB_WORDS
    for p in prbs:
        words[p // 64] |= 1 << (p % 64)
    return words


def bits_to_mask(bits):
    m = 0
    for i, b in enumerate(bits):
        if b:
            m |= 1 << i
    return m


def identity_precoding(nof_layers):
    """precoding_configuration::make_wideband(make_identity(n)) -- [1][n][n] complex."""
    w = np.zeros((1, nof_layers, nof_layers, 2), dtype=np.float32)
    for i in range(nof_layers):
        w[0, i, i, 0] = 1.0
    return w


def make_pdu(*, slot_index=0, rnti=1, bwp_start_rb=0, bwp_size_rb=52, qm=2, rv=0, n_id=0, ref_point=0,
             dmrs_symbols=(2,), dmrs_type=1, scrambling_id=0, n_scid=0, nof_cdm_groups_without_data=2,
             prb_start=0, prb_count=52, prbs=None, start_symbol=0, nof_symbols=14, base_graph=1,
             tbs_lbrm_bytes=TBS_LBRM_DEFAULT, reserved=(), ratio_dmrs_dB=0.0, ratio_data_dB=0.0,
             precoding=None, prg_size_rb=MAX_RB, tb_size_bytes=0, nof_codewords=1, cp=0, vrb_contiguous=None):
    """Builds a PdschPdu.  ``precoding`` is an array [nof_prg][nof_ports][nof_layers] complex64 or
    [...][2] float32; ``reserved`` a sequence of (prbs, re_bits[12], symbol_bits[14]).  The numpy weight
    array is attached to the returned struct (``_keepalive``) so the pointer stays valid."""
    pdu = PdschPdu()
    pdu.slot_index = slot_index
    pdu.rnti = rnti
    pdu.bwp_start_rb = bwp_start_rb
    pdu.bwp_size_rb = bwp_size_rb
    pdu.cp = cp
    pdu.qm = qm
    pdu.rv = rv
    pdu.nof_codewords = nof_codewords
    pdu.n_id = n_id
    pdu.ref_point = ref_point
    pdu.dmrs_symbol_mask = sum(1 << l for l in dmrs_symbols)
    pdu.dmrs_type = dmrs_type
    pdu.scrambling_id = scrambling_id
    pdu.n_scid = n_scid
    pdu.nof_cdm_groups_without_data = nof_cdm_groups_without_data
    pdu.start_symbol_index = start_symbol
    pdu.nof_symbols = nof_symbols
    pdu.ldpc_base_graph = base_graph
    pdu.tbs_lbrm_bytes = tbs_lbrm_bytes
    if prbs is None:
        prbs = list(range(prb_start, prb_start + prb_count))
    prbs = sorted(prbs)
    contiguous = len(prbs) > 0 and prbs[-1] - prbs[0] + 1 == len(prbs)
    pdu.vrb_contiguous = int(contiguous if vrb_contiguous is None else vrb_contiguous)
    for i, w in enumerate(prb_mask_words(prbs)):
        pdu.prb_mask[i] = w
    pdu.nof_reserved = len(reserved)
    for i, (rprbs, re_bits, sym_bits) in enumerate(reserved):
        for j, w in enumerate(prb_mask_words(rprbs)):
            pdu.reserved[i].prb_mask[j] = w
        pdu.reserved[i].re_mask = bits_to_mask(re_bits)
        pdu.reserved[i].symbol_mask = bits_to_mask(sym_bits)
    pdu.tb_size_bytes = tb_size_bytes
    pdu.ratio_pdsch_dmrs_to_sss_dB = ratio_dmrs_dB
    pdu.ratio_pdsch_data_to_sss_dB = ratio_data_dB
    if precoding is None:
        precoding = identity_precoding(1)
    w = np.asarray(precoding)
    if np.iscomplexobj(w):
        w = np.stack([w.real, w.imag], axis=-1)
    w = np.ascontiguousarray(w, dtype=np.float32)
    assert w.ndim == 4 and w.shape[3] == 2, "precoding must be [nof_prg][nof_ports][nof_layers] complex"
    pdu.nof_prg, pdu.nof_ports, pdu.nof_layers = w.shape[0], w.shape[1], w.shape[2]
    pdu.prg_size_rb = prg_size_rb
    pdu.precoding = w.ctypes.data_as(C.POINTER(C.c_float))
    pdu._keepalive = w
    return pdu


def declare(lib, prefix="nrphy_"):
    """Attaches argtypes/restypes for the entry points of include/mi355_nrphy.h found in ``lib``.
    The same signatures (with prefix ``oracle_``) are exported by the CPU oracle."""
    P = C.POINTER
    vp, u8p, u32, u64, i32 = C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int

    def sig(name, restype, *argtypes):
        fn = getattr(lib, prefix + name, None)
        if fn is not None:
            fn.restype = restype
            fn.argtypes = list(argtypes)

    sig("version", C.c_char_p)
    sig("strerror", C.c_char_p, i32)
    sig("create", i32, P(vp), i32)
    sig("destroy", i32, vp)
    sig("synchronize", i32, vp, vp)
    sig("pdsch_validate", i32, P(PdschPdu))
    sig("pdsch_derive", i32, P(PdschPdu), P(PdschDerived))
    sig("tbs_calculate", u32, u32, u32, u32, u32, C.c_float, u32, u32)
    sig("ofdm_symbol_size", u32, P(OfdmConfig), u32)
    sig("ofdm_slot_size", u32, P(OfdmConfig), u32)
    sig("pdsch_plan_create", i32, vp, u32, P(PdschPdu), P(u64), P(u32), u32, u32, u32, P(vp))
    sig("pdsch_plan_destroy", i32, vp)
    sig("pdsch_plan_nof_codeblocks", u32, vp)
    sig("pdsch_plan_codeword_bits", u64, vp)
    sig("pdsch_plan_codeword_offset", u64, vp, u32)
    sig("pdsch_plan_nof_sequences", i32, vp, P(u32), P(u32))
    sig("pdsch_plan_scrambling_form", i32, vp)
    sig("pdsch_plan_codeblock_dispatch", i32, vp)
    sig("pdsch_run", i32, vp, u8p, vp, u8p, u8p, i32, vp)
    sig("pdsch_plan_enable_timing", i32, vp, u32)
    sig("pdsch_plan_kernel_times", i32, vp, P(C.c_float), P(u32))
    sig("ofdm_plan_enable_timing", i32, vp, u32)
    sig("ofdm_plan_kernel_time", i32, vp, P(C.c_float), P(u32))
    sig("pdsch_process_host", i32, vp, P(PdschPdu), u8p, vp, u32, u32, u8p, u8p)
    sig("pdsch_async_create", i32, vp, u32, u32, u32, u32, P(vp))
    sig("pdsch_async_submit", i32, vp, P(PdschPdu), u8p, vp, vp)
    sig("pdsch_async_wait", i32, vp)
    sig("pdsch_async_wait_slot", i32, vp)
    sig("pdsch_async_destroy", i32, vp)
    sig("pdsch_encode_host", i32, vp, P(PdschEncoderCfg), u8p, u8p, u8p)
    sig("ldpc_encode", i32, vp, u32, u32, u32, u8p, u32, u32, u8p, u32, vp)
    sig("ofdm_plan_create", i32, vp, P(OfdmConfig), u32, P(vp))
    sig("ofdm_plan_destroy", i32, vp)
    sig("ofdm_plan_slot_stride", u32, vp)
    sig("ofdm_run", i32, vp, u32, vp, vp, vp, vp)
    sig("ofdm_modulate_symbol_host", i32, vp, vp, u32, u32, vp, u32)
    sig("dft_run", i32, vp, u32, i32, u32, vp, vp, vp)
    sig("dft_run_host", i32, vp, u32, i32, vp, vp)
    sig("ofdm_modulate_slot_host", i32, vp, vp, u32, vp)
    sig("ofdm_demod_run", i32, vp, u32, vp, vp, u32, vp, vp)
    sig("ofdm_demodulate_slot_host", i32, vp, vp, u32, u32, vp)
    sig("ofdm_demodulate_symbol_host", i32, vp, vp, u32, u32, u32, vp)
    sig("ldpc_decoder_scratch_bytes", i32, vp, P(LdpcDecoderCfg), u32, P(u64))
    sig("ldpc_decoder_prepare", i32, vp, P(LdpcDecoderCfg))
    sig("ldpc_decode", i32, vp, P(LdpcDecoderCfg), u32, vp, u32, vp, u32, vp, vp, vp)
    sig("ldpc_decode_host", i32, vp, P(LdpcDecoderCfg), vp, u8p, P(u32))
    sig("ldpc_rate_dematch", i32, vp, P(LdpcRateDematcherCfg), u32, vp, u32, vp, u32, i32, vp)
    sig("ldpc_rate_dematch_host", i32, vp, P(LdpcRateDematcherCfg), vp, vp, i32)
    sig("llr_descramble", i32, vp, u32, vp, u32, vp, C.c_size_t, vp, C.c_size_t, vp)
    sig("llr_descramble_host", i32, vp, u32, u32, vp, vp)
    sig("pdsch_process_slot_host", i32, vp, u32, vp, vp, vp, u32, u32)
    sig("pdsch_async_submit_slot", i32, vp, u32, vp, vp, vp, vp)
    sig("demodulate_soft", i32, vp, u32, u32, u32, vp, vp, vp, vp)
    sig("demodulate_soft_host", i32, vp, u32, u32, vp, vp, vp)
    sig("grid_put", i32, vp, vp, u32, u32, u32, P(GridRe), vp)
    sig("csi_rs_validate", i32, P(CsiRsCfg))
    sig("csi_rs_map", i32, vp, u32, P(CsiRsCfg), P(u32), vp, u32, u32, vp)
    sig("csi_rs_map_host", i32, vp, P(CsiRsCfg), vp, u32, u32)
    sig("pdcch_validate", i32, P(PdcchPdu))
    sig("pdcch_process", i32, vp, u32, P(PdcchPdu), P(u32), vp, u32, u32, vp)
    sig("pdcch_process_host", i32, vp, P(PdcchPdu), vp, u32, u32)
    sig("pdcch_encode_host", i32, vp, u8p, u32, u32, u32, u8p)
    sig("ssb_validate", i32, P(SsbPdu))
    sig("ssb_process", i32, vp, u32, P(SsbPdu), P(u32), vp, u32, u32, vp)
    sig("ssb_process_host", i32, vp, P(SsbPdu), vp, u32, u32)
    sig("pbch_encode_host", i32, vp, P(SsbPdu), u8p)
    sig("amplitude_control", i32, vp, P(AmplitudeCfg), u32, u32, vp, C.c_size_t, vp, C.c_size_t, vp, vp)
    sig("amplitude_metrics", i32, P(AmplitudeCfg), P(AmplitudeStats), P(AmplitudeMetrics))
    sig("amplitude_control_host", i32, vp, P(AmplitudeCfg), vp, u32, vp, P(AmplitudeMetrics))
    sig("iq_convert_ci16", i32, vp, u32, u32, vp, C.c_size_t, C.c_float, vp, C.c_size_t, vp)
    sig("iq_convert_ci16_host", i32, vp, vp, u32, C.c_float, vp)
    sig("ofdm_run_ci16", i32, vp, u32, vp, vp, P(IqWireCfg), vp, vp, vp)
    sig("ofh_compressed_prb_bytes", u32, P(OfhCompressionCfg))
    sig("ofh_compress", i32, vp, P(OfhCompressionCfg), u32, u32, vp, C.c_size_t, vp, C.c_size_t, vp)
    sig("ofh_compress_host", i32, vp, P(OfhCompressionCfg), u32, vp, vp)
    sig("ofh_decompress", i32, vp, P(OfhCompressionCfg), u32, u32, vp, C.c_size_t, vp, C.c_size_t, vp)
    sig("ofh_decompress_host", i32, vp, P(OfhCompressionCfg), u32, vp, vp)
    sig("ofh_ul_validate", i32, u32, P(OfhUlSection), u64, u32, u32, u32)
    sig("ofh_ul_write_grid", i32, vp, u32, P(OfhUlSection), vp, u64, vp, u32, u32, u32, vp)
    sig("ofh_ul_prach_validate", i32, u32, P(OfhUlPrachSection), u64, u64)
    sig("ofh_ul_write_prach", i32, vp, u32, P(OfhUlPrachSection), vp, u64, vp, u64, vp)
    sig("ofh_rx_create", i32, vp, P(OfhRxCfg), P(vp))
    sig("ofh_rx_destroy", i32, vp)
    sig("ofh_rx_reset", i32, vp, vp)
    sig("ofh_rx_validate", i32, P(OfhRxCfg), u32, P(OfhRxFrame), u32, P(OfhRxExpect), u64, u32, u32, u32)
    sig("ofh_rx_run", i32, vp, u32, P(OfhRxFrame), u32, P(OfhRxExpect), vp, u64, vp, u32, u32, u32, vp, vp)
    sig("ofh_rx_host", i32, vp, vp, u32, u32, P(OfhRxExpect), vp, u32, u32, P(OfhRxRecord))
    sig("ofh_dl_fragments", i32, P(OfhDlFlow), u32, P(OfhDlFragment), P(u32))
    sig("ofh_dl_validate", i32, u32, P(OfhDlFlow), u32, P(OfhDlSymbol), u32, u32, u32, u64, u32)
    sig("ofh_dl_write_frames", i32, vp, u32, P(OfhDlFlow), u32, P(OfhDlSymbol), vp, u32, u32, u32, vp, u64, u32, vp)
    sig("ofh_dl_frames_host", i32, vp, P(OfhDlFlow), P(OfhDlSymbol), vp, u32, vp, u64, u32)
    sig("pusch_decoder_sizes", i32, vp, P(PuschDecoderCfg), u32, P(u64), P(u64), P(u64), P(u32))
    sig("pusch_decoder_prepare", i32, vp, P(PuschDecoderCfg))
    sig("pusch_decode_batch", i32, vp, P(PuschDecoderCfg), u32, vp, u64, vp, vp, vp, vp, u32, vp, vp)
    sig("dl_slots_create", i32, vp, P(DlSlotsCfg), P(vp))
    sig("dl_slots_destroy", i32, vp)
    sig("dl_slots_wait_free", i32, vp)
    sig("dl_slot_open", i32, vp, P(u32))
    sig("dl_slot_close", i32, vp, u32)
    sig("dl_slot_pdsch", i32, vp, u32, u32, vp, vp)
    sig("dl_slot_pdcch", i32, vp, u32, u32, P(PdcchPdu))
    sig("dl_slot_ssb", i32, vp, u32, u32, P(SsbPdu))
    sig("dl_slot_csi_rs", i32, vp, u32, u32, P(CsiRsCfg))
    sig("dl_slot_put", i32, vp, u32, u32, P(GridRe))
    sig("dl_slot_load_grid", i32, vp, u32, vp)
    sig("dl_slot_modulate", i32, vp, u32, u32, vp, vp)
    sig("dl_slot_poll", i32, vp, u32)
    sig("dl_slot_wait", i32, vp, u32)
    sig("dl_slot_iq", vp, vp, u32, u32, P(u32))
    sig("dl_slot_read_grid", i32, vp, u32, vp)
    sig("dl_slot_amplitude_stats", P(AmplitudeStats), vp, u32, u32)
    sig("dl_slot_device_grid", vp, vp, u32)
    sig("dl_slot_stream", vp, vp, u32)
    sig("channel_equalize", i32, vp, u32, u32, u32, u32, u32, vp, vp, vp, C.c_float, vp, vp, vp)
    sig("channel_equalize_host", i32, vp, u32, u32, u32, u32, vp, vp, vp, C.c_float, vp, vp)
    sig("pusch_demod_validate", i32, P(PuschDemodCfg), u32, u32)
    sig("pusch_demod_codeword_bits", u64, P(PuschDemodCfg))
    sig("pusch_demod_plan_create", i32, vp, u32, P(PuschDemodCfg), P(u32), u32, u32, u32, P(u64), P(vp))
    sig("pusch_demod_plan_destroy", i32, vp)
    sig("pusch_demod_plan_codeword_bits", u64, vp, u32)
    sig("pusch_demod_run", i32, vp, vp, vp, vp, vp, u64, vp, vp)
    sig("pusch_demodulate_host", i32, vp, P(PuschDemodCfg), vp, u32, u32, vp, vp, vp, vp)
    sig("pusch_demod_validate_ex", i32, P(PuschDemodCfg), u32, u32, u32)
    sig("pusch_demod_plan_create_ex", i32, vp, u32, P(PuschDemodCfg), P(u32), u32, u32, u32, P(u64), u32, P(vp))
    sig("pusch_demodulate_host_ex", i32, vp, P(PuschDemodCfg), vp, u32, u32, vp, vp, u32, vp, vp)
    sig("pusch_demod_run_evm", i32, vp, vp, vp, vp, vp, u64, vp, vp, vp)
    sig("pusch_demodulate_host_evm", i32, vp, P(PuschDemodCfg), vp, u32, u32, vp, vp, u32, vp, vp, vp)
    sig("transform_precoding_nof_prb_valid", i32, u32)
    sig("transform_deprecode", i32, vp, u32, u32, vp, vp, vp)
    sig("transform_deprecode_host", i32, vp, u32, vp, vp)
    sig("pusch_chest_validate", i32, P(PuschChestCfg), u32, u32)
    sig("pusch_chest_plan_create", i32, vp, u32, P(PuschChestCfg), P(u32), u32, u32, u32, P(u64), P(vp))
    sig("pusch_chest_plan_destroy", i32, vp)
    sig("pusch_chest_run", i32, vp, vp, vp, vp, vp, vp)
    sig("pusch_chest_host", i32, vp, P(PuschChestCfg), vp, u32, u32, vp, vp, vp)
    sig("pusch_chest_validate_ex", i32, P(PuschChestCfg), P(PuschChestLowpapr), u32, u32)
    sig("pusch_chest_plan_create_ex", i32, vp, u32, P(PuschChestCfg), P(PuschChestLowpapr), P(u32), u32, u32, u32, P(u64), P(vp))
    sig("pusch_chest_host_ex", i32, vp, P(PuschChestCfg), P(PuschChestLowpapr), vp, u32, u32, vp, vp, vp)
    sig("pusch_lowpapr_sequence_host", i32, vp, u32, u32, vp)
    sig("prach_threshold", i32, P(PrachCfg), P(C.c_float), P(u32), P(u32))
    sig("prach_validate", i32, P(PrachCfg))
    sig("prach_window_width", u32, P(PrachCfg))
    sig("prach_plan_create", i32, vp, u32, P(PrachCfg), P(u64), u64, u64, P(vp))
    sig("prach_plan_destroy", i32, vp)
    sig("prach_plan_metric_stride", u32, vp)
    sig("prach_run", i32, vp, vp, vp, vp, vp, vp)
    sig("prach_detect_host", i32, vp, P(PrachCfg), vp, u64, u64, P(PrachResult), P(PrachPreamble), vp)
    sig("prach_generate_host", i32, vp, P(PrachCfg), u32, vp)
    sig("prach_demod_validate", i32, P(PrachDemodCfg))
    sig("prach_demod_sizes", i32, P(PrachDemodCfg), P(PrachDemodSizes))
    sig("prach_demod_plan_create", i32, vp, u32, P(PrachDemodCfg), P(u64), u64, P(u64), u64, u64, u64, u64, P(vp))
    sig("prach_demod_plan_destroy", i32, vp)
    sig("prach_demod_run", i32, vp, vp, vp, vp)
    sig("prach_demodulate_host", i32, vp, P(PrachDemodCfg), vp, u64, vp, u64, u64, u64, u64)
    sig("pucch_validate", i32, P(PucchCfg), u32, u32)
    sig("pucch_plan_create", i32, vp, u32, P(PucchCfg), P(u32), u32, u32, u32, P(u64), P(vp))
    sig("pucch_plan_destroy", i32, vp)
    sig("pucch_run", i32, vp, vp, vp, vp, vp, vp)
    sig("pucch_host", i32, vp, P(PucchCfg), vp, u32, u32, P(PucchResult), vp, vp)
    sig("uci_decoder_validate", i32, P(UciDecoderCfg))
    sig("uci_decoder_plan_create", i32, vp, u32, P(UciDecoderCfg), P(u64), P(u64), P(vp))
    sig("uci_decoder_plan_destroy", i32, vp)
    sig("uci_decoder_run", i32, vp, vp, vp, vp, vp)
    sig("uci_decode_host", i32, vp, P(UciDecoderCfg), vp, vp, P(u32))
    sig("pf2_validate", i32, P(Pf2Cfg), u32, u32)
    sig("pf2_sizes", i32, P(Pf2Cfg), P(u32), P(u32))
    sig("pf2_plan_create", i32, vp, u32, P(Pf2Cfg), P(u32), u32, u32, u32, P(u64), P(u64), P(u64), P(vp))
    sig("pf2_plan_destroy", i32, vp)
    sig("pf2_run", i32, vp, vp, vp, vp, vp, vp, vp, vp, vp)
    sig("pf2_host", i32, vp, P(Pf2Cfg), vp, u32, u32, vp, P(u32), P(Pf2Csi), vp, vp, vp)
    sig("srs_validate", i32, P(SrsCfg), u32, u32)
    sig("srs_info", i32, P(SrsCfg), u32, P(u32), P(u32), P(u32), P(u32), P(u32))
    sig("srs_plan_create", i32, vp, u32, P(SrsCfg), P(u32), u32, u32, u32, P(vp))
    sig("srs_plan_destroy", i32, vp)
    sig("srs_run", i32, vp, vp, vp, vp)
    sig("srs_host", i32, vp, P(SrsCfg), vp, u32, u32, P(SrsResult))
    sig("srs_sequence_host", i32, vp, P(SrsCfg), u32, vp)
    sig("ulsch_demux_validate", i32, P(UlschDemuxCfg))
    sig("ulsch_demux_sizes", i32, P(UlschDemuxCfg), P(UlschDemuxSizes))
    sig("ulsch_demux_plan_create", i32, vp, u32, P(UlschDemuxCfg), P(u64), P(u64), P(u64), P(u64), P(u64), P(vp))
    sig("ulsch_demux_plan_destroy", i32, vp)
    sig("ulsch_demux_run", i32, vp, vp, vp, vp, vp, vp, vp)
    sig("ulsch_demultiplex_host", i32, vp, P(UlschDemuxCfg), vp, vp, vp, vp, vp)
    sig("pusch_decode_codeblock_host", i32, vp, P(LdpcRateDematcherCfg), u32, u32, C.c_float, vp, vp, i32, u8p, P(u32))
    sig("ul_sch_info", i32, P(UlschInfoCfg), P(UlschInfo))
    sig("pusch_proc_validate", i32, P(PuschPdu), P(PuschProcOptions), u32, u32)
    sig("pusch_proc_derive", i32, P(PuschPdu), P(PuschProcOptions), u32, u32, P(PuschProcDerived))
    sig("pusch_proc_harq_bytes", i32, P(PuschPdu), P(PuschProcOptions), P(u64), P(u64))
    sig("pusch_proc_plan_create", i32, vp, u32, P(PuschPdu), P(PuschProcOptions), P(u32), u32, u32, u32, P(u64), P(u64), P(u64), P(u64),
        P(vp))
    sig("pusch_proc_plan_destroy", i32, vp)
    sig("pusch_proc_plan_harq_bytes", i32, vp, u32, P(u64), P(u64))
    sig("pusch_proc_run", i32, vp, vp, vp, vp, vp, vp, vp)
    sig("pusch_proc_host", i32, vp, P(PuschPdu), P(PuschProcOptions), vp, u32, u32, vp, vp, vp, vp, P(PuschResult))
    sig("pusch_evm_validate", i32, P(PuschPdu), P(PuschEvmOptions), u32, u32)
    sig("pusch_evm_plan_create", i32, vp, u32, P(PuschPdu), P(PuschEvmOptions), P(u32), u32, u32, u32, P(u64), P(u64), P(u64), P(u64),
        P(vp))
    sig("pusch_evm_host", i32, vp, P(PuschPdu), P(PuschEvmOptions), vp, u32, u32, vp, vp, vp, vp, P(PuschResult))
    sig("pusch_evm_slot", i32, vp, u32, u32, P(PuschPdu), P(PuschEvmOptions), P(u64), P(u64))
    sig("pusch_tp_validate", i32, P(PuschPdu), P(PuschTpDesc), P(PuschEvmOptions), u32, u32)
    sig("pusch_tp_derive", i32, P(PuschPdu), P(PuschTpDesc), P(PuschEvmOptions), u32, u32, P(PuschProcDerived), P(PuschChestLowpapr))
    sig("pusch_tp_harq_bytes", i32, P(PuschPdu), P(PuschTpDesc), P(PuschEvmOptions), P(u64), P(u64))
    sig("pusch_tp_plan_create", i32, vp, u32, P(PuschPdu), P(PuschTpDesc), P(PuschEvmOptions), P(u32), u32, u32, u32, P(u64), P(u64),
        P(u64), P(u64), P(vp))
    sig("pusch_tp_host", i32, vp, P(PuschPdu), P(PuschTpDesc), P(PuschEvmOptions), vp, u32, u32, vp, vp, vp, vp, P(PuschResult))
    sig("pusch_tp_slot", i32, vp, u32, u32, P(PuschPdu), P(PuschTpDesc), P(PuschEvmOptions), P(u64), P(u64))
    sig("pusch_csi2_size", i32, P(PuschCsi2Desc), vp, u32, P(u32))
    sig("pusch_csi2_validate", i32, P(PuschPdu), P(PuschCsi2Desc), P(PuschProcOptions), u32, u32)
    sig("pusch_csi2_variants", i32, P(PuschPdu), P(PuschCsi2Desc), P(PuschProcOptions), u32, u32, P(u32), P(u32), P(UlschInfo))
    sig("pusch_csi2_harq_bytes", i32, P(PuschPdu), P(PuschCsi2Desc), P(PuschProcOptions), P(u64), P(u64))
    sig("pusch_csi2_plan_create", i32, vp, u32, P(PuschPdu), P(PuschCsi2Desc), P(PuschProcOptions), P(u32), u32, u32, u32, P(u64),
        P(u64), P(u64), P(u64), P(u64), P(vp))
    sig("pusch_csi2_plan_destroy", i32, vp)
    sig("pusch_csi2_run", i32, vp, vp, vp, vp, vp, vp, vp, vp)
    sig("pusch_csi2_host", i32, vp, P(PuschPdu), P(PuschCsi2Desc), P(PuschProcOptions), vp, u32, u32, vp, vp, vp, vp, vp,
        P(PuschResult), P(PuschCsi2Result))
    sig("ofdm_demod_symbols", i32, vp, u32, vp, u32, C.c_float, vp, u32, u32, u32, vp, vp)
    sig("ul_slots_create", i32, vp, P(UlSlotsCfg), vp, P(vp))
    sig("ul_slots_destroy", i32, vp)
    sig("ul_slots_wait_free", i32, vp)
    sig("ul_slot_open", i32, vp, u32, P(u32))
    sig("ul_slot_close", i32, vp, u32)
    sig("ul_slot_samples", i32, vp, u32, u32, u32, P(vp))
    sig("ul_slot_load_grid", i32, vp, u32, vp)
    sig("ul_slot_device_grid", vp, vp, u32)
    sig("ul_slot_stream", vp, vp, u32)
    sig("ul_slot_symbols_written", i32, vp, u32, u32)
    sig("ul_slot_pusch", i32, vp, u32, u32, P(PuschPdu), P(PuschProcOptions), P(u64), P(u64))
    sig("ul_slot_pf01", i32, vp, u32, u32, P(PucchCfg))
    sig("ul_slot_pf2", i32, vp, u32, u32, P(Pf2Cfg))
    sig("ul_slot_srs", i32, vp, u32, u32, P(SrsCfg))
    sig("ul_slot_finish", i32, vp, u32, vp, vp)
    sig("ul_slot_poll", i32, vp, u32)
    sig("ul_slot_wait", i32, vp, u32)
    sig("ul_slot_read_grid", i32, vp, u32, vp)
    sig("ul_slot_pusch_results", vp, vp, u32, P(u32))
    sig("ul_slot_tb", vp, vp, u32, u32, P(u32))
    sig("ul_slot_pusch_uci", vp, vp, u32, u32, P(u32))
    sig("ul_slot_pf01_results", vp, vp, u32, P(u32))
    sig("ul_slot_format2_results", i32, vp, u32, u32, P(vp), P(u32), P(u32), P(Pf2Csi))
    sig("ul_slot_sounding_results", vp, vp, u32, P(u32))
    sig("prach_window_demod_run", i32, vp, vp, u32, C.c_float, vp, vp)
    sig("prach_windows_create", i32, vp, P(PrachWindowsCfg), P(vp))
    sig("prach_windows_destroy", i32, vp)
    sig("prach_windows_wait_free", i32, vp)
    sig("prach_windows_plans_made", u64, vp)
    sig("prach_window_open", i32, vp, P(PrachDemodCfg), P(u32), P(PrachCfg), vp, vp, P(u32))
    sig("prach_window_close", i32, vp, u32)
    sig("prach_window_samples", i32, vp, u32, u32, P(vp), P(u32))
    sig("prach_window_device_buffer", vp, vp, u32)
    sig("prach_window_stream", vp, vp, u32)
    sig("prach_window_buffer_written", i32, vp, u32)
    sig("prach_window_poll", i32, vp, u32)
    sig("prach_window_wait", i32, vp, u32)
    sig("prach_window_read_buffer", i32, vp, u32, vp)
    sig("prach_window_results", vp, vp, u32, P(u32))
    sig("prach_window_preambles", vp, vp, u32, u32)
    return lib


# Symbols include/mi355_nrphy.h declares; tests check the shared library exports every one.
ABI_SYMBOLS = [
    "nrphy_version", "nrphy_strerror", "nrphy_trace_enabled", "nrphy_create", "nrphy_destroy", "nrphy_synchronize",
    "nrphy_pdsch_validate", "nrphy_pdsch_derive", "nrphy_tbs_calculate", "nrphy_ofdm_symbol_size",
    "nrphy_ofdm_slot_size", "nrphy_pdsch_plan_create", "nrphy_pdsch_plan_destroy",
    "nrphy_pdsch_plan_nof_codeblocks", "nrphy_pdsch_plan_codeword_bits", "nrphy_pdsch_plan_codeword_offset",
    "nrphy_pdsch_plan_nof_sequences", "nrphy_pdsch_plan_scrambling_form", "nrphy_pdsch_plan_codeblock_dispatch",
    "nrphy_pdsch_run", "nrphy_pdsch_plan_enable_timing", "nrphy_pdsch_plan_kernel_times", "nrphy_pdsch_plan_timing_stride",
    "nrphy_ofdm_plan_enable_timing", "nrphy_ofdm_plan_kernel_time", "nrphy_ofdm_plan_timing_stride", "nrphy_pdsch_process_host", "nrphy_pdsch_encode_host", "nrphy_ldpc_encode", "nrphy_ofdm_plan_create",
    "nrphy_ofdm_plan_destroy", "nrphy_ofdm_plan_slot_stride", "nrphy_ofdm_run",
    "nrphy_ofdm_modulate_symbol_host", "nrphy_ofdm_modulate_slot_host", "nrphy_dft_run", "nrphy_dft_run_host",
    "nrphy_ofdm_demod_run", "nrphy_ofdm_demodulate_slot_host", "nrphy_ofdm_demodulate_symbol_host",
    "nrphy_ldpc_decode", "nrphy_ldpc_decode_host", "nrphy_ldpc_rate_dematch", "nrphy_ldpc_rate_dematch_host",
    "nrphy_pusch_decode_codeblock_host", "nrphy_pusch_decoder_sizes", "nrphy_pusch_decode_batch",
    "nrphy_ldpc_decoder_scratch_bytes", "nrphy_ldpc_decoder_prepare", "nrphy_pusch_decoder_prepare",
    "nrphy_csi_rs_validate", "nrphy_csi_rs_map", "nrphy_csi_rs_map_host", "nrphy_grid_put",
    "nrphy_llr_descramble", "nrphy_llr_descramble_host", "nrphy_demodulate_soft", "nrphy_demodulate_soft_host", "nrphy_pdsch_process_slot_host", "nrphy_pdsch_async_submit_slot",
    "nrphy_pdcch_validate", "nrphy_pdcch_process", "nrphy_pdcch_process_host", "nrphy_pdcch_encode_host",
    "nrphy_ssb_validate", "nrphy_ssb_process", "nrphy_ssb_process_host", "nrphy_pbch_encode_host",
    "nrphy_pdsch_async_create", "nrphy_pdsch_async_submit", "nrphy_pdsch_async_wait", "nrphy_pdsch_async_wait_slot",
    "nrphy_pdsch_async_destroy",
    "nrphy_pdsch_async_count_done",
    "nrphy_amplitude_control", "nrphy_amplitude_metrics", "nrphy_amplitude_control_host", "nrphy_iq_convert_ci16",
    "nrphy_iq_convert_ci16_host", "nrphy_ofdm_run_ci16", "nrphy_ofh_compressed_prb_bytes", "nrphy_ofh_compress",
    "nrphy_ofh_compress_host", "nrphy_ofh_decompress", "nrphy_ofh_decompress_host", "nrphy_ofh_ul_validate", "nrphy_ofh_ul_write_grid",
    "nrphy_ofh_ul_prach_validate", "nrphy_ofh_ul_write_prach",
    "nrphy_ofh_rx_create", "nrphy_ofh_rx_destroy", "nrphy_ofh_rx_reset", "nrphy_ofh_rx_validate", "nrphy_ofh_rx_run", "nrphy_ofh_rx_host",
    "nrphy_ofh_dl_fragments", "nrphy_ofh_dl_validate", "nrphy_ofh_dl_write_frames", "nrphy_ofh_dl_frames_host",
    "nrphy_dl_slots_create", "nrphy_dl_slots_destroy", "nrphy_dl_slots_wait_free", "nrphy_dl_slot_open", "nrphy_dl_slot_close",
    "nrphy_dl_slot_pdsch", "nrphy_dl_slot_pdcch", "nrphy_dl_slot_ssb", "nrphy_dl_slot_csi_rs", "nrphy_dl_slot_put",
    "nrphy_dl_slot_load_grid", "nrphy_dl_slot_modulate", "nrphy_dl_slot_poll", "nrphy_dl_slot_wait", "nrphy_dl_slot_iq",
    "nrphy_dl_slot_read_grid", "nrphy_dl_slot_device_grid", "nrphy_dl_slot_stream", "nrphy_dl_slot_amplitude_stats",
    "nrphy_channel_equalize", "nrphy_channel_equalize_host", "nrphy_pusch_demod_validate", "nrphy_pusch_demod_codeword_bits",
    "nrphy_pusch_demod_plan_create", "nrphy_pusch_demod_plan_destroy", "nrphy_pusch_demod_plan_codeword_bits",
    "nrphy_pusch_demod_run", "nrphy_pusch_demodulate_host",
    "nrphy_pusch_demod_validate_ex", "nrphy_pusch_demod_plan_create_ex", "nrphy_pusch_demodulate_host_ex",
    "nrphy_pusch_demod_run_evm", "nrphy_pusch_demodulate_host_evm",
    "nrphy_transform_precoding_nof_prb_valid", "nrphy_transform_deprecode", "nrphy_transform_deprecode_host",
    "nrphy_pusch_chest_validate", "nrphy_pusch_chest_plan_create", "nrphy_pusch_chest_plan_destroy", "nrphy_pusch_chest_run",
    "nrphy_pusch_chest_host",
    "nrphy_pusch_chest_validate_ex", "nrphy_pusch_chest_plan_create_ex", "nrphy_pusch_chest_host_ex",
    "nrphy_pusch_lowpapr_sequence_host",
    "nrphy_prach_threshold", "nrphy_prach_validate", "nrphy_prach_window_width", "nrphy_prach_plan_create", "nrphy_prach_plan_destroy",
    "nrphy_prach_plan_metric_stride", "nrphy_prach_run", "nrphy_prach_detect_host", "nrphy_prach_generate_host",
    "nrphy_prach_demod_validate", "nrphy_prach_demod_sizes", "nrphy_prach_demod_plan_create", "nrphy_prach_demod_plan_destroy",
    "nrphy_prach_demod_run", "nrphy_prach_demodulate_host",
    "nrphy_pucch_validate", "nrphy_pucch_plan_create", "nrphy_pucch_plan_destroy", "nrphy_pucch_run", "nrphy_pucch_host",
    "nrphy_uci_decoder_validate", "nrphy_uci_decoder_plan_create", "nrphy_uci_decoder_plan_destroy", "nrphy_uci_decoder_run",
    "nrphy_uci_decode_host",
    "nrphy_ulsch_demux_validate", "nrphy_ulsch_demux_sizes", "nrphy_ulsch_demux_plan_create", "nrphy_ulsch_demux_plan_destroy",
    "nrphy_ulsch_demux_run", "nrphy_ulsch_demultiplex_host",
    "nrphy_pf2_validate", "nrphy_pf2_sizes", "nrphy_pf2_plan_create", "nrphy_pf2_plan_destroy", "nrphy_pf2_run", "nrphy_pf2_host",
    "nrphy_srs_validate", "nrphy_srs_info", "nrphy_srs_plan_create", "nrphy_srs_plan_destroy", "nrphy_srs_run", "nrphy_srs_host",
    "nrphy_srs_sequence_host",
    "nrphy_ul_sch_info", "nrphy_pusch_proc_validate", "nrphy_pusch_proc_derive", "nrphy_pusch_proc_harq_bytes",
    "nrphy_pusch_proc_plan_create", "nrphy_pusch_proc_plan_destroy", "nrphy_pusch_proc_plan_harq_bytes", "nrphy_pusch_proc_run",
    "nrphy_pusch_proc_host",
    "nrphy_pusch_evm_validate", "nrphy_pusch_evm_plan_create", "nrphy_pusch_evm_host", "nrphy_pusch_evm_slot",
    "nrphy_pusch_tp_validate", "nrphy_pusch_tp_derive", "nrphy_pusch_tp_harq_bytes", "nrphy_pusch_tp_plan_create",
    "nrphy_pusch_tp_host", "nrphy_pusch_tp_slot",
    "nrphy_pusch_csi2_size", "nrphy_pusch_csi2_validate", "nrphy_pusch_csi2_variants", "nrphy_pusch_csi2_harq_bytes",
    "nrphy_pusch_csi2_plan_create", "nrphy_pusch_csi2_plan_destroy", "nrphy_pusch_csi2_run", "nrphy_pusch_csi2_host",
    "nrphy_ofdm_demod_symbols",
    "nrphy_ul_slots_create", "nrphy_ul_slots_destroy", "nrphy_ul_slots_wait_free", "nrphy_ul_slot_open", "nrphy_ul_slot_close",
    "nrphy_ul_slot_samples", "nrphy_ul_slot_load_grid", "nrphy_ul_slot_device_grid", "nrphy_ul_slot_stream",
    "nrphy_ul_slot_symbols_written", "nrphy_ul_slot_pusch", "nrphy_ul_slot_pf01", "nrphy_ul_slot_pf2", "nrphy_ul_slot_srs",
    "nrphy_ul_slot_finish", "nrphy_ul_slot_poll", "nrphy_ul_slot_wait", "nrphy_ul_slot_read_grid", "nrphy_ul_slot_pusch_results",
    "nrphy_ul_slot_tb", "nrphy_ul_slot_pusch_uci", "nrphy_ul_slot_pf01_results", "nrphy_ul_slot_format2_results",
    "nrphy_ul_slot_sounding_results",
    "nrphy_prach_window_demod_run",
    "nrphy_prach_windows_create", "nrphy_prach_windows_destroy", "nrphy_prach_windows_wait_free", "nrphy_prach_windows_plans_made",
    "nrphy_prach_window_open", "nrphy_prach_window_close", "nrphy_prach_window_samples", "nrphy_prach_window_device_buffer",
    "nrphy_prach_window_stream", "nrphy_prach_window_buffer_written", "nrphy_prach_window_poll", "nrphy_prach_window_wait",
    "nrphy_prach_window_read_buffer", "nrphy_prach_window_results", "nrphy_prach_window_preambles",
]
