"""The PDUs (g)-(j) of the CSI part 2 tests (tests/test_pusch_csi2_host.py, tests/test_pusch_csi2.py): PUSCH PDUs with a CSI part 2
size description, next to (a)-(f) of tests/test_pusch_processor.py, on the same 25 PRB x 4 port grid.

(g) 6 PRB, QPSK, one layer, one port, no HARQ-ACK, 6 bits of CSI part 1; one entry {offset 1, width 2} with the map 0, 1, 2, 7:
    size 0, the 1-bit and 2-bit placeholder paths, a short block.
(h) 12 PRB, 16-QAM, two ports, 4 HARQ-ACK bits, 12 bits of part 1 (polar); entry 0 {0, 1}, {5, 2} with 8 values and entry 1
    {10, 2} with 4: the sums 12, 24, 36, 48, 60 (polar part 2).
(i) 25 PRB, 16-QAM, two layers, four ports, 2 HARQ-ACK bits (a reserved set, puncturing, part 2 on reserved REs), 5 bits of part 1,
    which ends in its first symbol; sizes 40 and 150; two codeblocks.
(j) as (i) with 200 bits of part 1 at a beta offset of 20: part 1 runs past the first symbol that holds reserved REs, so part 2,
    which may take reserved REs, starts in an earlier symbol than part 1 ends in -- where the reference's streaming demultiplexer
    and the up-front placement of TS 38.212 Section 6.2.7 differ.
"""
import numpy as np

import backends
import test_pusch_processor as T
import uci_model

abi = backends.abi
lib = backends.pkg.lib

NPORTS, NSUBC = T.NPORTS, T.NSUBC

DESCS = {
    "g": [([(1, 2)], [0, 1, 2, 7])],
    "h": [([(0, 1), (5, 2)], [12, 12, 12, 24, 24, 24, 36, 36]), ([(10, 2)], [0, 0, 12, 24])],
    "i": [([(0, 1)], [40, 150])],
    "j": [([(0, 1)], [40, 150])],
}
SIZES = {"g": [0, 1, 2, 7], "h": [0, 12, 24, 36, 48, 60], "i": [0, 40, 150], "j": [0, 40, 150]}  # the variant tables
SELECTABLE = {"g": [0, 1, 2, 7], "h": [12, 24, 36, 48, 60], "i": [40, 150], "j": [40, 150]}  # the sizes some part 1 payload gives


def pdu_args():
    """(g)-(j): name -> keyword arguments of abi.make_pusch_pdu."""
    common = dict(alpha_scaling=0.8, beta_offset_harq_ack=10.0, beta_offset_csi_part1=6.25, beta_offset_csi_part2=6.25, rnti=0x4601,
                  tbs_lbrm_bytes=3168, dmrs_symbols=(2, 11))
    shapes = {
        "g": dict(prbs=range(0, 6), modulation=2, target_code_rate=449.0, nof_layers=1, rx_ports=(2,), nof_csi_part1=6),
        "h": dict(prbs=range(3, 15), modulation=4, target_code_rate=616.0, nof_layers=1, rx_ports=(1, 3), nof_harq_ack=4,
                  nof_csi_part1=12),
        "i": dict(prbs=range(0, 25), modulation=4, target_code_rate=616.0, nof_layers=2, rx_ports=(3, 2, 1, 0), nof_harq_ack=2,
                  nof_csi_part1=5),
        "j": dict(prbs=range(0, 25), modulation=4, target_code_rate=616.0, nof_layers=2, rx_ports=(3, 2, 1, 0), nof_harq_ack=2,
                  nof_csi_part1=200, beta_offset_csi_part1=20.0),
    }
    out = {}
    for i, (name, s) in enumerate(shapes.items()):
        a = dict(common, slot_index=2 + i, n_id=21 + i, scrambling_id=200 + i, n_scid=i % 2, nof_csi_part2_entries=len(DESCS[name]))
        a.update(s)
        tb_bits = lib.tbs_calculate(14, 12 * len(a["dmrs_symbols"]), 18, a["modulation"], a["target_code_rate"], a["nof_layers"],
                                    len(a["prbs"]))
        a.update(tb_size_bytes=tb_bits // 8, ldpc_base_graph=T.base_graph(tb_bits, a["target_code_rate"]))
        out[name] = a
    return out


def all_args():
    """(a)-(j)."""
    return dict(T.pdu_args(), **pdu_args())


def desc_of(name):
    return abi.make_pusch_csi2_desc(DESCS.get(name, ()))


def make(names, **override):
    """([abi.PuschPdu], [abi.PuschCsi2Desc]) of the names, from (a)-(j)."""
    args = all_args()
    return [abi.make_pusch_pdu(**dict(args[n], **override)) for n in names], [desc_of(n) for n in names]


def size_restated(entries, bits):
    """uci_part2_get_size in NumPy, as the reference writes it: per parameter the slice read into a word with its first bit lowest
    (bounded_bitset::to_uint64), the word's 64 bits reversed and shifted down by 64 - width."""
    total = 0
    for parameters, sizes in entries:
        index = 0
        for offset, width in parameters:
            word = sum(int(b) << j for j, b in enumerate(bits[offset:offset + width]))
            value = int(format(word, "064b")[::-1], 2) >> (64 - width) if width else 0
            index = (index << width) | value
        total += sizes[index]
    return total


def part1_for(name, size, rng):
    """A CSI part 1 payload of the PDU for which the description gives `size`."""
    n = all_args()[name]["nof_csi_part1"]
    for _ in range(10000):
        bits = rng.integers(0, 2, n, dtype=np.uint8)
        if size_restated(DESCS[name], bits) == size:
            return bits
    raise AssertionError((name, size))


def demux_dict(cfg):
    return {f[0]: int(getattr(cfg, f[0])) for f in abi.UlschDemuxCfg._fields_}


def demux_with_part2(base_demux, size, info):
    """The demultiplexer configuration of a variant: the PDU's without part 2, with the size and G^CSI-2."""
    d = demux_dict(base_demux)
    d.update(nof_csi_part2_bits=size, nof_enc_csi_part2_bits=info.nof_csi_part2_bits)
    return d


def part2_starts_before_part1_ends(demux):
    """The condition under which the reference's streaming demultiplexer and the up-front placement differ: a part 2 RE in a symbol
    before the one that holds the last part 1 RE."""
    symbols = list(uci_model.ulsch_symbols(demux))
    last_csi1 = max([l for l, s in enumerate(symbols) if s[2].any()], default=-1)
    first_csi2 = min([l for l, s in enumerate(symbols) if s[3].any()], default=99)
    return first_csi2 < last_csi1
