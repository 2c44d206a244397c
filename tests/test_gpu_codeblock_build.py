"""GPU tests of the first stage of a codeblock wave (build_codeblock in csrc/codeblock_build_device.h): segmentation of the transport
block -- the word-aligned path and the one for any bit offset -- and the table-free codeblock CRC (csrc/crc24b_fold.h).  Every
case runs with the scrambling sequences as words and as seeds (two kernels that share the stage); every grid (uint16 view) and
every codeword tap is compared bit for bit with the CPU oracle's pdsch_process, and the two forms with each other.  A small CPU
search (nrphy_pdsch_derive, no device) picks the smallest allocation with the property a case is about, and the case asserts
that property on the PDU it runs, so it cannot silently take the other path.
"""
import numpy as np
import pytest

import backends
import cases
import test_gpu_scrambling_words as sw

lib = backends.pkg.lib
pytestmark = pytest.mark.gpu

FOUR_LAYERS, THREE_LAYERS, ONE_LAYER = "four_layer_four_ports_0_0", "three_layer_four_ports_1_0", "single_port"


def nof_prb(pdu):
    return sum(bin(w).count("1") for w in pdu.prb_mask)


def both_forms(gpu_ctx_for, oracle, pdus, seed, env=None):
    """The PDUs, each on a grid of its own, in both forms of the scrambling sequences against the oracle and each other."""
    tbs = [cases.random_tb(np.random.default_rng(seed + i), p) for i, p in enumerate(pdus)]
    nof_subc = pdus[0].bwp_size_rb * 12
    want = sw.reference(oracle, pdus, tbs, nof_subc)
    grids = []
    for knob, form in sw.FORMS:
        ctx = gpu_ctx_for(dict(env or {}, NRPHY_SCR_WORDS=knob))
        grids.append(sw.run_form(ctx, pdus, tbs, want, nof_subc, form)[0])
    assert np.array_equal(grids[0], grids[1]), "words form against seeds form"


def first_bits(d):
    """Bit offset of every codeblock in the transport block."""
    return [cb * d["cb_info_bits"] for cb in range(d["nof_codeblocks"])]


def test_aligned_codeblocks_with_codeblock_crc(gpu_ctx_for, oracle):
    """info_bits a multiple of 32 and at least two codeblocks: every codeblock starts on a word boundary (the fast path), the
    codeblock CRC runs over whole words (pad = 0) and the last codeblock's boundary word carries the start of the TB CRC."""
    def holds(pdu):
        d = lib.derive(pdu)
        return d["nof_codeblocks"] >= 2 and d["cb_info_bits"] % 32 == 0
    a = sw.smallest(lambda n: sw.pdu_of(8, FOUR_LAYERS, n, 948), holds, range(1, 52))
    d = lib.derive(a)
    assert d["nof_codeblocks"] >= 2 and d["nof_cb_crc_bits"] == 24 and all(b % 32 == 0 for b in first_bits(d))
    assert (d["cb_info_bits"] - d["nof_tb_crc_bits"] - d["zero_pad"]) % 32 != 0  # a masked boundary word in the last codeblock
    both_forms(gpu_ctx_for, oracle, [a, sw.pdu_of(8, FOUR_LAYERS, nof_prb(a), 948, slot_index=1)], 71)


def test_codeblocks_that_start_inside_a_word(gpu_ctx_for, oracle):
    """info_bits no multiple of 32 and at least three codeblocks: the first takes the aligned path with a masked last word,
    most of the others start inside a word (the path for any offset), and the codeblock CRC's message is right-aligned (pad != 0)."""
    def holds(pdu):
        d = lib.derive(pdu)
        return d["nof_codeblocks"] >= 3 and sum(b % 32 != 0 for b in first_bits(d)) * 2 > d["nof_codeblocks"]
    a = sw.smallest(lambda n: sw.pdu_of(6, THREE_LAYERS, n, 873), holds, range(1, 52))
    d = lib.derive(a)
    assert d["nof_cb_crc_bits"] == 24 and d["cb_info_bits"] % 32 != 0
    assert sum(b % 32 != 0 for b in first_bits(d)) * 2 > d["nof_codeblocks"] >= 3
    both_forms(gpu_ctx_for, oracle, [a, sw.pdu_of(6, THREE_LAYERS, nof_prb(a), 873, slot_index=1)], 72)


@pytest.mark.parametrize("tb_crc_bits", [16, 24])
def test_one_codeblock_carries_the_transport_block_crc(gpu_ctx_for, oracle, tb_crc_bits):
    """One codeblock: no codeblock CRC; the aligned path's boundary word takes the TB CRC of 16 bits (a transport block of at
    most 3824 bits) or of 24 bits, which starts inside that word.  (The standard's sizes above 3824 bits are multiples of 64
    bits: the transport block is one byte shorter than the allocation's standard size.)"""
    def holds(pdu):
        d = lib.derive(pdu)
        return (lib.validate(pdu) == backends.abi.OK and d["nof_codeblocks"] == 1 and d["nof_tb_crc_bits"] == tb_crc_bits and
                (pdu.tb_size_bytes * 8) % 32 != 0)
    def make(n):
        size = sw.pdu_of(2, ONE_LAYER, n, 616, bwp=106).tb_size_bytes
        return sw.pdu_of(2, ONE_LAYER, n, 616, bwp=106, tb_size_bytes=size - 1)
    a = sw.smallest(make, holds, range(2, 105))
    d = lib.derive(a)
    assert d["nof_codeblocks"] == 1 and d["nof_cb_crc_bits"] == 0 and d["nof_tb_crc_bits"] == tb_crc_bits
    assert (a.tb_size_bytes * 8) % 32 != 0
    both_forms(gpu_ctx_for, oracle, [a], 73 + tb_crc_bits)


def test_last_codeblock_with_zero_padding(gpu_ctx_for, oracle):
    """A transport block whose size with its CRCs does not divide by the number of codeblocks: the last codeblock ends with zero
    padding behind the TB CRC.  (The standard's transport block sizes never need it; the segmenter, like the reference's, takes
    any size.)  The size is the largest below the standard's for the allocation that pads."""
    n = 6
    top = sw.pdu_of(8, FOUR_LAYERS, n, 948).tb_size_bytes
    def holds(pdu):
        d = lib.derive(pdu)
        return lib.validate(pdu) == backends.abi.OK and d["nof_codeblocks"] >= 3 and d["zero_pad"] > 0
    a = sw.smallest(lambda size: sw.pdu_of(8, FOUR_LAYERS, n, 948, tb_size_bytes=size), holds, range(top, top - 64, -1))
    d = lib.derive(a)
    assert d["zero_pad"] > 0 and d["nof_codeblocks"] >= 3
    assert d["nof_codeblocks"] * d["cb_info_bits"] == a.tb_size_bytes * 8 + d["nof_tb_crc_bits"] + d["zero_pad"]
    both_forms(gpu_ctx_for, oracle, [a], 75)


def test_base_graph_2_with_filler_bits(gpu_ctx_for, oracle):
    """Base graph 2, several codeblocks with a codeblock CRC, filler bits behind it: the words behind the CRC stay zero up to
    the parity region whatever the lifting size."""
    def holds(pdu):
        d = lib.derive(pdu)
        return d["nof_codeblocks"] >= 2 and d["nof_filler_bits"] > 0
    a = sw.smallest(lambda n: sw.pdu_of(2, ONE_LAYER, n, 616, bwp=106, base_graph=2), holds, range(1, 105))
    d = lib.derive(a)
    assert a.ldpc_base_graph == 2 and d["nof_codeblocks"] >= 2 and d["nof_filler_bits"] > 0 and d["nof_cb_crc_bits"] == 24
    both_forms(gpu_ctx_for, oracle, [a], 76)


def test_mixed_modulation_plan_runs_the_same_front_end(gpu_ctx_for, oracle):
    """Two PDUs of different modulations in one plan, dispatched to the one-launch codeblock_kernel (NRPHY_CB_DISPATCH=1), which
    shares build_codeblock with the per-bucket kernels: an aligned PDU with codeblock CRCs and one whose codeblocks start inside
    words."""
    aligned = sw.smallest(lambda n: sw.pdu_of(8, FOUR_LAYERS, n, 948),
                          lambda pdu: lib.derive(pdu)["nof_codeblocks"] >= 2 and lib.derive(pdu)["cb_info_bits"] % 32 == 0, range(1, 52))
    inside = sw.smallest(lambda n: sw.pdu_of(6, THREE_LAYERS, n, 873, rnti=6),
                         lambda pdu: lib.derive(pdu)["nof_codeblocks"] >= 2 and lib.derive(pdu)["cb_info_bits"] % 32 != 0, range(1, 52))
    assert aligned.qm != inside.qm
    da, di = lib.derive(aligned), lib.derive(inside)
    assert da["nof_codeblocks"] >= 2 and da["cb_info_bits"] % 32 == 0 and di["nof_codeblocks"] >= 2 and di["cb_info_bits"] % 32 != 0
    both_forms(gpu_ctx_for, oracle, [aligned, inside], 77, env={"NRPHY_CB_DISPATCH": "1"})
