"""GPU tests of the two forms in which a plan hands its distinct scrambling sequences from the prologue to the codeblock waves:
whole words c = x1 ^ x2, which the waves of every PDU that shares the sequence read from global memory, or a 31-word seed per
work item, which each wave expands in LDS.  Every case runs under NRPHY_SCR_WORDS=1 and =0; every grid (uint16 view) and
every codeword tap is compared bit for bit with the CPU oracle's pdsch_process, and the two forms with each other.  The shapes
are the smallest that have the property a case is about; the property is asserted from nrphy_pdsch_derive, not assumed.
"""
import numpy as np
import pytest

import backends
import cases
from pusch_chest_model import dev

abi = backends.abi
lib = backends.pkg.lib
pytestmark = pytest.mark.gpu

RE_CHUNK = 512       # resource elements per work item (csrc/nrphy_internal.h)
SCR_PARTS = 4        # workgroups a long sequence is split over; a part has at least 2048 words
BUDGET_BYTES = 4 << 20
NOF_PORTS = 4
FORMS = (("1", "words"), ("0", "seeds"))


def pdu_of(qm, codebook, n_prb, rate, *, bwp=52, base_graph=1, **kw):
    w = cases.codebook(codebook)
    layers = w.shape[2]
    args = dict(slot_index=0, rnti=5, n_id=3, bwp_start_rb=0, bwp_size_rb=bwp, qm=qm, dmrs_symbols=(2, 7, 11),
                nof_cdm_groups_without_data=2, prb_start=1, prb_count=n_prb, start_symbol=0, nof_symbols=12,
                base_graph=base_graph, precoding=w, tb_size_bytes=cases.tbs(12, 36, qm, rate, layers, n_prb) // 8)
    args.update(kw)
    return abi.make_pdu(**args)


def work_items(pdu):
    """(first codeword bit, resource elements) of every work item, in the plan's order, and the derived sizes."""
    d = lib.derive(pdu)
    lq = pdu.qm * pdu.nof_layers
    items, bit_cb = [], 0
    for cb in range(d["nof_codeblocks"]):
        e = d["rm_length_short"] if cb < d["nof_short_segments"] else d["rm_length_long"]
        for begin in range(0, e // lq, RE_CHUNK):
            items.append((bit_cb + begin * lq, min(RE_CHUNK, e // lq - begin)))
        bit_cb += e
    assert bit_cb == d["codeword_bits"]
    return items, d


def scr_words(pdu):
    """PduDev::scr_words: ceil(G / 32), the word a misaligned read runs into, and a seed's length."""
    return (lib.derive(pdu)["codeword_bits"] + 31) // 32 + 1 + 31


def reference(oracle, pdus, tbs, nof_subc):
    out = []
    for pdu, tb in zip(pdus, tbs):
        d = oracle.derive(pdu)
        out.append(oracle.pdsch_process(pdu, tb, NOF_PORTS, nof_subc, taps=True, codeword_bits=d["codeword_bits"]))
    return out


def run_form(ctx, pdus, tbs, want, nof_subc, form, taps=True):
    """Runs the PDUs, each on a grid of its own, on `ctx`; asserts the plan's form and compares with the oracle's `want`.
    Returns the grids as uint16."""
    import torch
    n = len(pdus)
    offs, pos = [], 0
    for tb in tbs:
        offs.append(pos)
        pos += (len(tb) + 15) & ~15
    buf = np.zeros(pos + 16, np.uint8)
    for o, tb in zip(offs, tbs):
        buf[o:o + len(tb)] = tb
    plan = lib.PdschPlan(ctx, pdus, offs, list(range(n)), n, NOF_PORTS, nof_subc)
    try:
        assert plan.scrambling_form == form
        d_grid = torch.full((n, NOF_PORTS, 14, nof_subc), 0x7FFF7FFF, dtype=torch.int32, device="cuda")
        d_rm = torch.zeros(plan.codeword_bits // 8, dtype=torch.uint8, device="cuda") if taps else None
        d_scr = torch.zeros(plan.codeword_bits // 8, dtype=torch.uint8, device="cuda") if taps else None
        torch.cuda.synchronize()
        plan.run(dev(buf), d_grid, d_cw_rm=d_rm, d_cw_scr=d_scr, zero_grids=True)
        ctx.synchronize()
        got = d_grid.cpu().numpy().view(np.uint16).reshape(n, NOF_PORTS, 14, nof_subc, 2)
        for i, (grid, orm, oscr) in enumerate(want):
            assert np.array_equal(got[i], grid), "%s form: grid of PDU %d" % (form, i)
            if taps:
                o = plan.codeword_offset(i) // 8
                assert np.array_equal(d_rm.cpu().numpy()[o:o + len(orm)], orm), "%s form: rate-matched codeword of PDU %d" % (form, i)
                assert np.array_equal(d_scr.cpu().numpy()[o:o + len(oscr)], oscr), "%s form: scrambled codeword of PDU %d" % (form, i)
        return got, plan.nof_sequences
    finally:
        plan.close()


def both_forms(gpu_ctx_for, oracle, pdus, tbs, nof_sequences=None):
    nof_subc = pdus[0].bwp_size_rb * 12
    want = reference(oracle, pdus, tbs, nof_subc)
    grids = []
    for knob, form in FORMS:
        got, nseq = run_form(gpu_ctx_for({"NRPHY_SCR_WORDS": knob}), pdus, tbs, want, nof_subc, form)
        if nof_sequences is not None:
            assert nseq == nof_sequences
        grids.append(got)
    assert np.array_equal(grids[0], grids[1]), "words form against seeds form"


def smallest(make, holds, candidates):
    n = next(n for n in candidates if holds(make(n)))
    return make(n)


def test_shared_words_aligned_short_and_long_codeblocks(gpu_ctx_for, oracle):
    """Two slots of one UE (the same c_init, other transport blocks, DM-RS of their own) on 4 layers of 256-QAM: Qm L = 32, one
    scrambling word per resource element.  At least three codeblocks, short and long ones of different lengths, every chunk
    on a word boundary: the aligned path, one dword at word0 + r."""
    def holds(pdu):
        items, d = work_items(pdu)
        return (d["nof_codeblocks"] >= 3 and 0 < d["nof_short_segments"] < d["nof_codeblocks"] and
                d["rm_length_short"] != d["rm_length_long"] and all(bit0 % 32 == 0 for bit0, _ in items))
    make = lambda n, **kw: pdu_of(8, "four_layer_four_ports_0_0", n, 948, **kw)
    a = smallest(make, holds, range(1, 50))
    n_prb = sum(bin(w).count("1") for w in a.prb_mask)
    pdus = [a, make(n_prb, slot_index=1)]
    rng = np.random.default_rng(61)
    both_forms(gpu_ctx_for, oracle, pdus, [cases.random_tb(rng, p) for p in pdus], nof_sequences=(1, 2))


@pytest.mark.parametrize("qm,codebook,rate,base_graph", [(6, "three_layer_four_ports_1_0", 873, 1), (2, "single_port", 616, 2)])
def test_shared_words_chunks_inside_a_word(gpu_ctx_for, oracle, qm, codebook, rate, base_graph):
    """The same on 3 layers of 64-QAM and on 1 layer of QPSK (Qm L = 18 and 2): codeblocks start inside a word, so the bits of
    a resource element come from two neighbouring global words.  With QPSK the last resource element does not reach the
    codeword's last word boundary: its two-word read runs past the codeword's last word and must stay inside the sequence."""
    def holds(pdu):
        items, d = work_items(pdu)
        return d["nof_codeblocks"] >= 2 and any(bit0 % 32 != 0 for bit0, _ in items)
    make = lambda n, **kw: pdu_of(qm, codebook, n, rate, base_graph=base_graph, **kw)
    a = smallest(make, holds, range(1, 50))
    n_prb = sum(bin(w).count("1") for w in a.prb_mask)
    pdus = [a, make(n_prb, slot_index=1)]
    if qm == 2:
        g, lq = lib.derive(a)["codeword_bits"], 2
        assert (g - lq) // 32 + 1 > (g - 1) // 32 and (g - lq) // 32 + 1 < scr_words(a)
    rng = np.random.default_rng(62)
    both_forms(gpu_ctx_for, oracle, pdus, [cases.random_tb(rng, p) for p in pdus], nof_sequences=(1, 2))


def test_words_several_items_per_codeblock_last_one_short(gpu_ctx_for, oracle):
    """One PDU, QPSK on one layer at a low rate: a codeblock takes more than RE_CHUNK resource elements, so it has several work
    items, the last of them short."""
    def holds(pdu):
        items, d = work_items(pdu)
        nre = d["rm_length_long"] // 2
        return nre > 2 * RE_CHUNK and nre % RE_CHUNK != 0
    a = smallest(lambda n: pdu_of(2, "single_port", n, 120, bwp=106, base_graph=2), holds, range(20, 100))
    rng = np.random.default_rng(63)
    both_forms(gpu_ctx_for, oracle, [a], [cases.random_tb(rng, a)])


def test_words_sequence_split_into_all_parts(gpu_ctx_for, oracle):
    """A sequence long enough for the prologue to walk it in SCR_PARTS parts (a part per 2048 words): the parts between them
    write every word once, the words at the part boundaries included."""
    make = lambda n: pdu_of(8, "four_layer_four_ports_0_0", n, 948, bwp=106)
    a = smallest(make, lambda pdu: scr_words(pdu) >> 11 >= SCR_PARTS, range(1, 105))
    rng = np.random.default_rng(64)
    both_forms(gpu_ctx_for, oracle, [a], [cases.random_tb(rng, a)])


def test_budget_rule_chooses_the_form(gpu_ctx_for, oracle, monkeypatch):
    """With NRPHY_SCR_WORDS unset the plan stores words while its distinct sequences take at most 4 MiB, else seeds.  36 headline
    PDUs of 36 UEs are just over (36 x 29,193 words), the first 35 of them just under; both plans equal the oracle."""
    base, _, nof_subc, _ = cases.baseline_config(3)
    per_pdu = scr_words(base) * 4
    n_over = BUDGET_BYTES // per_pdu + 1
    assert (n_over - 1) * per_pdu <= BUDGET_BYTES < n_over * per_pdu
    pdus = [cases.baseline_config(3, rnti=1 + i)[0] for i in range(n_over)]
    rng = np.random.default_rng(65)
    tbs = [cases.random_tb(rng, p) for p in pdus]
    want = reference(oracle, pdus, tbs, nof_subc)
    monkeypatch.delenv("NRPHY_SCR_WORDS", raising=False)
    ctx = gpu_ctx_for({})
    _, nseq = run_form(ctx, pdus, tbs, want, nof_subc, "seeds", taps=False)
    assert nseq[0] == n_over
    _, nseq = run_form(ctx, pdus[:-1], tbs[:-1], want[:-1], nof_subc, "words", taps=False)
    assert nseq[0] == n_over - 1
