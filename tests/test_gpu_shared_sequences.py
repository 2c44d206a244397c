"""GPU tests of the prologue's shared sequences: a plan generates every distinct scrambling sequence and every distinct set of
DM-RS sequences once per run, and the PDUs that ask for the same ones read the same seeds and DM-RS words.  Every grid and
codeword is compared bit for bit with the CPU oracle's pdsch_process, as tests/test_gpu_parity.py does.
"""
import numpy as np
import pytest

import backends
import cases
from pusch_chest_model import dev

abi = backends.abi
lib = backends.pkg.lib
pytestmark = pytest.mark.gpu

RE_CHUNK = 512      # resource elements per work item (csrc/nrphy_internal.h)
BWP_RB = 52
PRB_START = 3
RE_PER_PRB = 9 * 12  # 12 symbols, three of them DM-RS symbols with both CDM groups reserved


def small_pdu(n_prb, **kw):
    """16-QAM on four layers at R = 658/1024: 10.3 information bits per resource element, so that a codeblock of up to 8448
    bits takes more than RE_CHUNK resource elements."""
    w = cases.codebook("four_layer_four_ports_0_0")
    tb_bits = cases.tbs(12, 36, 4, 658, 4, n_prb)
    args = dict(slot_index=0, rnti=5, n_id=3, bwp_start_rb=0, bwp_size_rb=BWP_RB, qm=4, dmrs_symbols=(2, 7, 11),
                nof_cdm_groups_without_data=2, prb_start=PRB_START, prb_count=n_prb, start_symbol=0, nof_symbols=12,
                base_graph=1, precoding=w, tb_size_bytes=tb_bits // 8)
    args.update(kw)
    return abi.make_pdu(**args)


def several_items(pdu):
    d = lib.derive(pdu)
    return d["nof_codeblocks"] >= 2 and d["rm_length_long"] // (pdu.qm * pdu.nof_layers) > RE_CHUNK


@pytest.fixture(scope="module")
def smallest_prb_count():
    """The smallest allocation of small_pdu's kind whose transport block segments into at least two codeblocks and whose long
    codeblock exceeds RE_CHUNK resource elements: a PDU then has several work items and a codeblock two."""
    n = next(n for n in range(1, BWP_RB - 2) if several_items(small_pdu(n)))
    assert n * RE_PER_PRB > 2 * RE_CHUNK and not several_items(small_pdu(n - 1))
    return n


def run_plan(ctx, oracle, pdus, tbs, *, grids=True, taps=False, plan=None):
    """Runs the PDUs, each on a grid of its own, and compares every output with the oracle's.  Returns the plan."""
    import torch
    nof_ports, nof_subc, n = 4, pdus[0].bwp_size_rb * 12, len(pdus)
    offs, pos = [], 0
    for tb in tbs:
        offs.append(pos)
        pos += (len(tb) + 15) & ~15
    buf = np.zeros(pos + 16, np.uint8)
    for o, tb in zip(offs, tbs):
        buf[o:o + len(tb)] = tb
    if plan is None:
        plan = lib.PdschPlan(ctx, pdus, offs, list(range(n)), n, nof_ports, nof_subc)
    d_grid = torch.full((n, nof_ports, 14, nof_subc), 0x7FFF7FFF, dtype=torch.int32, device="cuda") if grids else None
    d_rm = torch.zeros(plan.codeword_bits // 8, dtype=torch.uint8, device="cuda") if taps else None
    d_scr = torch.zeros(plan.codeword_bits // 8, dtype=torch.uint8, device="cuda") if taps else None
    torch.cuda.synchronize()
    plan.run(dev(buf), d_grid, d_cw_rm=d_rm, d_cw_scr=d_scr, zero_grids=True)
    ctx.synchronize()
    for i, (pdu, tb) in enumerate(zip(pdus, tbs)):
        d = oracle.derive(pdu)
        want, orm, oscr = oracle.pdsch_process(pdu, tb, nof_ports, nof_subc, taps=True, codeword_bits=d["codeword_bits"])
        if grids:
            got = d_grid[i].cpu().numpy().view(np.uint16).reshape(nof_ports, 14, nof_subc, 2)
            assert np.array_equal(got, want), "grid of PDU %d" % i
        if taps:
            o = plan.codeword_offset(i) // 8
            assert np.array_equal(d_rm.cpu().numpy()[o:o + len(orm)], orm), "rate-matched codeword of PDU %d" % i
            assert np.array_equal(d_scr.cpu().numpy()[o:o + len(oscr)], oscr), "scrambled codeword of PDU %d" % i
    return plan


def test_shared_sequences_five_pdus(gpu_ctx, oracle, smallest_prb_count):
    """One plan, five PDUs on five grids:
        A        rnti 5, slot 0
        A again  unchanged: shares both sequences with the first
        A'       A in slot 3: the same scrambling sequence, DM-RS of its own (a workgroup with DM-RS work only)
        B        rnti 6 with a DM-RS scrambling identity of its own: shares nothing
        C        rnti 5 on one more PRB: the same c_init, another codeword layout, and DM-RS sequences a word longer (they run
                 from subcarrier 0 to the last PRB: 12 x 13 -> 12 x 14 bits, 5 -> 6 whole words): shares nothing
    Scrambling keys (c_init, layout): {A, A, A'}, {B}, {C} = 3; DM-RS keys (symbols' c_init, length): {A, A}, {A'}, {B}, {C} = 4.
    Every grid equals the oracle's, in a first run and in a second one with other transport blocks."""
    n = smallest_prb_count
    a = small_pdu(n)
    pdus = [a, small_pdu(n), small_pdu(n, slot_index=3), small_pdu(n, rnti=6, scrambling_id=7), small_pdu(n + 1)]
    d = lib.derive(a)
    assert d["nof_codeblocks"] >= 2 and d["rm_length_long"] // 16 > RE_CHUNK
    assert (12 * (PRB_START + n) + 31) // 32 != (12 * (PRB_START + n + 1) + 31) // 32, "C's DM-RS sequences must differ in length"
    rng = np.random.default_rng(51)
    plan = run_plan(gpu_ctx, oracle, pdus, [cases.random_tb(rng, p) for p in pdus])
    assert plan.nof_sequences == (3, 4)
    run_plan(gpu_ctx, oracle, pdus, [cases.random_tb(rng, p) for p in pdus], plan=plan)
    plan.close()


def test_shared_sequence_split_into_parts(gpu_ctx, oracle):
    """Two identical PDUs whose codeword has at least 8192 words: the one sequence they share is walked in four parts."""
    w = cases.codebook("four_layer_four_ports_0_0")
    n_prb = 80
    mk = lambda: abi.make_pdu(slot_index=4, rnti=9, n_id=1, bwp_start_rb=0, bwp_size_rb=106, qm=8, dmrs_symbols=(2, 7, 11),
                              nof_cdm_groups_without_data=2, prb_start=3, prb_count=n_prb, start_symbol=0, nof_symbols=12,
                              base_graph=1, precoding=w, tb_size_bytes=cases.tbs(12, 36, 8, 948, 4, n_prb) // 8)
    pdus = [mk(), mk()]
    assert lib.derive(pdus[0])["codeword_bits"] >= 8192 * 32
    rng = np.random.default_rng(52)
    plan = run_plan(gpu_ctx, oracle, pdus, [cases.random_tb(rng, p) for p in pdus])
    assert plan.nof_sequences == (1, 1)
    plan.close()


def test_shared_sequences_codeword_taps(gpu_ctx, oracle, smallest_prb_count):
    """Encode only (no grid) with the codeword taps: two PDUs that share their sequences, other transport blocks -- the
    rate-matched and the scrambled codeword of both equal the oracle's."""
    pdus = [small_pdu(smallest_prb_count), small_pdu(smallest_prb_count)]
    rng = np.random.default_rng(53)
    plan = run_plan(gpu_ctx, oracle, pdus, [cases.random_tb(rng, p) for p in pdus], grids=False, taps=True)
    assert plan.nof_sequences == (1, 1)
    plan.close()
