"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs, against the
golden vectors generated from the compiled reference, and -- at BASELINE sizes -- through size-independent properties.

Bit-exact for everything integer (codewords, scrambled bits) and for the bf16 grid; 1e-5 relative for the fp32 IQ.
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import backends
import cases
from pusch_chest_model import dev

abi = backends.abi
lib = backends.pkg.lib
pytestmark = pytest.mark.gpu

LIFTING_SIZES = cases.LIFTING_SIZES


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------------------------------
# LDPC encoder: all 102 lifted graphs, several output lengths (mirrors ldpc_enc_dec_test.cpp LDPCEncTest)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg", [1, 2])
def test_ldpc_encoder_all_graphs_vs_oracle(gpu_ctx, oracle, bg):
    import torch
    rng = np.random.default_rng(100 + bg)
    kb, nshort = (22, 66) if bg == 1 else (10, 50)
    for zc in LIFTING_SIZES:
        n_cb = 3
        kbytes = (kb * zc + 7) // 8
        msgs = np.zeros((n_cb, kbytes + 3), np.uint8)
        for i in range(n_cb):
            msgs[i, :kbytes] = np.packbits(rng.integers(0, 2, kb * zc, dtype=np.uint8))
        d_msg = dev(msgs)
        full = nshort * zc
        for out_bits in sorted({full, (kb + 2) * zc, full - 3 * zc - 1, kb * zc + 2 * zc + 5}):
            stride = (out_bits + 7) // 8 + 5
            d_out = torch.zeros((n_cb, stride), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            gpu_ctx.ldpc_encode(bg, zc, d_msg, msgs.shape[1], out_bits, d_out, stride, n_cb)
            gpu_ctx.synchronize()
            out = d_out.cpu().numpy()
            for i in range(n_cb):
                want = oracle.ldpc_encode(bg, zc, msgs[i, :kbytes], out_bits)
                assert np.array_equal(out[i, : len(want)], want), (bg, zc, out_bits, i)
                assert not out[i, len(want):].any()


def test_ldpc_encoder_vs_reference_golden(gpu_ctx):
    import torch
    g = np.load(os.path.join(cases.GOLDEN, "ldpc_encoder.npz"))
    for bg, zc in g["keys"]:
        msg = g["msg_%d_%d" % (bg, zc)]
        want = g["out_%d_%d" % (bg, zc)]
        out_bits = (66 if bg == 1 else 50) * int(zc)
        d_msg = dev(np.concatenate([msg, np.zeros(4, np.uint8)]))
        d_out = torch.zeros(len(want) + 4, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.ldpc_encode(int(bg), int(zc), d_msg, len(msg) + 4, out_bits, d_out, len(want) + 4, 1)
        gpu_ctx.synchronize()
        assert np.array_equal(d_out.cpu().numpy()[: len(want)], want), (bg, zc)


def test_ldpc_encoder_linearity_full_size(gpu_ctx):
    """Size-independent property at the maximum size: the code is linear, encode(a ^ b) == encode(a) ^ encode(b)."""
    import torch
    rng = np.random.default_rng(7)
    n_cb, kbytes, out_bits = 512, 8448 // 8, 66 * 384
    a = rng.integers(0, 256, (n_cb, kbytes), dtype=np.uint8)
    b = rng.integers(0, 256, (n_cb, kbytes), dtype=np.uint8)
    outs = []
    for m in (a, b, a ^ b):
        d_out = torch.zeros((n_cb, out_bits // 8), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.ldpc_encode(1, 384, dev(m), kbytes, out_bits, d_out, out_bits // 8, n_cb)
        gpu_ctx.synchronize()
        outs.append(d_out.cpu().numpy())
    assert np.array_equal(outs[0] ^ outs[1], outs[2])
    assert np.array_equal(outs[0][:, : (20 * 384) // 8], a[:, (2 * 384) // 8: (22 * 384) // 8])  # systematic part


# ---------------------------------------------------------------------------------------------------------------------
# PDSCH processor
# ---------------------------------------------------------------------------------------------------------------------
def run_single(gpu_ctx, oracle, pdu, tb, nof_ports, nof_subc):
    d = oracle.derive(pdu)
    assert lib.derive(pdu) == d
    grid, rm, scr = gpu_ctx.pdsch_process_host(pdu, tb, nof_ports, nof_subc, taps=True)
    ogrid, orm, oscr = oracle.pdsch_process(pdu, tb, nof_ports, nof_subc, taps=True, codeword_bits=d["codeword_bits"])
    assert np.array_equal(rm, orm), "rate-matched codeword differs"
    assert np.array_equal(scr, oscr), "scrambled codeword differs"
    bad = np.argwhere(grid != ogrid)
    assert bad.size == 0, "grid differs at %s ..." % bad[:4].tolist()
    return grid, rm


@pytest.mark.parametrize("cfg", [1, 2, 3])
def test_pdsch_baseline_configs_vs_oracle_and_golden(gpu_ctx, oracle, cfg):
    pdu, nof_ports, nof_subc, _ = cases.baseline_config(cfg)
    name = "cfg%d" % cfg
    g = np.load(os.path.join(cases.GOLDEN, "pdsch_processor.npz"))
    tb = np.random.default_rng(int(g[name + "_tb_seed"])).integers(0, 256, pdu.tb_size_bytes, dtype=np.uint8)
    grid, rm = run_single(gpu_ctx, oracle, pdu, tb, nof_ports, nof_subc)
    # Reference-generated golden: codeword and grid hashes.
    assert sha(rm) == str(g[name + "_cw_sha"])
    assert sha(grid) == str(g[name + "_grid_sha"])


def test_pdsch_unit_test_like_pdus(gpu_ctx, oracle):
    g = np.load(os.path.join(cases.GOLDEN, "pdsch_processor.npz"))
    for i, pdu in enumerate(cases.unit_test_like_pdus(np.random.default_rng(2024))):
        name = "unit%02d" % i
        assert lib.validate(pdu) == 0
        tb = np.random.default_rng(int(g[name + "_tb_seed"])).integers(0, 256, pdu.tb_size_bytes, dtype=np.uint8)
        grid, rm = run_single(gpu_ctx, oracle, pdu, tb, 4, 26 * 12)
        assert sha(rm) == str(g[name + "_cw_sha"]), name
        assert sha(grid) == str(g[name + "_grid_sha"]), name


def test_pdsch_diagonal_precoding_variants(gpu_ctx, oracle):
    """Weight matrices full of exact zeros: the layer sum then adds signed zeros, whose sign survives into the bf16 grid
    when a port's sum is zero; the grid must stay bit-exact."""
    rng = np.random.default_rng(606)
    for name, w in cases.diagonal_precoding_variants():
        layers = w.shape[2]
        for qm in (2, 8):
            nre = 30 * 12 * 12
            tb_bits = oracle.tbs(12, 12, 0, qm, 700.0 if qm == 8 else 400.0, layers, 30)
            pdu = abi.make_pdu(bwp_size_rb=30, qm=qm, dmrs_symbols=(2, 11), prb_start=0, prb_count=30, start_symbol=1,
                               nof_symbols=13, precoding=w, tb_size_bytes=tb_bits // 8, ratio_data_dB=1.5,
                               nof_cdm_groups_without_data=2, scrambling_id=77, n_id=5, rnti=4321)
            run_single(gpu_ctx, oracle, pdu, cases.random_tb(rng, pdu), w.shape[1], 30 * 12)


def test_pdsch_extended_cyclic_prefix(gpu_ctx, oracle):
    """Extended cyclic prefix end to end: PDSCH grid and codeword bit-exact, then the 12-symbol OFDM slot."""
    import torch
    rng = np.random.default_rng(1212)
    for pdu, nof_ports, nof_subc in cases.extended_cp_pdus(oracle.tbs):
        assert gpu_ctx.lib.nrphy_pdsch_validate(C.byref(pdu)) == 0
        grid, _ = run_single(gpu_ctx, oracle, pdu, cases.random_tb(rng, pdu), nof_ports, nof_subc)
        cfg = abi.OfdmConfig(2, nof_subc // 12, 512, 1, 0.05, 3.5e9)
        plan = lib.OfdmPlan(gpu_ctx, cfg, nof_ports)
        slot = pdu.slot_index % 4
        iq = plan.modulate_slot_host(grid, slot)
        want = oracle.ofdm_slot(cfg, grid, slot)
        assert iq.shape == want.shape and iq.shape[1] == 12 * (512 + 128)
        assert rel_err(iq, want) < 1e-5
        plan.close()
    bad = cases.extended_cp_pdus(oracle.tbs)[0][0]
    bad.dmrs_symbol_mask |= 1 << 12
    bad.nof_symbols = 13
    assert gpu_ctx.lib.nrphy_pdsch_validate(C.byref(bad)) == abi.ERR_INVALID_PDU


def edge_case_pdus():
    rng = np.random.default_rng(99)
    w22 = (rng.standard_normal((3, 2, 2, 2)) * 0.5).astype(np.float32)       # 3 PRGs, complex random weights
    w42 = (rng.standard_normal((1, 4, 2, 2)) * 0.5).astype(np.float32)
    w43 = (rng.standard_normal((2, 4, 3, 2)) * 0.5).astype(np.float32)
    out = []
    # E > Ncb wrap-around repetition (config 1 style) with rv 2 and 3.
    for rv in (2, 3):
        out.append(("wrap_rv%d" % rv, abi.make_pdu(bwp_size_rb=52, qm=2, dmrs_symbols=(2, 11), prb_count=52,
                                                   nof_symbols=14, base_graph=2, rv=rv, tb_size_bytes=100), 1, 52 * 12))
    # Tiny LBRM buffer (the reference benchmark's quirk: Nref of a few hundred bits).
    out.append(("tiny_lbrm", abi.make_pdu(bwp_size_rb=30, qm=6, dmrs_symbols=(3,), prb_start=2, prb_count=20,
                                          nof_symbols=10, start_symbol=1, tbs_lbrm_bytes=3168, tb_size_bytes=4000,
                                          precoding=w22, prg_size_rb=8), 2, 30 * 12))
    # One CDM group without data: data shares the DM-RS symbols on the other comb.
    out.append(("cdm1", abi.make_pdu(bwp_size_rb=24, qm=4, dmrs_symbols=(2, 9), nof_cdm_groups_without_data=1,
                                     prb_start=0, prb_count=24, nof_symbols=13, tb_size_bytes=1500, rv=1,
                                     precoding=abi.identity_precoding(1)), 1, 24 * 12))
    # Four layers but only one CDM group without data: data RE share the second DM-RS comb and DM-RS must win
    # (the reference maps DM-RS after the data; here that forces the separate, later DM-RS launch).
    out.append(("cdm1_l4", abi.make_pdu(bwp_size_rb=30, qm=6, dmrs_symbols=(2, 10), nof_cdm_groups_without_data=1,
                                        prb_start=4, prb_count=21, nof_symbols=12, start_symbol=1, tb_size_bytes=5000,
                                        precoding=abi.identity_precoding(4)), 4, 30 * 12))
    # No CDM group without data at all: data on every RE of the DM-RS symbols, DM-RS overwrites its comb.
    out.append(("cdm0", abi.make_pdu(bwp_size_rb=20, qm=2, dmrs_symbols=(3,), nof_cdm_groups_without_data=0,
                                     prb_start=0, prb_count=20, nof_symbols=8, start_symbol=2, tb_size_bytes=300,
                                     precoding=abi.identity_precoding(2)), 2, 20 * 12))
    # 2 layers on 4 ports with random complex weights, PRB0 reference point, BWP offset, power ratios.
    out.append(("l2p4", abi.make_pdu(bwp_start_rb=5, bwp_size_rb=40, qm=8, dmrs_symbols=(2, 3), prb_start=9,
                                     prb_count=17, nof_symbols=12, start_symbol=2, ref_point=1, tb_size_bytes=7000,
                                     precoding=w42, ratio_dmrs_dB=3.0, ratio_data_dB=-1.25, slot_index=13,
                                     scrambling_id=40000, n_scid=1, rnti=65535, n_id=1023), 4, 48 * 12))
    # 3 layers, 2 PRGs, smallest transport blocks (CRC16, BG2 with Kb 6/8/9).
    for nbytes in (3, 10, 30, 75, 85):
        out.append(("small%d" % nbytes, abi.make_pdu(bwp_size_rb=20, qm=2, dmrs_symbols=(2,), prb_start=3, prb_count=4,
                                                     nof_symbols=9, base_graph=2, tb_size_bytes=nbytes,
                                                     precoding=w43, prg_size_rb=10), 4, 20 * 12))
    # Zero-pad on the last codeblock and CB sizes that are not byte aligned.
    for nbytes in (1057, 2111, 3341):
        out.append(("pad%d" % nbytes, abi.make_pdu(bwp_size_rb=60, qm=6, dmrs_symbols=(2, 7), prb_count=55,
                                                   nof_symbols=14, tb_size_bytes=nbytes, base_graph=2, rv=1), 1,
                    60 * 12))
    return out


def test_pdsch_edge_cases(gpu_ctx, oracle):
    rng = np.random.default_rng(5)
    for name, pdu, nof_ports, nof_subc in edge_case_pdus():
        assert lib.validate(pdu) == 0, name
        assert oracle.validate(pdu) == 0, name
        try:
            run_single(gpu_ctx, oracle, pdu, cases.random_tb(rng, pdu), nof_ports, nof_subc)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))


def test_pdsch_batched_plan_mixed_cell(gpu_ctx, oracle):
    """BASELINE config 4 shape: several cells x 4 PDUs per grid in ONE plan, TBs concatenated in one device buffer."""
    import torch
    rng = np.random.default_rng(11)
    n_cells = 3
    pdus, offs, gidx, tbs = [], [], [], []
    pos = 0
    for c in range(n_cells):
        cell_pdus, nof_ports, nof_subc = cases.mixed_cell(c, slot_index=c)
        for p in cell_pdus:
            tb = cases.random_tb(rng, p)
            pdus.append(p)
            offs.append(pos)
            gidx.append(c)
            tbs.append(tb)
            pos += (len(tb) + 15) & ~15
    buf = np.zeros(pos + 16, np.uint8)
    for o, tb in zip(offs, tbs):
        buf[o:o + len(tb)] = tb
    plan = lib.PdschPlan(gpu_ctx, pdus, offs, gidx, n_cells, nof_ports, nof_subc)
    d_grid = torch.full((n_cells, nof_ports, 14, nof_subc), 0x7FFF7FFF, dtype=torch.int32, device="cuda")
    d_rm = torch.zeros(plan.codeword_bits // 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    plan.run(dev(buf), d_grid, d_cw_rm=d_rm, zero_grids=True)
    gpu_ctx.synchronize()
    grids = d_grid.cpu().numpy().view(np.uint16).reshape(n_cells, nof_ports, 14, nof_subc, 2)
    rm = d_rm.cpu().numpy()
    for c in range(n_cells):
        want = np.zeros((nof_ports, 14, nof_subc, 2), np.uint16)
        for i in range(4 * c, 4 * c + 4):
            d = oracle.derive(pdus[i])
            g, orm, _ = oracle.pdsch_process(pdus[i], tbs[i], nof_ports, nof_subc, taps=True,
                                             codeword_bits=d["codeword_bits"])
            want |= g  # PDUs of one cell occupy disjoint RE
            o = plan.codeword_offset(i) // 8
            assert np.array_equal(rm[o:o + len(orm)], orm), (c, i)
        assert np.array_equal(grids[c], want), c
    plan.close()


@pytest.mark.parametrize("regions", ["1", "2", "3", "8"])
@pytest.mark.parametrize("parts", ["1", "4"])
def test_pdsch_prologue_work_split(gpu_ctx_for, oracle, regions, parts):
    """The prologue's work lists however they are cut (knobs of the context): a TB-CRC workgroup per 1 / 2 / 3 / 8 regions of
    16 KiB (the next region's words in flight), a scrambling sequence in one or four parts -- transport blocks of one and of
    many regions, with CRC16 and CRC24A, lengths that are no multiple of four bytes, on 16-byte boundaries (16-byte loads) and
    off them (single words); >= 128 PDUs so that the big-batch rules apply.  Rate-matched codeword (carries the CRCs) and grid
    equal the oracle's."""
    import torch
    gpu_ctx = gpu_ctx_for({"NRPHY_CRC_REGIONS": regions, "NRPHY_SCR_PARTS_BIG": parts})
    rng = np.random.default_rng(int(regions) * 10 + int(parts))
    big, nof_ports, nof_subc, _ = cases.baseline_config(3)       # 108,573 bytes: 7 regions, an odd length
    shapes = [big]
    # a mid-sized block (64-QAM on 60 PRB, ~2.6 regions) and a tiny one with CRC16
    shapes.append(cases.abi.make_pdu(slot_index=3, rnti=7, n_id=5, bwp_start_rb=0, bwp_size_rb=273, qm=6, dmrs_symbols=(2, 7, 11),
                                     nof_cdm_groups_without_data=2, prb_start=4, prb_count=60, start_symbol=0, nof_symbols=12,
                                     base_graph=1, precoding=cases.codebook("four_layer_four_ports_0_0"),
                                     tb_size_bytes=cases.tbs(12, 36, 6, 873, 4, 60) // 8))
    shapes.append(cases.abi.make_pdu(slot_index=5, rnti=9, n_id=2, bwp_start_rb=0, bwp_size_rb=273, qm=2, dmrs_symbols=(2, 7, 11),
                                     nof_cdm_groups_without_data=2, prb_start=100, prb_count=3, start_symbol=0, nof_symbols=12,
                                     base_graph=2, precoding=cases.codebook("four_layer_four_ports_0_0"),
                                     tb_size_bytes=cases.tbs(12, 36, 2, 120, 4, 3) // 8))
    n = 132
    pdus = [shapes[0] if i % 44 == 0 else shapes[1 + i % 2] for i in range(n)]
    # grids: every PDU its own (the three shapes overlap in frequency)
    offs, tbs, pos = [], [], 0
    for i, p in enumerate(pdus):
        tb = cases.random_tb(rng, p)
        pos = (pos + 15) & ~15
        if i % 3 == 1:
            pos += 4 * (1 + i % 3)  # off the 16-byte boundary (a multiple of four, as the interface asks)
        offs.append(pos)
        tbs.append(tb)
        pos += len(tb)
    buf = np.zeros(pos + 32, np.uint8)
    for o, tb in zip(offs, tbs):
        buf[o:o + len(tb)] = tb
    plan = lib.PdschPlan(gpu_ctx, pdus, offs, list(range(n)), n, nof_ports, nof_subc)
    d_grid = torch.full((n, nof_ports, 14, nof_subc), 0x7FFF7FFF, dtype=torch.int32, device="cuda")
    d_rm = torch.zeros(plan.codeword_bits // 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    plan.run(dev(buf), d_grid, d_cw_rm=d_rm, zero_grids=True)
    gpu_ctx.synchronize()
    rm = d_rm.cpu().numpy()
    grids = d_grid.cpu().numpy().view(np.uint16).reshape(n, nof_ports, 14, nof_subc, 2)
    for i in list(range(0, n, 11)) + [44, 88, n - 1]:
        d = oracle.derive(pdus[i])
        g, orm, _ = oracle.pdsch_process(pdus[i], tbs[i], nof_ports, nof_subc, taps=True, codeword_bits=d["codeword_bits"])
        o = plan.codeword_offset(i) // 8
        assert np.array_equal(rm[o:o + len(orm)], orm), i
        assert np.array_equal(grids[i], g), i
    plan.close()


def test_pdsch_overlapping_scrambling_seeds(gpu_ctx, oracle):
    """A shape a seeded sweep found: 64-QAM on three layers, codeblocks of 518 resource elements -- a work item of 512 and one of
    6, whose 31-word scrambling seeds overlap the next codeblock's -- and a sequence long enough to be walked in two parts: the
    seed of the item behind one that runs past the end of a part (or of a block of 31 rows) got none of its words from that part.
    Codeword taps and grid equal the oracle's."""
    rng = np.random.default_rng(1001)
    pdu, nof_ports, nof_subc = list(cases.random_pdus(oracle.tbs, rng, 80))[52]
    d = oracle.derive(pdu)
    assert (pdu.qm, pdu.nof_layers) == (6, 3) and d["rm_length_short"] // 18 > 512, "the generator changed: pick the shape by hand"
    tb = cases.random_tb(np.random.default_rng(7), pdu)
    want, orm, oscr = oracle.pdsch_process(pdu, tb, nof_ports, nof_subc, taps=True, codeword_bits=d["codeword_bits"])
    got, rm, scr = gpu_ctx.pdsch_process_host(pdu, tb, nof_ports, nof_subc, taps=True)
    assert np.array_equal(rm, orm) and np.array_equal(scr, oscr)
    assert np.array_equal(got, want)


def test_pdsch_seed_walk_boundaries(gpu_ctx, oracle):
    """The constructive net around the prologue's seed walk (cases.seed_walk_pdus): PDUs in which a short tail item -- 1 ... 40
    resource elements, its 31-word seed overlapping its neighbours' -- starts -31 ... +1 words around the end of a 31-row block
    or of a sequence part, for 2 ... 32 bits per resource element.  Each PDU alone through the host-span call (a plan of one PDU:
    up to four parts) and all of them in one batched plan: scrambled codeword and grid equal the oracle's.  The library as it
    was before the round-3 fix (commit 13d24f2) fails this test on the first PDU of either kind (checked once, round 4, with
    NRPHY_LIB_SO on a build of that commit: profiles/r04_seed_walk_regression.txt)."""
    import torch
    rng = np.random.default_rng(404)
    picked = cases.seed_walk_pdus(oracle.tbs, rng, 96, max_draws=120000)
    kinds = {h[3] for *_, h in picked}
    assert len(picked) >= 40 and kinds == {"block", "part"}, (len(picked), kinds)
    assert len({h[0] for *_, h in picked}) >= 6 and len({h[2] for *_, h in picked}) >= 28, "the generator lost its spread"
    want = []
    for pdu, nof_ports, nof_subc, hit in picked:
        tb = cases.random_tb(rng, pdu)
        d = oracle.derive(pdu)
        g, orm, oscr = oracle.pdsch_process(pdu, tb, nof_ports, nof_subc, taps=True, codeword_bits=d["codeword_bits"])
        want.append((tb, g, oscr))
        got, rm, scr = gpu_ctx.pdsch_process_host(pdu, tb, nof_ports, nof_subc, taps=True)
        assert np.array_equal(scr, oscr), hit
        assert np.array_equal(rm, orm) and np.array_equal(got, g), hit
    # the same PDUs in one plan (batched path, device pointers), grouped by port count
    for ports in sorted({p[1] for p in picked}):
        idx = [i for i, p in enumerate(picked) if p[1] == ports]
        pdus = [picked[i][0] for i in idx]
        nof_subc = picked[idx[0]][2]
        offs, total = [], 0
        for q in pdus:
            offs.append(total)
            total += (q.tb_size_bytes + 255) & ~255
        buf = np.zeros(total + 64, np.uint8)
        for o, i in zip(offs, idx):
            buf[o:o + len(want[i][0])] = want[i][0]
        plan = lib.PdschPlan(gpu_ctx, pdus, offs, list(range(len(pdus))), len(pdus), ports, nof_subc)
        d_grid = torch.full((len(pdus), ports, 14, nof_subc), 0x7FFF7FFF, dtype=torch.int32, device="cuda")
        d_scr = torch.zeros(plan.codeword_bits // 8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plan.run(dev(buf), d_grid, d_cw_scr=d_scr, zero_grids=True)
        gpu_ctx.synchronize()
        scr = d_scr.cpu().numpy()
        grids = d_grid.cpu().numpy().view(np.uint16).reshape(len(pdus), ports, 14, nof_subc, 2)
        for k, i in enumerate(idx):
            o = plan.codeword_offset(k) // 8
            assert np.array_equal(scr[o:o + len(want[i][2])], want[i][2]), picked[i][3]
            assert np.array_equal(grids[k], want[i][1]), picked[i][3]
        plan.close()


def test_pdsch_full_size_batch_properties(gpu_ctx, oracle):
    """At BASELINE size (config 3, 64 slots in one launch): identical inputs give identical grids (no cross-slot
    interference), different TBs differ, and one slot of the batch matches the oracle bit for bit."""
    import torch
    pdu, nof_ports, nof_subc, _ = cases.baseline_config(3)
    n = 64
    rng = np.random.default_rng(3)
    tb_a, tb_b = cases.random_tb(rng, pdu), cases.random_tb(rng, pdu)
    stride = (pdu.tb_size_bytes + 63) & ~63
    buf = np.zeros(n * stride + 64, np.uint8)
    for i in range(n):
        buf[i * stride: i * stride + pdu.tb_size_bytes] = tb_b if i == 5 else tb_a
    plan = lib.PdschPlan(gpu_ctx, [pdu] * n, [i * stride for i in range(n)], list(range(n)), n, nof_ports, nof_subc)
    assert plan.nof_codeblocks == 104 * n
    d_grid = torch.zeros((n, nof_ports, 14, nof_subc), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    plan.run(dev(buf), d_grid)
    gpu_ctx.synchronize()
    g = d_grid.cpu().numpy()
    for i in range(1, n):
        if i != 5:
            assert np.array_equal(g[i], g[0]), i
    assert not np.array_equal(g[5], g[0])
    want = oracle.pdsch_process(pdu, tb_b, nof_ports, nof_subc)
    assert np.array_equal(g[5].view(np.uint16).reshape(want.shape), want)
    # Unallocated RE stay zero: PRB 270-272 and symbols 12-13.
    assert not g[:, :, 12:, :].any() and not g[:, :, :, 270 * 12:].any()
    plan.close()


def test_pdsch_invalid_pdus_are_refused(gpu_ctx):
    """Error behaviour of the boundary: what the reference asserts on is returned as NRPHY_ERR_INVALID_PDU."""
    pdu, nof_ports, nof_subc, _ = cases.baseline_config(1)
    tb = np.zeros(pdu.tb_size_bytes, np.uint8)
    pdu.dmrs_type = 2
    with pytest.raises(lib.NrphyError) as e:
        gpu_ctx.pdsch_process_host(pdu, tb, nof_ports, nof_subc)
    assert e.value.status == abi.ERR_INVALID_PDU
    pdu.dmrs_type = 1
    with pytest.raises(lib.NrphyError) as e:
        gpu_ctx.pdsch_process_host(pdu, tb, nof_ports, 12 * 10)   # grid smaller than the allocation
    assert e.value.status == abi.ERR_ARGUMENT


# ---------------------------------------------------------------------------------------------------------------------
# OFDM modulator + DFT
# ---------------------------------------------------------------------------------------------------------------------
def rel_err(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("size", [128, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096, 4608, 6144, 9216, 12288,
                                  18432, 24576, 36864, 49152])
@pytest.mark.parametrize("inverse", [0, 1])
def test_dft_vs_oracle(gpu_ctx, oracle, size, inverse):
    """Every size of the reference's generic DFT (dft_processor_generic_impl.cpp:190-208), both directions."""
    import torch
    rng = np.random.default_rng(size + inverse)
    batch = 5 if size <= 6144 else 3
    x = (rng.standard_normal((batch, size)) + 1j * rng.standard_normal((batch, size))).astype(np.complex64)
    d_in = dev(x.view(np.float32))
    d_out = torch.zeros_like(d_in)
    torch.cuda.synchronize()
    gpu_ctx.dft(size, inverse, batch, d_in, d_out)
    gpu_ctx.synchronize()
    out = d_out.cpu().numpy().view(np.complex64)
    for i in range(batch):
        want = oracle.dft(x[i], inverse)
        assert rel_err(out[i], want) < 1e-5   # north-star tolerance; reference test uses MSE < 1e-6 / peak < 1e-3


@pytest.mark.parametrize("name", ["n4096", "n2048", "n1024", "n1536", "n3072", "n768", "n384", "x512", "x2048", "n6144",
                                  "n4608"])
def test_ofdm_modulator_vs_oracle_and_reference_golden(gpu_ctx, oracle, name):
    import torch
    g = np.load(os.path.join(cases.GOLDEN, "ofdm_sizes.npz" if name in ("n6144", "n4608") else "ofdm_modulator.npz"))
    mu, bw, n, fc, slot = g[name + "_cfg"][:5]
    ext = int(g[name + "_cfg"][5]) if len(g[name + "_cfg"]) > 5 else 0   # x...: extended cyclic prefix, 12 symbols
    nsymb = 12 if ext else 14
    cfg = abi.OfdmConfig(int(mu), int(bw), int(n), ext, 1.0 / np.sqrt(n), float(fc))
    grid = g[name + "_grid"]
    plan = lib.OfdmPlan(gpu_ctx, cfg, 1)
    assert plan.slot_stride == lib.slot_size(cfg, 0)
    d_iq = torch.zeros((1, 1, plan.slot_stride, 2), dtype=torch.float32, device="cuda")
    d_slot = dev(np.array([int(slot)], np.uint32).view(np.int32))
    torch.cuda.synchronize()
    plan.run(1, dev(grid.view(np.uint32).view(np.int32)), d_iq, d_slot_index=d_slot)
    gpu_ctx.synchronize()
    iq = d_iq.cpu().numpy().view(np.complex64).reshape(-1)
    want = oracle.ofdm_slot(cfg, grid, int(slot))[0]
    assert rel_err(iq[: len(want)], want) < 1e-5
    assert rel_err(iq[: len(want)], g[name + "_iq"][0]) < 1e-5   # reference output (its own test allows 5e-5)
    # Structure checks of ofdm_modulator_unittest.cpp: the cyclic prefix repeats the symbol tail.
    off = 0
    for l in range(nsymb):
        size = lib.symbol_size(cfg, nsymb * int(slot) + l)
        cp = size - int(n)
        assert cp == (int(n) // 4 if ext else cp)
        assert np.array_equal(iq[off: off + cp], iq[off + int(n): off + size])
        off += size
    assert off == len(want)
    # Host-span single-symbol entry point (ofdm_symbol_modulator::modulate semantics).
    sym = nsymb * int(slot) + 3
    one = plan.modulate_symbol_host(grid, 0, sym)
    start = sum(lib.symbol_size(cfg, nsymb * int(slot) + l) for l in range(3))
    assert np.array_equal(one, iq[start: start + len(one)])
    plan.close()


def bf16_to_f32(raw):
    return (raw.astype(np.uint32) << 16).view(np.float32)


def assert_bf16_grids_close(got, want, min_exact=0.99):
    """cbf16 grids out of different float FFTs: at most one bf16 ulp apart, almost all identical."""
    a, b = bf16_to_f32(got), bf16_to_f32(want)
    scale = np.abs(b).max()
    assert np.all(np.abs(a - b) <= np.maximum(np.abs(b), 1e-3 * scale) * 2.0 ** -7)
    assert np.mean(got == want) >= min_exact


@pytest.mark.parametrize("name", ["d4096", "d2048w", "d1536", "d512w", "dx1024w", "d6144", "d4608w"])
def test_ofdm_demodulator_vs_oracle_and_reference_golden(gpu_ctx, oracle, name):
    """Receive side of seam C (ofdm_slot_demodulator): device path against the oracle and the reference's output."""
    import torch
    g = np.load(os.path.join(cases.GOLDEN, "ofdm_sizes.npz" if name in ("d6144", "d4608w") else "ofdm_demodulator.npz"))
    mu, bw, n, fc, slot, wo = g[name + "_cfg"][:6]
    ext = int(g[name + "_cfg"][6]) if len(g[name + "_cfg"]) > 6 else 0   # dx...: extended cyclic prefix
    slot, wo = int(slot), int(wo)
    cfg = abi.OfdmConfig(int(mu), int(bw), int(n), ext, 1.0 / np.sqrt(n), float(fc))
    iq = g[name + "_iq"]
    nof_ports = iq.shape[0]
    plan = lib.OfdmPlan(gpu_ctx, cfg, nof_ports)
    # Two slots in one launch (the second one with the ports swapped) in the layout nrphy_ofdm_run writes.
    buf = np.zeros((2, nof_ports, plan.slot_stride), np.complex64)
    buf[0, :, : iq.shape[1]] = iq
    buf[1, :, : iq.shape[1]] = iq[::-1]
    d_grid = torch.zeros((2, nof_ports, 14, int(bw) * 12), dtype=torch.int32, device="cuda")
    d_slot = dev(np.array([slot, slot], np.uint32).view(np.int32))
    torch.cuda.synchronize()
    plan.demod_run(2, dev(buf.view(np.float32)), d_grid, d_slot_index=d_slot, window_offset=wo)
    gpu_ctx.synchronize()
    got = d_grid.cpu().numpy().view(np.uint16).reshape(2, nof_ports, 14, int(bw) * 12, 2)
    want = oracle.ofdm_demod_slot(cfg, iq, slot, wo)
    assert_bf16_grids_close(got[0], want)
    assert_bf16_grids_close(got[1], want[::-1])
    assert_bf16_grids_close(got[0], g[name + "_grid"])   # the reference's own output
    # Host-span entry point (ofdm_slot_demodulator::demodulate semantics).
    assert np.array_equal(plan.demodulate_slot_host(iq, slot, wo), got[0])
    # Host-span single-symbol entry point (ofdm_symbol_demodulator::demodulate semantics).
    nsymb = 12 if ext else 14
    sym = nsymb * slot + 5
    start = sum(lib.symbol_size(cfg, nsymb * slot + l) for l in range(5))
    row = plan.demodulate_symbol_host(iq[0, start: start + lib.symbol_size(cfg, sym)], sym, wo)
    assert np.array_equal(row, got[0, 0, 5])
    # A window offset beyond the shortest cyclic prefix is rejected (ofdm_demodulator_impl.cpp:58-63).
    shortest_cp = (144 * int(n)) // 2048   # ofdm_demodulator_impl.cpp:63, also with extended cyclic prefix
    assert gpu_ctx.lib.nrphy_ofdm_demod_run(plan.handle, 1, d_grid.data_ptr(), None, shortest_cp,
                                            d_grid.data_ptr(), None) == abi.ERR_ARGUMENT
    plan.close()


def test_ofdm_modulate_demodulate_round_trip(gpu_ctx):
    """Transmit and receive chains back to back on the device: the grid comes back up to bf16 rounding."""
    import torch
    rng = np.random.default_rng(5)
    n, bw, slots = 2048, 106, 3
    cfg = abi.OfdmConfig(0, bw, n, 0, 1.0 / np.sqrt(n), 2.6e9)
    grid = (rng.standard_normal((slots, 2, 14, bw * 12, 2)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    plan = lib.OfdmPlan(gpu_ctx, cfg, 2)
    d_grid = dev(grid.view(np.uint32).view(np.int32))
    d_iq = torch.zeros((slots, 2, plan.slot_stride, 2), dtype=torch.float32, device="cuda")
    d_back = torch.zeros_like(d_grid)
    torch.cuda.synchronize()
    plan.run(slots, d_grid, d_iq)
    plan.demod_run(slots, d_iq, d_back)
    gpu_ctx.synchronize()
    back = d_back.cpu().numpy().view(np.uint16).reshape(grid.shape)
    assert_bf16_grids_close(back, grid, min_exact=0.9)
    plan.close()


def test_end_to_end_slot_batch(gpu_ctx, oracle):
    """PDSCH + OFDM chained on the device for a small batch of config-2 slots, against the oracle chain."""
    import torch
    pdu, nof_ports, nof_subc, ofdm = cases.baseline_config(2)
    n = 3
    rng = np.random.default_rng(21)
    tbs = [cases.random_tb(rng, pdu) for _ in range(n)]
    stride = (pdu.tb_size_bytes + 63) & ~63
    buf = np.zeros(n * stride + 64, np.uint8)
    for i, tb in enumerate(tbs):
        buf[i * stride: i * stride + len(tb)] = tb
    plan = lib.PdschPlan(gpu_ctx, [pdu] * n, [i * stride for i in range(n)], list(range(n)), n, nof_ports, nof_subc)
    oplan = lib.OfdmPlan(gpu_ctx, ofdm, nof_ports)
    d_grid = torch.zeros((n, nof_ports, 14, nof_subc), dtype=torch.int32, device="cuda")
    d_iq = torch.zeros((n, nof_ports, oplan.slot_stride, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    plan.run(dev(buf), d_grid)
    torch.cuda.synchronize()
    oplan.run(n, d_grid, d_iq)
    gpu_ctx.synchronize()
    iq = d_iq.cpu().numpy().view(np.complex64).reshape(n, nof_ports, -1)
    for i in range(n):
        grid = oracle.pdsch_process(pdu, tbs[i], nof_ports, nof_subc)
        want = oracle.ofdm_slot(ofdm, grid, 0)
        assert rel_err(iq[i], want) < 1e-5


def test_pdsch_encode_host_seam_b(gpu_ctx, oracle):
    """Seam B (pdsch_encoder::encode / hw_accelerator_pdsch_enc in TB mode): TB -> rate-matched, interleaved codeword
    from the encoder configuration alone (no allocation), bit-exact against the oracle's encoder."""
    rng = np.random.default_rng(12)
    pdus = [cases.baseline_config(c)[0] for c in (1, 2, 3)] + cases.unit_test_like_pdus(rng)[::3]
    for pdu in pdus:
        d = oracle.derive(pdu)
        tb = cases.random_tb(rng, pdu)
        want = oracle.pdsch_encode(pdu, tb)
        bits, packed = gpu_ctx.pdsch_encode_host(pdu.ldpc_base_graph, pdu.rv, pdu.qm, d["n_ref"], pdu.nof_layers,
                                                 d["nof_re"] * pdu.nof_layers, tb)
        assert bits.size == d["codeword_bits"]
        assert np.array_equal(packed, want[: packed.size])
        assert np.array_equal(np.packbits(bits), packed)
    # unlimited buffer (Nref = 0) and a bad configuration
    pdu = pdus[1]
    d = oracle.derive(pdu)
    bits, _ = gpu_ctx.pdsch_encode_host(1, 0, 6, 0, 2, d["nof_re"] * 2, cases.random_tb(rng, pdu))
    assert bits.size == d["codeword_bits"]
    cfg = abi.PdschEncoderCfg(1, 0, 5, 0, 2, 100, 10)
    buf = np.zeros(16, np.uint8)
    assert gpu_ctx.lib.nrphy_pdsch_encode_host(gpu_ctx.handle, C.byref(cfg), buf.ctypes.data, None, None) == abi.ERR_INVALID_PDU


def test_host_span_calls_from_several_threads(gpu_ctx, oracle):
    """The reference runs one processor instance per worker thread; the adaptors of all of them share one context.
    Host-span calls (shared staging buffers, one stream) must serialise correctly."""
    import threading
    rng = np.random.default_rng(99)
    jobs = []
    for cfg in (1, 2, 1, 2):
        pdu, nof_ports, nof_subc, _ = cases.baseline_config(cfg, slot_index=len(jobs))
        tb = cases.random_tb(rng, pdu)
        jobs.append((pdu, tb, nof_ports, nof_subc, oracle.pdsch_process(pdu, tb, nof_ports, nof_subc)))
    errors = []

    def worker(job):
        pdu, tb, nof_ports, nof_subc, want = job
        for _ in range(5):
            got = gpu_ctx.pdsch_process_host(pdu, tb, nof_ports, nof_subc)
            if not np.array_equal(got, want):
                errors.append("mismatch")

    threads = [threading.Thread(target=worker, args=(j,)) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors


def test_mixed_host_span_calls_from_several_threads(gpu_ctx, oracle):
    """The downlink processor of the reference dispatches PDSCH, NZP-CSI-RS and the lower PHY's modulator from different
    threads; their adaptors share one context, whose staging buffers (one grid buffer among them) they all use."""
    import threading
    rng = np.random.default_rng(4242)
    pdu, nof_ports, nof_subc, ocfg = cases.baseline_config(2)
    tb = cases.random_tb(rng, pdu)
    want_pdsch = oracle.pdsch_process(pdu, tb, nof_ports, nof_subc)
    name, ccfg, c_ports, c_subc = next(iter(cases.csi_rs_cases(rng)))
    cgrid = (rng.standard_normal((c_ports, 14, c_subc, 2)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    want_csi = oracle.csi_rs_map(ccfg, cgrid)
    oplan = lib.OfdmPlan(gpu_ctx, ocfg, nof_ports)
    n = lib.slot_size(ocfg, 0)
    want_iq = oracle.ofdm_slot(ocfg, want_pdsch, 0)
    errors = []

    def pdsch():
        for _ in range(8):
            if not np.array_equal(gpu_ctx.pdsch_process_host(pdu, tb, nof_ports, nof_subc), want_pdsch):
                errors.append("pdsch")

    def csi():
        for _ in range(8):
            if not np.array_equal(gpu_ctx.csi_rs_map_host(ccfg, cgrid), want_csi):
                errors.append("csi-rs")

    def ofdm():
        for _ in range(8):
            iq = np.zeros((nof_ports, n), np.complex64)
            rc = gpu_ctx.lib.nrphy_ofdm_modulate_slot_host(oplan.handle, want_pdsch.ctypes.data, 0, iq.ctypes.data)
            if rc != 0 or rel_err(iq, want_iq) > 1e-5:
                errors.append("ofdm")

    threads = [threading.Thread(target=f) for f in (pdsch, csi, ofdm, pdsch, csi, ofdm)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    oplan.close()
    assert not errors, sorted(set(errors))


@pytest.mark.parametrize("zero_copy", [None, "1", "3"])
def test_pdsch_async_queue_keeps_pdus_in_flight(gpu_ctx, oracle, zero_copy, monkeypatch):
    """nrphy_pdsch_async_*: several PDUs in flight through the host-span seam (what an asynchronous pdsch_processor
    drop-in uses); every completion fires exactly once on a runtime thread with the PDU's grid, also when the shapes
    alternate (cached plans) and when the queue is full (NRPHY_ERR_CAPACITY, then retry).  Also with the kernels reading
    the transport block from, and writing the grid to, the pinned staging (NRPHY_ASYNC_ZERO_COPY, read at queue creation)."""
    import threading
    import time
    if zero_copy is None:
        monkeypatch.delenv("NRPHY_ASYNC_ZERO_COPY", raising=False)
    else:
        monkeypatch.setenv("NRPHY_ASYNC_ZERO_COPY", zero_copy)
    rng = np.random.default_rng(606)
    pdus = []
    for cfg in (1, 2, 1, 2, 2, 1):
        pdu, nof_ports, nof_subc, _ = cases.baseline_config(cfg, slot_index=len(pdus) % 3)
        pdus.append((pdu, nof_ports, nof_subc))
    nof_ports = max(p[1] for p in pdus)
    nof_subc = max(p[2] for p in pdus)
    q = lib.PdschAsyncQueue(gpu_ctx, 3, nof_ports, nof_subc, max(p[0].tb_size_bytes for p in pdus))
    results, lock, threads_seen = {}, threading.Lock(), set()
    jobs = []
    for i in range(24):
        pdu = pdus[i % len(pdus)][0]
        tb = cases.random_tb(rng, pdu)
        jobs.append((pdu, tb))
    full = 0
    for i, (pdu, tb) in enumerate(jobs):
        def on_done(status, grid, i=i):
            with lock:
                results.setdefault(i, []).append((status, grid))
                threads_seen.add(threading.get_ident())
        while not q.submit(pdu, tb, on_done):
            full += 1
            time.sleep(0.0005)
    q.wait()
    assert sorted(results) == list(range(len(jobs))) and all(len(v) == 1 for v in results.values())
    assert threading.get_ident() not in threads_seen, "completions come from a runtime thread, not from the submitter"
    for i, (pdu, tb) in enumerate(jobs):
        status, grid = results[i][0]
        assert status == 0
        want = oracle.pdsch_process(pdu, tb, nof_ports, nof_subc)
        assert np.array_equal(grid, want), i
    q.close()


@pytest.mark.parametrize("table_cap", [None, "512"])
def test_pdsch_async_live_traffic_every_pdu_differs(gpu_ctx, oracle, table_cap, monkeypatch):
    """The asynchronous seam on live traffic: no two consecutive submits carry the same PDU (slot index, RNTI, identities,
    allocation, MCS, reserved patterns, weights all drawn), as in a gNB, where the reference derives its per-PDU state on
    every call (pdsch_processor_concurrent_impl.cpp:55-207).  Every operation builds its plan into the slot's staging (no
    allocation or blocking copy on the submit path); shapes that come back -- the same allocation with another RNTI and
    transport block -- take their RE tables and zero-fill lists from the slot's shape cache.  With a table space too small
    for any plan (NRPHY_ASYNC_TABLE_CAP) every operation takes the slow path with memory of its own.  Grids bit-exact."""
    import threading
    monkeypatch.delenv("NRPHY_ASYNC_ZERO_COPY", raising=False)
    if table_cap is None:
        monkeypatch.delenv("NRPHY_ASYNC_TABLE_CAP", raising=False)
    else:
        monkeypatch.setenv("NRPHY_ASYNC_TABLE_CAP", table_cap)
    rng = np.random.default_rng(31337)
    drawn = cases.random_pdus(oracle.tbs, rng, 20)
    nof_ports, nof_subc = 4, max(p[2] for p in drawn)
    jobs = []
    for pdu, _, _ in drawn:
        jobs.append((pdu, cases.random_tb(rng, pdu)))
    for k, (pdu, _, _) in enumerate(drawn[:12]):
        # the same shape again under another identity: allocation, symbols, DM-RS and reserved patterns, layers and ports kept
        twin = abi.PdschPdu.from_buffer_copy(pdu)
        twin._keepalive = getattr(pdu, "_keepalive", None)
        twin.rnti = int(rng.integers(1, 65520))
        twin.n_id = int(rng.integers(0, 1024))
        twin.slot_index = (pdu.slot_index + 1 + k) % 20
        twin.scrambling_id = int(rng.integers(0, 65536))
        jobs.append((twin, cases.random_tb(rng, twin)))
    q = lib.PdschAsyncQueue(gpu_ctx, 3, nof_ports, nof_subc, max(j[0].tb_size_bytes for j in jobs))
    results, lock = {}, threading.Lock()
    order = list(rng.permutation(len(jobs))) + list(rng.permutation(len(jobs)))
    for n, i in enumerate(order):
        def on_done(status, grid, n=n):
            with lock:
                results.setdefault(n, []).append((status, grid))
        while not q.submit(jobs[i][0], jobs[i][1], on_done):
            q.wait_slot()
    q.wait()
    assert sorted(results) == list(range(len(order))) and all(len(v) == 1 for v in results.values())
    want = {}
    for n, i in enumerate(order):
        status, grid = results[n][0]
        assert status == 0
        if i not in want:
            want[i] = oracle.pdsch_process(jobs[i][0], jobs[i][1], nof_ports, nof_subc)
        assert np.array_equal(grid, want[i]), (n, i)
    q.close()


def test_pdsch_async_shape_cache_starts_over(gpu_ctx, oracle, monkeypatch):
    """A full shape cache starts over (PlanShapeCache::MAX_ENTRIES = 256 in csrc/pdsch_plan.h), and nothing stale survives.

    A queue of depth 1 has one cache.  On a grid of 1 port every distinct allocation adds two entries, one RE mapping and
    one zero-fill list, and a plan clears the cache first when it finds more than 256 entries: 129 shapes leave 258, so the
    130th shape arrives at an empty cache.  140 distinct shapes are submitted (the cache then holds shapes 130 ... 140); then
    the first 10 again under another RNTI and transport block, which have to be rebuilt; then the last 10 again, which the
    restarted cache serves.  Another MAX_ENTRIES wants another count of shapes here: more than MAX_ENTRIES / 2 + 1 of them
    before the ones that come back.  Every grid bit-exact, every status 0, every completion exactly once."""
    import threading
    monkeypatch.delenv("NRPHY_ASYNC_ZERO_COPY", raising=False)
    monkeypatch.delenv("NRPHY_ASYNC_TABLE_CAP", raising=False)
    rng = np.random.default_rng(256)
    nof_ports, nof_prb = 1, 24
    nof_subc = 12 * nof_prb
    runs = [(start, length) for length in range(1, nof_prb + 1) for start in range(0, nof_prb - length + 1)][:140]
    assert len(set(runs)) == 140

    def job(run, rnti):
        start, length = run
        tb_bits = oracle.tbs(4, 12, 0, 2, 300.0, 1, length)  # as cases.random_pdus: 4 symbols, one DM-RS symbol, two CDM groups
        pdu = abi.make_pdu(slot_index=rnti % 20, rnti=rnti, bwp_start_rb=0, bwp_size_rb=nof_prb, qm=2, n_id=rnti % 1024,
                           dmrs_symbols=(2,), nof_cdm_groups_without_data=2, prb_start=start, prb_count=length, start_symbol=2,
                           nof_symbols=4, base_graph=2, precoding=abi.identity_precoding(1), tb_size_bytes=tb_bits // 8)
        return pdu, cases.random_tb(rng, pdu)

    jobs = [job(run, 1 + k) for k, run in enumerate(runs)]
    jobs += [job(run, 1001 + k) for k, run in enumerate(runs[:10])]
    jobs += [job(run, 2001 + k) for k, run in enumerate(runs[-10:])]
    q = lib.PdschAsyncQueue(gpu_ctx, 1, nof_ports, nof_subc, max(j[0].tb_size_bytes for j in jobs))
    results, lock = {}, threading.Lock()
    for n, (pdu, tb) in enumerate(jobs):
        def on_done(status, grid, n=n):
            with lock:
                results.setdefault(n, []).append((status, grid))
        while not q.submit(pdu, tb, on_done):
            q.wait_slot()
    q.wait()
    assert sorted(results) == list(range(len(jobs))) and all(len(v) == 1 for v in results.values())
    for n, (pdu, tb) in enumerate(jobs):
        status, grid = results[n][0]
        assert status == 0, n
        assert np.array_equal(grid, oracle.pdsch_process(pdu, tb, nof_ports, nof_subc)), n
    q.close()


def test_host_span_dft_and_slot_modulator(gpu_ctx, oracle):
    """The host-span entry points the srsRAN adaptors call (dft_processor::run, ofdm_slot_modulator::modulate)."""
    rng = np.random.default_rng(77)
    x = (rng.standard_normal(1024) + 1j * rng.standard_normal(1024)).astype(np.complex64)
    out = np.zeros_like(x)
    rc = gpu_ctx.lib.nrphy_dft_run_host(gpu_ctx.handle, 1024, 1, x.ctypes.data, out.ctypes.data)
    assert rc == 0 and rel_err(out, oracle.dft(x, 1)) < 1e-5
    assert gpu_ctx.lib.nrphy_dft_run_host(gpu_ctx.handle, 1000, 1, x.ctypes.data, out.ctypes.data) == abi.ERR_ARGUMENT
    cfg = abi.OfdmConfig(1, 51, 2048, 0, 0.5, 3.6e9)
    grid = (rng.standard_normal((2, 14, 51 * 12, 2)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    plan = lib.OfdmPlan(gpu_ctx, cfg, 2)
    for slot in (0, 1):
        n = lib.slot_size(cfg, slot)
        iq = np.zeros((2, n), np.complex64)
        assert gpu_ctx.lib.nrphy_ofdm_modulate_slot_host(plan.handle, grid.ctypes.data, slot, iq.ctypes.data) == 0
        assert rel_err(iq, oracle.ofdm_slot(cfg, grid, slot)) < 1e-5
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# LDPC decoder ("next" row, receive side): bit-exact hard bits and iteration counts against the oracle, which is pinned
# to the reference's generic decoder (tests/test_oracle.py)
# ---------------------------------------------------------------------------------------------------------------------
DECODER_KERNELS = {  # environment a context is created under -> which form of the decoder its launches take
    "default": {},                                  # two checks per lane, messages per edge: in LDS where the occupancy rule allows, else in the scratch slot
    "lds-messages": {"NRPHY_DECODER_LDSMSG": "2"},  # ... in LDS wherever a workgroup's LDS can hold them
    "slot-messages": {"NRPHY_DECODER_LDSMSG": "0"}, # ... always in the codeblock's slot of the caller's scratch
    "one-check": {"NRPHY_DECODER_PAIRS": "0"},      # one check per lane, compressed records in the slot (what odd lifting sizes always take)
}


@pytest.mark.parametrize("kernel", list(DECODER_KERNELS))
@pytest.mark.parametrize("case", cases.LDPC_DECODE_CASES)
def test_ldpc_decoder_vs_oracle(gpu_ctx_for, oracle, case, kernel):
    """Every form of the decoder kernel: two checks per lane in packed 16-bit arithmetic (even lifting sizes) with the messages
    per edge in LDS or in the codeblock's slot, and one check per lane with compressed records -- hard bits and iteration counts
    of all equal the oracle's."""
    gpu_ctx = gpu_ctx_for(DECODER_KERNELS[kernel])
    bg, zc, extra, tail, crc_id, filler, amp, sigma = case
    rng = np.random.default_rng(zc * 1000 + extra)
    nof_llr = cases.ldpc_decode_nof_llr(case)
    msg, llr = cases.make_ldpc_llrs(oracle, rng, bg, zc, nof_llr, crc_id, filler, amp, sigma)
    for crc in (crc_id, 0):
        for iters in (1, 3, 8):
            it_o, bits_o = oracle.ldpc_decode(bg, zc, filler, crc, iters, 0.8, llr)
            it_g, bits_g = gpu_ctx.ldpc_decode_host(bg, zc, filler, crc, iters, 0.8, llr)
            assert it_g == it_o, (crc, iters)
            assert np.array_equal(bits_g, bits_o), (crc, iters, int(np.count_nonzero(bits_g != bits_o)))
    # other scaling factors, saturated and "certain" inputs
    hard = llr.copy()
    hard[::7] = np.where(hard[::7] >= 0, 127, -127)
    hard[5::11] = 0
    for scaling in (0.5, 0.75, 0.95):
        it_o, bits_o = oracle.ldpc_decode(bg, zc, filler, crc_id, 6, scaling, hard)
        it_g, bits_g = gpu_ctx.ldpc_decode_host(bg, zc, filler, crc_id, 6, scaling, hard)
        assert it_g == it_o and np.array_equal(bits_g, bits_o), scaling
    # all-zero input: nothing to decode (ldpc_decoder_impl.cpp:88-97)
    zero = np.zeros(nof_llr, np.int8)
    assert gpu_ctx.ldpc_decode_host(bg, zc, filler, crc_id, 8, 0.8, zero)[0] == 0
    it, bits = gpu_ctx.ldpc_decode_host(bg, zc, filler, 0, 8, 0.8, zero)
    assert it == 0 and bits.all()


@pytest.mark.parametrize("bg", [1, 2])
def test_ldpc_decoder_reference_unit_tests_all_graphs(gpu_ctx, oracle, bg):
    """The reference's LDPCDecTest / ZeroLLR / AlmostZeroLLR (ldpc_enc_dec_test.cpp:287-358) through the C ABI: all 51
    lifting sizes, noiseless codeblocks at the test's four lengths, no CRC, 6 iterations; bit-exact with the oracle too."""
    rng = np.random.default_rng(300 + bg)
    for zc in LIFTING_SIZES:
        for length in cases.ldpc_dec_test_lengths(bg, zc):
            msg, llr = cases.noiseless_llrs(oracle, rng, bg, zc, zc // 3, length)
            it, bits = gpu_ctx.ldpc_decode_host(bg, zc, zc // 3, 0, 6, 0.8, llr)
            assert it == 0 and np.array_equal(bits, msg), (zc, length)
        full = (66 if bg == 1 else 50) * zc
        zero = np.zeros(full, np.int8)
        it, bits = gpu_ctx.ldpc_decode_host(bg, zc, 0, 0, 6, 0.8, zero)
        assert it == 0 and bits.all()
        for i in range((24 if bg == 1 else 12) * zc + 2, full, 3):
            zero[i] = 1 if i % 2 == 0 else -1
        it, bits = gpu_ctx.ldpc_decode_host(bg, zc, 0, 0, 6, 0.8, zero)
        assert bits.all()
        # a noisy codeblock per lifting size against the oracle, with the CRC that size would carry
        crc_id = 16 if (22 if bg == 1 else 10) * zc < 3824 else 0x24A
        if (22 if bg == 1 else 10) * zc - zc // 3 > 40:
            _, noisy = cases.make_ldpc_llrs(oracle, rng, bg, zc, full - 2 * zc, crc_id, zc // 3, 12, 5)
            want = oracle.ldpc_decode(bg, zc, zc // 3, crc_id, 6, 0.8, noisy)
            got = gpu_ctx.ldpc_decode_host(bg, zc, zc // 3, crc_id, 6, 0.8, noisy)
            assert got[0] == want[0] and np.array_equal(got[1], want[1]), zc


def test_ldpc_decoder_batch_and_argument_checks(gpu_ctx, oracle):
    """A batch of codeblocks of one configuration resident in HBM, each with its own noise; strides; refusals."""
    import torch
    bg, zc, filler, crc_id = 1, 384, 72, 0x24B
    nof_llr, n_cb = 22 * 384 + 4 * 384 - 2 * 384 + 200, 24
    rng = np.random.default_rng(4242)
    stride = nof_llr + 57
    llrs = np.zeros((n_cb, stride), np.int8)
    want = []
    for i in range(n_cb):
        _, llr = cases.make_ldpc_llrs(oracle, rng, bg, zc, nof_llr, crc_id, filler, 20, 6 + i % 6)
        llrs[i, :nof_llr] = llr
        llrs[i, nof_llr:] = 99  # must never be read
        want.append(oracle.ldpc_decode(bg, zc, filler, crc_id, 6, 0.8, llr))
    k = 22 * zc
    out = torch.zeros((n_cb, k // 8 + 8), dtype=torch.uint8, device="cuda")
    its = torch.full((n_cb,), 77, dtype=torch.int32, device="cuda")
    cfg = abi.LdpcDecoderCfg(bg, zc, filler, crc_id, nof_llr, 6, 0.8)
    gpu_ctx.ldpc_decode(cfg, n_cb, dev(llrs), stride, out, out.shape[1], its)
    torch.cuda.synchronize()
    got_bits = np.unpackbits(out.cpu().numpy()[:, : k // 8], axis=1)
    for i in range(n_cb):
        assert int(its[i]) == want[i][0], i
        assert np.array_equal(got_bits[i], want[i][1]), i
    assert {w[0] for w in want} != {0}, "the batch should hold codeblocks that converge"
    llr0 = llrs[0, :nof_llr]
    for bad in [dict(base_graph=3), dict(lifting_size=17), dict(max_iterations=0), dict(scaling_factor=1.0),
                dict(crc_poly=5), dict(nof_llr=22 * 384), dict(nof_filler_bits=22 * 384)]:
        c = abi.LdpcDecoderCfg(bg, zc, filler, crc_id, nof_llr, 6, 0.8)
        for name, value in bad.items():
            setattr(c, name, value)
        packed = np.zeros(k // 8, np.uint8)
        rc = gpu_ctx.lib.nrphy_ldpc_decode_host(gpu_ctx.handle, C.byref(c), llr0.ctypes.data, packed.ctypes.data, None)
        assert rc == abi.ERR_ARGUMENT, bad


def test_ldpc_decoder_scratch_pool_streams_and_graph(gpu_ctx, oracle):
    """The decoder's messages per edge live in a caller-owned pool that stops growing with the batch: a batch far larger than
    the pool (workgroups claim and release slots), two decodes in flight on two streams with a scratch each, and a decode
    captured in a hipGraph after nrphy_ldpc_decoder_prepare -- all bit-exact against the oracle."""
    import torch
    bg, zc, filler, crc_id = 2, 32, 8, 0x24B
    nof_llr = 50 * zc
    rng = np.random.default_rng(99)
    base = 40
    llr_base, want = [], []
    for i in range(base):
        _, llr = cases.make_ldpc_llrs(oracle, rng, bg, zc, nof_llr, crc_id, filler, 20, 7 + i % 5)
        llr_base.append(llr)
        want.append(oracle.ldpc_decode(bg, zc, filler, crc_id, 5, 0.8, llr))
    cfg = abi.LdpcDecoderCfg(bg, zc, filler, crc_id, nof_llr, 5, 0.8)
    n_cb = 20000
    pool = gpu_ctx.ldpc_decoder_scratch_bytes(cfg, n_cb)
    assert pool < gpu_ctx.ldpc_decoder_scratch_bytes(cfg, 1) * n_cb // 2, "the pool does not grow with the batch"
    llrs = np.stack([llr_base[i % base] for i in range(n_cb)])
    k = 10 * zc
    d_llr = dev(llrs)
    outs = [torch.zeros((n_cb, k // 8), dtype=torch.uint8, device="cuda") for _ in range(2)]
    its = [torch.full((n_cb,), 77, dtype=torch.int32, device="cuda") for _ in range(2)]
    scratch = [torch.empty(pool, dtype=torch.uint8, device="cuda") for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    assert gpu_ctx.lib.nrphy_ldpc_decoder_prepare(gpu_ctx.handle, C.byref(cfg)) == 0
    torch.cuda.synchronize()
    for q in range(2):
        gpu_ctx.ldpc_decode(cfg, n_cb, d_llr, nof_llr, outs[q], k // 8, its[q], stream=streams[q].cuda_stream, d_scratch=scratch[q])
    torch.cuda.synchronize()
    for q in range(2):
        got_its = its[q].cpu().numpy()
        got_bits = np.unpackbits(outs[q].cpu().numpy(), axis=1)
        for i in list(range(0, n_cb, 397)) + [n_cb - 1]:
            assert got_its[i] == want[i % base][0] and np.array_equal(got_bits[i], want[i % base][1]), (q, i)
        assert np.array_equal(got_its, np.array([want[i % base][0] for i in range(n_cb)], np.int32))
    # captured: the call neither allocates nor synchronises once the configuration is prepared
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    outs[0].zero_()
    its[0].fill_(55)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        gpu_ctx.ldpc_decode(cfg, n_cb, d_llr, nof_llr, outs[0], k // 8, its[0], stream=torch.cuda.current_stream().cuda_stream,
                            d_scratch=scratch[0])
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(its[0].cpu().numpy(), np.array([want[i % base][0] for i in range(n_cb)], np.int32))


def test_ldpc_encode_decode_round_trip_full_size(gpu_ctx, oracle):
    """Size-independent property at the config-3 shape: every codeblock the GPU encoder produces, with errors inside the
    code's reach, decodes back to its message (encode -> corrupt -> decode)."""
    import torch
    bg, zc, n_cb = 1, 384, 104
    k, e = 22 * zc, 8960
    rng = np.random.default_rng(31)
    msgs = rng.integers(0, 2, (n_cb, k), dtype=np.uint8)
    msgs[:, k - 72:] = 0
    for i in range(n_cb):
        crc = oracle.crc_bits(0x24B, msgs[i, : k - 72 - 24])
        msgs[i, k - 96: k - 72] = [(crc >> (23 - b)) & 1 for b in range(24)]
    d_msg = dev(np.packbits(msgs, axis=1))
    d_cb = torch.zeros((n_cb, (e + 7) // 8), dtype=torch.uint8, device="cuda")
    gpu_ctx.ldpc_encode(bg, zc, d_msg, d_msg.shape[1], e, d_cb, d_cb.shape[1], n_cb)
    torch.cuda.synchronize()
    bits = np.unpackbits(d_cb.cpu().numpy(), axis=1)[:, :e].astype(np.float64)
    llr = (1.0 - 2.0 * bits) * 24 + rng.normal(0.0, 9.0, bits.shape)
    llr = np.clip(np.rint(llr), -120, 120).astype(np.int8)
    assert np.count_nonzero((llr < 0) != (bits > 0)) > 100, "the channel should flip some bits"
    # the rate dematcher hands over the whole circular buffer: what was not transmitted is zero
    nof_llr = 66 * zc
    llr = np.concatenate([llr, np.zeros((n_cb, nof_llr - e), np.int8)], axis=1)
    out = torch.zeros((n_cb, k // 8), dtype=torch.uint8, device="cuda")
    its = torch.zeros((n_cb,), dtype=torch.int32, device="cuda")
    cfg = abi.LdpcDecoderCfg(bg, zc, 72, 0x24B, nof_llr, 10, 0.8)
    gpu_ctx.ldpc_decode(cfg, n_cb, dev(llr), nof_llr, out, k // 8, its)
    torch.cuda.synchronize()
    assert int(its.min()) >= 1
    assert np.array_equal(np.unpackbits(out.cpu().numpy(), axis=1)[:, : k - 72], msgs[:, : k - 72])


# ---------------------------------------------------------------------------------------------------------------------
# LDPC rate dematcher ("next" row, receive side): bit-exact soft buffers against the oracle (pinned to the reference's
# generic implementation in tests/test_oracle.py), new data and HARQ combining
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.LDPC_DEMATCH_CASES)
def test_ldpc_rate_dematcher_vs_oracle(gpu_ctx, oracle, case):
    bg, zc, e, rv, qm, nref, nf = case
    rng = np.random.default_rng(e * 7 + rv)
    n = (66 if bg == 1 else 50) * zc
    llr = rng.integers(-127, 128, e).astype(np.int8)
    llr[rng.integers(0, e, e // 10)] = 0
    old = rng.integers(-127, 128, n).astype(np.int8)
    for new_data in (1, 0):
        want = oracle.ldpc_rate_dematch(bg, zc, rv, qm, nref, nf, new_data, llr, old)
        got = gpu_ctx.ldpc_rate_dematch_host(bg, zc, rv, qm, nref, nf, new_data, llr, old)
        assert np.array_equal(got, want), (new_data, int(np.count_nonzero(got != want)))
    # a second transmission on top of the first (rv cycling as HARQ does)
    soft = gpu_ctx.ldpc_rate_dematch_host(bg, zc, rv, qm, nref, nf, 1, llr, old)
    want = oracle.ldpc_rate_dematch(bg, zc, rv, qm, nref, nf, 1, llr, old)
    for rv2 in (2, 3, 1):
        llr2 = rng.integers(-120, 121, e).astype(np.int8)
        soft = gpu_ctx.ldpc_rate_dematch_host(bg, zc, rv2, qm, nref, nf, 0, llr2, soft)
        want = oracle.ldpc_rate_dematch(bg, zc, rv2, qm, nref, nf, 0, llr2, want)
        assert np.array_equal(soft, want), rv2


def test_ldpc_rate_dematch_then_decode_batch(gpu_ctx, oracle):
    """The receive chain on a config-3 slot resident in HBM: 104 codeblocks rate matched by the oracle, noisy LLRs, GPU rate
    dematcher into soft buffers with a padded stride, GPU decoder on the soft buffers; every codeblock comes back."""
    import torch
    pdu, nof_ports, nof_subc, _ = cases.baseline_config(3)
    d = oracle.derive(pdu)
    bg, zc, nf, n_cb = 1, d["lifting_size"], d["nof_filler_bits"], 8
    e, k, n = d["rm_length_short"], 22 * d["lifting_size"], 66 * d["lifting_size"]
    rng = np.random.default_rng(17)
    msgs, llrs = [], np.zeros((n_cb, e + 32), np.int8)
    for i in range(n_cb):
        payload = rng.integers(0, 2, k - nf - 24, dtype=np.uint8)
        crc = oracle.crc_bits(0x24B, payload)
        msg = np.concatenate([payload, [(crc >> (23 - b)) & 1 for b in range(24)], np.zeros(nf, np.uint8)]).astype(np.uint8)
        cb = oracle.ldpc_encode(bg, zc, np.packbits(msg), n)
        rm = np.unpackbits(oracle.rate_match(bg, zc, 0, 8, 0, nf, cb, e))[:e]
        llrs[i, :e] = np.clip(np.rint((1.0 - 2.0 * rm) * 24 + rng.normal(0, 8.0, e)), -120, 120).astype(np.int8)
        msgs.append(msg)
    stride = n + 64
    soft = torch.full((n_cb, stride), 55, dtype=torch.int8, device="cuda")
    dcfg = abi.LdpcRateDematcherCfg(bg, zc, 0, 8, 0, nf, e)
    gpu_ctx.ldpc_rate_dematch(dcfg, n_cb, dev(llrs), llrs.shape[1], soft, stride, True)
    torch.cuda.synchronize()
    soft_host = soft.cpu().numpy()
    for i in range(n_cb):
        want = oracle.ldpc_rate_dematch(bg, zc, 0, 8, 0, nf, 1, llrs[i, :e], np.full(n, 55, np.int8))
        assert np.array_equal(soft_host[i, :n], want), i
    assert np.all(soft_host[:, n:] == 55), "nothing beyond a codeblock's soft buffer may be written"
    out = torch.zeros((n_cb, k // 8), dtype=torch.uint8, device="cuda")
    its = torch.zeros((n_cb,), dtype=torch.int32, device="cuda")
    gpu_ctx.ldpc_decode(abi.LdpcDecoderCfg(bg, zc, nf, 0x24B, n, 8, 0.8), n_cb, soft, stride, out, k // 8, its)
    torch.cuda.synchronize()
    bits = np.unpackbits(out.cpu().numpy(), axis=1)
    for i in range(n_cb):
        it_o, bits_o = oracle.ldpc_decode(bg, zc, nf, 0x24B, 8, 0.8, soft_host[i, :n])
        assert int(its[i]) == it_o >= 1 and np.array_equal(bits[i], bits_o)
        assert np.array_equal(bits[i, : k - nf], msgs[i][: k - nf])


def test_pusch_decode_codeblock_host_harq(gpu_ctx, oracle):
    """The per-codeblock accelerator operation (rate dematcher + decoder, host spans): a first transmission too noisy
    to decode, then retransmissions with other redundancy versions combined into the same soft buffer until the CRC
    passes -- every step bit-exact with the oracle's dematcher and decoder run one after the other."""
    rng = np.random.default_rng(909)
    for bg, zc, qm, e, nf, crc_id in ((1, 384, 8, 8960, 72, 0x24B), (2, 144, 2, 2000, 104, 16), (1, 64, 4, 1800, 0, 0x24A)):
        kb, n = (22, 66 * zc) if bg == 1 else (10, 50 * zc)
        k = kb * zc
        crc_len = 16 if crc_id == 16 else 24
        payload = rng.integers(0, 2, k - nf - crc_len, dtype=np.uint8)
        crc = oracle.crc_bits(crc_id, payload)
        msg = np.concatenate([payload, [(crc >> (crc_len - 1 - i)) & 1 for i in range(crc_len)],
                              np.zeros(nf, np.uint8)]).astype(np.uint8)
        cb = oracle.ldpc_encode(bg, zc, np.packbits(msg), n)
        soft_gpu = rng.integers(-120, 121, n).astype(np.int8)  # stale content: rv 0 as new data rebuilds the whole buffer
        soft_cpu = soft_gpu.copy()
        decoded = False
        for tx, rv in enumerate((0, 2, 3, 1)):
            tx_bits = np.unpackbits(oracle.rate_match(bg, zc, rv, qm, 0, nf, cb, e))[:e]
            llr = np.clip(np.rint((1.0 - 2.0 * tx_bits) * 8 + rng.normal(0, 7.0, e)), -120, 120).astype(np.int8)
            soft_cpu = oracle.ldpc_rate_dematch(bg, zc, rv, qm, 0, nf, tx == 0, llr, soft_cpu)
            it_o, bits_o = oracle.ldpc_decode(bg, zc, nf, crc_id, 6, 0.8, soft_cpu)
            it_g, bits_g, soft_gpu = gpu_ctx.pusch_decode_codeblock_host(bg, zc, rv, qm, 0, nf, crc_id, 6, 0.8, tx == 0,
                                                                        llr, soft_gpu)
            assert np.array_equal(soft_gpu, soft_cpu), (zc, tx)
            assert it_g == it_o and np.array_equal(bits_g, bits_o), (zc, tx)
            if it_g:
                assert np.array_equal(bits_g[: k - nf], msg[: k - nf])
                decoded = True
                break
        assert decoded, "HARQ combining of four transmissions should decode (%d, %d)" % (bg, zc)


def test_device_entry_points_in_a_hip_graph(gpu_ctx, oracle):
    """nrphy_pdsch_run / nrphy_ofdm_run neither allocate nor synchronise, so a step can be captured in a hipGraph and
    replayed on new transport blocks (two runs of the plan per graph here)."""
    import torch
    pdu, nof_ports, nof_subc, ocfg = cases.baseline_config(2)
    slots = 3
    pdus = [cases.baseline_config(2, slot_index=i)[0] for i in range(slots)]
    tb_bytes = (pdu.tb_size_bytes + 3) & ~3
    plan = lib.PdschPlan(gpu_ctx, pdus, [i * tb_bytes for i in range(slots)], list(range(slots)), slots, nof_ports, nof_subc)
    oplan = lib.OfdmPlan(gpu_ctx, ocfg, nof_ports)
    d_tb = [torch.zeros(slots * tb_bytes, dtype=torch.uint8, device="cuda") for _ in range(2)]
    d_grid = [torch.zeros((slots, nof_ports, 14, nof_subc), dtype=torch.int32, device="cuda") for _ in range(2)]
    d_iq = [torch.zeros((slots, nof_ports, oplan.slot_stride, 2), dtype=torch.float32, device="cuda") for _ in range(2)]
    d_slot = dev(np.zeros(slots, np.int32))
    rng = np.random.default_rng(5150)

    def two_steps(stream):
        for k in range(2):
            plan.run(d_tb[k], d_grid[k], zero_grids=True, stream=stream)
            oplan.run(slots, d_grid[k], d_iq[k], d_slot_index=d_slot, stream=stream)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        two_steps(s.cuda_stream)   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        two_steps(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for _ in range(3):
        tbs = []
        for k in range(2):
            h = np.zeros(slots * tb_bytes, np.uint8)
            for i in range(slots):
                h[i * tb_bytes: i * tb_bytes + pdu.tb_size_bytes] = cases.random_tb(rng, pdu)
            d_tb[k].copy_(torch.from_numpy(h))
            tbs.append(h)
        graph.replay()
        torch.cuda.synchronize()
        for k in range(2):
            for i in (0, slots - 1):
                grid = d_grid[k][i].cpu().numpy().view(np.uint16).reshape(nof_ports, 14, nof_subc, 2)
                tb = tbs[k][i * tb_bytes: i * tb_bytes + pdu.tb_size_bytes]
                assert np.array_equal(grid, oracle.pdsch_process(pdus[i], tb, nof_ports, nof_subc)), (k, i)
                iq = d_iq[k][i].cpu().numpy().view(np.complex64).reshape(nof_ports, -1)
                want = oracle.ofdm_slot(ocfg, grid, 0)
                assert rel_err(iq[:, : want.shape[1]], want) < 1e-5
    plan.close()
    oplan.close()


def test_mixed_modulation_batch_takes_bucket_launches_side_by_side(gpu_ctx, oracle):
    """A batch big enough and mixed enough for one codeblock launch per (modulation, layers) bucket: 80 cell-slots of BASELINE
    config 4 (QPSK / 16 / 64 / 256-QAM on 68 PRB each: four buckets, 4,400 work items) plus a few one- and two-layer PDUs in
    grids of their own (more buckets than side streams).  The bucket launches run side by side on streams of the plan, forked
    from and joined to the caller's stream; the run is capturable (the streams exist since plan creation).  Sampled grids
    bit-exact against the oracle, eagerly and from a graph replay on new transport blocks."""
    import torch
    rng = np.random.default_rng(4044)
    pdus, grid_of = [], []
    nof_ports, nof_subc = 4, 273 * 12
    for g in range(80):
        cell, _, _ = cases.mixed_cell(g % 4, slot_index=g % 20)
        pdus += cell
        grid_of += [g] * len(cell)
    w1, w2 = cases.codebook("single_port"), cases.codebook("two_layer_two_ports_0")
    for k, (qm, w) in enumerate(((2, w1), (6, w2), (8, w1))):
        layers = w.shape[2]
        tb_bits = cases.tbs(12, 36, qm, 600, layers, 60)
        pdus.append(abi.make_pdu(slot_index=k, rnti=77 + k, n_id=5, bwp_size_rb=273, qm=qm, dmrs_symbols=(2, 7, 11),
                                 prb_start=10 * k, prb_count=60, nof_symbols=12, base_graph=1, precoding=w,
                                 tb_size_bytes=tb_bits // 8))
        grid_of.append(80 + k)
    nof_grids = 83
    tb_offsets, off = [], 0
    for q in pdus:
        tb_offsets.append(off)
        off += (q.tb_size_bytes + 7) & ~3
    plan = lib.PdschPlan(gpu_ctx, pdus, tb_offsets, grid_of, nof_grids, nof_ports, nof_subc)
    d_tb = torch.zeros(off, dtype=torch.uint8, device="cuda")
    d_grid = torch.zeros((nof_grids, nof_ports, 14, nof_subc), dtype=torch.int32, device="cuda")

    def fresh_blocks():
        h = np.zeros(off, np.uint8)
        for q, o in zip(pdus, tb_offsets):
            h[o: o + q.tb_size_bytes] = cases.random_tb(rng, q)
        d_tb.copy_(torch.from_numpy(h))
        return h

    def check(h, grids):
        for g in grids:
            want = None
            for q, o, gi in zip(pdus, tb_offsets, grid_of):
                if gi == g:
                    part = oracle.pdsch_process(q, h[o: o + q.tb_size_bytes], nof_ports, nof_subc)
                    want = part if want is None else np.bitwise_or(want, part)
            got = d_grid[g].cpu().numpy().view(np.uint16).reshape(want.shape)
            assert np.array_equal(got, want), g

    s = torch.cuda.Stream()
    h = fresh_blocks()
    torch.cuda.synchronize()
    plan.run(d_tb, d_grid, zero_grids=True, stream=s.cuda_stream)
    torch.cuda.synchronize()
    check(h, (0, 37, 79, 80, 81, 82))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        plan.run(d_tb, d_grid, zero_grids=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for _ in range(2):
        h = fresh_blocks()
        d_grid.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check(h, (1, 42, 78, 80, 82))
    plan.close()


def test_single_run_graph_replay_and_eager_interleaved(gpu_ctx, oracle):
    """Every run of a plan is self-contained (no TB-CRC state is carried between runs): a graph holding ONE run -- the
    natural step -- replays correctly any number of times, also with eager runs of the same plan in between."""
    import torch
    pdu, nof_ports, nof_subc, _ = cases.baseline_config(2)
    tb_bytes = (pdu.tb_size_bytes + 3) & ~3
    plan = lib.PdschPlan(gpu_ctx, [pdu], [0], [0], 1, nof_ports, nof_subc)
    d_tb = torch.zeros(tb_bytes, dtype=torch.uint8, device="cuda")
    d_grid = torch.zeros((1, nof_ports, 14, nof_subc), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan.run(d_tb, d_grid, zero_grids=True, stream=s.cuda_stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        plan.run(d_tb, d_grid, zero_grids=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rng = np.random.default_rng(77)
    for k in range(5):
        tb = cases.random_tb(rng, pdu)
        h = np.zeros(tb_bytes, np.uint8)
        h[: tb.size] = tb
        d_tb.copy_(torch.from_numpy(h))
        if k == 3:  # an eager run between two replays
            with torch.cuda.stream(s):
                plan.run(d_tb, d_grid, zero_grids=True, stream=s.cuda_stream)
            torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        grid = d_grid[0].cpu().numpy().view(np.uint16).reshape(nof_ports, 14, nof_subc, 2)
        assert np.array_equal(grid, oracle.pdsch_process(pdu, tb, nof_ports, nof_subc)), k
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# PUSCH decoder at transport-block level ("next" row): segmentation, rate dematching, decoding, concatenation, TB CRC
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["cfg2", "cfg1", "bg2_multi"])
@pytest.mark.parametrize("early_stop", [1, 0])
def test_pusch_decoder_transport_blocks_harq(gpu_ctx, oracle, shape, early_stop):
    """Two transport blocks through the whole receive-side coding chain on the GPU, twice (rv 0 as new data at an SNR
    where some codeblocks fail, then rv 2 combined): soft buffers, codeblock flags, iteration statistics and transport
    blocks against pusch_decoder_impl restated on the oracle; the transmit side is the oracle's PDSCH encoder."""
    import torch
    rng = np.random.default_rng({"cfg2": 21, "cfg1": 22, "bg2_multi": 23}[shape])
    pdu, nof_ports, nof_subc, amp, sigma = cases.pusch_decoder_shape(oracle, shape)
    d = oracle.derive(pdu)
    n_tb, C, n = 2, d["nof_codeblocks"], d["full_length"]
    G = d["codeword_bits"]
    cfgs = [abi.PuschDecoderCfg(pdu.ldpc_base_graph, pdu.qm, rv, pdu.nof_layers, d["n_ref"], pdu.tb_size_bytes,
                                G // pdu.qm, 6, early_stop, 1 if i == 0 else 0) for i, rv in enumerate((0, 2))]
    soft_bytes, state_bytes, ncb = gpu_ctx.pusch_decoder_sizes(cfgs[0], n_tb)
    assert (soft_bytes, ncb) == (C * n, C)
    d_soft = torch.full((n_tb, soft_bytes), 33, dtype=torch.int8, device="cuda")     # stale content on purpose
    d_state = torch.full((state_bytes,), 0x5A, dtype=torch.uint8, device="cuda")
    d_tb = torch.zeros((n_tb, pdu.tb_size_bytes + 5), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((n_tb, 4), dtype=torch.int32, device="cuda")
    tbs = [cases.random_tb(rng, pdu) for _ in range(n_tb)]
    soft = [np.full((C, n), 33, np.int8) for _ in range(n_tb)]
    cb_ok = [np.full(C, 1, np.uint8) for _ in range(n_tb)]     # garbage flags: new data must clear them
    cb_msg = [np.zeros((C, d["segment_length"]), np.uint8) for _ in range(n_tb)]
    stride = G + 13
    seen_partial = False
    for tx, cfg in enumerate(cfgs):
        llrs = np.zeros((n_tb, stride), np.int8)
        for i in range(n_tb):
            pdu.rv = cfg.rv
            _, rm, _ = oracle.pdsch_process(pdu, tbs[i], nof_ports, nof_subc, taps=True, codeword_bits=G)
            bits = np.unpackbits(rm)[:G].astype(np.float64)
            llrs[i, :G] = np.clip(np.rint((1 - 2 * bits) * amp + rng.normal(0, sigma, G)), -120, 120).astype(np.int8)
        pdu.rv = 0
        gpu_ctx.pusch_decode_batch(cfg, n_tb, dev(llrs), stride, d_soft, d_state, d_tb, d_tb.shape[1], d_res)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy()
        got_soft = d_soft.cpu().numpy().reshape(n_tb, C, n)
        for i in range(n_tb):
            tb_ok, n_ok, it_sum, it_max, tb = cases.pusch_decode_expected(oracle, d, cfg, llrs[i, :G], soft[i], cb_ok[i], cb_msg[i])
            assert np.array_equal(got_soft[i], soft[i]), (tx, i)
            assert tuple(res[i]) == (int(tb_ok), n_ok, it_sum, it_max), (tx, i, res[i], (tb_ok, n_ok, it_sum, it_max))
            if tb_ok:
                assert np.array_equal(d_tb[i].cpu().numpy()[: pdu.tb_size_bytes], tb)
                assert np.array_equal(tb, tbs[i])
            seen_partial |= 0 < n_ok < C or (tx == 0 and not tb_ok)
    assert all(int(r[0]) == 1 for r in res), "the retransmission should complete every transport block"
    assert seen_partial, "the first transmission should leave work for the second (pick a lower SNR)"


def test_transmit_receive_loop_full_size(gpu_ctx):
    """Size-independent property at the BASELINE config-3 shape: transport blocks -> GPU PDSCH encoder chain (rate-matched
    codeword tap) -> noisy LLRs -> GPU UL-SCH decoder (rate dematcher, LDPC, concatenation, CRC24A) give the transport
    blocks back, a first transmission that is too noisy included (HARQ retransmission with rv 3 completes it)."""
    import torch
    pdu, nof_ports, nof_subc, _ = cases.baseline_config(3)
    slots = 4
    d = lib.derive(pdu)
    G, tb_size = d["codeword_bits"], pdu.tb_size_bytes
    tb_stride = (tb_size + 3) & ~3
    d_tb = torch.randint(0, 256, (slots, tb_stride), dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(808)
    cfg0 = abi.PuschDecoderCfg(pdu.ldpc_base_graph, pdu.qm, 0, pdu.nof_layers, d["n_ref"], tb_size, G // pdu.qm, 8, 1, 1)
    soft_bytes, state_bytes, _ = gpu_ctx.pusch_decoder_sizes(cfg0, slots)
    d_soft = torch.zeros((slots, soft_bytes), dtype=torch.int8, device="cuda")
    d_state = torch.zeros((state_bytes,), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((slots, tb_stride), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((slots, 4), dtype=torch.int32, device="cuda")
    first_ok = None
    for tx, (rv, sigma) in enumerate(((0, 11.0), (3, 9.0))):
        pdus = []
        for i in range(slots):
            p = cases.baseline_config(3, slot_index=i)[0]
            p.rv = rv
            pdus.append(p)
        plan = lib.PdschPlan(gpu_ctx, pdus, [i * tb_stride for i in range(slots)], list(range(slots)), slots, nof_ports, nof_subc)
        d_cw = torch.zeros((plan.codeword_bits + 7) // 8 + 64, dtype=torch.uint8, device="cuda")
        plan.run(d_tb.reshape(-1), None, d_cw_rm=d_cw)
        gpu_ctx.synchronize()
        cw = d_cw.cpu().numpy()
        offs = [plan.codeword_offset(i) for i in range(slots)]
        bits = np.stack([np.unpackbits(cw[o // 8: o // 8 + (G + 7) // 8])[:G] for o in offs]).astype(np.float32)
        llr = np.clip(np.rint((1 - 2 * bits) * 20 + rng.normal(0, sigma, bits.shape)), -120, 120).astype(np.int8)
        cfg = abi.PuschDecoderCfg(pdu.ldpc_base_graph, pdu.qm, rv, pdu.nof_layers, d["n_ref"], tb_size, G // pdu.qm, 8, 1,
                                  1 if tx == 0 else 0)
        gpu_ctx.pusch_decode_batch(cfg, slots, dev(llr), G, d_soft, d_state, d_out, tb_stride, d_res)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy()
        if tx == 0:
            first_ok = res[:, 0].copy()
        plan.close()
    assert not first_ok.all(), "the first transmission should fail for some transport blocks (raise its noise)"
    assert res[:, 0].all(), res
    assert torch.equal(d_out[:, :tb_size], d_tb[:, :tb_size])


# ---------------------------------------------------------------------------------------------------------------------
# NZP-CSI-RS generator ("next" row, section 8f-2): bit-exact grids against the oracle (pinned to the reference's
# nzp_csi_rs_generator_impl in tests/test_oracle.py)
# ---------------------------------------------------------------------------------------------------------------------
def test_nzp_csi_rs_vs_oracle(gpu_ctx, oracle):
    import torch
    rng = np.random.default_rng(7415)
    batch = []
    for name, cfg, nof_ports, nof_subc in cases.csi_rs_cases(rng):
        assert gpu_ctx.lib.nrphy_csi_rs_validate(C.byref(cfg)) == 0, name
        grid = (rng.standard_normal((nof_ports, 14, nof_subc, 2)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        want = oracle.csi_rs_map(cfg, grid)
        got = gpu_ctx.csi_rs_map_host(cfg, grid)
        assert np.array_equal(got, want), (name, int(np.count_nonzero(got != want)))
        if nof_ports == 4 and nof_subc == 624:
            batch.append((cfg, grid, want))
    # several signals in one call, two of them into the same grid (disjoint symbols), device-resident grids
    assert len(batch) >= 4
    n_grids = len(batch) - 1
    grids = np.stack([b[1] for b in batch[:n_grids]])
    idx = list(range(n_grids)) + [0]
    want0 = oracle.csi_rs_map(batch[-1][0], batch[0][2])
    d_grid = dev(grids.view(np.uint32).reshape(n_grids, 4, 14, 624).view(np.int32))
    gpu_ctx.csi_rs_map([b[0] for b in batch], idx, d_grid, 4, 624)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    got = d_grid.cpu().numpy().view(np.uint16).reshape(n_grids, 4, 14, 624, 2)
    assert np.array_equal(got[0], want0)
    for i in range(1, n_grids):
        assert np.array_equal(got[i], batch[i][2]), i
    # refusals: a row beyond 5, a density the row does not allow, per-PRG precoding
    bad = abi.make_csi_rs(row=4, start_rb=0, nof_rb=52, k0=0, l0=5, density="one")
    bad.density = abi.CSI_DENSITY["three"]
    assert gpu_ctx.lib.nrphy_csi_rs_validate(C.byref(bad)) == abi.ERR_ARGUMENT
    bad = abi.make_csi_rs(row=2, start_rb=0, nof_rb=52, k0=0, l0=5, density="one")
    bad.nof_prg = 2
    assert gpu_ctx.lib.nrphy_csi_rs_validate(C.byref(bad)) == abi.ERR_ARGUMENT
    bad.nof_prg, bad.row = 1, 6
    assert gpu_ctx.lib.nrphy_csi_rs_validate(C.byref(bad)) == abi.ERR_ARGUMENT


# ---------------------------------------------------------------------------------------------------------------------
# Downlink control channels: PDCCH and SS/PBCH block processors on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_pdcch_processor_vs_oracle_and_reference_golden(gpu_ctx, oracle):
    """pdcch_processor::process through the C ABI: the reference's outputs (tests/golden/dl_control.npz), random PDUs
    against the oracle in grids full of other data, the encoder alone, and a batch of DCIs into device-resident grids."""
    import torch
    import test_oracle
    g = np.load(os.path.join(cases.GOLDEN, "dl_control.npz"))
    for i in range(int(g["n_pdcch"])):
        pdu, enc, grid = test_oracle.dl_control_golden("pdcch", i)
        assert gpu_ctx.lib.nrphy_pdcch_validate(C.byref(pdu)) == 0, i
        payload = np.array(list(pdu.payload)[: pdu.payload_size], np.uint8)
        assert np.array_equal(np.packbits(gpu_ctx.pdcch_encode_host(payload, pdu.rnti, 108 * pdu.aggregation_level)), enc), i
        assert np.array_equal(gpu_ctx.pdcch_process_host(pdu, np.zeros_like(grid)), grid), i
    rng = np.random.default_rng(8212)
    batch = []
    for i in range(60):
        pdu = cases.random_pdcch(rng)
        grid = (rng.standard_normal((4, 14, 52 * 12, 2)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        want = oracle.pdcch_process(pdu, grid)
        got = gpu_ctx.pdcch_process_host(pdu, grid)
        assert np.array_equal(got, want), (i, int(np.count_nonzero(got != want)))
        batch.append((pdu, grid, want))
    # 60 DCIs in one call: three per grid (their candidates may overlap: each is checked in a grid of its own below, the
    # shared grids only have to equal the oracle applied in the same order)
    n_grids = 20
    grids = np.stack([b[1] for b in batch[:n_grids]])
    idx = [i % n_grids for i in range(60)]
    want = grids.copy()
    for i, (pdu, _, _) in enumerate(batch):
        want[idx[i]] = oracle.pdcch_process(pdu, want[idx[i]])
    d_grid = dev(grids.view(np.uint32).reshape(n_grids, 4, 14, 624).view(np.int32))
    # candidates of one grid can collide; launch them one grid-set at a time so that the order is the oracle's
    for first in (0, 20, 40):
        gpu_ctx.pdcch_process([b[0] for b in batch[first: first + 20]], idx[first: first + 20], d_grid, 4, 624)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    got = d_grid.cpu().numpy().view(np.uint16).reshape(n_grids, 4, 14, 624, 2)
    assert np.array_equal(got, want)
    # refusals: a payload that leaves no room for the CRC (K >= E), a candidate beyond the CORESET, PRGs that do not
    # cover the allocation, an aggregation level that does not exist
    ok = abi.make_pdcch(payload=np.zeros(40, np.uint8), rnti=1, cce_index=0, aggregation_level=2, duration=2,
                        frequency_resources=(0, 1, 2, 3))
    assert gpu_ctx.lib.nrphy_pdcch_validate(C.byref(ok)) == 0
    for change in (dict(payload=np.zeros(90, np.uint8), aggregation_level=1), dict(cce_index=7), dict(aggregation_level=3),
                   dict(prg_size_rb=4), dict(duration=4)):
        kw = dict(payload=np.zeros(40, np.uint8), rnti=1, cce_index=0, aggregation_level=2, duration=2, frequency_resources=(0, 1, 2, 3))
        kw.update(change)
        bad = abi.make_pdcch(**kw)
        assert gpu_ctx.lib.nrphy_pdcch_validate(C.byref(bad)) == abi.ERR_INVALID_PDU, change
        assert oracle.pdcch_validate(bad) == abi.ERR_INVALID_PDU, change


def test_ssb_processor_vs_oracle_and_reference_golden(gpu_ctx, oracle):
    """ssb_processor::process through the C ABI: reference outputs, random blocks (cases A-C, both half frames, several
    ports) and case D with L_max = 64 against the oracle, the PBCH encoder alone, a batch into device grids."""
    import torch
    import test_oracle
    g = np.load(os.path.join(cases.GOLDEN, "dl_control.npz"))
    for i in range(int(g["n_ssb"])):
        pdu, enc, grid = test_oracle.dl_control_golden("ssb", i)
        assert np.array_equal(np.packbits(gpu_ctx.pbch_encode_host(pdu)), enc), i
        assert np.array_equal(gpu_ctx.ssb_process_host(pdu, np.zeros_like(grid)), grid), i
    rng = np.random.default_rng(8213)
    batch = []
    for i in range(40):
        pdu = cases.random_ssb(rng, nof_ports=3)
        grid = (rng.standard_normal((3, 14, 52 * 12, 2)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        want = oracle.ssb_process(pdu, grid)
        assert np.array_equal(gpu_ctx.pbch_encode_host(pdu), oracle.pbch_encode(pdu)), i
        got = gpu_ctx.ssb_process_host(pdu, grid)
        assert np.array_equal(got, want), (i, int(np.count_nonzero(got != want)))
        batch.append((pdu, grid, want))
    groups = (0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12, 13, 15, 16, 17, 18)
    for idx in (0, 13, 37, 63):
        first = (4, 8, 16, 20)[idx % 4] + 28 * groups[idx // 4]
        pdu = abi.make_ssb(pattern_case="D", ssb_idx=idx, L_max=64, phys_cell_id=777, payload=rng.integers(0, 2, 32, dtype=np.uint8),
                           sfn=1000 + idx % 20, numerology=3, slot_index=first // 14, common_scs=3, subcarrier_offset=5,
                           offset_to_pointA=4, ports=(1,))
        grid = np.zeros((2, 14, 52 * 12, 2), np.uint16)
        assert np.array_equal(gpu_ctx.ssb_process_host(pdu, grid), oracle.ssb_process(pdu, grid)), idx
    grids = np.stack([b[1] for b in batch])
    d_grid = dev(grids.view(np.uint32).reshape(len(batch), 3, 14, 624).view(np.int32))
    gpu_ctx.ssb_process([b[0] for b in batch], list(range(len(batch))), d_grid, 3, 624)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    got = d_grid.cpu().numpy().view(np.uint16).reshape(len(batch), 3, 14, 624, 2)
    for i, b in enumerate(batch):
        assert np.array_equal(got[i], b[2]), i
    # refusals: a slot that does not hold the candidate, a port beyond the grid, a block beyond the grid
    pdu = cases.random_ssb(rng, nof_ports=2)
    pdu.slot_index = (pdu.slot_index + 1) % (10 << pdu.numerology)
    assert gpu_ctx.lib.nrphy_ssb_validate(C.byref(pdu)) == abi.ERR_INVALID_PDU and oracle.ssb_validate(pdu) == abi.ERR_INVALID_PDU
    pdu = cases.random_ssb(rng, nof_ports=3)
    with pytest.raises(lib.NrphyError):
        gpu_ctx.ssb_process_host(pdu, np.zeros((1, 14, 18 * 12, 2), np.uint16))


def test_whole_downlink_slot_in_one_device_grid(gpu_ctx, oracle):
    """Every downlink grid writer of a slot on the device, in the order the reference's downlink processor applies them
    (PDCCH, PDSCH with its DM-RS, SS/PBCH block, NZP-CSI-RS): the grid in HBM equals the oracle's grid and the OFDM
    modulator turns it into IQ without the grid ever visiting the host."""
    import torch
    rng = np.random.default_rng(2718)
    nof_ports, nof_rb = 2, 52
    nof_subc = 12 * nof_rb
    w2 = cases.codebook("two_layer_two_ports_0")
    # PDSCH on symbols 2-13 of PRBs 22-51 (below it the SS/PBCH block: PRBs 0-19 on symbols 2-5; PDCCH on symbols 0-1)
    tbs = lib.tbs_calculate(12, 12, 0, 4, 490, 2, 30)
    pdsch = abi.make_pdu(bwp_size_rb=nof_rb, qm=4, rnti=17, n_id=5, dmrs_symbols=(2, 11), prb_start=22, prb_count=30,
                         start_symbol=2, nof_symbols=12, precoding=w2, tb_size_bytes=tbs // 8, slot_index=0)
    tb = cases.random_tb(rng, pdsch)
    pdcch = [abi.make_pdcch(payload=rng.integers(0, 2, 41, dtype=np.uint8), rnti=17, cce_index=0, aggregation_level=4, duration=2,
                            frequency_resources=tuple(range(8)), mapping="interleaved", reg_bundle_size=6, interleaver_size=2,
                            shift_index=3, n_id_dmrs=5, n_id_data=5, n_rnti=17, bwp_size_rb=nof_rb,
                            precoding=np.array([[1.0, 1.0j]], np.complex64) / np.sqrt(2)),
             abi.make_pdcch(payload=rng.integers(0, 2, 39, dtype=np.uint8), rnti=0xFFFF, cce_index=4, aggregation_level=4, duration=2,
                            frequency_resources=tuple(range(8)), mapping="interleaved", reg_bundle_size=6, interleaver_size=2,
                            shift_index=3, n_id_dmrs=5, n_id_data=5, bwp_size_rb=nof_rb)]
    ssb = abi.make_ssb(pattern_case="A", ssb_idx=0, L_max=4, phys_cell_id=5, payload=rng.integers(0, 2, 32, dtype=np.uint8),
                       sfn=100, ports=(0,))
    csi = abi.make_csi_rs(row=3, start_rb=0, nof_rb=nof_rb, k0=4, l0=13, density="one", scrambling_id=5,
                          precoding=np.eye(2, dtype=np.complex64)[None])
    # expected: the oracle's writers applied in the same order to one grid
    want = np.zeros((nof_ports, 14, nof_subc, 2), np.uint16)
    for p in pdcch:
        want = oracle.pdcch_process(p, want)
    pg = oracle.pdsch_process(pdsch, tb, nof_ports, nof_subc)
    mask = pg.view(np.uint32) != 0
    want.view(np.uint32)[mask] = pg.view(np.uint32)[mask]
    want = oracle.ssb_process(ssb, want)
    want = oracle.csi_rs_map(csi, want)
    # device: PDSCH plan (zero-fills everything it does not map), then the other writers on the same stream
    tb_bytes = (pdsch.tb_size_bytes + 3) & ~3
    h = np.zeros(tb_bytes, np.uint8)
    h[: tb.size] = tb
    d_tb = dev(h)
    d_grid = torch.full((1, nof_ports, 14, nof_subc), -1, dtype=torch.int32, device="cuda")
    plan = lib.PdschPlan(gpu_ctx, [pdsch], [0], [0], 1, nof_ports, nof_subc)
    torch.cuda.synchronize()
    plan.run(d_tb, d_grid, zero_grids=True)
    gpu_ctx.pdcch_process(pdcch[:1], [0], d_grid, nof_ports, nof_subc)
    gpu_ctx.pdcch_process(pdcch[1:], [0], d_grid, nof_ports, nof_subc)
    gpu_ctx.ssb_process([ssb], [0], d_grid, nof_ports, nof_subc)
    gpu_ctx.csi_rs_map([csi], [0], d_grid, nof_ports, nof_subc)
    ocfg = abi.OfdmConfig(0, nof_rb, 1024, 0, 1.0 / np.sqrt(1024), 2.4e9)
    oplan = lib.OfdmPlan(gpu_ctx, ocfg, nof_ports)
    d_iq = torch.zeros((1, nof_ports, oplan.slot_stride, 2), dtype=torch.float32, device="cuda")
    oplan.run(1, d_grid, d_iq)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    got = d_grid[0].cpu().numpy().view(np.uint16).reshape(nof_ports, 14, nof_subc, 2)
    assert np.array_equal(got, want), int(np.count_nonzero(got != want))
    iq = d_iq[0].cpu().numpy().view(np.complex64).reshape(nof_ports, -1)
    assert rel_err(iq, oracle.ofdm_slot(ocfg, want, 0)) < 1e-5
    plan.close()
    oplan.close()


# ---------------------------------------------------------------------------------------------------------------------
# The downlink slot pipeline (nrphy_dl_slots_*): seams A and C on one device-resident grid, the slot modulated at grid
# hand-over (pdxch_processor_impl.cpp:97-112), IQ served from pinned memory (process_symbol, :47-95)
# ---------------------------------------------------------------------------------------------------------------------
def _slot_writers(rng, nof_rb):
    """The PDUs of test_whole_downlink_slot_in_one_device_grid: PDCCH x 2, PDSCH, SS/PBCH block, CSI-RS."""
    w2 = cases.codebook("two_layer_two_ports_0")
    tbs = lib.tbs_calculate(12, 12, 0, 4, 490, 2, 30)
    pdsch = abi.make_pdu(bwp_size_rb=nof_rb, qm=4, rnti=17, n_id=5, dmrs_symbols=(2, 11), prb_start=22, prb_count=30,
                         start_symbol=2, nof_symbols=12, precoding=w2, tb_size_bytes=tbs // 8, slot_index=0)
    tb = cases.random_tb(rng, pdsch)
    pdcch = [abi.make_pdcch(payload=rng.integers(0, 2, 41, dtype=np.uint8), rnti=17, cce_index=0, aggregation_level=4, duration=2,
                            frequency_resources=tuple(range(8)), mapping="interleaved", reg_bundle_size=6, interleaver_size=2,
                            shift_index=3, n_id_dmrs=5, n_id_data=5, n_rnti=17, bwp_size_rb=nof_rb,
                            precoding=np.array([[1.0, 1.0j]], np.complex64) / np.sqrt(2)),
             abi.make_pdcch(payload=rng.integers(0, 2, 39, dtype=np.uint8), rnti=0xFFFF, cce_index=4, aggregation_level=4, duration=2,
                            frequency_resources=tuple(range(8)), mapping="interleaved", reg_bundle_size=6, interleaver_size=2,
                            shift_index=3, n_id_dmrs=5, n_id_data=5, bwp_size_rb=nof_rb)]
    ssb = abi.make_ssb(pattern_case="A", ssb_idx=0, L_max=4, phys_cell_id=5, payload=rng.integers(0, 2, 32, dtype=np.uint8),
                       sfn=100, ports=(0,))
    csi = abi.make_csi_rs(row=3, start_rb=0, nof_rb=nof_rb, k0=4, l0=13, density="one", scrambling_id=5,
                          precoding=np.eye(2, dtype=np.complex64)[None])
    return pdsch, tb, pdcch, ssb, csi


def _merge(want, part):
    mask = part.view(np.uint32) != 0
    want.view(np.uint32)[mask] = part.view(np.uint32)[mask]
    return want


@pytest.mark.parametrize("first", ["pdcch", "pdsch", "pdsch-zero-copy"])
def test_dl_slot_pipeline_whole_slot_tb_to_iq(gpu_ctx, oracle, monkeypatch, first):
    """Every grid writer of a slot through nrphy_dl_slot_* into the slot's device grid, the grid handed over with
    nrphy_dl_slot_modulate, IQ read from the slot's pinned buffer: grid bit-exact (read back only to check), IQ <= 1e-5, the
    completion handler called once from another thread, poll / wait / iq as process_symbol uses them.  `first` = which writer
    meets the still undefined grid (a PDSCH run clears what it does not map itself, the others need the memset)."""
    import threading
    if first == "pdsch-zero-copy":   # (NRPHY_DL_SLOT_ZERO_COPY=3: no copy down, no copy up; read when the pool is created)
        monkeypatch.setenv("NRPHY_DL_SLOT_ZERO_COPY", "3")
    rng = np.random.default_rng(2718)
    nof_ports, nof_rb = 2, 52
    nof_subc = 12 * nof_rb
    pdsch, tb, pdcch, ssb, csi = _slot_writers(rng, nof_rb)
    ocfg = abi.OfdmConfig(0, nof_rb, 1024, 0, 1.0 / np.sqrt(1024), 2.4e9)
    pool = lib.DlSlotPool(gpu_ctx, ocfg, nof_ports, 2, 65536)
    want = np.zeros((nof_ports, 14, nof_subc, 2), np.uint16)
    sid = pool.open()
    assert sid is not None and pool.poll(sid) == abi.ERR_NOT_READY
    if first == "pdcch":
        pool.pdcch(sid, pdcch)
        for p in pdcch:
            want = oracle.pdcch_process(p, want)
    assert pool.pdsch(sid, [pdsch], [tb]) == 0
    want = _merge(want, oracle.pdsch_process(pdsch, tb, nof_ports, nof_subc))
    if first != "pdcch":
        pool.pdcch(sid, pdcch[:1])
        pool.pdcch(sid, pdcch[1:])
        for p in pdcch:
            want = oracle.pdcch_process(p, want)
    pool.ssb(sid, [ssb])
    want = oracle.ssb_process(ssb, want)
    pool.csi_rs(sid, [csi])
    want = oracle.csi_rs_map(csi, want)
    # a channel the library does not generate, merged from the host as sparse resource elements
    entries = [abi.GridRe(1, 0, 600 + k, 0x3F800000 + k) for k in range(7)]
    pool.put(sid, entries)
    for e in entries:
        want.view(np.uint32).reshape(nof_ports, 14, nof_subc)[e.port, e.symbol, e.subc] = e.value
    calls, me, called = [], threading.get_ident(), threading.Event()

    def on_done(status, slot_id):
        calls.append((status, slot_id, threading.get_ident()))
        called.set()

    assert pool.modulate(sid, 0, on_done) == 0
    assert pool.modulate(sid, 0) == abi.ERR_ARGUMENT            # once per open
    assert pool.pdsch(sid, [pdsch], [tb]) == abi.ERR_ARGUMENT   # the grid has been handed over
    assert pool.wait(sid) == 0 and pool.poll(sid) == 0
    # The runtime thread marks the slot done, then runs the handler, which needs the GIL this thread holds once wait()
    # returns: the handler may still be on its way (the ABI orders it after the IQ copy, not before wait's return).
    assert called.wait(10.0)
    assert len(calls) == 1 and calls[0][:2] == (0, sid) and calls[0][2] != me
    want_iq = oracle.ofdm_slot(ocfg, want, 0)
    for port in range(nof_ports):
        assert rel_err(pool.iq(sid, port), want_iq[port]) < 1e-5
    assert np.array_equal(pool.read_grid(sid), want)
    pool.close(sid)
    assert pool.poll(sid) == abi.ERR_ARGUMENT
    assert len(calls) == 1   # once, also after close
    pool.destroy()


def test_dl_slot_pipeline_slots_in_flight_and_host_grids(gpu_ctx, oracle):
    """Several slots open at once, BASELINE config 3's PDU in each with another transport block, slot index and RNTI; PDSCH
    arriving PDU by PDU in two calls per slot; capacity statuses; a slot reused after close starts from zeros; and seam C
    alone: a grid computed elsewhere loaded from a host span (nrphy_dl_slot_load_grid) and an untouched slot (silence)."""
    rng = np.random.default_rng(4242)
    pdu0, nof_ports, nof_subc, ocfg = cases.baseline_config(3)
    depth = 3
    # two PDUs per slot: the upper and the lower half of config 3's allocation, submitted in separate calls
    def half(lo, count, rnti, slot_index):
        tbs = cases.tbs(12, 36, 8, 948, 4, count)
        return abi.make_pdu(bwp_size_rb=273, qm=8, rnti=rnti, n_id=7, dmrs_symbols=(2, 7, 11), prb_start=lo, prb_count=count,
                            start_symbol=0, nof_symbols=12, precoding=cases.codebook("four_layer_four_ports_0_0"),
                            tb_size_bytes=tbs // 8, slot_index=slot_index, nof_cdm_groups_without_data=2)
    jobs, ids = [], []
    for k in range(depth):
        a, b = half(0, 130, 100 + k, k), half(130, 140, 200 + k, k)
        jobs.append(((a, cases.random_tb(rng, a)), (b, cases.random_tb(rng, b))))
    pool = lib.DlSlotPool(gpu_ctx, ocfg, nof_ports, depth, jobs[0][0][0].tb_size_bytes + jobs[0][1][0].tb_size_bytes + 16)
    for k in range(depth):
        sid = pool.open()
        assert sid is not None
        ids.append(sid)
    assert pool.open() is None                                  # all `depth` slots are open
    for k, sid in enumerate(ids):                               # interleaved across the slots, as concurrent slots would be
        assert pool.pdsch(sid, [jobs[k][0][0]], [jobs[k][0][1]]) == 0
    for k, sid in enumerate(ids):
        assert pool.pdsch(sid, [jobs[k][1][0]], [jobs[k][1][1]]) == 0
        assert pool.modulate(sid, k % 2) == 0
    big = half(0, 270, 9, 0)
    for k, sid in enumerate(ids):
        assert pool.wait(sid) == 0
        want = np.zeros((nof_ports, 14, nof_subc, 2), np.uint16)
        for pdu, tb in jobs[k]:
            want = _merge(want, oracle.pdsch_process(pdu, tb, nof_ports, nof_subc))
        assert np.array_equal(pool.read_grid(sid), want), k
        want_iq = oracle.ofdm_slot(ocfg, want, k % 2)
        for port in range(nof_ports):
            got = pool.iq(sid, port)
            assert got.size == lib.slot_size(ocfg, k % 2) and rel_err(got, want_iq[port]) < 1e-5
        pool.close(sid)
    # reuse: nothing of the previous slot is left; more transport-block bytes than the slot holds are refused
    sid = pool.open()
    assert pool.pdsch(sid, [jobs[0][0][0]], [jobs[0][0][1]]) == 0
    assert pool.pdsch(sid, [big], [cases.random_tb(rng, big)]) == abi.ERR_CAPACITY
    want = oracle.pdsch_process(jobs[0][0][0], jobs[0][0][1], nof_ports, nof_subc)
    assert np.array_equal(pool.read_grid(sid), want)
    pool.close(sid)
    # seam C alone: a host grid, and an untouched slot
    grid = ((rng.standard_normal((nof_ports, 14, nof_subc, 2)) * 0.5).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    a, b = pool.open(), pool.open()
    pool.load_grid(a, grid)
    assert pool.modulate(a, 1) == 0 and pool.modulate(b, 0) == 0
    assert pool.wait(a) == 0 and pool.wait(b) == 0
    want_iq = oracle.ofdm_slot(ocfg, grid, 1)
    for port in range(nof_ports):
        assert rel_err(pool.iq(a, port), want_iq[port]) < 1e-5
        assert not pool.iq(b, port).any()
    pool.close(a)
    pool.close(b)
    pool.destroy()


def test_dl_slot_pdsch_after_other_writers_touches_only_its_own_elements(gpu_ctx, oracle):
    """A PDSCH run that is not the slot's first writer (zero_grids = 0) behaves like the reference's mapper: it writes the PDU's data
    and pilot elements and nothing else.  One layer with two CDM groups without data: the elements of the reserved, pilot-less group
    in the DM-RS symbols keep what the slot held before -- the DM-RS waves used to clear them whatever the run was told (found by the
    slot-pipeline leg of the device sweep in round 4: a PDCCH under a DM-RS symbol lost a few elements)."""
    import ctypes as C
    rng = np.random.default_rng(6006)
    nof_ports, nof_rb = 2, 52
    nof_subc = 12 * nof_rb
    ocfg = abi.OfdmConfig(0, nof_rb, 1024, 0, 1.0, 2.4e9)
    pool = lib.DlSlotPool(gpu_ctx, ocfg, nof_ports, 1, 65536)
    for layers, groups in ((1, 2), (2, 2), (1, 1)):
        w = (rng.standard_normal((1, nof_ports, layers)) + 1j * rng.standard_normal((1, nof_ports, layers))).astype(np.complex64) / 2
        tbs = cases.tbs(12, 6 * groups * 2, 4, 490, layers, 30)
        pdu = abi.make_pdu(bwp_size_rb=nof_rb, qm=4, rnti=23, n_id=9, dmrs_symbols=(2, 11), prb_start=11, prb_count=30, start_symbol=2,
                           nof_symbols=12, precoding=w, tb_size_bytes=tbs // 8, nof_cdm_groups_without_data=groups)
        tb = cases.random_tb(rng, pdu)
        before = ((rng.standard_normal((nof_ports, 14, nof_subc, 2)) * 0.5).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        want = before.copy()
        rc = oracle._f("pdsch_process")(C.byref(pdu), tb.ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p), nof_ports, nof_subc, None, None)
        assert rc == 0
        sid = pool.open()
        pool.load_grid(sid, before)
        assert pool.pdsch(sid, [pdu], [tb]) == 0
        got = pool.read_grid(sid)
        assert np.array_equal(got, want), (layers, groups, int(np.count_nonzero(got != want)))
        assert not np.array_equal(got, before)
        pool.close(sid)
    pool.destroy()


def test_dl_slot_pipeline_driven_from_several_threads(gpu_ctx, oracle):
    """Different slots of one pool driven from different host threads at the same time (the reference processes several slots on
    several downlink executors): four threads, each opening, filling (two PDSCH calls), handing over, waiting for and closing its own
    slots, a dozen times over, with fewer pool slots than threads x 2 so that open() also meets a full pool.  Every slot's IQ equals the
    oracle's for ITS transport blocks."""
    import threading
    rng = np.random.default_rng(8128)
    nof_ports, nof_rb = 2, 52
    nof_subc = 12 * nof_rb
    ocfg = abi.OfdmConfig(0, nof_rb, 1024, 0, 1.0 / np.sqrt(1024), 2.4e9)
    w2 = cases.codebook("two_layer_two_ports_0")

    def make(lo, count, rnti, slot_index):
        tbs = cases.tbs(12, 12, 4, 490, 2, count)
        return abi.make_pdu(bwp_size_rb=nof_rb, qm=4, rnti=rnti, n_id=5, dmrs_symbols=(2, 11), prb_start=lo, prb_count=count, start_symbol=2,
                            nof_symbols=12, precoding=w2, tb_size_bytes=tbs // 8, slot_index=slot_index)

    nthreads, rounds = 4, 12
    work = [[(make(0, 20, 100 + t, r % 10), make(20, 32, 200 + t, r % 10)) for r in range(rounds)] for t in range(nthreads)]
    tbs_ = [[tuple(cases.random_tb(rng, q) for q in pair) for pair in row] for row in work]
    want = {}
    for t in (0, nthreads - 1):   # the oracle's IQ for two of the threads (the others are checked for completion and status)
        for r in (0, rounds - 1):
            g = np.zeros((nof_ports, 14, nof_subc, 2), np.uint16)
            for q, tb in zip(work[t][r], tbs_[t][r]):
                g = _merge(g, oracle.pdsch_process(q, tb, nof_ports, nof_subc))
            want[(t, r)] = oracle.ofdm_slot(ocfg, g, 0)
    pool = lib.DlSlotPool(gpu_ctx, ocfg, nof_ports, 5, 65536)
    errors, results = [], {}

    def drive(t):
        try:
            for r in range(rounds):
                sid = pool.open()
                while sid is None:
                    pool.wait_free()
                    sid = pool.open()
                for q, tb in zip(work[t][r], tbs_[t][r]):
                    assert pool.pdsch(sid, [q], [tb]) == 0
                assert pool.modulate(sid, 0) == 0 and pool.wait(sid) == 0
                if (t, r) in want:
                    results[(t, r)] = np.stack([pool.iq(sid, p) for p in range(nof_ports)])
                pool.close(sid)
        except Exception as e:   # noqa: BLE001 -- reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=drive, args=(t,)) for t in range(nthreads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
    assert not errors, errors
    assert sorted(results) == sorted(want)
    for key, iq in results.items():
        assert rel_err(iq, want[key]) < 1e-5, key
    pool.destroy()


@pytest.mark.parametrize("zero_copy", [0, 1, 2, 3])
def test_dl_slot_pipeline_wire_format(gpu_ctx, oracle, monkeypatch, zero_copy):
    """A pool created with iq_format 1: the slot leaves the device as complex int16 after the amplitude controller
    (nrphy_ofdm_run_ci16) -- half the bytes over PCIe; within one LSB of the oracle's chain.  IQ and measurements share one
    pinned block (one copy up).  zero_copy: NRPHY_DL_SLOT_ZERO_COPY, read when the pool is created -- bit 0: the kernels read
    the pinned staging in place, bit 1: the modulator writes the pinned IQ block in place."""
    monkeypatch.setenv("NRPHY_DL_SLOT_ZERO_COPY", str(zero_copy))
    rng = np.random.default_rng(515)
    nof_ports, nof_rb = 2, 106
    ocfg = abi.OfdmConfig(0, nof_rb, 2048, 0, 1.0 / np.sqrt(2048), 3.5e9)
    wire = abi.IqWireCfg(abi.AmplitudeCfg(0, 1, -10.0, 1.0, -6.0), 32767.0)
    pool = lib.DlSlotPool(gpu_ctx, ocfg, nof_ports, 1, 65536, wire_cfg=wire)
    pdu, _, nof_subc, _ = cases.baseline_config(2)
    tb = cases.random_tb(rng, pdu)
    sid = pool.open()
    assert pool.pdsch(sid, [pdu], [tb]) == 0 and pool.modulate(sid, 0) == 0 and pool.wait(sid) == 0
    grid = oracle.pdsch_process(pdu, tb, nof_ports, nof_subc)
    ref_iq = oracle.ofdm_slot(ocfg, grid, 0)
    for port in range(nof_ports):
        y, _ = oracle.amplitude_control(wire.amplitude, ref_iq[port])
        want = oracle.iq_convert_ci16(y, wire.ci16_scale).reshape(-1, 2)
        got = pool.iq(sid, port)
        assert got.shape == want.shape and np.abs(got.astype(np.int32) - want.astype(np.int32)).max() <= 1
        assert np.mean(got == want) > 0.999
        # the amplitude controller's measurements of the buffer, next to the samples in pinned memory
        y2, m = oracle.amplitude_control(wire.amplitude, ref_iq[port])
        st = pool.amplitude_stats(sid, port)
        assert st.nof_samples == want.shape[0] and abs(int(st.nof_clipped) - int(m["nof_clipped"])) <= 2   # (a sample on the ceiling: 1e-7 apart)
        assert abs(st.sum_power - m["stats"].sum_power) <= 1e-4 * m["stats"].sum_power
        assert abs(st.peak_power - m["stats"].peak_power) <= 1e-5 * m["stats"].peak_power
    pool.close(sid)
    pool.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# Lower-PHY tail: amplitude controller, radio sample format, fronthaul compression
# ---------------------------------------------------------------------------------------------------------------------
def test_amplitude_controller_and_ci16_vs_oracle(gpu_ctx, oracle):
    """amplitude_controller::process and the cf32 -> ci16 conversion through the C ABI: samples bit for bit, clip counts
    and peak power exactly, the power sum to float accuracy; a batch of strided device buffers; running counters."""
    import torch
    rng = np.random.default_rng(83)
    running = abi.AmplitudeMetrics()
    want_processed = want_clipped = 0
    cfg_run = abi.AmplitudeCfg(0, 1, -1.0, 1.0, -6.0)
    for t in range(30):
        n = int(rng.integers(1, 5000))
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * float(rng.choice([0.1, 0.5, 1.0]))
        cfg = abi.AmplitudeCfg(int(rng.integers(0, 2)), int(rng.integers(0, 2)), float(rng.choice([0.0, -3.0, 2.5])),
                               float(rng.choice([1.0, 2.0])), float(rng.choice([-0.1, -6.0, -12.0])))
        want, wm = oracle.amplitude_control(cfg, x)
        got, m = gpu_ctx.amplitude_control_host(cfg, x)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), t
        assert m.nof_clipped_samples == wm["nof_clipped"] and m.nof_processed_samples == wm["nof_processed"]
        assert m.peak_power_fs == np.float32(wm["peak_power_fs"]) and m.gain_dB == np.float32(wm["gain_dB"])
        for k in ("avg_power_fs", "papr_lin"):
            assert abs(getattr(m, k) - wm[k]) <= 2e-5 * max(1e-9, abs(wm[k])), k
        scale = float(rng.choice([32767.0, 1000.0, 20000.0]))
        assert np.array_equal(gpu_ctx.iq_convert_ci16_host(x, scale), oracle.iq_convert_ci16(x, scale)), t
        # one controller object over many buffers: the counters accumulate
        _, wr = oracle.amplitude_control(cfg_run, x)
        gpu_ctx.amplitude_control_host(cfg_run, x, running)
        want_processed += wr["nof_processed"]
        want_clipped += wr["nof_clipped"]
    assert (running.nof_processed_samples, running.nof_clipped_samples) == (want_processed, want_clipped)
    assert abs(running.clipping_probability - want_clipped / want_processed) < 1e-12
    x = np.zeros(37, np.complex64)
    x.real, x.imag = np.arange(37) + 0.5, -(np.arange(37) + 0.5)
    for k in (1.0, 2000.0):
        assert np.array_equal(gpu_ctx.iq_convert_ci16_host(x * k, 1.0), oracle.iq_convert_ci16(x * k, 1.0))
    # batch: 7 buffers of 1000 samples inside rows of 1024, in place
    buf = (rng.standard_normal((7, 1024)) + 1j * rng.standard_normal((7, 1024))).astype(np.complex64)
    d = dev(buf.view(np.float32))
    d_stats = torch.zeros((7, 4), dtype=torch.int32, device="cuda")
    cfg = abi.AmplitudeCfg(0, 1, 0.0, 1.0, -3.0)
    gpu_ctx.amplitude_control(cfg, 7, 1000, d, d, d_stats, in_stride=1024, out_stride=1024)
    d16 = torch.zeros((7, 1024, 2), dtype=torch.int16, device="cuda")
    gpu_ctx.iq_convert_ci16(7, 1000, d, 5000.0, d16, in_stride=1024, out_stride=1024)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    got = d.cpu().numpy().view(np.complex64).reshape(7, 1024)
    stats = d_stats.cpu().numpy()
    for i in range(7):
        want, wm = oracle.amplitude_control(cfg, buf[i, :1000])
        assert np.array_equal(got[i, :1000].view(np.uint32), want.view(np.uint32)) and np.array_equal(got[i, 1000:], buf[i, 1000:])
        assert stats[i, 2] == wm["nof_clipped"] and stats[i, 3] == 1000
        assert stats[i, 1].view(np.float32) == np.float32(wm["stats"].peak_power)
        assert np.array_equal(d16[i, :1000].cpu().numpy().reshape(-1), oracle.iq_convert_ci16(want, 5000.0))


def test_ofh_compression_vs_oracle(gpu_ctx, oracle):
    """Open Fronthaul compression (none and BFP, 8-16 bits) of grid PRBs: host-span calls against the oracle, then a
    whole batch of grids compressed row by row in one call."""
    import torch
    rng = np.random.default_rng(84)
    for t in range(120):
        typ, w, nprb = int(rng.integers(0, 2)), int(rng.integers(8, 17)), int(rng.integers(1, 276))
        x = (rng.standard_normal((nprb, 12, 2)) * float(rng.choice([0.01, 0.2, 0.33]))).astype(np.float32)
        prbs = (x.view(np.uint32) >> 16).astype(np.uint16)
        if t % 7 == 0:
            prbs[0] = 0
        cfg = abi.OfhCompressionCfg(typ, w, float(rng.choice([1.0, 0.5, 0.9])))
        got, want = gpu_ctx.ofh_compress_host(cfg, prbs), oracle.ofh_compress(cfg, prbs)
        assert np.array_equal(got, want), (typ, w, nprb, int(np.count_nonzero(got != want)))
    for w, typ in ((9, 0), (16, 0), (12, 0), (9, 1), (14, 1)):   # exact ties
        gain = ((1 << (w - 1)) - 1) if typ == 0 else 32767
        vals = (np.arange(24 * 5) % 40 - 20 + 0.5).astype(np.float32)
        prbs = (vals.view(np.uint32) >> 16).astype(np.uint16).reshape(5, 12, 2)
        cfg = abi.OfhCompressionCfg(typ, w, 1.0 / gain)
        assert np.array_equal(gpu_ctx.ofh_compress_host(cfg, prbs), oracle.ofh_compress(cfg, prbs)), (w, typ)
    # 3 grids x 2 ports x 14 symbols x 106 PRBs in one call, BFP 9 bits (28 bytes per PRB)
    cfg = abi.OfhCompressionCfg(1, 9, 0.8)
    grids = ((rng.standard_normal((3, 2, 14, 106 * 12, 2)) * 0.25).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    d_grid = dev(grids.view(np.uint32).reshape(3, 2, 14, 106 * 12).view(np.int32))
    d_out = torch.zeros((3 * 2 * 14, 106 * 28), dtype=torch.uint8, device="cuda")
    gpu_ctx.ofh_compress(cfg, 3 * 2 * 14, 106, d_grid, d_out)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    rows = grids.reshape(3 * 2 * 14, 106, 12, 2)
    for r in (0, 17, 83):
        assert np.array_equal(got[r], oracle.ofh_compress(cfg, rows[r])), r
    bad = abi.OfhCompressionCfg(1, 7, 1.0)   # below 8 bits the reference's packer has no defined result
    with pytest.raises(lib.NrphyError):
        gpu_ctx.ofh_compress_host(bad, rows[0])


def test_ofdm_modulator_wire_format_output(gpu_ctx, oracle):
    """nrphy_ofdm_run_ci16: modulator + amplitude controller + int16 conversion in one kernel equals the three separate
    device steps bit for bit, the oracle's chain to one LSB (its FFT differs by 1e-7), and the measurements agree."""
    import torch
    rng = np.random.default_rng(85)
    # amplitude settings: clipping everywhere (every wave takes the exact path), nowhere (no wave does: gain -20 dB under a
    # -1 dBFS ceiling), in some waves only (ceiling at about 3.5 sigma), and clipping disabled with saturating conversions
    amps = (abi.AmplitudeCfg(0, 1, -2.0, 1.0, -9.0), abi.AmplitudeCfg(0, 1, -20.0, 1.0, -1.0),
            abi.AmplitudeCfg(0, 1, -10.0, 1.0, -6.0), abi.AmplitudeCfg(0, 0, 6.0, 1.0, -1.0))
    for k, (mu, bw, n, ext, ports, slots) in enumerate(((1, 273, 4096, 0, 2, 3), (1, 273, 4096, 0, 1, 1), (1, 273, 4096, 0, 1, 2),
                                                        (1, 273, 4096, 0, 1, 1), (0, 52, 1024, 0, 1, 2), (2, 24, 512, 1, 1, 2),
                                                        (0, 270, 6144, 0, 1, 1), (0, 52, 1024, 0, 1, 2),
                                                        (1, 273, 4608, 0, 2, 2), (1, 100, 4608, 1, 1, 1))):   # 4608: 288 threads, a half wavefront
        ocfg = abi.OfdmConfig(mu, bw, n, ext, 1.0 / np.sqrt(n), 3.5e9)
        grid = ((rng.standard_normal((slots, ports, 14, bw * 12, 2)) * 0.5).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        plan = lib.OfdmPlan(gpu_ctx, ocfg, ports)
        d_grid = dev(grid.view(np.uint32).reshape(slots, ports, 14, bw * 12).view(np.int32))
        d_slot = dev(np.arange(slots, dtype=np.uint32).view(np.int32) % (1 << mu))
        # round scales make exact ties (x.5) common -- bf16 grid values times powers of two: the product has to be rounded to
        # float BEFORE the integer rounding, as the reference's two steps do (a fused multiply-add breaks such ties by the
        # unrounded product; the seeded sweep found that in round 4, see IqSinkCi16::pack_plain)
        wire = abi.IqWireCfg(amps[k % len(amps)], (32767.0, 20000.0, 40000.0)[k % 3])
        d_iq16 = torch.zeros((slots, ports, plan.slot_stride, 2), dtype=torch.int16, device="cuda")
        d_stats = torch.zeros((slots * ports, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        plan.run_ci16(slots, d_grid, wire, d_iq16, d_slot_index=d_slot, d_stats=d_stats)
        # the same in three steps
        d_iq = torch.zeros((slots, ports, plan.slot_stride, 2), dtype=torch.float32, device="cuda")
        plan.run(slots, d_grid, d_iq, d_slot_index=d_slot)
        gpu_ctx.synchronize()
        torch.cuda.synchronize()
        fused, stats = d_iq16.cpu().numpy(), d_stats.cpu().numpy()
        iq = d_iq.cpu().numpy().view(np.complex64).reshape(slots, ports, -1)
        for s in range(slots):
            size = lib.slot_size(ocfg, int(s % (1 << mu)))
            for p in range(ports):
                y, m = oracle.amplitude_control(wire.amplitude, iq[s, p, :size])
                want = oracle.iq_convert_ci16(y, wire.ci16_scale).reshape(-1, 2)
                # fused vs (device modulator -> oracle tail): the conversion's tail rule does not apply to a fused slot
                # (every value takes the vector path), so compare away from exact ties
                assert np.abs(fused[s, p, :size].astype(np.int32) - want.astype(np.int32)).max() <= 1
                assert np.mean(fused[s, p, :size] == want) > 0.9999
                st = stats[s * ports + p]
                assert st[3] == size and st[2] == m["nof_clipped"], (st, m["nof_clipped"])
                assert st[1].view(np.float32) == np.float32(m["stats"].peak_power)
                assert abs(st[0].view(np.float32) - m["stats"].sum_power) <= 1e-4 * m["stats"].sum_power
                # against the oracle's own modulator: one LSB
                ref_iq = oracle.ofdm_slot(ocfg, grid[s], int(s % (1 << mu)))[p]
                y2, _ = oracle.amplitude_control(wire.amplitude, ref_iq)
                want2 = oracle.iq_convert_ci16(y2, wire.ci16_scale).reshape(-1, 2)
                assert np.abs(fused[s, p, :size].astype(np.int32) - want2.astype(np.int32)).max() <= 1
        plan.close()


def test_ofdm_modulator_wire_format_rounds_the_scaled_sample_first(gpu_ctx, oracle):
    """The configurations on which the seeded sweep (profiles/fuzz_sweep.py wire, base 0) caught the wire-format conversion rounding
    exact ties (x.5) as a fused multiply-add does -- by the unrounded product -- where the reference rounds the product to float
    first: 1.5e-4 of the samples one LSB off, five of these twelve configurations over the limit of 1e-4.  Same generator, same
    checks as the sweep leg; the library of the commit before the fix fails here."""
    import torch
    rng = np.random.default_rng(16180)
    for t in range(12):
        size = int(rng.choice([256, 512, 1024, 1536, 2048, 4096, 4608, 6144]))
        mu, ext = int(rng.integers(0, 4)), int(rng.integers(0, 5) == 0)
        bw, ports, slots = int(rng.integers(1, min(275, (size - 1) // 12) + 1)), int(rng.integers(1, 4)), int(rng.integers(1, 4))
        ocfg = abi.OfdmConfig(mu, bw, size, ext, float(rng.uniform(0.5, 2.0)) / np.sqrt(size), float(rng.choice([0.0, 2.4e9, 3.5e9])))
        amp = abi.AmplitudeCfg(0, int(rng.integers(0, 2)), float(rng.uniform(-20, 6)), float(rng.choice([1.0, 2.0])), float(rng.uniform(-12, -0.5)))
        wire = abi.IqWireCfg(amp, float(rng.choice([32767.0, 20000.0, 40000.0])))
        grid = ((rng.standard_normal((slots, ports, 14, bw * 12, 2)) * rng.uniform(0.2, 1.0)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        plan = lib.OfdmPlan(gpu_ctx, ocfg, ports)
        d_grid = dev(grid.view(np.uint32).reshape(slots, ports, 14, bw * 12).view(np.int32))
        d_slot = dev((np.arange(slots, dtype=np.uint32) % (1 << mu)).view(np.int32))
        d_iq16 = torch.zeros((slots, ports, plan.slot_stride, 2), dtype=torch.int16, device="cuda")
        d_stats = torch.zeros((slots * ports, 4), dtype=torch.int32, device="cuda")
        d_iq = torch.zeros((slots, ports, plan.slot_stride, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        plan.run_ci16(slots, d_grid, wire, d_iq16, d_slot_index=d_slot, d_stats=d_stats)
        plan.run(slots, d_grid, d_iq, d_slot_index=d_slot)
        gpu_ctx.synchronize()
        torch.cuda.synchronize()
        fused, stats = d_iq16.cpu().numpy(), d_stats.cpu().numpy()
        iq = d_iq.cpu().numpy().view(np.complex64).reshape(slots, ports, -1)
        for s in range(slots):
            ssz = lib.slot_size(ocfg, int(s % (1 << mu)))
            for p in range(ports):
                y, m = oracle.amplitude_control(wire.amplitude, iq[s, p, :ssz])
                # (pad the oracle's call so that every sample lies in the vector part of the reference's conversion, as the sweep does)
                want = oracle.iq_convert_ci16(np.concatenate([y, np.zeros(8, np.complex64)]), wire.ci16_scale).reshape(-1, 2)[:ssz]
                assert np.abs(fused[s, p, :ssz].astype(np.int32) - want.astype(np.int32)).max() <= 1, (t, size)
                assert np.mean(fused[s, p, :ssz] == want) > 0.9999, (t, size, int((fused[s, p, :ssz] != want).sum()), 2 * ssz)
                assert stats[s * ports + p][2] == m["nof_clipped"] and stats[s * ports + p][3] == ssz
        plan.close()


def test_grid_put_sparse_host_writes(gpu_ctx):
    """nrphy_grid_put: resource elements of CPU-generated channels merged into a device grid; later entries win, the
    rest of the grid is untouched, out-of-range entries are refused."""
    import torch
    rng = np.random.default_rng(99)
    nof_ports, nof_subc = 3, 624
    grid = rng.integers(0, 2 ** 32, (nof_ports, 14, nof_subc), dtype=np.uint32)
    d_grid = dev(grid.view(np.int32))
    entries, want = [], grid.copy()
    for _ in range(700):
        e = (int(rng.integers(0, nof_ports)), int(rng.integers(0, 14)), int(rng.integers(0, nof_subc)), int(rng.integers(0, 2 ** 32)))
        entries.append(e)
    entries += [entries[5][:3] + (123,), entries[5][:3] + (456,), entries[17][:3] + (789,)]   # duplicates: the last one wins
    for p, l, k, v in entries:
        want[p, l, k] = v
    gpu_ctx.grid_put(d_grid, nof_ports, nof_subc, entries)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d_grid.cpu().numpy().view(np.uint32), want)
    bad = (abi.GridRe * 1)(abi.GridRe(nof_ports, 0, 0, 1))
    assert gpu_ctx.lib.nrphy_grid_put(gpu_ctx.handle, d_grid.data_ptr(), nof_ports, nof_subc, 1, bad, None) == abi.ERR_ARGUMENT


def test_llr_descramble_host_cases(gpu_ctx, oracle):
    """Soft-bit descrambling, the cases of tests/test_oracle.py::test_oracle_vs_ref_llr_descrambling (oracle pinned to the
    compiled reference there) plus chunk boundaries of the kernel (65536 soft bits per workgroup) and the longest
    PUSCH codeword; every int8 value including -128."""
    rng = np.random.default_rng(44)
    for c_init, n in ((1 << 15, 256), (0x12345678, 100003), (5, 15), (0x7FFFFFFF, 17), ((0x4601 << 15) + 935, 52416),
                      (77, 1), (78, 33), (79, 6 * 32 + 5), (80, 65536), (81, 65537), (82, 65535), (83, 2 * 65536 + 16),
                      (0x7ABCDEF0, 273 * 12 * 14 * 8 * 4), (84, 1 << 21)):
        llr = rng.integers(-128, 128, n).astype(np.int8)
        got = gpu_ctx.llr_descramble_host(c_init, llr)
        assert np.array_equal(got, oracle.prg_apply_xor_llr(c_init, 0, llr)), (c_init, n)
    assert gpu_ctx.llr_descramble_host(3, np.zeros(0, np.int8)).size == 0
    one = np.zeros(16, np.int8)
    assert gpu_ctx.lib.nrphy_llr_descramble_host(gpu_ctx.handle, 1, (1 << 21) + 1, one.ctypes.data, one.ctypes.data) == abi.ERR_ARGUMENT


def test_llr_descramble_batch_strided_in_place(gpu_ctx, oracle):
    """A batch of codewords with their own c_init in device memory: out of place with different strides, in place, rows
    that are not 16-byte aligned (byte path), and padding between rows left untouched."""
    import torch
    rng = np.random.default_rng(45)
    for n_cw, length, in_stride, out_stride in ((5, 70000, 70016, 70400), (3, 4097, 4099, 4101), (64, 1000, 1008, 1008), (2, 131072, 131072, 131072)):
        c_init = rng.integers(0, 1 << 31, n_cw).astype(np.uint32)
        src = rng.integers(-128, 128, (n_cw, in_stride)).astype(np.int8)
        dst0 = rng.integers(-128, 128, (n_cw, out_stride)).astype(np.int8)
        d_ci, d_src, d_dst = dev(c_init.view(np.int32)), dev(src), dev(dst0)
        gpu_ctx.llr_descramble(d_ci, n_cw, length, d_src, in_stride, d_dst, out_stride)
        gpu_ctx.synchronize()
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
        for r in range(n_cw):
            assert np.array_equal(got[r, :length], oracle.prg_apply_xor_llr(int(c_init[r]), 0, src[r, :length])), (n_cw, length, r)
        assert np.array_equal(got[:, length:], dst0[:, length:])
        assert np.array_equal(d_src.cpu().numpy(), src)
        gpu_ctx.llr_descramble(d_ci, n_cw, length, d_src, in_stride, d_src, in_stride)   # in place
        gpu_ctx.synchronize()
        torch.cuda.synchronize()
        again = d_src.cpu().numpy()
        assert np.array_equal(again[:, :length], got[:, :length]) and np.array_equal(again[:, length:], src[:, length:])


def test_pdsch_random_pdus(gpu_ctx, oracle):
    """Fuzz: the 40 random PDUs of tests/test_oracle.py::test_oracle_vs_ref_random_pdus (same seed, so the oracle side of
    every one of them is pinned to the compiled reference) plus 40 more, codeword taps and grid bit-exact."""
    rng = np.random.default_rng(20240611)
    for i, (pdu, nof_ports, nof_subc) in enumerate(cases.random_pdus(oracle.tbs, rng, 40)):
        if oracle.validate(pdu) != 0:
            assert gpu_ctx.lib.nrphy_pdsch_validate(C.byref(pdu)) != 0
            continue
        run_single(gpu_ctx, oracle, pdu, cases.random_tb(rng, pdu), nof_ports, nof_subc)
    rng = np.random.default_rng(777)
    refused = 0
    for pdu, nof_ports, nof_subc in cases.random_pdus(oracle.tbs, rng, 40):
        if oracle.validate(pdu) != 0:
            continue
        if oracle.derive(pdu)["nof_re"] == 0:
            # every allocated symbol carries DM-RS on both CDM groups: nothing to transmit on; the reference runs into
            # its assertions, this library refuses the PDU
            with pytest.raises(lib.NrphyError):
                gpu_ctx.pdsch_process_host(pdu, cases.random_tb(rng, pdu), nof_ports, nof_subc)
            refused += 1
            continue
        run_single(gpu_ctx, oracle, pdu, cases.random_tb(rng, pdu), nof_ports, nof_subc)
    assert refused <= 3


def per_prg_reach(pdu, nof_subc):
    """(PRGs the allocation touches, whether a PRB of it lies beyond the last PRG and takes that PRG's weights)."""
    prbs = [p for p in range(nof_subc // 12) if (int(pdu.prb_mask[p // 64]) >> (p % 64)) & 1]
    return {min(p // pdu.prg_size_rb, pdu.nof_prg - 1) for p in prbs}, prbs[-1] >= pdu.nof_prg * pdu.prg_size_rb


def test_pdsch_random_pdus_per_prg(gpu_ctx, oracle):
    """Fuzz with weights per PRG: 24 random PDUs with 2-4 PRGs of random complex weights, each a host call of its own, codeword
    taps and grid bit-exact against the oracle.  The allocation spans all of its PRGs; in some draws it runs on beyond the
    last one."""
    rng = np.random.default_rng(20250321)
    draws = cases.random_pdus_per_prg(oracle.tbs, rng, 24)
    assert len(draws) == 24
    beyond = 0
    for i, (pdu, nof_ports, nof_subc) in enumerate(draws):
        touched, runs_on = per_prg_reach(pdu, nof_subc)
        assert 2 <= pdu.nof_prg <= 4 and touched == set(range(pdu.nof_prg)), i
        beyond += runs_on
        assert oracle.validate(pdu) == 0, i
        try:
            run_single(gpu_ctx, oracle, pdu, cases.random_tb(rng, pdu), nof_ports, nof_subc)
        except AssertionError as e:
            raise AssertionError("draw %d (Qm %d, %d layers, %d ports, %d PRGs of %d PRB): %s" % (
                i, pdu.qm, pdu.nof_layers, pdu.nof_ports, pdu.nof_prg, pdu.prg_size_rb, e))
    assert 0 < beyond < len(draws)


def test_receive_side_random_configurations(gpu_ctx, oracle):
    """Fuzz of the receive-side coding kernels against the oracle: random (base graph, lifting size, lengths, filler bits,
    CRC, noise, iterations, scaling) for the decoder; random (lifting size, E, rv, modulation, Nref, filler bits, new data
    or combining, arbitrary int8 contents) for the rate dematcher."""
    rng = np.random.default_rng(31337)
    sizes = cases.LIFTING_SIZES
    for _ in range(30):
        bg = int(rng.integers(1, 3))
        zc = int(rng.choice(sizes[8:]))
        kb, n_short = (22, 66) if bg == 1 else (10, 50)
        k = kb * zc
        crc_id = int(rng.choice([16, 0x24A, 0x24B]))
        crc_len = 16 if crc_id == 16 else 24
        nf = int(rng.integers(0, max(1, min(k - crc_len - 8, (kb - 2) * zc - 1) // 2)))
        nof_llr = int(rng.integers(k + 2 * zc - 2 * zc + 2 * zc, n_short * zc + 1))
        nof_llr = max(nof_llr, k + 2 * zc)
        amp, sigma = float(rng.uniform(6, 30)), float(rng.uniform(2, 14))
        _, llr = cases.make_ldpc_llrs(oracle, rng, bg, zc, nof_llr, crc_id, nf, amp, sigma)
        llr[rng.integers(0, nof_llr, nof_llr // 50)] = 127          # a few certain bits ...
        llr[rng.integers(0, nof_llr, nof_llr // 50)] = 0            # ... and a few erasures
        iters, scaling = int(rng.integers(1, 11)), float(rng.choice([0.5, 0.75, 0.8, 0.9]))
        crc = crc_id if rng.integers(0, 4) else 0
        want = oracle.ldpc_decode(bg, zc, nf, crc, iters, scaling, llr)
        got = gpu_ctx.ldpc_decode_host(bg, zc, nf, crc, iters, scaling, llr)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]), (bg, zc, nf, crc, iters, scaling, nof_llr)
    for _ in range(60):
        bg = int(rng.integers(1, 3))
        zc = int(rng.choice(sizes[4:]))
        n = (66 if bg == 1 else 50) * zc
        nof_sys = ((22 if bg == 1 else 10) - 2) * zc
        qm = int(rng.choice([1, 2, 4, 6, 8]))
        e = qm * int(rng.integers(1, max(2, min(3 * n, 60000) // qm)))
        nf = int(rng.integers(0, nof_sys // 2))
        nref = int(rng.choice([0, 0, int(rng.integers(nof_sys + 1, n + 1))]))
        rv, new_data = int(rng.integers(0, 4)), int(rng.integers(0, 2))
        llr = rng.integers(-127, 128, e).astype(np.int8)
        old = rng.integers(-127, 128, n).astype(np.int8)
        want = oracle.ldpc_rate_dematch(bg, zc, rv, qm, nref, nf, new_data, llr, old)
        got = gpu_ctx.ldpc_rate_dematch_host(bg, zc, rv, qm, nref, nf, new_data, llr, old)
        assert np.array_equal(got, want), (bg, zc, e, rv, qm, nref, nf, new_data, int(np.count_nonzero(got != want)))


def test_ofdm_random_configurations(gpu_ctx, oracle):
    """Fuzz of the OFDM modulator and demodulator against the oracle: random numerology, bandwidth, DFT size, cyclic
    prefix, centre frequency, scale, slot and (demodulator) window offset, 1-3 ports."""
    rng = np.random.default_rng(4096)
    for _ in range(24):
        n = int(rng.choice([128, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096, 4608, 6144]))
        mu = int(rng.integers(0, 4))
        ext = int(rng.integers(0, 4) == 0)
        bw = int(rng.integers(1, min(275, (n - 1) // 12) + 1))
        ports = int(rng.integers(1, 4))
        cfg = abi.OfdmConfig(mu, bw, n, ext, float(rng.uniform(0.01, 2.0)), float(rng.choice([0.0, 2.4e9, 3.5e9, 28e9])))
        slot = int(rng.integers(0, 1 << mu))
        grid = (rng.standard_normal((ports, 14, bw * 12, 2)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        plan = lib.OfdmPlan(gpu_ctx, cfg, ports)
        iq = plan.modulate_slot_host(grid, slot)
        want = oracle.ofdm_slot(cfg, grid, slot)
        assert iq.shape == want.shape and rel_err(iq, want) < 1e-5, (mu, bw, n, ext, slot)
        wo = int(rng.integers(0, (144 * n) // 2048))   # the reference bounds the offset by the normal cyclic prefix
        rx = (rng.standard_normal(want.shape) + 1j * rng.standard_normal(want.shape)).astype(np.complex64)
        got = plan.demodulate_slot_host(rx, slot, wo)
        ref_grid = oracle.ofdm_demod_slot(cfg, rx, slot, wo)
        nsymb = 12 if ext else 14
        assert_bf16_grids_close(got[:, :nsymb], ref_grid[:, :nsymb])
        plan.close()


def test_rate_matcher_buffer_ending_inside_the_filler_bits(gpu_ctx, oracle):
    """The corner the reference leaves undefined (cases.RM_CORNER_CASES): device == TS 38.212 evaluated bit by bit == oracle, through
    the encoder seam and, for the PDUs the seeded sweep found, through the whole processor."""
    rng = np.random.default_rng(3)
    for case in cases.RM_CORNER_CASES:
        bg, rv, qm, nref, tb_bytes, nsym = case
        tb = rng.integers(0, 256, tb_bytes, dtype=np.uint8)
        want = cases.rm_corner_expected(oracle, case, tb)
        got = np.asarray(gpu_ctx.pdsch_encode_host(bg, rv, qm, nref, 1, nsym, tb)[0])[: want.size]
        assert np.array_equal(got, want), case
    found = 0
    for base, seed in ((1000000, 2), (4000000, 0), (4000000, 3), (6000000, 2)):
        rng = np.random.default_rng(base + 1000 + seed)
        for pdu, nof_ports, nof_subc in cases.random_pdus(oracle.tbs, rng, 80):
            if oracle.validate(pdu) != 0 or oracle.derive(pdu)["nof_re"] == 0:
                continue
            tb = cases.random_tb(rng, pdu)
            rng.integers(0, 3)   # (the sweep's draw of a reference processor)
            d = oracle.derive(pdu)
            fs = d["segment_length"] - 2 * d["lifting_size"] - d["nof_filler_bits"]
            if not (d["nof_filler_bits"] and fs < d["n_cb"] < fs + d["nof_filler_bits"]):
                continue
            found += 1
            want, orm, oscr = oracle.pdsch_process(pdu, tb, nof_ports, nof_subc, taps=True, codeword_bits=d["codeword_bits"])
            got, rm, scr = gpu_ctx.pdsch_process_host(pdu, tb, nof_ports, nof_subc, taps=True)
            assert np.array_equal(rm, orm) and np.array_equal(scr, oscr) and np.array_equal(got, want), (base, seed, d)
    assert found >= 4


def test_pdsch_random_pdus_in_one_plan(gpu_ctx, oracle):
    """Fuzz of the batched path: 32 random PDUs (different allocations, layers, code rates, cyclic prefixes) in ONE plan,
    each into its own grid of a common shape, run twice on the same grids (the second run must overwrite everything the
    first one wrote: zero-fill lists, DM-RS and data of a different transport block set)."""
    import torch
    rng = np.random.default_rng(90210)
    drawn = [x for x in cases.random_pdus(oracle.tbs, rng, 36) if oracle.validate(x[0]) == 0 and oracle.derive(x[0])["nof_re"] > 0][:32]
    nof_ports, nof_subc = 4, max(x[2] for x in drawn)
    pdus = [x[0] for x in drawn]
    n = len(pdus)
    plan = None
    d_grid = torch.full((n, nof_ports, 14, nof_subc), 0x7FFF7FFF, dtype=torch.int32, device="cuda")
    for run in range(2):
        offs, tbs, pos = [], [], 0
        for p in pdus:
            tb = cases.random_tb(rng, p)
            offs.append(pos)
            tbs.append(tb)
            pos += (len(tb) + 15) & ~15
        buf = np.zeros(pos + 16, np.uint8)
        for o, tb in zip(offs, tbs):
            buf[o:o + len(tb)] = tb
        if plan is None:
            plan = lib.PdschPlan(gpu_ctx, pdus, offs, list(range(n)), n, nof_ports, nof_subc)
        d_rm = torch.zeros(plan.codeword_bits // 8 + 8, dtype=torch.uint8, device="cuda")
        plan.run(dev(buf), d_grid, d_cw_rm=d_rm, zero_grids=True)
        gpu_ctx.synchronize()
        grids = d_grid.cpu().numpy().view(np.uint16).reshape(n, nof_ports, 14, nof_subc, 2)
        rm = d_rm.cpu().numpy()
        for i, p in enumerate(pdus):
            d = oracle.derive(p)
            want, orm, _ = oracle.pdsch_process(p, tbs[i], nof_ports, nof_subc, taps=True, codeword_bits=d["codeword_bits"])
            assert np.array_equal(grids[i], want), (run, i, int(np.count_nonzero(grids[i] != want)))
            o = plan.codeword_offset(i) // 8
            assert np.array_equal(rm[o:o + len(orm)], orm), (run, i)
    plan.close()


def test_pusch_decoder_random_shapes(gpu_ctx, oracle):
    """Fuzz of the transport-block decoder: random transport-block sizes, base graphs, modulations, layers, limited-buffer
    sizes and redundancy-version orders, three transmissions each (the first as new data), against the restated
    pusch_decoder_impl (itself pinned to the compiled reference on fixed shapes)."""
    import torch
    rng = np.random.default_rng(5252)
    done = 0
    while done < 10:
        layers, qm = int(rng.integers(1, 5)), int(rng.choice([2, 4, 6, 8]))
        n_prb, nsym = int(rng.integers(2, 60)), int(rng.integers(6, 14))
        rate = float(rng.uniform(100, 800))
        tb_bits = oracle.tbs(nsym, 12, 0, qm, rate, layers, n_prb)
        if tb_bits < 40 or tb_bits > 120000:
            continue
        r = rate / 1024
        bg = 2 if (tb_bits <= 292 or (tb_bits <= 3824 and r <= 0.67) or r <= 0.25) else 1
        pdu = abi.make_pdu(bwp_size_rb=n_prb, qm=qm, dmrs_symbols=(2,), prb_start=0, prb_count=n_prb, start_symbol=0,
                           nof_symbols=nsym, precoding=abi.identity_precoding(layers), tb_size_bytes=tb_bits // 8, base_graph=bg,
                           tbs_lbrm_bytes=int(rng.choice([3168, 20000, abi.TBS_LBRM_DEFAULT])), nof_cdm_groups_without_data=2)
        if oracle.validate(pdu) != 0:
            continue
        d = oracle.derive(pdu)
        if d["nof_re"] == 0 or d["nof_codeblocks"] > 12:
            continue
        C, n, G = d["nof_codeblocks"], d["full_length"], d["codeword_bits"]
        tb = cases.random_tb(rng, pdu)
        cfg0 = abi.PuschDecoderCfg(bg, qm, 0, layers, d["n_ref"], pdu.tb_size_bytes, G // qm, 6, 1, 1)
        soft_bytes, state_bytes, _ = gpu_ctx.pusch_decoder_sizes(cfg0, 1)
        d_soft = torch.full((1, soft_bytes), -7, dtype=torch.int8, device="cuda")
        d_state = torch.full((state_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
        d_tb = torch.zeros((1, pdu.tb_size_bytes + 3), dtype=torch.uint8, device="cuda")
        d_res = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
        soft = np.full((C, n), -7, np.int8)
        cb_ok = np.ones(C, np.uint8)
        cb_msg = np.zeros((C, d["segment_length"]), np.uint8)
        amp = 8.0
        sigma = float(rng.uniform(3.0, 9.0))
        early = int(rng.integers(0, 2))
        for tx, rv in enumerate([0] + [int(x) for x in rng.permutation([1, 2, 3])[:2]]):
            cfg = abi.PuschDecoderCfg(bg, qm, rv, layers, d["n_ref"], pdu.tb_size_bytes, G // qm, 6, early, 1 if tx == 0 else 0)
            pdu.rv = rv
            _, rm, _ = oracle.pdsch_process(pdu, tb, layers, 12 * n_prb, taps=True, codeword_bits=G)
            pdu.rv = 0
            bits = np.unpackbits(rm)[:G].astype(np.float64)
            llr = np.clip(np.rint((1 - 2 * bits) * amp + rng.normal(0, sigma, G)), -120, 120).astype(np.int8)
            want = cases.pusch_decode_expected(oracle, d, cfg, llr, soft, cb_ok, cb_msg)
            gpu_ctx.pusch_decode_batch(cfg, 1, dev(llr[None, :]), G, d_soft, d_state, d_tb, d_tb.shape[1], d_res)
            torch.cuda.synchronize()
            res = tuple(int(x) for x in d_res.cpu().numpy()[0])
            assert res == (int(want[0]), want[1], want[2], want[3]), (done, tx, rv, res, want[:4], C, d["lifting_size"])
            assert np.array_equal(d_soft.cpu().numpy().reshape(C, n), soft), (done, tx)
            if want[0]:
                assert np.array_equal(d_tb.cpu().numpy()[0, : pdu.tb_size_bytes], tb)
                break
        done += 1


# ---- the reference's own unit-test configurations (tests/golden/ref_test_configs.npz) ---------------------------------
# Every configuration of the six test-data headers SURVEY.md section 8c lists, read from the headers themselves
# (oracle/ref/ref_testdata.cpp), with the compiled reference's outputs on seeded payloads as the expected values.

@pytest.fixture(scope="module")
def ref_cfgs():
    return np.load(os.path.join(cases.GOLDEN, "ref_test_configs.npz"))


def device_processor_case(gpu_ctx, g, key, nof_subc):
    pdu = cases.pdsch_pdu_from_fixture(g, key)
    assert lib.validate(pdu) == 0, key
    tb = cases.ref_test_config_tb(g, key, pdu.tb_size_bytes)
    grid, rm, _ = gpu_ctx.pdsch_process_host(pdu, tb, pdu.nof_ports, nof_subc, taps=True)
    assert sha(rm) == str(g[key + "_cw_sha"]), key
    assert sha(grid) == str(g[key + "_grid_sha"]), key
    return pdu, grid


def test_ref_test_configs_pdsch_processor(gpu_ctx, ref_cfgs):
    g = ref_cfgs
    assert int(g["proc_count"]) == 24
    for i in range(24):
        device_processor_case(gpu_ctx, g, "proc_%d" % i, int(g["proc_%d_rg" % i][0]) * 12)


def test_ref_test_configs_pdsch_encoder(gpu_ctx, ref_cfgs):
    g = ref_cfgs
    assert g["enc_cfg"].shape == (168, 7)
    for i, (bg, rv, qm, nref, layers, nsym, tb_bytes) in enumerate(g["enc_cfg"].tolist()):
        tb = np.random.default_rng([ord("e"), i]).integers(0, 256, tb_bytes, dtype=np.uint8)
        bits, packed = gpu_ctx.pdsch_encode_host(bg, rv, qm, nref, layers, nsym, tb)
        assert sha(packed) == str(g["enc_cw_sha"][i]), i
        assert np.array_equal(np.packbits(bits), packed)


def test_ref_test_configs_pdsch_modulator(gpu_ctx, ref_cfgs):
    g = ref_cfgs
    assert int(g["mod_count"]) == 36
    for i in range(36):
        key = "mod_%d" % i
        pdu = cases.pdsch_pdu_from_fixture(g, key)
        device_processor_case(gpu_ctx, g, key, (pdu.bwp_start_rb + pdu.bwp_size_rb) * 12)


def test_ref_test_configs_ldpc_segmenter(gpu_ctx, oracle, ref_cfgs):
    """The header's known answers from nrphy_pdsch_derive; the segments themselves are internal to the codeblock kernel, so
    their content is checked through the codeword: the test's own 150-symbol configuration, and one long enough for
    redundancy version 0 to carry every systematic bit past the first 2 Zc."""
    g = ref_cfgs
    assert g["seg_cases"].shape == (11, 4)
    for i, (tbs_bits, bg, nof_segments, segment_length) in enumerate(g["seg_cases"].tolist()):
        pdu = abi.make_pdu(base_graph=bg, tb_size_bytes=tbs_bits // 8, prb_count=52, qm=2)
        d = lib.derive(pdu)
        assert (d["nof_codeblocks"], d["segment_length"]) == (nof_segments, segment_length)
        tb = np.random.default_rng([ord("s"), i]).integers(0, 256, tbs_bits // 8, dtype=np.uint8)
        for nsym in (150, nof_segments * segment_length):
            _, packed = gpu_ctx.pdsch_encode_host(bg, 0, 2, 0, 1, nsym, tb)
            assert np.array_equal(packed, oracle.pdsch_encode_cfg(bg, 0, 2, 0, 1, nsym, tb)), (i, nsym)


def test_ref_test_configs_ofdm_modulator(gpu_ctx, ref_cfgs):
    g = ref_cfgs
    assert g["ofdm_cases"].shape[0] == 20
    for i, row in enumerate(g["ofdm_cases"]):
        cfg = abi.OfdmConfig(int(row[0]), int(row[1]), int(row[2]), int(row[3]), float(row[4]), float(row[5]))
        plan = lib.OfdmPlan(gpu_ctx, cfg, 1)
        iq = plan.modulate_slot_host(cases.ref_test_config_grid(row, i), int(row[7]))
        plan.close()
        assert iq.shape[1] == int(row[8])
        want = g["ofdm_%d_iq" % i]
        got = iq[0, g["ofdm_%d_idx" % i]]
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), i
        energy = float(np.sum(np.abs(iq.astype(np.complex128)) ** 2))
        assert abs(energy - float(g["ofdm_%d_energy" % i])) <= 1e-5 * energy


def test_ref_test_configs_dmrs_pdsch(gpu_ctx, ref_cfgs):
    g = ref_cfgs
    assert int(g["dmrs_count"]) == 192 and int(np.sum(g["dmrs_info"][:, 2])) == 96
    for i in range(192):
        key = "dmrs_%d" % i
        pdu = cases.pdsch_pdu_from_fixture(g, key)
        if not g["dmrs_info"][i, 2]:
            assert lib.validate(pdu) != 0, key
            continue
        nof_subc = pdu.bwp_size_rb * 12
        _, grid = device_processor_case(gpu_ctx, g, key, nof_subc)
        written = np.unpackbits(g[key + "_written"])[: pdu.nof_ports * 14 * nof_subc].astype(bool)
        assert sha(grid.view(np.uint32).reshape(-1)[written]) == str(g[key + "_values_sha"]), key


# ---- soft demodulator -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("modulation", [0, 1, 2, 4, 6, 8])
def test_demodulate_soft_vs_oracle_and_golden(gpu_ctx, oracle, modulation):
    """nrphy_demodulate_soft: every soft bit equals the reference's at the same position of the span (vector arithmetic for the
    leading multiple of the batch, generic for the tail), on boundary / tie / near-zero values and non-positive variances; the
    hashes are those of the compiled reference."""
    import torch
    g = np.load(os.path.join(cases.GOLDEN, "demod.npz"))
    for k, n in enumerate(g["lengths"].tolist()):
        for kind in (0, 1, 2):
            sym, noise = cases.demod_inputs(np.random.default_rng([modulation, n, kind]), modulation, n, kind)
            got = gpu_ctx.demodulate_soft_host(modulation, sym, noise)
            want = oracle.demodulate_soft(modulation, sym, noise)
            assert np.array_equal(got, want), (modulation, n, kind, np.flatnonzero(got != want)[:4])
            assert sha(got) == str(g["sha_%d_%d" % (modulation, kind)][k])
    # batched form: spans of odd and even lengths back to back (rows then start at any alignment)
    rng = np.random.default_rng(77 + modulation)
    qm = max(modulation, 1)
    for nof_spans, span_len in ((5, 1003), (3, 64), (7, 1), (2, 4099)):
        sym, noise = cases.demod_inputs(rng, modulation, nof_spans * span_len, 1)
        d_llr = torch.zeros(nof_spans * span_len * qm + 32, dtype=torch.int8, device="cuda")
        gpu_ctx.demodulate_soft(modulation, nof_spans, span_len, dev(sym.view(np.float32)), dev(noise), d_llr)
        gpu_ctx.synchronize()
        got = d_llr.cpu().numpy()
        assert not got[nof_spans * span_len * qm:].any()
        for r in range(nof_spans):
            want = oracle.demodulate_soft(modulation, sym[r * span_len:(r + 1) * span_len], noise[r * span_len:(r + 1) * span_len])
            assert np.array_equal(got[r * span_len * qm:(r + 1) * span_len * qm], want), (modulation, nof_spans, span_len, r)
    assert gpu_ctx.lib.nrphy_demodulate_soft(gpu_ctx.handle, 3, 1, 16, None, None, None, None) == abi.ERR_ARGUMENT
    assert gpu_ctx.lib.nrphy_demodulate_soft(gpu_ctx.handle, 8, 1, 16, None, None, None, None) == abi.ERR_ARGUMENT
    assert gpu_ctx.lib.nrphy_demodulate_soft(gpu_ctx.handle, 8, 0, 16, None, None, None, None) == abi.OK


def test_pdsch_process_slot_host_all_pdus_of_a_slot(gpu_ctx, oracle):
    """nrphy_pdsch_process_slot_host: the four PDUs of a config-4 cell-slot in one plan and one launch equal the four separate
    reference-shaped calls into the same grid; resource elements other channels wrote before stay."""
    rng = np.random.default_rng(404)
    pdus, nof_ports, nof_subc = cases.mixed_cell(2, slot_index=7)
    tbs = [cases.random_tb(rng, q) for q in pdus]
    grid = np.zeros((nof_ports, 14, nof_subc, 2), np.uint16)
    grid[:, 0, :, :] = 0x3F80          # what other channels left: all of symbol 0 (inside the allocations, so mostly replaced) ...
    grid[:, 13, ::7, 0] = 0x4000       # ... and scattered elements of symbol 13 (outside: the PDUs span symbols 0 to 11)
    before = grid.copy()
    want = before.copy()
    mapped = np.zeros(grid.shape[:3], bool)
    for q, tb in zip(pdus, tbs):
        part = oracle.pdsch_process(q, tb, nof_ports, nof_subc)
        m = part.view(np.uint32).reshape(part.shape[:3]) != 0
        want[m] = part[m]
        mapped |= m
    got = gpu_ctx.pdsch_process_slot_host(pdus, tbs, grid.copy())
    # every resource element a PDU maps (data, DM-RS and the zeros of its reserved positions) is the oracle's; the rest is kept
    single = before.copy()
    for q, tb in zip(pdus, tbs):
        single = gpu_ctx.pdsch_process_host(q, tb, nof_ports, nof_subc, grid=single)
    assert np.array_equal(got, single)
    assert np.array_equal(got[mapped], want[mapped])
    untouched = (single == before).all(axis=-1) & ~mapped
    assert np.array_equal(got[untouched], before[untouched])
    assert gpu_ctx.lib.nrphy_pdsch_process_slot_host(gpu_ctx.handle, 0, None, None, got.ctypes.data, nof_ports, nof_subc) == abi.OK


@pytest.mark.parametrize("qm,rate,snr_db", [(2, 449, 6.0), (4, 616, 14.0), (6, 719, 21.0), (8, 797, 28.0), (2, 120, -1.0)])
def test_link_all_modulations_through_soft_demodulator(gpu_ctx, oracle, qm, rate, snr_db):
    """The receive chain on real soft bits, in the manner of the reference's pxsch_bler_test (one layer, 30 kHz, DM-RS in
    symbols 2 and 7, 10 iterations): transport blocks -> device PDSCH chain (scrambled codeword tap) -> constellation symbols
    (TS 38.211 Section 5.1) + white noise -> nrphy_demodulate_soft -> nrphy_llr_descramble -> nrphy_pusch_decode_batch.
    A few dB above the code's threshold every block comes back; 12 dB lower none passes its CRC (no false positive)."""
    import torch
    nprb, slots = 52, 6
    tb_bits = oracle.tbs(12, 12, 0, qm, float(rate), 1, nprb)
    bg = 2 if (rate <= 256 or tb_bits <= 292 or (tb_bits <= 3824 and rate <= 686)) else 1
    pdus = [abi.make_pdu(slot_index=i, rnti=0x1234, bwp_size_rb=nprb, qm=qm, dmrs_symbols=(2, 7), prb_start=0, prb_count=nprb,
                         nof_symbols=14, base_graph=bg, tb_size_bytes=tb_bits // 8, nof_cdm_groups_without_data=2,
                         precoding=np.ones((1, 1, 1), np.complex64)) for i in range(slots)]
    pdu = pdus[0]
    d = lib.derive(pdu)
    G, tb_size = d["codeword_bits"], pdu.tb_size_bytes
    nsym = G // qm
    tb_stride = (tb_size + 3) & ~3
    rng = np.random.default_rng(1000 * qm + rate)
    d_tb = dev(rng.integers(0, 256, (slots, tb_stride), dtype=np.uint8))   # seeded: the verdicts below must not vary from run to run
    plan = lib.PdschPlan(gpu_ctx, pdus, [i * tb_stride for i in range(slots)], list(range(slots)), slots, 1, nprb * 12)
    d_cw = torch.zeros((plan.codeword_bits + 7) // 8 + 64, dtype=torch.uint8, device="cuda")
    plan.run(d_tb.reshape(-1), None, d_cw_scr=d_cw)
    gpu_ctx.synchronize()
    cw = d_cw.cpu().numpy()
    sym = np.zeros((slots, nsym), np.complex64)
    for i in range(slots):
        o = plan.codeword_offset(i)
        assert o % 8 == 0
        pts, sc = oracle.modulate(qm, cw[o // 8: o // 8 + (G + 7) // 8], nsym)
        sym[i] = (pts[:, 0] + 1j * pts[:, 1]) * sc
    assert abs(np.mean(np.abs(sym) ** 2) - 1.0) < 0.05
    d_c_init = dev(np.array([(p.rnti << 15) + p.n_id for p in pdus], np.uint32).view(np.int32))
    cfg = abi.PuschDecoderCfg(bg, qm, 0, 1, d["n_ref"], tb_size, nsym, 10, 1, 1)
    soft_bytes, state_bytes, _ = gpu_ctx.pusch_decoder_sizes(cfg, slots)
    for good in (True, False):
        nv = float(10.0 ** (-(snr_db if good else snr_db - 12.0) / 10.0))
        noisy = sym + (rng.standard_normal(sym.shape) + 1j * rng.standard_normal(sym.shape)).astype(np.complex64) * np.float32(
            np.sqrt(nv / 2))
        d_llr_scr = torch.zeros((slots, G), dtype=torch.int8, device="cuda")
        d_llr = torch.zeros_like(d_llr_scr)
        gpu_ctx.demodulate_soft(qm, slots, nsym, dev(noisy.view(np.float32)), dev(np.full((slots, nsym), nv, np.float32)), d_llr_scr)
        gpu_ctx.llr_descramble(d_c_init, slots, G, d_llr_scr, G, d_llr, G)
        d_soft = torch.zeros((slots, soft_bytes), dtype=torch.int8, device="cuda")
        d_state = torch.zeros((state_bytes,), dtype=torch.uint8, device="cuda")
        d_out = torch.zeros((slots, tb_stride), dtype=torch.uint8, device="cuda")
        d_res = torch.zeros((slots, 4), dtype=torch.int32, device="cuda")
        gpu_ctx.pusch_decode_batch(cfg, slots, d_llr, G, d_soft, d_state, d_out, tb_stride, d_res)
        gpu_ctx.synchronize()
        torch.cuda.synchronize()
        ok = d_res.cpu().numpy()[:, 0]
        if good:
            assert ok.all(), (qm, rate, ok)
            assert torch.equal(d_out[:, :tb_size], d_tb[:, :tb_size])
            # the soft bits agree with the oracle's on the same symbols (first slot)
            want = oracle.demodulate_soft(qm, noisy[0], np.full(nsym, nv, np.float32))
            assert np.array_equal(d_llr_scr[0].cpu().numpy(), want)
        else:
            assert not ok.any(), (qm, rate, ok)
    plan.close()


def test_pdsch_async_slot_batches_in_flight(gpu_ctx, oracle):
    """nrphy_pdsch_async_submit_slot: whole slots (four PDUs each, one plan and one launch per slot) in flight on the queue's
    streams; every slot's grid comes back once, from a runtime thread, equal to the oracle's four PDUs in one grid."""
    import threading
    import time
    rng = np.random.default_rng(909)
    slots = []
    for i in range(10):
        pdus, nof_ports, nof_subc = cases.mixed_cell(i % 3, slot_index=i % 5)
        slots.append((pdus, [cases.random_tb(rng, q) for q in pdus]))
    total_tb = max(sum(((q.tb_size_bytes + 7) & ~3) for q in pdus) for pdus, _ in slots)
    q = lib.PdschAsyncQueue(gpu_ctx, 3, nof_ports, nof_subc, total_tb)
    results, lock, threads_seen = {}, threading.Lock(), set()
    for i, (pdus, tbs) in enumerate(slots):
        def on_done(status, grid, i=i):
            with lock:
                results.setdefault(i, []).append((status, grid))
                threads_seen.add(threading.get_ident())
        while not q.submit_slot(pdus, tbs, on_done):
            time.sleep(0.0005)
    q.wait()
    assert sorted(results) == list(range(len(slots))) and all(len(v) == 1 for v in results.values())
    assert threading.get_ident() not in threads_seen
    for i, (pdus, tbs) in enumerate(slots):
        status, grid = results[i][0]
        assert status == 0
        want = None
        for pdu, tb in zip(pdus, tbs):
            part = oracle.pdsch_process(pdu, tb, nof_ports, nof_subc)
            want = part if want is None else np.bitwise_or(want, part)   # disjoint allocations
        assert np.array_equal(grid, want), i
    # too many transport-block bytes for the queue's staging: refused, nothing in flight afterwards
    small = lib.PdschAsyncQueue(gpu_ctx, 1, nof_ports, nof_subc, 64)
    with pytest.raises(Exception):
        small.submit_slot(slots[0][0], slots[0][1], lambda *a: None)
    small.wait()
    small.close()
    q.close()


def test_whole_slot_chain_in_a_hip_graph(gpu_ctx, oracle):
    """The plan-based / descriptor-free device entry points added in round 2 are capturable too: PDSCH -> OFDM with wire-format
    output (measurements on), and on the receive side soft demodulation -> descrambling, in one graph replayed on new inputs;
    the replayed results equal the eager ones bit for bit.  (The PDCCH / SS-PBCH / CSI-RS writers copy their host descriptors
    at the call, like a plan creation, and therefore stay outside a graph: they run eagerly between the replays here.)"""
    import torch
    rng = np.random.default_rng(2468)
    nof_ports, nof_rb = 2, 52
    nof_subc = 12 * nof_rb
    tbs = lib.tbs_calculate(12, 12, 0, 4, 490, 2, 30)
    pdsch = abi.make_pdu(bwp_size_rb=nof_rb, qm=4, rnti=17, n_id=5, dmrs_symbols=(2, 11), prb_start=22, prb_count=30,
                         start_symbol=2, nof_symbols=12, precoding=cases.codebook("two_layer_two_ports_0"),
                         tb_size_bytes=tbs // 8, slot_index=0)
    pdcch = abi.make_pdcch(payload=rng.integers(0, 2, 41, dtype=np.uint8), rnti=17, cce_index=0, aggregation_level=4, duration=2,
                           frequency_resources=tuple(range(8)), mapping="interleaved", reg_bundle_size=6, interleaver_size=2,
                           shift_index=3, n_id_dmrs=5, n_id_data=5, n_rnti=17, bwp_size_rb=nof_rb,
                           precoding=np.array([[1.0, 1.0j]], np.complex64) / np.sqrt(2))
    ssb = abi.make_ssb(pattern_case="A", ssb_idx=0, L_max=4, phys_cell_id=5, payload=rng.integers(0, 2, 32, dtype=np.uint8),
                       sfn=100, ports=(0,))
    csi = abi.make_csi_rs(row=3, start_rb=0, nof_rb=nof_rb, k0=4, l0=13, density="one", scrambling_id=5,
                          precoding=np.eye(2, dtype=np.complex64)[None])
    ocfg = abi.OfdmConfig(0, nof_rb, 1024, 0, 1.0 / np.sqrt(1024), 2.4e9)
    plan = lib.PdschPlan(gpu_ctx, [pdsch], [0], [0], 1, nof_ports, nof_subc)
    oplan = lib.OfdmPlan(gpu_ctx, ocfg, nof_ports)
    wire = abi.IqWireCfg(abi.AmplitudeCfg(0, 1, -12.0, 1.0, -3.0), 32767.0)
    tb_bytes = (pdsch.tb_size_bytes + 3) & ~3
    d_tb = torch.zeros(tb_bytes, dtype=torch.uint8, device="cuda")
    d_grid = torch.zeros((1, nof_ports, 14, nof_subc), dtype=torch.int32, device="cuda")
    d_iq16 = torch.zeros((1, nof_ports, oplan.slot_stride, 2), dtype=torch.int16, device="cuda")
    d_stats = torch.zeros((nof_ports, 4), dtype=torch.int32, device="cuda")
    nsym, qm = 1000, 6
    d_sym = torch.zeros((nsym, 2), dtype=torch.float32, device="cuda")
    d_nv = torch.full((nsym,), 0.01, dtype=torch.float32, device="cuda")
    d_llr = torch.zeros(nsym * qm, dtype=torch.int8, device="cuda")
    d_c_init = dev(np.array([12345], np.int32))

    def chain(stream):
        plan.run(d_tb, d_grid, zero_grids=True, stream=stream)
        oplan.run_ci16(1, d_grid, wire, d_iq16, d_stats=d_stats, stream=stream)
        gpu_ctx.demodulate_soft(qm, 1, nsym, d_sym, d_nv, d_llr, stream=stream)
        gpu_ctx.llr_descramble(d_c_init, 1, nsym * qm, d_llr, nsym * qm, d_llr, nsym * qm, stream=stream)

    def new_inputs():
        tb = cases.random_tb(rng, pdsch)
        d_tb[: tb.size].copy_(torch.from_numpy(tb))
        d_sym.copy_(torch.from_numpy(rng.uniform(-1.2, 1.2, (nsym, 2)).astype(np.float32)))
        return tb

    s = torch.cuda.Stream()
    new_inputs()
    with torch.cuda.stream(s):
        chain(s.cuda_stream)   # warm-up outside the capture (tables, the wire-format run's record buffer)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        chain(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for _ in range(3):
        tb = new_inputs()
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (d_grid, d_iq16, d_stats, d_llr)]
        with torch.cuda.stream(s):
            chain(s.cuda_stream)
        torch.cuda.synchronize()
        for a, b in zip(got, (d_grid, d_iq16, d_stats, d_llr)):
            assert torch.equal(a, b)
        grid = got[0][0].cpu().numpy().view(np.uint16).reshape(nof_ports, 14, nof_subc, 2)
        assert np.array_equal(grid, oracle.pdsch_process(pdsch, tb, nof_ports, nof_subc))
        # the other grid writers, eagerly, on the replayed grid: the oracle's slot
        with torch.cuda.stream(s):
            gpu_ctx.pdcch_process([pdcch], [0], d_grid, nof_ports, nof_subc, stream=s.cuda_stream)
            gpu_ctx.ssb_process([ssb], [0], d_grid, nof_ports, nof_subc, stream=s.cuda_stream)
            gpu_ctx.csi_rs_map([csi], [0], d_grid, nof_ports, nof_subc, stream=s.cuda_stream)
        torch.cuda.synchronize()
        want = oracle.pdsch_process(pdsch, tb, nof_ports, nof_subc)
        want = oracle.pdcch_process(pdcch, want)
        want = oracle.ssb_process(ssb, want)
        want = oracle.csi_rs_map(csi, want)
        assert np.array_equal(d_grid[0].cpu().numpy().view(np.uint16).reshape(nof_ports, 14, nof_subc, 2), want)
    plan.close()
    oplan.close()


# ---- the reference's unit-test configurations of the round-2 components (tests/golden/ref_test_configs2.npz) ----------------
class DeviceApi2:
    """The calls test_oracle.check_ref_test_configs2 needs, through the C ABI."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.pdcch_process, self.pdcch_encode = ctx.pdcch_process_host, ctx.pdcch_encode_host
        self.ssb_process, self.pbch_encode = ctx.ssb_process_host, ctx.pbch_encode_host
        self.csi_rs_map, self.demodulate_soft, self.ofh_compress = ctx.csi_rs_map_host, ctx.demodulate_soft_host, ctx.ofh_compress_host

    def pdcch_validate(self, pdu):
        return self.ctx.lib.nrphy_pdcch_validate(C.byref(pdu))

    def ssb_validate(self, pdu):
        return self.ctx.lib.nrphy_ssb_validate(C.byref(pdu))

    def csi_rs_validate(self, cfg):
        return self.ctx.lib.nrphy_csi_rs_validate(C.byref(cfg))

    def ofdm_demod_slot(self, cfg, iq, slot_index, window_offset):
        plan = lib.OfdmPlan(self.ctx, cfg, iq.shape[0])
        try:
            return plan.demodulate_slot_host(iq, slot_index, window_offset)
        finally:
            plan.close()


@pytest.mark.parametrize("what", ["pdcch", "ssb", "csi", "dm", "od", "ofh", "pe", "pb"])
def test_ref_test_configs2(gpu_ctx, what):
    """All 114 / 240 / 102 / 12 / 20 / 36 / 29 / 232 configurations of the pdcch_processor, ssb_processor, nzp_csi_rs_generator,
    demodulation_mapper, ofdm_demodulator, ofh_compression, pdcch_encoder and pbch_encoder test-data headers on the device; expected
    values from the compiled reference (12 case-E blocks that cross the slot boundary are refused, compression types outside the ABI
    are skipped as recorded in the fixture)."""
    import test_oracle
    g = np.load(os.path.join(cases.GOLDEN, "ref_test_configs2.npz"))
    test_oracle.check_ref_test_configs2(DeviceApi2(gpu_ctx), g, what)
