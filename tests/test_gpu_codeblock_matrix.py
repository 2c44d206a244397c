"""Every compiled copy of the codeblock kernels' output stage (csrc/re_map_device.h, phase_b_grid<QM, L, P, WORDS>) against
the CPU oracle: one small PDU for each of the 80 combinations of modulation order, layer count, port count and precoding path
(wideband weights in scalar registers, or weights per PRG read from memory), all of them in one plan, run in both scrambling
forms and under both dispatches of the codeblock launch.  Every grid and both codeword taps are compared bit for bit with
oracle.pdsch_process; a float64 restatement of modulation, layer mapping and precoding, which shares no code with the oracle,
checks the weight indexing on its own.  The properties the shapes were chosen for are asserted from nrphy_pdsch_derive and
the PDUs themselves in a device-free test.  tests/test_oracle.py pins the oracle's side of the 40 per-PRG PDUs to the
reference's modulator.
"""
import numpy as np
import pytest

import backends
import cases

abi = backends.abi
lib = backends.pkg.lib

RE_CHUNK = cases.RE_CHUNK   # resource elements per work item (csrc/nrphy_internal.h)
WAVE = 64
NOF_PORTS = 4               # every PDU maps into a 4-port grid of its own
GRID_RB = 12
NOF_SUBC = GRID_RB * 12
PRB_START, PRB_COUNT = 1, 10
NOF_SYMBOLS = 12
PRG_SIZE_RB, NOF_PRG = 4, 3
FORMS = {"words": "1", "seeds": "0"}       # NRPHY_SCR_WORDS
DISPATCHES = {"bucket": "2", "mixed": "1"}  # NRPHY_CB_DISPATCH


# ---------------------------------------------------------------------------------------------------------------------
# What a PDU says about its resource elements and its rate matching, restated here in NumPy from the PDU's fields
# ---------------------------------------------------------------------------------------------------------------------
def bit(words, i):
    return (int(words[i // 64]) >> (i % 64)) & 1


def data_re_mask(pdu, nof_subc):
    """[14][nof_subc] bool: the resource elements that carry data (TS 38.211 Section 7.3.1.5/6): the allocated PRBs on the
    allocated symbols, without the DM-RS combs of the CDM groups without data and without the reserved patterns."""
    mask = np.zeros((14, nof_subc), bool)
    prbs = [p for p in range(nof_subc // 12) if bit(pdu.prb_mask, p)]
    for l in range(pdu.start_symbol_index, pdu.start_symbol_index + pdu.nof_symbols):
        for p in prbs:
            mask[l, 12 * p:12 * p + 12] = True
            if (pdu.dmrs_symbol_mask >> l) & 1:
                for group in range(pdu.nof_cdm_groups_without_data):   # type 1: group g sits on the subcarriers k = g mod 2
                    mask[l, 12 * p + group:12 * p + 12:2] = False
    for i in range(pdu.nof_reserved):
        pat = pdu.reserved[i]
        for l in range(14):
            if (pat.symbol_mask >> l) & 1:
                for p in range(nof_subc // 12):
                    if bit(pat.prb_mask, p):
                        for k in range(12):
                            if (pat.re_mask >> k) & 1:
                                mask[l, 12 * p + k] = False
    return mask


def work_items(pdu, d):
    """(first resource element within the PDU, resource elements) of every work item, in the plan's order."""
    lq = pdu.qm * pdu.nof_layers
    items, bit_cb = [], 0
    for cb in range(d["nof_codeblocks"]):
        e = d["rm_length_short"] if cb < d["nof_short_segments"] else d["rm_length_long"]
        for begin in range(0, e // lq, RE_CHUNK):
            items.append((bit_cb // lq + begin, min(RE_CHUNK, e // lq - begin)))
        bit_cb += e
    assert bit_cb == d["codeword_bits"]
    return items


def wrap_status(d):
    """"wrap" when the bit selection of every codeblock runs around the end of the circular buffer (TS 38.212 Section
    5.4.2.1: E bits from k0 on, the filler bits skipped), "straight" when that of none does, else "some"."""
    zc = d["lifting_size"]
    nsys = d["segment_length"] - 2 * zc                   # the filler bits end here in the circular buffer
    fs, fe = min(nsys - d["nof_filler_bits"], d["n_cb"]), min(nsys, d["n_cb"])
    valid = d["n_cb"] - (fe - fs)
    rank0 = d["k0"] if d["k0"] < fs else (fs if d["k0"] < fe else d["k0"] - (fe - fs))
    lengths = ([d["rm_length_short"]] if d["nof_short_segments"] else []) + \
              ([d["rm_length_long"]] if d["nof_short_segments"] < d["nof_codeblocks"] else [])
    wraps = [rank0 + e > valid for e in lengths]
    return "wrap" if all(wraps) else ("some" if any(wraps) else "straight")


def crosses_symbol(pdu, d):
    """Whether a group of WAVE consecutive resource elements of a work item starts in one OFDM symbol and ends in another."""
    start = np.concatenate([[0], np.cumsum(data_re_mask(pdu, NOF_SUBC).sum(axis=1))])
    symbol_of = lambda re: int(np.searchsorted(start, re, side="right")) - 1
    for re0, count in work_items(pdu, d):
        for r0 in range(0, count, WAVE):
            if symbol_of(re0 + r0) != symbol_of(re0 + r0 + min(WAVE, count - r0) - 1):
                return True
    return False


# ---------------------------------------------------------------------------------------------------------------------
# The fixture: one PDU per (Qm, layers, ports, precoding path), from a fixed seed, no device involved
# ---------------------------------------------------------------------------------------------------------------------
def combination_name(c):
    return "Qm %d, %d layer(s), %d port(s), %s" % (c["qm"], c["layers"], c["ports"], ("per-PRG" if c["per_prg"] else "wideband") +
                                                  (", allocation beyond the last PRG" if c.get("beyond") else ""))


def build_matrix():
    """[dict(qm, layers, ports, per_prg, pdu, tb, derived, wrap, cdm1, reserved)] for the 80 combinations.  The attributes
    rotate with the position of the combination in its (Qm, layers) set and with Qm, so that none of them follows the
    precoding path; the transport block size is the first of a few rates at which the shape has the wanted rate-matching
    case and the work items the census asks for."""
    rng = np.random.default_rng(808080)
    out = []
    for q, qm in enumerate((2, 4, 6, 8), start=1):
        for layers in (1, 2, 3, 4):
            combos = [(ports, per_prg) for ports in range(layers, 5) for per_prg in (False, True)]
            n = len(combos)
            for i, (ports, per_prg) in enumerate(combos):
                want_wrap = (i + q + layers) % 2 == 0
                cdm1 = layers <= 2 and (i + q) % 4 == 1
                has_reserved = (i - q) % min(n, 3) == 0
                start = (i + layers) % 3
                dmrs = (start + 2, start + 9)
                reserved = []
                if has_reserved:   # on two symbols without DM-RS: a table-driven symbol kind
                    reserved = [([2, 3, 6, 9], [0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0],
                                 [1 if l in (start + 5, start + 6) else 0 for l in range(14)])]
                nof_prg = NOF_PRG if per_prg else 1
                w = ((rng.standard_normal((nof_prg, ports, layers)) + 1j * rng.standard_normal((nof_prg, ports, layers))) / 2)
                common = dict(slot_index=int(rng.integers(0, 20)), rnti=int(rng.integers(1, 65520)), bwp_start_rb=0,
                              bwp_size_rb=GRID_RB, qm=qm, n_id=int(rng.integers(0, 1024)), dmrs_symbols=dmrs,
                              scrambling_id=int(rng.integers(0, 65536)), n_scid=i & 1, ref_point=(i >> 1) & 1,
                              nof_cdm_groups_without_data=1 if cdm1 else 2, prb_start=PRB_START, prb_count=PRB_COUNT,
                              start_symbol=start, nof_symbols=NOF_SYMBOLS, reserved=reserved,
                              ratio_dmrs_dB=(0.0, -3.0, 3.0)[i % 3], ratio_data_dB=(-3.0, 0.0, 1.5, 2.25)[(i + q) % 4],
                              precoding=w.astype(np.complex64), prg_size_rb=PRG_SIZE_RB if per_prg else abi.MAX_RB)
                found = None
                base_graph = 1 + ((i >> 1) + q) % 2
                rvs = (0, 2, 3) if want_wrap else (0, 1)
                rv = rvs[(i + q) % len(rvs)]
                probe = abi.make_pdu(base_graph=base_graph, rv=rv, tb_size_bytes=8, **common)
                g_bits = int(data_re_mask(probe, NOF_SUBC).sum()) * qm * layers
                for rate in ((0.16, 0.12, 0.2, 0.08, 0.1) if want_wrap else (0.7, 0.8, 0.6, 0.75, 0.9, 0.5)):
                    pdu = abi.make_pdu(base_graph=base_graph, rv=rv, tb_size_bytes=max(4, int(g_bits * rate) // 8), **common)
                    if lib.validate(pdu) != 0:
                        continue
                    d = lib.derive(pdu)
                    items = work_items(pdu, d)
                    if (wrap_status(d) == ("wrap" if want_wrap else "straight") and len(items) >= 2 and items[-1][1] % WAVE != 0
                            and crosses_symbol(pdu, d)):
                        found = (pdu, d)
                        break
                assert found is not None, "no shape for %s" % combination_name(dict(qm=qm, layers=layers, ports=ports, per_prg=per_prg))
                pdu, d = found
                tb = rng.integers(0, 256, pdu.tb_size_bytes, dtype=np.uint8)
                tb.setflags(write=False)
                out.append(dict(qm=qm, layers=layers, ports=ports, per_prg=per_prg, pdu=pdu, tb=tb, derived=d,
                                wrap=want_wrap, cdm1=cdm1, reserved=has_reserved))
    return out


MATRIX = build_matrix()


def per_prg_combinations():
    """The 40 combinations with weights per PRG (tests/test_oracle.py pins the oracle's data RE of these to the reference)."""
    return [c for c in MATRIX if c["per_prg"]]


def build_beyond_last_prg():
    """The 40 per-PRG combinations again with the last PRG taken away: PRBs 8-10 of the allocation then lie beyond the last
    PRG and take its weights (include/mi355_nrphy.h).  The reference is undefined there, so these are not part of the pin in
    tests/test_oracle.py; the oracle and the float64 model are the yardsticks."""
    out = []
    for c in per_prg_combinations():
        pdu = abi.PdschPdu.from_buffer_copy(bytes(c["pdu"]))
        pdu.nof_prg = NOF_PRG - 1
        cases.attach_weights(pdu, c["pdu"]._keepalive.reshape(NOF_PRG, -1)[:NOF_PRG - 1].copy())
        out.append(dict(c, pdu=pdu, beyond=True))
    return out


BEYOND = build_beyond_last_prg()
SETS = {"matrix": MATRIX, "beyond": BEYOND}


def test_matrix_census():
    """Device-free: the fixture holds what the GPU tests below rely on, asserted from nrphy_pdsch_derive and the PDUs."""
    want = {(qm, layers, ports, per_prg) for qm in (2, 4, 6, 8) for layers in (1, 2, 3, 4) for ports in range(layers, 5)
            for per_prg in (False, True)}
    have = [(c["qm"], c["layers"], c["ports"], c["per_prg"]) for c in MATRIX]
    assert len(want) == 80 and len(have) == 80 and set(have) == want
    oracle = backends.oracle()
    for c in MATRIX:
        pdu, name = c["pdu"], combination_name(c)
        assert lib.validate(pdu) == 0 and oracle.validate(pdu) == 0, name
        d = lib.derive(pdu)
        assert d == c["derived"] == oracle.derive(pdu), name
        assert (pdu.qm, pdu.nof_layers, pdu.nof_ports) == (c["qm"], c["layers"], c["ports"]), name
        mask = data_re_mask(pdu, NOF_SUBC)
        assert int(mask.sum()) == d["nof_re"], name                     # the NumPy RE mask agrees with the library's count
        assert bin(pdu.dmrs_symbol_mask).count("1") == 2 and pdu.nof_symbols == NOF_SYMBOLS, name
        subc = np.flatnonzero(mask.any(axis=0))
        assert subc[0] == 12 * PRB_START and subc[-1] == 12 * (PRB_START + PRB_COUNT) - 1, name
        if c["per_prg"]:
            # the path phase_b takes: weights per PRG from memory (P = 0)
            assert pdu.nof_prg == NOF_PRG >= 3 and pdu.prg_size_rb == PRG_SIZE_RB, name
            prg = np.minimum(subc // (12 * pdu.prg_size_rb), pdu.nof_prg - 1)
            assert set(prg.tolist()) == set(range(pdu.nof_prg)), name    # every PRG touched, the last one included
            size = 12 * pdu.prg_size_rb
            assert 0 < int((prg == 0).sum()) < size and 0 < int((prg == pdu.nof_prg - 1).sum()) < size, name   # both ends partly
            assert 12 * (PRB_START + PRB_COUNT) <= pdu.nof_prg * size, name  # inside the PRGs: defined in the reference's mapper too
        else:
            assert pdu.nof_prg == 1, name                                # the path with the weights in scalar registers (P = ports)
        items = work_items(pdu, d)
        assert len(items) >= 2 and sum(n for _, n in items) == d["nof_re"], name
        assert items[-1][1] % WAVE != 0, name
        assert crosses_symbol(pdu, d), name
        assert wrap_status(d) == ("wrap" if c["wrap"] else "straight"), name
        # symbol kinds: a symbol whose data RE are not one contiguous run is table driven (csrc/pdsch_plan_build.cpp)
        table_rows = [l for l in range(14) if mask[l].any() and np.flatnonzero(mask[l])[-1] - np.flatnonzero(mask[l])[0] + 1 != mask[l].sum()]
        dmrs_rows = [l for l in range(14) if (pdu.dmrs_symbol_mask >> l) & 1]
        assert c["cdm1"] == (pdu.nof_cdm_groups_without_data == 1), name
        if c["cdm1"]:
            assert all(l in table_rows and mask[l].sum() == 6 * PRB_COUNT for l in dmrs_rows), name   # data on the DM-RS symbols
        else:
            assert not any(mask[l].any() for l in dmrs_rows), name
        assert c["reserved"] == (pdu.nof_reserved > 0), name
        if c["reserved"]:
            rows = [l for l in range(14) if (pdu.reserved[0].symbol_mask >> l) & 1]
            assert rows and all(l not in dmrs_rows and l in table_rows for l in rows), name
    for qm in (2, 4, 6, 8):
        for layers in (1, 2, 3, 4):
            group = [c for c in MATRIX if (c["qm"], c["layers"]) == (qm, layers)]
            assert {c["wrap"] for c in group} == {True, False}, (qm, layers)
            assert any(c["reserved"] for c in group), (qm, layers)
            assert any(c["cdm1"] for c in group) == (layers <= 2), (qm, layers)
    assert {c["pdu"].ldpc_base_graph for c in MATRIX} == {1, 2}
    assert {c["pdu"].rv for c in MATRIX} >= {0, 1, 2}
    # no attribute follows the precoding path (or the other way round)
    for attribute in ("wrap", "cdm1", "reserved"):
        assert {(c[attribute], c["per_prg"]) for c in MATRIX} == {(a, b) for a in (True, False) for b in (True, False)}, attribute
    assert {(c["wrap"], c["pdu"].ldpc_base_graph) for c in MATRIX} == {(a, b) for a in (True, False) for b in (1, 2)}
    for per_prg in (False, True):
        assert {c["pdu"].ldpc_base_graph for c in MATRIX if c["per_prg"] == per_prg} == {1, 2}
        assert len({c["pdu"].rv for c in MATRIX if c["per_prg"] == per_prg}) >= 3


def test_beyond_last_prg_census():
    """Device-free: in every PDU of the second set the last PRG holds RE of its own and RE of PRBs beyond it."""
    assert [(c["qm"], c["layers"], c["ports"]) for c in BEYOND] == [(c["qm"], c["layers"], c["ports"]) for c in per_prg_combinations()]
    for c in BEYOND:
        pdu, name = c["pdu"], combination_name(c)
        assert lib.validate(pdu) == 0 and lib.derive(pdu) == c["derived"], name
        assert pdu.nof_prg == NOF_PRG - 1 >= 2 and pdu.prg_size_rb == PRG_SIZE_RB, name
        subc = np.flatnonzero(data_re_mask(pdu, NOF_SUBC).any(axis=0))
        prg = subc // (12 * pdu.prg_size_rb)
        assert (prg == pdu.nof_prg - 1).any() and (prg >= pdu.nof_prg).any() and (prg == 0).any(), name
        w = pdu._keepalive.reshape(pdu.nof_prg, -1)
        assert np.array_equal(w, per_prg_weights(c)[:pdu.nof_prg]), name


def per_prg_weights(c):
    """The weights of the matrix PDU the combination of the second set was made from, [NOF_PRG][...] float32."""
    twin = next(m for m in per_prg_combinations() if (m["qm"], m["layers"], m["ports"]) == (c["qm"], c["layers"], c["ports"]))
    return twin["pdu"]._keepalive.reshape(NOF_PRG, -1)


# ---------------------------------------------------------------------------------------------------------------------
# An independent float64 model of what follows the scrambled codeword: TS 38.211 Sections 5.1, 7.3.1.3 and 7.3.1.4
# ---------------------------------------------------------------------------------------------------------------------
def qam_points(bits, qm):
    """TS 38.211 Sections 5.1.3-5.1.6: bits [n][qm] (0 / 1) -> complex128 [n]."""
    s = 1.0 - 2.0 * bits.astype(np.float64)
    if qm == 2:
        re, im, norm = s[:, 0], s[:, 1], 2.0
    elif qm == 4:
        re, im, norm = s[:, 0] * (2 - s[:, 2]), s[:, 1] * (2 - s[:, 3]), 10.0
    elif qm == 6:
        re, im, norm = s[:, 0] * (4 - s[:, 2] * (2 - s[:, 4])), s[:, 1] * (4 - s[:, 3] * (2 - s[:, 5])), 42.0
    else:
        re = s[:, 0] * (8 - s[:, 2] * (4 - s[:, 4] * (2 - s[:, 6])))
        im = s[:, 1] * (8 - s[:, 3] * (4 - s[:, 5] * (2 - s[:, 7])))
        norm = 170.0
    return (re + 1j * im) / np.sqrt(norm)


def model_grid(c, scrambled):
    """(exact [ports][14][nof_subc] complex128, magnitude sum [ports][14][nof_subc] float64, data RE mask): the data RE of the
    PDU from its scrambled codeword (packed MSB first) -- modulation, the amplitude of ratio_pdsch_data_to_sss_dB, layer
    mapping (symbol i goes to layer i mod L of RE i div L), and for subcarrier k and port p the sum over the layers of
    x_l w[min(k div (12 prg_size_rb), nof_prg - 1)][p][l].  The second array is sum_l |x_l| |w_l|, for the tolerance."""
    pdu, d = c["pdu"], c["derived"]
    layers, ports = pdu.nof_layers, pdu.nof_ports
    bits = np.unpackbits(np.asarray(scrambled))[:d["codeword_bits"]].reshape(-1, pdu.qm)
    x = qam_points(bits, pdu.qm) * 10.0 ** (-float(pdu.ratio_pdsch_data_to_sss_dB) / 20.0)
    x = x.reshape(d["nof_re"], layers)
    w = pdu._keepalive.astype(np.float64).reshape(pdu.nof_prg, ports, layers, 2)
    w = w[..., 0] + 1j * w[..., 1]
    mask = data_re_mask(pdu, NOF_SUBC)
    exact = np.zeros((ports, 14, NOF_SUBC), np.complex128)
    bound = np.zeros((ports, 14, NOF_SUBC), np.float64)
    symbol, subc = np.nonzero(mask)                  # row-major: symbols in order, subcarriers ascending within a symbol
    prg = np.minimum(subc // (12 * pdu.prg_size_rb), pdu.nof_prg - 1)
    for p in range(ports):
        exact[p, symbol, subc] = (x * w[prg, p, :]).sum(axis=1)
        bound[p, symbol, subc] = (np.abs(x) * np.abs(w[prg, p, :])).sum(axis=1)
    return exact, bound, mask


def assert_model_close(c, grid_u16, scrambled):
    """Per real and imaginary component: |got - exact| <= 2^-8 |exact| + 2^-20 sum_l |x_l| |w_l|.  The first term is half a
    bf16 unit in the last place (8 significant bits), the second a generous bound for the float32 arithmetic before that
    rounding (three roundings in the scaled weight, two in a product, L - 1 in the sum: well under 16 units of 2^-24)."""
    exact, bound, mask = model_grid(c, scrambled)
    ports = c["pdu"].nof_ports
    got = backends.grid_to_complex(grid_u16[:ports]).astype(np.complex128)
    name = combination_name(c)
    for part in (np.real, np.imag):
        err = np.abs(part(got) - part(exact))[:, mask]
        tol = (2.0 ** -8 * np.abs(part(exact)) + 2.0 ** -20 * bound)[:, mask]
        bad = np.argwhere(err > tol)
        assert bad.size == 0, "%s: %d data RE off the float64 model, first (port, RE) %s: error %.3e, tolerance %.3e" % (
            name, len(bad), bad[0].tolist(), err[tuple(bad[0])], tol[tuple(bad[0])])


@pytest.mark.parametrize("which", list(SETS))
def test_model_agrees_with_the_oracle_on_the_cpu(want, which):
    """Device-free: the float64 model against the oracle's grids, so that the model itself is known to be right before a GPU
    grid meets it."""
    for c, (grid, _, scr) in zip(SETS[which], want[which]):
        assert_model_close(c, grid, scr)


# ---------------------------------------------------------------------------------------------------------------------
# The GPU runs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def want():
    """oracle.pdsch_process of every PDU of both sets, once per module, read-only: {set: [(grid uint16, rate-matched,
    scrambled codeword)]}."""
    oracle = backends.oracle()
    out = {}
    for which, combinations in SETS.items():
        out[which] = []
        for c in combinations:
            res = oracle.pdsch_process(c["pdu"], c["tb"], NOF_PORTS, NOF_SUBC, taps=True, codeword_bits=c["derived"]["codeword_bits"])
            for a in res:
                a.setflags(write=False)
            out[which].append(res)
    return out


@pytest.fixture(scope="module")
def run_matrix(gpu_ctx_for):
    """run_matrix(form, dispatch, which="matrix") -> dict(grids uint16 [n][ports][14][subc][2], rm, scr, offsets, form,
    dispatch): all the PDUs of the set (the 80 of the matrix) in ONE plan, each on a grid of its own, on a context created under
    that form and dispatch; one run per triple, kept."""
    import torch
    from pusch_chest_model import dev
    done = {}

    def run(form, dispatch, which="matrix"):
        if (form, dispatch, which) in done:
            return done[(form, dispatch, which)]
        combinations = SETS[which]
        ctx = gpu_ctx_for({"NRPHY_SCR_WORDS": FORMS[form], "NRPHY_CB_DISPATCH": DISPATCHES[dispatch]})
        n = len(combinations)
        offs, pos = [], 0
        for c in combinations:
            offs.append(pos)
            pos += (len(c["tb"]) + 15) & ~15
        buf = np.zeros(pos + 16, np.uint8)
        for o, c in zip(offs, combinations):
            buf[o:o + len(c["tb"])] = c["tb"]
        plan = lib.PdschPlan(ctx, [c["pdu"] for c in combinations], offs, list(range(n)), n, NOF_PORTS, NOF_SUBC)
        try:
            res = dict(form=plan.scrambling_form, dispatch=plan.codeblock_dispatch)
            d_grid = torch.full((n, NOF_PORTS, 14, NOF_SUBC), 0x7FFF7FFF, dtype=torch.int32, device="cuda")
            d_rm = torch.zeros(plan.codeword_bits // 8, dtype=torch.uint8, device="cuda")
            d_scr = torch.zeros(plan.codeword_bits // 8, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            plan.run(dev(buf), d_grid, d_cw_rm=d_rm, d_cw_scr=d_scr, zero_grids=True)
            ctx.synchronize()
            res["grids"] = d_grid.cpu().numpy().view(np.uint16).reshape(n, NOF_PORTS, 14, NOF_SUBC, 2)
            res["rm"], res["scr"] = d_rm.cpu().numpy(), d_scr.cpu().numpy()
            res["offsets"] = [plan.codeword_offset(i) // 8 for i in range(n)]
        finally:
            plan.close()
        done[(form, dispatch, which)] = res
        return res

    return run


def mismatch(got, grid):
    bad = np.argwhere(got != grid)
    return "%d words differ, first at (port, symbol, subcarrier, re/im) %s" % (len(bad), bad[0].tolist())


def assert_bit_exact(res, combinations, want, form, dispatch):
    assert res["form"] == form and res["dispatch"] == dispatch
    failures = []
    for i, (c, (grid, orm, oscr)) in enumerate(zip(combinations, want)):
        o = res["offsets"][i]
        if not np.array_equal(res["rm"][o:o + len(orm)], orm):
            failures.append("%s: rate-matched codeword" % combination_name(c))
        if not np.array_equal(res["scr"][o:o + len(oscr)], oscr):
            failures.append("%s: scrambled codeword" % combination_name(c))
        if not np.array_equal(res["grids"][i], grid):
            failures.append("%s: grid, %s" % (combination_name(c), mismatch(res["grids"][i], grid)))
    assert not failures, "%s form, %s dispatch: %d of %d checks failed:\n%s" % (form, dispatch, len(failures), 3 * len(combinations),
                                                                                "\n".join(failures[:12]))


def assert_model(res, combinations):
    for i, c in enumerate(combinations):
        o = res["offsets"][i]
        nb = (c["derived"]["codeword_bits"] + 7) // 8
        assert_model_close(c, res["grids"][i], res["scr"][o:o + nb])


@pytest.mark.gpu
@pytest.mark.parametrize("dispatch", list(DISPATCHES))
@pytest.mark.parametrize("form", list(FORMS))
def test_matrix_bit_exact_against_the_oracle(run_matrix, want, form, dispatch):
    """All 80 combinations in one plan: every grid (the planes of the ports a PDU does not use included: the run clears grids
    that held 0x7FFF7FFF) and both codeword taps bit for bit; the plan took the form and the dispatch asked for."""
    assert_bit_exact(run_matrix(form, dispatch), MATRIX, want["matrix"], form, dispatch)


@pytest.mark.gpu
def test_matrix_four_runs_give_identical_grids(run_matrix):
    first = run_matrix("words", "bucket")
    for form in FORMS:
        for dispatch in DISPATCHES:
            res = run_matrix(form, dispatch)
            for i, c in enumerate(MATRIX):
                assert np.array_equal(res["grids"][i], first["grids"][i]), "%s: %s form, %s dispatch against words, bucket" % (
                    combination_name(c), form, dispatch)
            assert np.array_equal(res["rm"], first["rm"]) and np.array_equal(res["scr"], first["scr"]), (form, dispatch)


@pytest.mark.gpu
@pytest.mark.parametrize("dispatch", list(DISPATCHES))
@pytest.mark.parametrize("form", list(FORMS))
def test_matrix_data_re_against_the_float64_model(run_matrix, form, dispatch):
    """The GPU grid's data RE against the float64 restatement, from the GPU's own scrambled codeword tap (which the test above
    compares bit for bit): an index mistake in PRG, port or layer that the kernel and the oracle shared would show here."""
    assert_model(run_matrix(form, dispatch), MATRIX)


@pytest.mark.gpu
@pytest.mark.parametrize("dispatch", list(DISPATCHES))
@pytest.mark.parametrize("form", list(FORMS))
def test_allocation_beyond_the_last_prg(run_matrix, want, form, dispatch):
    """The 40 per-PRG combinations with one PRG fewer than the allocation spans, in one plan: the PRBs beyond the last PRG take
    its weights.  Bit for bit against the oracle, and against the float64 model, which states that rule on its own."""
    res = run_matrix(form, dispatch, "beyond")
    assert_bit_exact(res, BEYOND, want["beyond"], form, dispatch)
    assert_model(res, BEYOND)
