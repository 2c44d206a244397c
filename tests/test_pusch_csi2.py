"""PUSCH processor with CSI part 2 (nrphy_pusch_csi2_*) on the GPU: the PDUs (g)-(j) of tests/pusch_csi2_cases.py.

The transmitter is the one of tests/test_pusch_processor.py with a CSI part 1 payload chosen so that the description gives the
size the test wants, a part 2 payload of that size, and the UL-SCH rate-matched to what the part 2 leaves.  The comparison partner
is the chain driven by this test through the existing entry points -- nrphy_pusch_chest_run, _demod_run, nrphy_ulsch_demux_* with
the size, nrphy_uci_decoder_run, nrphy_pusch_decode_batch -- with the size the test knows.  Every comparison is byte for byte:
transport blocks, HARQ soft and state blocks, every UCI payload byte and status, both result records.

Reference pin: tests/golden/record_pusch_csi2_reference.cpp ran the reference's pusch_processor_impl with pdu.uci.csi_part2_size set on
the grids of (g), (h) and (i) for every selectable size at the good SNR and of (h) at -12 dB; the CRC verdict, the transport block,
the three UCI payloads and the three statuses are pinned exactly.  (j) lies where the reference's streaming demultiplexer and the
up-front placement differ and is compared with the hand-driven chain only.
"""
import ctypes as C
import os

import numpy as np
import pytest

import backends
import pusch_chest_model as chest_model
import pusch_csi2_cases as K
import test_pusch_processor as T
import uci_model
from test_pusch_channel_estimator import BETA, MEAS_DTYPE

abi = backends.abi
lib = backends.pkg.lib
dev, as_i32 = chest_model.dev, chest_model.as_i32
NPORTS, NSUBC, OPTIONS = T.NPORTS, T.NSUBC, T.OPTIONS
CSI2_DTYPE = np.dtype(abi.PuschCsi2Result)
HARQ_FILL, HARQ_TAIL = 0x11, 256


def plain_of(pdu):
    """The PDU without its description: what the existing entry points take."""
    p = abi.PuschPdu.from_buffer_copy(pdu)
    p.nof_csi_part2_entries = 0
    return p


class Variant:
    """One PDU with the part 2 size a transmission has: the configurations of the existing stages, written out by the test."""

    def __init__(self, name, pdu, desc, size):
        self.name, self.pdu, self.size, self.described = name, pdu, size, desc.nof_entries != 0
        self.base = lib.pusch_proc_derive(plain_of(pdu), OPTIONS, NPORTS, NSUBC)
        self.sizes, infos = lib.pusch_csi2_variants(pdu, desc, OPTIONS, NPORTS, NSUBC)
        self.index = self.sizes.index(size)
        self.info = infos[self.index]
        qm = pdu.modulation
        self.demux = K.demux_with_part2(self.base.demux, size, self.info) if self.base.nof_uci else None
        self.nof_sch_bits = self.info.nof_ul_sch_bits if pdu.has_codeword and self.base.nof_uci else self.base.nof_sch_bits
        self.uci = [(part, abi.make_uci_decoder(bits, enc, qm)) for part, bits, enc in (
            ("harq", pdu.nof_harq_ack, self.info.nof_harq_ack_bits), ("csi1", pdu.nof_csi_part1, self.info.nof_csi_part1_bits),
            ("csi2", size, self.info.nof_csi_part2_bits)) if bits]
        self.decoder = None
        if self.base.has_decoder:
            self.decoder = abi.PuschDecoderCfg.from_buffer_copy(self.base.decoder)
            self.decoder.nof_ch_symbols = self.nof_sch_bits // qm


def transmit(ctx, v, rng, channel_rng):
    """T.transmit with a part 2: the payloads and the noiseless received grid of one Variant.  The channel has a generator of its
    own, so that it does not depend on the payloads."""
    pdu, d, s = v.pdu, v.base, T.Sent()
    qm, layers = pdu.modulation, pdu.nof_tx_layers
    s.tb = rng.integers(0, 256, pdu.tb_size_bytes, dtype=np.uint8)
    sch = np.zeros(v.nof_sch_bits, np.uint8)
    if d.has_decoder:
        sch, _ = ctx.pdsch_encode_host(pdu.ldpc_base_graph, pdu.rv, qm, d.decoder.nref, layers, v.nof_sch_bits // qm, s.tb)
    s.harq = rng.integers(0, 2, pdu.nof_harq_ack, dtype=np.uint8)
    s.csi1 = K.part1_for(v.name, v.size, rng) if v.described else rng.integers(0, 2, pdu.nof_csi_part1, dtype=np.uint8)
    s.csi2 = rng.integers(0, 2, v.size, dtype=np.uint8)
    if d.nof_uci:
        coded = [uci_model.encode(m, e, qm) if m.size else np.zeros(0, np.uint8)
                 for m, e in ((s.harq, v.info.nof_harq_ack_bits), (s.csi1, v.info.nof_csi_part1_bits), (s.csi2, v.info.nof_csi_part2_bits))]
        codeword = uci_model.ulsch_multiplex(v.demux, sch, coded[0], coded[1], coded[2])
    else:
        codeword = sch
    assert codeword.size == d.codeword_bits
    symbols = T.modulate(T.scramble(codeword, pdu.rnti, pdu.n_id), qm).reshape(-1, layers)
    prbs = chest_model.prbs_of(d.chest)
    subc = (12 * np.array(prbs)[:, None] + np.arange(12)).ravel()
    x = np.zeros((layers, 14, NSUBC), np.complex128)
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
    k = np.arange(NSUBC)
    H = np.zeros((pdu.nof_rx_ports, layers, NSUBC), np.complex128)
    for p in range(pdu.nof_rx_ports):
        for layer in range(layers):
            g = (1.0 if (p % layers) == layer else 0.35) * np.exp(1j * channel_rng.uniform(0, 2 * np.pi))
            H[p, layer] = g * np.exp(-2j * np.pi * k * 3 / 4096.0) * (1 + 0.3 * np.exp(-2j * np.pi * k * channel_rng.uniform(1, 8) / 4096.0))
    rot = np.exp(2j * np.pi * (250.0 / 15000.0) * np.array(chest_model.epochs(0), np.float64))
    s.clean = np.zeros((NPORTS, 14, NSUBC), np.complex128)
    for p in range(pdu.nof_rx_ports):
        s.clean[pdu.rx_ports[p]] = np.einsum("lk,lmk->mk", H[p], x) * rot[:, None]
    return s


class Layout(T.Layout):
    """T.Layout with a place for every PDU's part 2 payload behind the other UCI bytes, and a tail behind the HARQ arena."""

    def __init__(self, names, plain):
        super().__init__(plain, OPTIONS)
        self.csi2 = []
        for n in names:
            self.csi2.append(self.uci_bytes)
            self.uci_bytes += max(K.SIZES.get(n, [0])) + 3
        self.harq_used = self.harq_bytes
        self.harq_bytes += HARQ_TAIL


def fresh_harq(layout):
    """The HARQ arena before a first transmission: every soft and state block zeroed -- a soft buffer limited by N_ref is not
    written beyond it, and the decoder reads the whole block --, HARQ_FILL between and behind the blocks."""
    import torch
    arena = torch.full((layout.harq_bytes,), HARQ_FILL, dtype=torch.uint8, device="cuda")
    for soft_at, state_at, (soft, state) in zip(layout.soft, layout.state, layout.sizes):
        arena[soft_at:soft_at + soft] = 0
        arena[state_at:state_at + state] = 0
    return arena


class Buffers(T.Buffers):
    def __init__(self, layout, n, d_harq=None):
        super().__init__(layout, n, fresh_harq(layout) if d_harq is None else d_harq)
        self.csi2_whole, self.csi2 = T.guarded(n * CSI2_DTYPE.itemsize)
        self.layout = layout

    def read(self):
        out = super().read()
        assert T.guards_intact(self.csi2_whole)
        assert (out["harq"][self.layout.harq_used:] == HARQ_FILL).all()  # nothing behind the last state block
        out["csi2"] = self.csi2.cpu().numpy().copy().view(CSI2_DTYPE)
        return out


class HandChain:
    """T.HandChain for Variants: the demultiplexer gets the part 2 size, the UCI decoder a third message, the transport-block
    decoder the shorter length."""

    def __init__(self, ctx, variants, layout, gidx, ngrids):
        import torch
        self.ctx, self.v, self.layout, self.n = ctx, variants, layout, len(variants)
        bases = [v.base for v in variants]
        sizes = [d.chest.nof_tx_layers * d.chest.nof_rx_ports * 14 * NSUBC for d in bases]
        offs = [int(o) for o in np.cumsum([0] + sizes)[:-1]]
        self.cplan = lib.PuschChestPlan(ctx, [d.chest for d in bases], gidx, ngrids, NPORTS, NSUBC, offs)
        self.dplan = lib.PuschDemodPlan(ctx, [d.demod for d in bases], gidx, ngrids, NPORTS, NSUBC, offs)
        self.stride = T.align(max(d.codeword_bits for d in bases), 16)
        self.with_uci = [i for i, v in enumerate(variants) if v.uci]
        self.sch_off, self.status_of, self.demux, self.uci_plan = {}, {}, None, None
        sch = llr = 0
        stream_off = {"harq": [], "csi1": [], "csi2": []}
        cfgs, llr_offs, msg_offs = [], [], []
        for i in self.with_uci:
            v = variants[i]
            self.sch_off[i] = sch
            sch += T.align(v.nof_sch_bits, 16)
            for part in stream_off:
                stream_off[part].append(0)
            msg = {"harq": layout.uci[i], "csi1": layout.uci[i] + v.pdu.nof_harq_ack, "csi2": layout.csi2[i]}
            for part, cfg in v.uci:
                stream_off[part][-1] = llr
                self.status_of[(i, part)] = len(cfgs)
                cfgs.append(cfg)
                llr_offs.append(llr)
                msg_offs.append(msg[part])
                llr += T.align(cfg.llr_length, 16)
        if self.with_uci:
            self.demux = lib.UlschDemuxPlan(ctx, [abi.make_ulsch_demux(**variants[i].demux) for i in self.with_uci],
                                            [i * self.stride for i in self.with_uci], [self.sch_off[i] for i in self.with_uci],
                                            stream_off["harq"], stream_off["csi1"], stream_off["csi2"])
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

    def run(self, d_grid, B):
        L = self.layout
        self.cplan.run(d_grid, self.ce, self.nv, self.meas)
        self.dplan.run(d_grid, self.ce, self.nv, self.llr, self.stride, self.sinr)
        if self.demux is not None:
            self.demux.run(self.llr, self.sch, self.uci_llr, self.uci_llr, self.uci_llr)
            self.uci_plan.run(self.uci_llr, B.uci, self.status)
        for i, v in enumerate(self.v):
            if v.decoder is not None:
                llr = self.sch[self.sch_off[i]:] if v.uci else self.llr[i]
                self.ctx.pusch_decode_batch(v.decoder, 1, llr, v.nof_sch_bits, B.harq[L.soft[i]:].view(T.torch_int8()), B.harq[L.state[i]:],
                                            B.tb[L.tb[i]:], v.decoder.tb_size_bytes, self.res[i])

    def read(self):
        return dict(res=self.res.cpu().numpy().view(np.uint32).copy(), status=self.status.cpu().numpy().view(np.uint32).copy(),
                    sinr=self.sinr.cpu().numpy().copy(), meas=self.meas.cpu().numpy().reshape(-1).view(MEAS_DTYPE).reshape(self.n, 4, 2).copy(),
                    status_of=self.status_of)

    def close(self):
        for p in (self.cplan, self.dplan, self.demux, self.uci_plan):
            if p is not None:
                p.close()


class Scenario:
    """PDUs `names`, each on a grid of its own, the ones with a description transmitted with part 2 of sizes[name] bits."""

    def __init__(self, ctx, names, sizes, seed=2025, described=True, **override):
        self.names = names
        self.pdus, self.descs = K.make(names, **override)
        if not described:  # the same PDUs without their descriptions, sent without part 2: what nrphy_pusch_proc_run takes
            self.pdus, self.descs, sizes = [plain_of(p) for p in self.pdus], [abi.make_pusch_csi2_desc(()) for _ in names], {}
        self.plain = [plain_of(p) for p in self.pdus]
        self.sent_as = [Variant(n, p, d, sizes.get(n, 0)) for n, p, d in zip(names, self.pdus, self.descs)]
        # generators per PDU, so that a PDU is sent over the same channel alone and in a batch, whatever its part 2
        self.sent = [transmit(ctx, v, np.random.default_rng([seed, ord(v.name)]), np.random.default_rng([seed, ord(v.name), 1]))
                     for v in self.sent_as]
        self.layout = Layout(names, self.plain)
        self.gidx = list(range(len(names)))

    def grids(self, seed=77, snr=None):
        rng = np.random.default_rng(seed)
        return np.stack([T.noisy(s, T.GOOD_SNR[(p.modulation, p.nof_tx_layers)] if snr is None else snr, rng)
                         for s, p in zip(self.sent, self.pdus)])

    def plan(self, ctx):
        L = self.layout
        return lib.PuschCsi2Plan(ctx, self.pdus, self.descs, OPTIONS, self.gidx, len(self.names), NPORTS, NSUBC, L.soft, L.state, L.tb,
                                 L.uci, L.csi2)

    def run_plan(self, ctx, plan, d_grid, d_harq=None):
        B = Buffers(self.layout, len(self.names), d_harq)
        plan.run(d_grid, B.harq, B.tb, B.uci, B.result, B.csi2)
        ctx.synchronize()
        return B.read()

    def run_hand(self, ctx, d_grid, d_harq=None, received_as=None):
        """received_as: the Variants the receiver is expected to find; those sent unless given."""
        chain = HandChain(ctx, received_as or self.sent_as, self.layout, self.gidx, len(self.names))
        H = Buffers(self.layout, len(self.names), d_harq)
        chain.run(d_grid, H)
        ctx.synchronize()
        want, want_buf = chain.read(), H.read()
        chain.close()
        return want_buf, want

    def without_part2(self):
        return [Variant(n, p, d, 0) for n, p, d in zip(self.names, self.pdus, self.descs)]

    def check(self, got, want_buf, want, received_as=None):
        """Everything the processor wrote against the hand-driven chain, and the part 2 records against what the test knows."""
        variants = received_as or self.sent_as
        T.assert_equal_to_the_hand_chain(self.names, self.plain, [v.base for v in variants], self.layout, got, want_buf, want,
                                         OPTIONS.csi_sinr_calc_method)
        for i, v in enumerate(variants):
            r, what = got["csi2"][i], (self.names[i], v.size)
            status = want["status"][want["status_of"][(i, "csi2")]] if v.size else abi.UCI_STATUS_UNKNOWN
            assert (r["status"], r["nof_csi_part2"], r["csi_part2_offset"], r["nof_enc_bits"], r["variant"], r["reserved_"]) == \
                (status, v.size, self.layout.csi2[i] if v.size else 0, v.info.nof_csi_part2_bits, v.index, 0), what
            assert r["nof_ul_sch_bits"] == v.info.nof_ul_sch_bits, what

    def check_decoded(self, got):
        """At the good SNR: what was sent is what was found."""
        L = self.layout
        for i, (name, p, s, v) in enumerate(zip(self.names, self.pdus, self.sent, self.sent_as)):
            r = got["result"][i]
            if p.nof_csi_part1:
                at = L.uci[i] + p.nof_harq_ack
                assert r["csi_part1_status"] == abi.UCI_STATUS_VALID, name
                assert got["uci"][at:at + p.nof_csi_part1].tobytes() == s.csi1.tobytes(), name
            if v.size >= 12:  # a CRC stands behind the verdict
                assert got["csi2"][i]["status"] == abi.UCI_STATUS_VALID, name
                assert got["uci"][L.csi2[i]:L.csi2[i] + v.size].tobytes() == s.csi2.tobytes(), name
            if name != "j":  # (j) loses a quarter of its UL-SCH REs to part 1: no verdict is asked for
                assert r["tb_crc_ok"] == p.has_codeword, (name, r)
                assert got["tb"][L.tb[i]:L.tb[i] + p.tb_size_bytes].tobytes() == s.tb.tobytes(), name


COMBINED = dict(g=7, h=36, i=150, j=40)
ALONE = [(n, {n: s}) for n in "ghij" for s in K.SELECTABLE[n]]


@pytest.mark.gpu
@pytest.mark.parametrize("names,sizes", ALONE + [("ghijac", COMBINED)], ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v.values())))
def test_processor_equals_the_hand_driven_chain(gpu_ctx, names, sizes):
    sc = Scenario(gpu_ctx, names, sizes)
    d_grid = dev(as_i32(sc.grids()))
    plan = sc.plan(gpu_ctx)
    got = sc.run_plan(gpu_ctx, plan, d_grid)
    plan.close()
    want_buf, want = sc.run_hand(gpu_ctx, d_grid)
    sc.check(got, want_buf, want)
    sc.check_decoded(got)
    if names != "ghijac":
        return
    # (a) and (c), which have no description: their records and bytes are nrphy_pusch_proc_run's, on a plan of just those two
    L, two = sc.layout, [names.index("a"), names.index("c")]
    pick = lambda xs: [xs[i] for i in two]
    proc = lib.PuschProcPlan(gpu_ctx, pick(sc.plain), OPTIONS, two, len(names), NPORTS, NSUBC, pick(L.soft), pick(L.state), pick(L.tb),
                             pick(L.uci))
    B = Buffers(L, 2)
    proc.run(d_grid, B.harq, B.tb, B.uci, B.result)
    gpu_ctx.synchronize()
    alone = B.read()
    proc.close()
    for k, i in enumerate(two):
        p = sc.pdus[i]
        assert alone["result"][k].tobytes() == got["result"][i].tobytes(), names[i]
        assert alone["tb"][L.tb[i]:L.tb[i] + p.tb_size_bytes].tobytes() == got["tb"][L.tb[i]:L.tb[i] + p.tb_size_bytes].tobytes()
        n_uci = p.nof_harq_ack + p.nof_csi_part1
        assert alone["uci"][L.uci[i]:L.uci[i] + n_uci].tobytes() == got["uci"][L.uci[i]:L.uci[i] + n_uci].tobytes()
        soft, state = L.sizes[i]
        for at, size in ((L.soft[i], soft), (L.state[i], state)):
            assert alone["harq"][at:at + size].tobytes() == got["harq"][at:at + size].tobytes(), names[i]
        assert got["csi2"][i].tobytes() == np.array([(0, 0, 0, 0, sc.sent_as[i].info.nof_ul_sch_bits, 0, 0)], CSI2_DTYPE).tobytes()


@pytest.mark.gpu
def test_part1_not_decodable_is_the_processor_without_part2(gpu_ctx):
    """(h) at -12 dB: CSI part 1 fails its CRC, no feedback happens, and everything is nrphy_pusch_proc_run's on the PDU without
    description -- the part 2 region of d_uci_bits keeps the sentinel."""
    sc = Scenario(gpu_ctx, "h", dict(h=48))
    L = sc.layout
    proc = lib.PuschProcPlan(gpu_ctx, sc.plain, OPTIONS, sc.gidx, 1, NPORTS, NSUBC, L.soft, L.state, L.tb, L.uci)
    # 12 bits behind a 6-bit CRC in 204 soft bits can survive -12 dB: the first noise seed at which the existing processor finds
    # part 1 invalid is the case
    for seed in range(78, 94):
        d_grid = dev(as_i32(sc.grids(seed=seed, snr=T.BAD_SNR)))
        B = Buffers(L, 1)
        proc.run(d_grid, B.harq, B.tb, B.uci, B.result)
        gpu_ctx.synchronize()
        want = B.read()
        if want["result"][0]["csi_part1_status"] == abi.UCI_STATUS_INVALID:
            break
    proc.close()
    print("noise seed", seed)
    assert want["result"][0]["csi_part1_status"] == abi.UCI_STATUS_INVALID, "no noise seed of 78..93 leaves part 1 invalid"
    plan = sc.plan(gpu_ctx)
    got = sc.run_plan(gpu_ctx, plan, d_grid)
    plan.close()
    assert got["result"][0]["csi_part1_status"] == abi.UCI_STATUS_INVALID  # the case is what it claims to be
    for k in ("result", "tb", "uci", "harq"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert (got["uci"][L.csi2[0]:] == T.SENTINEL).all()
    base = sc.without_part2()[0]
    assert got["csi2"][0].tobytes() == np.array([(0, 0, 0, 0, base.info.nof_ul_sch_bits, 0, 0)], CSI2_DTYPE).tobytes()
    # ... and the hand-driven chain without part 2 agrees
    want_buf, hand = sc.run_hand(gpu_ctx, d_grid, received_as=[base])
    sc.check(got, want_buf, hand, received_as=[base])


@pytest.mark.gpu
def test_workspace_reuse(gpu_ctx):
    """One plan, three runs in a row whose grids select a large variant, then a small one, then size 0 (for (h), whose smallest
    size is 12: 60, 12, 36): each equals a run on a fresh plan, and the hand-driven chain."""
    scs = [Scenario(gpu_ctx, "gh", dict(g=g, h=h), seed=40 + k) for k, (g, h) in enumerate(((7, 60), (1, 12), (0, 36)))]
    plan = scs[0].plan(gpu_ctx)
    for sc in scs:
        d_grid = dev(as_i32(sc.grids()))
        got = sc.run_plan(gpu_ctx, plan, d_grid)
        fresh_plan = sc.plan(gpu_ctx)
        fresh = sc.run_plan(gpu_ctx, fresh_plan, d_grid)
        fresh_plan.close()
        for k in got:
            assert got[k].tobytes() == fresh[k].tobytes(), (k, [v.size for v in sc.sent_as])
        want_buf, want = sc.run_hand(gpu_ctx, d_grid)
        sc.check(got, want_buf, want)
        sc.check_decoded(got)
        assert [int(r["variant"]) for r in got["csi2"]] == [v.index for v in sc.sent_as]
    # a fourth run on the same plan: (h) at -12 dB, its part 1 invalid (the first noise seed at which the hand-driven chain without
    # part 2 finds it so), straight after a run that selected a part 2 for it -- no stale part 2 status, stream or select word
    sc = scs[0]
    received_as = [sc.sent_as[0], sc.without_part2()[1]]
    good = sc.grids()
    for seed in range(78, 94):
        grids = np.stack([good[0], sc.grids(seed=seed, snr=T.BAD_SNR)[1]])
        d_grid = dev(as_i32(grids))
        want_buf, want = sc.run_hand(gpu_ctx, d_grid, received_as=received_as)
        if want["status"][want["status_of"][(1, "csi1")]] == abi.UCI_STATUS_INVALID:
            break
    assert want["status"][want["status_of"][(1, "csi1")]] == abi.UCI_STATUS_INVALID, "no noise seed of 78..93 leaves part 1 invalid"
    got = sc.run_plan(gpu_ctx, plan, d_grid)
    sc.check(got, want_buf, want, received_as=received_as)
    assert [int(r["variant"]) for r in got["csi2"]] == [sc.sent_as[0].index, 0] and got["csi2"][1]["status"] == abi.UCI_STATUS_UNKNOWN
    assert (got["uci"][sc.layout.csi2[1]:sc.layout.csi2[1] + 60] == T.SENTINEL).all()
    plan.close()


@pytest.mark.gpu
def test_retransmission_with_the_other_size(gpu_ctx):
    """(i) with rv 0 and new_data 1 and part 2 of 40 bits, then rv 2 and new_data 0 with 150 bits, on the same HARQ blocks: the
    soft buffers see exactly one rate dematching per transmission, the selected variant's."""
    import torch
    first = Scenario(gpu_ctx, "i", dict(i=40), seed=5, rv=0, new_data=1)
    second = Scenario(gpu_ctx, "i", dict(i=150), seed=5, rv=2, new_data=0)
    assert second.sent[0].tb.tobytes() == first.sent[0].tb.tobytes()
    h_proc = fresh_harq(first.layout)
    h_hand = h_proc.clone()
    for k, sc in enumerate((first, second)):
        d_grid = dev(as_i32(sc.grids(seed=90 + k)))
        plan = sc.plan(gpu_ctx)
        got = sc.run_plan(gpu_ctx, plan, d_grid, h_proc)
        plan.close()
        want_buf, want = sc.run_hand(gpu_ctx, d_grid, h_hand)
        sc.check(got, want_buf, want)
        assert torch.equal(h_proc, h_hand)
        assert got["csi2"][0]["variant"] == sc.sent_as[0].index and got["result"][0]["tb_crc_ok"] == 1


@pytest.mark.gpu
def test_nothing_outside_the_sized_regions_is_written(gpu_ctx):
    """Sentinels around and between the output regions: the transport blocks, the UCI bytes with the part 2 payloads of the
    selected size, the HARQ blocks, both result arrays (their guards are checked by Buffers.read)."""
    names = "ghijac"
    sc = Scenario(gpu_ctx, names, COMBINED)
    plan = sc.plan(gpu_ctx)
    got = sc.run_plan(gpu_ctx, plan, dev(as_i32(sc.grids())))
    plan.close()
    L = sc.layout
    tb_written, uci_written, harq_written = (np.zeros(a.size, bool) for a in (got["tb"], got["uci"], got["harq"]))
    for i, (p, v) in enumerate(zip(sc.pdus, sc.sent_as)):
        tb_written[L.tb[i]:L.tb[i] + p.tb_size_bytes] = True
        uci_written[L.uci[i]:L.uci[i] + p.nof_harq_ack + p.nof_csi_part1] = True
        uci_written[L.csi2[i]:L.csi2[i] + v.size] = True
        soft, state = L.sizes[i]
        harq_written[L.soft[i]:L.soft[i] + soft] = True
        harq_written[L.state[i]:L.state[i] + state] = True
    assert (got["tb"][~tb_written] == T.SENTINEL).all()
    assert (got["uci"][~uci_written] == T.SENTINEL).all()
    assert (got["harq"][~harq_written] == HARQ_FILL).all()
    assert [int(r["variant"]) for r in got["csi2"]] == [v.index for v in sc.sent_as]
    assert set(got["uci"][uci_written]) <= {0, 1}


@pytest.mark.gpu
def test_host_form_equals_the_plan_route(gpu_ctx):
    for size in (0, 2, 7):
        sc = Scenario(gpu_ctx, "g", dict(g=size), seed=60 + size)
        grids = sc.grids()
        plan = sc.plan(gpu_ctx)
        got = sc.run_plan(gpu_ctx, plan, dev(as_i32(grids)))
        plan.close()
        p, L = sc.pdus[0], sc.layout
        result, csi2_result, tb, uci, csi2 = gpu_ctx.pusch_csi2_host(p, sc.descs[0], OPTIONS, grids[0], csi2_fill=T.SENTINEL)
        r = got["result"][0]
        for f, _ in abi.PuschResult._fields_:
            if f not in ("harq_ack_offset", "csi_part1_offset"):
                assert np.array(getattr(result, f), T.RESULT_DTYPE[f]).tobytes() == np.array(r[f]).tobytes(), f
        assert (result.harq_ack_offset, result.csi_part1_offset) == (0, p.nof_harq_ack)
        c = got["csi2"][0]
        for f, _ in abi.PuschCsi2Result._fields_:
            if f != "csi_part2_offset":
                assert getattr(csi2_result, f) == c[f], f
        assert csi2_result.csi_part2_offset == 0 and csi2_result.nof_csi_part2 == size
        assert tb.tobytes() == got["tb"][L.tb[0]:L.tb[0] + p.tb_size_bytes].tobytes()
        assert uci.tobytes() == got["uci"][L.uci[0]:L.uci[0] + uci.size].tobytes()
        assert csi2.size == 7 and csi2.tobytes() == got["uci"][L.csi2[0]:L.csi2[0] + 7].tobytes()
        assert (csi2[size:] == T.SENTINEL).all()


# =======================================================================================================================
# Reference pin: tests/golden/record_pusch_csi2_reference.cpp
# =======================================================================================================================
REC_CASES = [(n, s, True) for n in "ghi" for s in K.SELECTABLE[n]] + [("h", 48, False)]
REC_BAD_NOISE_SEED = 79
GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
REC_RES = ("tb_crc_ok", "nof_codeblocks", "harq_ack_status", "csi_part1_status", "csi_part2_status")


def recorded_scenario(ctx, name, size, good):
    """The transmission of one recorded case and its grid [NPORTS][14][NSUBC]: what the tests above send."""
    sc = Scenario(ctx, name, {name: size})
    return sc, (sc.grids() if good else sc.grids(seed=REC_BAD_NOISE_SEED, snr=T.BAD_SNR))[0]


def write_recorder_inputs(ctx, directory):
    """The recorder's inputs: per case the allocated region of the grid (inputs_grids.npy, uint32) and one line of numbers
    (inputs_cases.txt, the order the recorder reads: the PDU, then the description)."""
    words, lines, at = [], [], 0
    for name, size, good in REC_CASES:
        sc, grid = recorded_scenario(ctx, name, size, good)
        p = sc.pdus[0]
        region = T.allocated(p, grid).ravel()
        prbs = [b for b in range(T.NPRB_GRID) if (p.prb_mask[0] >> b) & 1]
        snr = T.GOOD_SNR[(p.modulation, p.nof_tx_layers)] if good else T.BAD_SNR
        desc = []
        for parameters, sizes in K.DESCS[name]:
            desc += [len(parameters)] + [v for pair in parameters for v in pair] + [len(sizes)] + list(sizes)
        lines.append(" ".join(repr(v) for v in [
            "ghij".index(name), size, int(good), snr, p.numerology, p.slot_index, p.rnti, p.n_id, p.scrambling_id, p.n_scid, p.modulation,
            p.target_code_rate, p.has_codeword, p.rv, p.ldpc_base_graph, p.new_data, p.tb_size_bytes, p.tbs_lbrm_bytes, p.nof_harq_ack,
            p.nof_csi_part1, p.alpha_scaling, p.beta_offset_harq_ack, p.beta_offset_csi_part1, p.beta_offset_csi_part2,
            p.start_symbol_index, p.nof_symbols, p.dmrs_symbol_mask, p.nof_tx_layers, p.nof_rx_ports,
            -1 if p.dc_position == abi.PUSCH_CHEST_NO_DC else p.dc_position, prbs[0], len(prbs), at, len(K.DESCS[name])] + desc))
        words.append(region)
        at += region.size
    np.save(os.path.join(directory, "inputs_grids.npy"), np.concatenate(words).astype(np.uint32))
    open(os.path.join(directory, "inputs_cases.txt"), "w").write("\n".join(lines) + "\n")


def recording():
    import json
    cases = json.load(open(os.path.join(GOLDEN, "pusch_csi2_reference_cases.json")))
    load = lambda name: np.load(os.path.join(GOLDEN, "pusch_csi2_reference_%s.npy" % name))
    grids, results, tb, uci = load("grids"), load("results"), load("tb"), load("uci")
    for c, row in zip(cases, results):
        c["name"] = "ghij"[c["pdu"]]
        p = K.make(c["name"])[0][0]
        assert (c["nof_rx_ports"], c["tb_size_bytes"], c["nof_harq_ack"], c["nof_csi_part1"]) == \
            (p.nof_rx_ports, p.tb_size_bytes, p.nof_harq_ack, p.nof_csi_part1), c  # the recording is of today's (g)-(i)
        c["ref"] = dict(zip(REC_RES, (int(v) for v in row)))
        c["tb"] = tb[c["tb_off"]:c["tb_off"] + c["tb_size_bytes"]]
        n1 = c["nof_harq_ack"] + c["nof_csi_part1"]
        c["uci"] = uci[c["uci_off"]:c["uci_off"] + n1]
        c["csi2"] = uci[c["uci_off"] + n1:c["uci_off"] + n1 + c["nof_csi_part2"]]
        n = c["nof_rx_ports"] * 14 * 12 * c["prb_count"]
        grid = np.zeros((NPORTS, 14, NSUBC), np.uint32)
        region = grids[c["grid_off"]:c["grid_off"] + n].reshape(c["nof_rx_ports"], 14, 12 * c["prb_count"])
        grid[[p.rx_ports[i] for i in range(p.nof_rx_ports)], :, 12 * c["prb_start"]:12 * (c["prb_start"] + c["prb_count"])] = region
        c["grid"] = grid
    return cases


def test_recording_is_not_vacuous():
    """Every case the recorder was given is there; each lies where the reference's streaming demultiplexer and the up-front placement
    agree; at the good SNR the reference found CSI part 1 valid, sized part 2 as the transmitter did and decoded the block."""
    cases = recording()
    assert [(c["name"], c["size"], bool(c["good"])) for c in cases] == REC_CASES and len(cases) == 12
    for c in cases:
        pdu, desc = K.make(c["name"])
        base = lib.pusch_proc_derive(plain_of(pdu[0]), OPTIONS, NPORTS, NSUBC)
        sizes, infos = lib.pusch_csi2_variants(pdu[0], desc[0], OPTIONS, NPORTS, NSUBC)
        for s, i in zip(sizes[1:], infos[1:]):  # no part 2 RE in a symbol before the one that holds the last part 1 RE
            assert not K.part2_starts_before_part1_ends(K.demux_with_part2(base.demux, s, i)), (c["name"], s)
        if c["good"]:
            assert c["ref"]["csi_part1_status"] == abi.UCI_STATUS_VALID and c["nof_csi_part2"] == c["size"], c["name"]
            assert c["ref"]["tb_crc_ok"] == 1, (c["name"], c["size"])
            assert c["ref"]["csi_part2_status"] == (abi.UCI_STATUS_VALID if c["size"] else abi.UCI_STATUS_UNKNOWN), (c["name"], c["size"])
    assert {c["nof_csi_part2"] for c in cases} >= {0, 1, 2, 7, 12, 60, 40, 150}


@pytest.mark.gpu
def test_processor_against_the_recording_of_the_reference(gpu_ctx):
    """Every recorded case: the CRC verdict, the transport block where it passed, the three UCI payloads and the three statuses are
    exactly the reference's.  The channel state information is left to the pin of tests/test_pusch_processor.py."""
    cases = recording()
    for c in cases:
        name = c["name"]
        pdus, descs = K.make(name)
        layout = Layout(name, [plain_of(pdus[0])])
        plan = lib.PuschCsi2Plan(gpu_ctx, pdus, descs, OPTIONS, [0], 1, NPORTS, NSUBC, layout.soft, layout.state, layout.tb, layout.uci,
                                 layout.csi2)
        B = Buffers(layout, 1)
        plan.run(dev(as_i32(c["grid"][None])), B.harq, B.tb, B.uci, B.result, B.csi2)
        gpu_ctx.synchronize()
        got = B.read()
        plan.close()
        r, r2, ref, p, what = got["result"][0], got["csi2"][0], c["ref"], pdus[0], (name, c["size"], c["good"])
        assert (r["tb_crc_ok"], r["nof_codeblocks"]) == (ref["tb_crc_ok"], ref["nof_codeblocks"]), what
        if r["tb_crc_ok"]:
            assert got["tb"][layout.tb[0]:layout.tb[0] + p.tb_size_bytes].tobytes() == c["tb"].tobytes(), what
        assert (r["harq_ack_status"], r["csi_part1_status"], r2["status"]) == \
            (ref["harq_ack_status"], ref["csi_part1_status"], ref["csi_part2_status"]), what
        assert got["uci"][layout.uci[0]:layout.uci[0] + c["uci"].size].tobytes() == c["uci"].tobytes(), what
        assert r2["nof_csi_part2"] == c["nof_csi_part2"], what
        assert got["uci"][layout.csi2[0]:layout.csi2[0] + c["csi2"].size].tobytes() == c["csi2"].tobytes(), what


if __name__ == "__main__":  # python tests/test_pusch_csi2.py DIRECTORY (on a GPU): the recorder's inputs
    import sys
    write_recorder_inputs(lib.Context(0), sys.argv[1])
