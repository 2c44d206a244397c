"""The uplink slot pipeline (nrphy_ul_slots_* / nrphy_ul_slot_*) on the GPU: baseband samples delivered run by run, every receiver
of the slot on the slot's device grid, results from pinned memory -- against the same slot driven by hand with the stand-alone
entry points: nrphy_ofdm_demodulate_slot_host on the same samples (widened in numpy for an int16 pool), then nrphy_pusch_proc_host,
nrphy_pucch_host, nrphy_pf2_host and nrphy_srs_host per PDU on the grid it returns.  Everything is compared byte for byte.

The slot is the small grid of test_pusch_processor.py (25 PRB, 15 kHz) on a 384-point transform with two receive ports: PUSCH
(a) on PRBs 0-5 without UCI and (b) on PRBs 10-17 with one HARQ-ACK bit, transmitted by that test's transmitter; a format 0
PUCCH on symbols 0-1 of PRB 24; a format 1 PUCCH on PRB 23; a format 2 PUCCH on PRBs 20-21 of symbols 12-13; an SRS on PRBs 6-9
of symbol 13.  The transmit grid is modulated by the library's own modulator, noise is added to the samples, and an int16 pool
gets them quantised."""
import ctypes as C
import threading

import numpy as np
import pytest

import backends
import ofh_ul_model
import pucch2_model
import pucch_model
import srs_model
from pusch_chest_model import dev, from_cbf16, to_cbf16
from test_ofh_uplink import cfg_of, section
from test_pusch_processor import NSUBC, OPTIONS, Layout, make_pdus, transmit
from test_srs_estimator import make_cfg as make_srs_cfg
from test_srs_estimator import to_abi as srs_to_abi

abi = backends.abi
lib = backends.pkg.lib

pytestmark = pytest.mark.gpu

NPORTS, NPRB, DFT = 2, NSUBC // 12, 384
OFDM = abi.OfdmConfig(0, NPRB, DFT, 0, 1.0 / np.sqrt(DFT), 2.0e9)
CI16_SCALE = 10000.0   # 1 / scale is not a power of two
RUNS = ((0, 2), (2, 7), (9, 5))
SNR_DB = 20.0
LIMITS = dict(max_pusch=2, max_pucch=2, max_pf2=1, max_srs=1, max_uci_bits=64)


def sym_offsets():
    off = [0]
    for l in range(14):
        off.append(off[-1] + lib.symbol_size(OFDM, l))
    return off


class Slot:
    """The PDUs of the slot, what was sent, the samples (complex64 and int16) and, per sample format, what the hand-driven chain
    gives.  Made once per session."""
    cache = {}

    @classmethod
    def get(cls, ctx):
        if "slot" not in cls.cache:
            cls.cache["slot"] = cls(ctx)
        return cls.cache["slot"]

    def __init__(self, ctx):
        rng = np.random.default_rng(2026)
        self.pdus = [make_pdus("a", rx_ports=(0,))[0], make_pdus("b", rx_ports=(0, 1))[0]]
        derived = [lib.pusch_proc_derive(p, OPTIONS, NPORTS, NSUBC) for p in self.pdus]
        assert None not in derived
        self.sent = [transmit(ctx, p, d, rng) for p, d in zip(self.pdus, derived)]
        self.layout = Layout(self.pdus, OPTIONS)
        self.max_tb_bytes = sum(p.tb_size_bytes for p in self.pdus)
        grid = sum(s.clean[:NPORTS] for s in self.sent)
        gains = [0.9, 0.7j]
        self.f0 = pucch_model.make_cfg(0, 24, 2, 0, bwp_size_rb=NPRB, n_id=40, slot_index=6, initial_cyclic_shift=3, nof_harq_ack=2, ports=(0, 1))
        self.f1 = pucch_model.make_cfg(1, 23, 10, 4, bwp_size_rb=NPRB, n_id=40, slot_index=6, initial_cyclic_shift=2, nof_harq_ack=2, ports=(1, 0))
        self.f2 = pucch2_model.make_cfg(20, 2, 2, 12, bwp_size_rb=NPRB, n_id=40, n_id_0=41, rnti=4097, slot_index=6, nof_harq_ack=4,
                                        nof_csi_part1=8, rx_ports=(0, 1))
        self.f2_message = rng.integers(0, 2, 12).astype(np.uint8)
        pucch_model.add_to_grid(grid, pucch_model.transmit(self.f0, [1, 0]), gains, delay=1.0)
        pucch_model.add_to_grid(grid, pucch_model.transmit(self.f1, [0, 1]), gains, delay=2.0)
        pucch2_model.add_to_grid(grid, pucch2_model.transmit(self.f2, self.f2_message), gains, delay=2.0)
        self.srs = make_srs_cfg(0, 2, freq_shift=6, rx_ports=[0, 1], sequence_id=7)
        grid = grid + from_cbf16(srs_model.transmit(self.srs, NPORTS, NSUBC, [[0.8], [0.6j]], delay_bins=2)).astype(np.complex128)
        self.pucch_cfgs = [pucch_model.to_abi(abi, self.f0), pucch_model.to_abi(abi, self.f1)]
        self.pf2_cfg = pucch2_model.to_abi(abi, self.f2)
        self.srs_cfg = srs_to_abi(self.srs)
        self.plan = lib.OfdmPlan(ctx, OFDM, NPORTS)
        tx = to_cbf16(grid.astype(np.complex64)).view(np.uint16).reshape(NPORTS, 14, NSUBC, 2)
        iq = self.plan.modulate_slot_host(tx, 0)
        sigma = np.sqrt(0.5 * 10 ** (-SNR_DB / 10))
        self.cf32 = (iq + sigma * (rng.standard_normal(iq.shape) + 1j * rng.standard_normal(iq.shape))).astype(np.complex64)
        q = np.rint(self.cf32.view(np.float32).astype(np.float64) * CI16_SCALE)
        self.ci16 = np.clip(q, -32768, 32767).astype(np.int16).reshape(NPORTS, -1, 2)
        self.off = sym_offsets()
        assert self.off[14] == self.cf32.shape[1] == lib.slot_size(OFDM, 0)
        self.want = {}

    def samples(self, fmt):
        return self.ci16 if fmt == abi.IQ_CI16 else self.cf32

    def widened(self, fmt):
        if fmt == abi.IQ_CF32:
            return self.cf32
        conv = self.ci16.astype(np.float32) * (np.float32(1.0) / np.float32(CI16_SCALE))
        return np.ascontiguousarray(conv).view(np.complex64).reshape(NPORTS, -1)

    def by_hand(self, ctx, fmt):
        """grid, then every receiver's host call on it: a dict of byte strings."""
        if fmt not in self.want:
            grid = self.plan.demodulate_slot_host(self.widened(fmt), 0)
            words = grid.view(np.uint32).reshape(NPORTS, 14, NSUBC)
            w = dict(grid=grid.tobytes(), pusch=[], tb=[], uci=[])
            for p in self.pdus:
                r, tb, uci = ctx.pusch_proc_host(p, OPTIONS, words)
                w["pusch"].append(bytes(r))
                w["tb"].append(tb.tobytes())
                w["uci"].append(uci.tobytes())
                w.setdefault("crc", []).append(int(r.tb_crc_ok))
            w["pucch"] = [bytes(ctx.pucch_host(c, words)[0]) for c in self.pucch_cfgs]
            f2 = ctx.pf2_host(self.pf2_cfg, words)
            w["pf2"] = (f2["message"].tobytes(), f2["status"], bytes(f2["csi"]))
            w["srs"] = bytes(ctx.srs_host(self.srs_cfg, words))
            self.want[fmt] = w
        return self.want[fmt]


def make_pool(ctx, slot, fmt, depth=1, d_harq=None, **limits):
    import torch
    kw = dict(LIMITS, max_tb_bytes=slot.max_tb_bytes)
    kw.update(limits)
    if d_harq is None:
        d_harq = torch.zeros(slot.layout.harq_bytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
    return lib.UlSlots(ctx, OFDM, NPORTS, depth, iq_format=fmt, iq_scale=CI16_SCALE, d_harq=d_harq, **kw)


def deliver(pool, slot, sid, first, n, fmt):
    x = slot.samples(fmt)
    lo, hi = slot.off[min(first, 14)], slot.off[min(first + n, 14)]   # (a run the pool must refuse still gets a valid span)
    return pool.samples(sid, first, n, [x[p, lo: max(hi, lo + 1)] for p in range(NPORTS)])


def drive(pool, slot, sid, fmt, on_done=None):
    """The whole slot: the format 0 PUCCH of symbols 0-1 right after the first run, every other receiver after the last."""
    L = slot.layout
    assert deliver(pool, slot, sid, *RUNS[0], fmt) == abi.OK
    assert pool.pucch(sid, slot.pucch_cfgs[:1]) == abi.OK
    assert deliver(pool, slot, sid, *RUNS[1], fmt) == abi.OK
    assert deliver(pool, slot, sid, *RUNS[2], fmt) == abi.OK
    assert pool.pusch(sid, slot.pdus[:1], OPTIONS, L.soft[:1], L.state[:1]) == abi.OK
    assert pool.pucch(sid, slot.pucch_cfgs[1:]) == abi.OK
    assert pool.pf2(sid, [slot.pf2_cfg]) == abi.OK
    assert pool.pusch(sid, slot.pdus[1:], OPTIONS, L.soft[1:], L.state[1:]) == abi.OK
    assert pool.srs(sid, [slot.srs_cfg]) == abi.OK
    assert pool.finish(sid, on_done) == abi.OK
    assert pool.wait(sid) == abi.OK and pool.poll(sid) == abi.OK


def assert_equals_by_hand(pool, sid, want):
    got = pool.pusch_results(sid)
    assert [bytes(r) for r in got] == want["pusch"]
    assert [pool.tb(sid, i).tobytes() for i in range(len(got))] == want["tb"]
    assert [pool.uci_bits(sid, i).tobytes() for i in range(len(got))] == want["uci"]
    assert [bytes(r) for r in pool.pucch_results(sid)] == want["pucch"]
    message, status, csi = pool.pf2_result(sid, 0)
    assert (message.tobytes(), status, bytes(csi)) == want["pf2"]
    assert [bytes(r) for r in pool.srs_results(sid)] == [want["srs"]]
    assert pool.read_grid(sid).tobytes() == want["grid"]


@pytest.mark.parametrize("fmt", [abi.IQ_CF32, abi.IQ_CI16], ids=["cf32", "ci16"])
def test_one_slot_equals_the_hand_driven_chain(gpu_ctx, fmt):
    slot = Slot.get(gpu_ctx)
    want = slot.by_hand(gpu_ctx, fmt)
    # the comparison is about something: both transport blocks decode, the PUCCHs are detected, the format 2 message comes back
    assert want["crc"] == [1, 1] and want["tb"] == [s.tb.tobytes() for s in slot.sent]
    assert want["uci"][1] == slot.sent[1].harq.tobytes() and want["pf2"][:2] == (slot.f2_message.tobytes(), abi.UCI_STATUS_VALID)
    pool = make_pool(gpu_ctx, slot, fmt)
    calls = []
    sid = pool.open(0)
    assert pool.poll(sid) == abi.ERR_NOT_READY
    drive(pool, slot, sid, fmt, on_done=lambda status, slot_id: calls.append((status, slot_id)))
    assert calls == [(abi.OK, sid)]
    assert_equals_by_hand(pool, sid, want)
    results = pool.pucch_results(sid)
    assert [r.status for r in results] == [abi.PUCCH_STATUS_VALID] * 2 and list(results[0].harq_ack) == [1, 0] and list(results[1].harq_ack) == [0, 1]
    pool.close(sid)
    assert pool.poll(sid) == abi.ERR_ARGUMENT
    pool.destroy()


def test_symbols_not_delivered_read_zero(gpu_ctx):
    slot = Slot.get(gpu_ctx)
    want = np.frombuffer(slot.by_hand(gpu_ctx, abi.IQ_CF32)["grid"], np.uint16).reshape(NPORTS, 14, NSUBC, 2)
    pool = make_pool(gpu_ctx, slot, abi.IQ_CF32)
    sid = pool.open(0)
    drive(pool, slot, sid, abi.IQ_CF32)
    pool.close(sid)
    again = pool.open(0)
    assert again == sid
    assert deliver(pool, slot, again, *RUNS[0], abi.IQ_CF32) == abi.OK
    grid = pool.read_grid(again)
    assert np.array_equal(grid[:, :2], want[:, :2]) and not np.any(grid[:, 2:])
    assert pool.pusch_results(again) == [] and pool.pucch_results(again) == []
    pool.close(again)
    pool.destroy()


def test_order_and_capacity(gpu_ctx):
    slot = Slot.get(gpu_ctx)
    want = slot.by_hand(gpu_ctx, abi.IQ_CF32)
    L, fmt = slot.layout, abi.IQ_CF32
    pool = make_pool(gpu_ctx, slot, fmt, depth=2)
    sid = pool.open(0)
    other = pool.open(0)
    assert sid is not None and other is not None and pool.open(0) is None   # beyond depth
    assert gpu_ctx.lib.nrphy_ul_slot_open(pool.handle, 0, C.byref(C.c_uint32())) == abi.ERR_CAPACITY
    assert gpu_ctx.lib.nrphy_ul_slot_open(pool.handle, 1, C.byref(C.c_uint32())) == abi.ERR_ARGUMENT   # 15 kHz: one slot per subframe
    pool.close(other)
    assert pool.finish(other) == abi.ERR_ARGUMENT and pool.pucch(other, slot.pucch_cfgs[:1]) == abi.ERR_ARGUMENT   # not open
    # receivers before their last symbol, sample runs out of order
    assert pool.pucch(sid, slot.pucch_cfgs[:1]) == abi.ERR_ARGUMENT
    assert deliver(pool, slot, sid, 1, 2, fmt) == abi.ERR_ARGUMENT
    assert deliver(pool, slot, sid, 0, 15, fmt) == abi.ERR_ARGUMENT and deliver(pool, slot, sid, 0, 0, fmt) == abi.ERR_ARGUMENT
    assert deliver(pool, slot, sid, *RUNS[0], fmt) == abi.OK
    assert deliver(pool, slot, sid, *RUNS[0], fmt) == abi.ERR_ARGUMENT             # twice
    assert deliver(pool, slot, sid, 3, 2, fmt) == abi.ERR_ARGUMENT                 # skips symbol 2
    assert pool.pucch(sid, slot.pucch_cfgs[1:]) == abi.ERR_ARGUMENT                # format 1 ends on symbol 13
    assert pool.pucch(sid, slot.pucch_cfgs) == abi.ERR_ARGUMENT                    # ... and takes the deliverable one with it
    assert pool.pf2(sid, [slot.pf2_cfg]) == abi.ERR_ARGUMENT and pool.srs(sid, [slot.srs_cfg]) == abi.ERR_ARGUMENT
    assert pool.pusch(sid, slot.pdus[:1], OPTIONS, L.soft[:1], L.state[:1]) == abi.ERR_ARGUMENT
    assert pool.symbols_written(sid, 1) == abi.ERR_ARGUMENT and pool.symbols_written(sid, 15) == abi.ERR_ARGUMENT
    assert pool.pucch(sid, slot.pucch_cfgs[:1]) == abi.OK
    assert deliver(pool, slot, sid, *RUNS[1], fmt) == abi.OK and deliver(pool, slot, sid, *RUNS[2], fmt) == abi.OK
    assert deliver(pool, slot, sid, 14, 1, fmt) == abi.ERR_ARGUMENT
    # invalid PDUs: the status of the stand-alone plan call
    bad = make_pdus("a", rx_ports=(0,), dmrs_type=2)
    assert lib.pusch_proc_validate(bad[0], OPTIONS, NPORTS, NSUBC) == abi.ERR_ARGUMENT
    assert pool.pusch(sid, bad, OPTIONS, L.soft[:1], L.state[:1]) == abi.ERR_ARGUMENT
    assert pool.pusch(sid, [slot.pdus[0], bad[0]], OPTIONS, L.soft, L.state) == abi.ERR_ARGUMENT
    assert pool.pusch(sid, make_pdus("a", rx_ports=(2,)), OPTIONS, L.soft[:1], L.state[:1]) == abi.ERR_ARGUMENT   # a port the grid does not have
    assert pool.pusch(sid, slot.pdus[:1], OPTIONS, None, None) == abi.ERR_ARGUMENT                               # a codeword without HARQ blocks
    f1_bad = pucch_model.to_abi(abi, dict(slot.f1, initial_cyclic_shift=12))
    assert pool.pucch(sid, [f1_bad]) == abi.ERR_ARGUMENT
    # capacity: one PDU beyond max_pusch, one PUCCH beyond max_pucch, and nothing of a refused call stays
    assert pool.pusch(sid, slot.pdus + slot.pdus[:1], OPTIONS, L.soft + L.soft[:1], L.state + L.state[:1]) == abi.ERR_CAPACITY
    assert pool.pucch(sid, slot.pucch_cfgs[1:] * 2) == abi.ERR_CAPACITY
    assert pool.pf2(sid, [slot.pf2_cfg] * 2) == abi.ERR_CAPACITY and pool.srs(sid, [slot.srs_cfg] * 2) == abi.ERR_CAPACITY
    assert pool.pusch(sid, slot.pdus[:1], OPTIONS, L.soft[:1], L.state[:1]) == abi.OK
    assert pool.pucch(sid, slot.pucch_cfgs[1:]) == abi.OK
    assert pool.pucch(sid, slot.pucch_cfgs[1:]) == abi.ERR_CAPACITY
    assert pool.pf2(sid, [slot.pf2_cfg]) == abi.OK
    assert pool.pf2(sid, [slot.pf2_cfg]) == abi.ERR_CAPACITY
    assert pool.pusch(sid, slot.pdus[1:], OPTIONS, L.soft[1:], L.state[1:]) == abi.OK
    assert pool.pusch(sid, slot.pdus[:1], OPTIONS, L.soft[:1], L.state[:1]) == abi.ERR_CAPACITY
    assert pool.srs(sid, [slot.srs_cfg]) == abi.OK
    assert pool.wait(sid) == abi.ERR_ARGUMENT and pool.poll(sid) == abi.ERR_NOT_READY   # nothing to wait for yet
    assert pool.finish(sid) == abi.OK
    assert pool.finish(sid) == abi.ERR_ARGUMENT                                           # twice
    assert pool.pucch(sid, slot.pucch_cfgs[:1]) == abi.ERR_ARGUMENT                       # a receiver after finish
    assert pool.srs(sid, [slot.srs_cfg]) == abi.ERR_ARGUMENT and deliver(pool, slot, sid, 0, 1, fmt) == abi.ERR_ARGUMENT
    assert pool.load_grid(sid, np.zeros((NPORTS, 14, NSUBC, 2), np.uint16)) == abi.ERR_ARGUMENT
    assert pool.wait(sid) == abi.OK
    assert_equals_by_hand(pool, sid, want)
    pool.close(sid)
    pool.destroy()
    # a transport block one byte beyond max_tb_bytes, a UCI bit beyond max_uci_bits; the edge itself is accepted
    for limits, status in ((dict(max_tb_bytes=slot.max_tb_bytes - 1), abi.ERR_CAPACITY), (dict(max_uci_bits=12), abi.ERR_CAPACITY),
                           (dict(max_uci_bits=13), abi.OK)):
        pool = make_pool(gpu_ctx, slot, fmt, **limits)
        sid = pool.open(0)
        for run in RUNS:
            assert deliver(pool, slot, sid, *run, fmt) == abi.OK
        assert pool.pusch(sid, slot.pdus[:1], OPTIONS, L.soft[:1], L.state[:1]) == abi.OK
        assert pool.pf2(sid, [slot.pf2_cfg]) == abi.OK     # 12 bits of the 13 the slot's UCI takes
        assert pool.pusch(sid, slot.pdus[1:], OPTIONS, L.soft[1:], L.state[1:]) == status
        assert pool.finish(sid) == abi.OK and pool.wait(sid) == abi.OK
        got = pool.pusch_results(sid)
        assert [bytes(r) for r in got] == want["pusch"][:len(got)] and len(got) == (2 if status == abi.OK else 1)
        pool.close(sid)
        pool.destroy()


def test_harq_across_slots_with_three_slots_in_flight(gpu_ctx):
    """One UE's (a) with rv 0 at -4 dB, where it cannot decode, and with rv 2 in a later slot on the same HARQ blocks, where the two
    combined do (test_pusch_processor.py's retransmission case); a third slot with another UE runs beside them.  Three threads, one
    slot each, all three open at once; only the retransmission waits, for the first transmission's completion."""
    import torch
    slot = Slot.get(gpu_ctx)
    rng = np.random.default_rng(5)
    first = make_pdus("a", rx_ports=(0,), rv=0, new_data=1)[0]
    second = make_pdus("a", rx_ports=(0,), rv=2, new_data=0)[0]
    other = slot.pdus[1]
    L = Layout([first, other], OPTIONS)
    sigma = np.sqrt(0.5 * 10 ** (4.0 / 10))
    samples, tb = [], None
    for pdu in (first, second):
        sent = transmit(gpu_ctx, pdu, lib.pusch_proc_derive(pdu, OPTIONS, NPORTS, NSUBC), np.random.default_rng(5))
        assert tb is None or tb == sent.tb.tobytes()
        tb = sent.tb.tobytes()
        iq = slot.plan.modulate_slot_host(to_cbf16(sent.clean[:NPORTS].astype(np.complex64)).view(np.uint16).reshape(NPORTS, 14, NSUBC, 2), 0)
        samples.append((iq + sigma * (rng.standard_normal(iq.shape) + 1j * rng.standard_normal(iq.shape))).astype(np.complex64))
    # by hand: the two transmissions one after the other on one pair of HARQ blocks
    soft, state = (np.full(n, 0x11, t) for n, t in zip(L.sizes[0], (np.int8, np.uint8)))
    want = []
    for pdu, iq in zip((first, second), samples):
        words = slot.plan.demodulate_slot_host(iq, 0).view(np.uint32).reshape(NPORTS, 14, NSUBC)
        r, got_tb, _ = gpu_ctx.pusch_proc_host(pdu, OPTIONS, words, soft, state)
        want.append((bytes(r), got_tb.tobytes(), int(r.tb_crc_ok), int(r.ldpc_iterations_sum)))
    assert [w[2] for w in want] == [0, 1] and want[1][1] == tb
    d_harq = torch.full((L.harq_bytes,), 0x11, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pool = make_pool(gpu_ctx, slot, abi.IQ_CF32, depth=3, d_harq=d_harq)
    done, lock, first_done, errors, sids = [], threading.Lock(), threading.Event(), [], {}
    all_open = threading.Barrier(3)

    def on_done(status, slot_id):
        with lock:
            done.append((status, slot_id))
        if slot_id == sids.get("first"):
            first_done.set()

    def ue(name, pdu, iq, k):
        try:
            sid = pool.open(0)
            sids[name] = sid
            all_open.wait(timeout=60)
            for f, n in RUNS:
                assert pool.samples(sid, f, n, [iq[p, slot.off[f]: slot.off[f + n]] for p in range(NPORTS)]) == abi.OK
            if name == "second":
                assert first_done.wait(timeout=60)
            assert pool.pusch(sid, [pdu], OPTIONS, [L.soft[k]], [L.state[k]]) == abi.OK
            assert pool.finish(sid, on_done) == abi.OK
            assert pool.wait(sid) == abi.OK
        except BaseException as e:  # noqa: BLE001 (reported by the main thread)
            errors.append((name, repr(e)))
            first_done.set()

    threads = [threading.Thread(target=ue, args=a) for a in (("first", first, samples[0], 0), ("second", second, samples[1], 0),
                                                             ("other", other, slot.cf32, 1))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert sorted(sids.values()) == [0, 1, 2] and sorted(done) == [(abi.OK, 0), (abi.OK, 1), (abi.OK, 2)]
    for name, w in (("first", want[0]), ("second", want[1])):
        r = pool.pusch_results(sids[name])
        assert len(r) == 1 and (bytes(r[0]), pool.tb(sids[name], 0).tobytes()) == w[:2], name
        assert (int(r[0].tb_crc_ok), int(r[0].ldpc_iterations_sum)) == w[2:], name
    by_hand = slot.by_hand(gpu_ctx, abi.IQ_CF32)
    r = pool.pusch_results(sids["other"])
    assert (bytes(r[0]), pool.tb(sids["other"], 0).tobytes(), pool.uci_bits(sids["other"], 0).tobytes()) == \
        (by_hand["pusch"][1], by_hand["tb"][1], by_hand["uci"][1])
    harq = d_harq.cpu().numpy()
    assert harq[L.soft[0]: L.soft[0] + L.sizes[0][0]].tobytes() == soft.tobytes()
    assert harq[L.state[0]: L.state[0] + L.sizes[0][1]].tobytes() == state.tobytes()
    for sid in sids.values():
        pool.close(sid)
    pool.destroy()


def test_device_grid_path(gpu_ctx):
    """Split 7.2: the slot's grid arrives as BFP-9 records, written by nrphy_ofh_ul_write_grid on the slot's stream into the slot's
    grid; the PUSCH on it gives what nrphy_pusch_proc_host gives on the grid nrphy_ofh_decompress_host makes of the records."""
    import torch
    slot = Slot.get(gpu_ctx)
    rng = np.random.default_rng(12)
    clean = slot.sent[0].clean[:NPORTS]
    rx = 0.2 * (clean + 0.05 * (rng.standard_normal(clean.shape) + 1j * rng.standard_normal(clean.shape)))
    rec = ofh_ul_model.record_bytes(1, 9)
    payload, dicts = np.zeros(1 + NPORTS * 14 * NPRB * rec, np.uint8), []
    want = np.zeros((NPORTS, 14, NSUBC), np.uint32)
    for port in range(NPORTS):
        for l in range(14):
            q = ofh_ul_model.quantise(np.stack([rx[port, l].real, rx[port, l].imag], axis=-1).reshape(NPRB, 24))
            data, _ = ofh_ul_model.bfp_compress(q, 9)
            at = 1 + (port * 14 + l) * NPRB * rec
            payload[at: at + data.size] = data
            dicts.append(dict(payload_offset=at, grid_index=0, port=port, symbol=l, start_prb=0, nof_prbs=NPRB, type=1, data_width=9))
            want[port, l] = gpu_ctx.ofh_decompress_host(cfg_of(1, 9), data).view(np.uint32).reshape(NSUBC)
    pdu = slot.pdus[0]
    r, tb, _ = gpu_ctx.pusch_proc_host(pdu, OPTIONS, want)
    assert r.tb_crc_ok == 1 and tb.tobytes() == slot.sent[0].tb.tobytes()
    pool = make_pool(gpu_ctx, slot, abi.IQ_CF32)
    sid = pool.open(0)
    d_payload = dev(payload)
    torch.cuda.synchronize()
    d_grid = C.c_void_p(pool.device_grid(sid))
    assert d_grid.value and pool.stream(sid)
    arr = (abi.OfhUlSection * len(dicts))(*[section(**d) for d in dicts])
    assert gpu_ctx.lib.nrphy_ofh_ul_write_grid(gpu_ctx.handle, len(dicts), arr, C.c_void_p(d_payload.data_ptr()), payload.size, d_grid, 1,
                                               NPORTS, NSUBC, C.c_void_p(pool.stream(sid))) == abi.OK
    assert pool.pusch(sid, [pdu], OPTIONS, slot.layout.soft[:1], slot.layout.state[:1]) == abi.ERR_ARGUMENT   # not declared yet
    assert pool.symbols_written(sid, 14) == abi.OK
    assert pool.pusch(sid, [pdu], OPTIONS, slot.layout.soft[:1], slot.layout.state[:1]) == abi.OK
    assert pool.finish(sid) == abi.OK and pool.wait(sid) == abi.OK
    got = pool.pusch_results(sid)
    assert [bytes(x) for x in got] == [bytes(r)] and pool.tb(sid, 0).tobytes() == tb.tobytes()
    assert pool.read_grid(sid).tobytes() == want.tobytes()
    pool.close(sid)
    # a host grid in place of the samples: load_grid counts as every symbol delivered
    sid = pool.open(0)
    assert pool.load_grid(sid, want.view(np.uint16).reshape(NPORTS, 14, NSUBC, 2)) == abi.OK
    assert pool.pusch(sid, [pdu], OPTIONS, slot.layout.soft[:1], slot.layout.state[:1]) == abi.OK
    assert pool.finish(sid) == abi.OK and pool.wait(sid) == abi.OK
    assert [bytes(x) for x in pool.pusch_results(sid)] == [bytes(r)] and pool.tb(sid, 0).tobytes() == tb.tobytes()
    pool.close(sid)
    pool.destroy()


@pytest.mark.parametrize("ext,slot_index,fmt", [(0, 1, abi.IQ_CF32), (0, 2, abi.IQ_CI16), (1, 3, abi.IQ_CI16), (1, 1, abi.IQ_CF32)],
                         ids=["normal-slot1-cf32", "normal-slot2-ci16", "extended-slot3-ci16", "extended-slot1-cf32"])
def test_slots_of_the_subframe_and_extended_cyclic_prefix(gpu_ctx, ext, slot_index, fmt):
    """60 kHz: four slots per subframe whose symbols start at different samples (the long cyclic prefix falls into slots 0 and 2),
    12 symbols with extended cyclic prefix.  The grid of a slot delivered in three runs equals nrphy_ofdm_demodulate_slot_host of
    the same samples for that slot index, and the order rules hold at the slot's own number of symbols."""
    cfg = abi.OfdmConfig(2, NPRB, DFT, ext, 1.0 / np.sqrt(DFT), 2.0e9)
    nsymb = 12 if ext else 14
    off = [0]
    for l in range(nsymb):
        off.append(off[-1] + lib.symbol_size(cfg, nsymb * slot_index + l))
    assert off[-1] == lib.slot_size(cfg, slot_index)
    rng = np.random.default_rng(100 * ext + slot_index)
    iq = (rng.standard_normal((NPORTS, off[-1])) + 1j * rng.standard_normal((NPORTS, off[-1]))).astype(np.complex64)
    x = iq
    if fmt == abi.IQ_CI16:
        x = np.clip(np.rint(iq.view(np.float32).astype(np.float64) * 3000.0), -32768, 32767).astype(np.int16).reshape(NPORTS, -1, 2)
        iq = np.ascontiguousarray(x.astype(np.float32) * (np.float32(1.0) / np.float32(CI16_SCALE))).view(np.complex64).reshape(NPORTS, -1)
    plan = lib.OfdmPlan(gpu_ctx, cfg, NPORTS)
    want = plan.demodulate_slot_host(iq, slot_index)
    assert want[:, :nsymb].any() and not want[:, nsymb:].any()
    plan.close()
    pool = lib.UlSlots(gpu_ctx, cfg, NPORTS, 1, iq_format=fmt, iq_scale=CI16_SCALE, max_pucch=1)
    assert gpu_ctx.lib.nrphy_ul_slot_open(pool.handle, 4, C.byref(C.c_uint32())) == abi.ERR_ARGUMENT
    span = lambda f, n: [x[p, off[min(f, nsymb)]: off[min(f + n, nsymb)]] if f < nsymb else x[p, :1] for p in range(NPORTS)]
    sid = pool.open(slot_index)
    for f, n in ((0, 2), (2, 7)):
        assert pool.samples(sid, f, n, span(f, n)) == abi.OK
    assert pool.samples(sid, 9, nsymb - 8, span(9, nsymb - 8)) == abi.ERR_ARGUMENT   # one symbol more than the slot has
    assert pool.symbols_written(sid, nsymb + 1) == abi.ERR_ARGUMENT
    assert pool.samples(sid, 9, nsymb - 9, span(9, nsymb - 9)) == abi.OK
    for f in (nsymb, nsymb + 1, 14):
        assert pool.samples(sid, f, 1, span(f, 1)) == abi.ERR_ARGUMENT
    assert pool.read_grid(sid).tobytes() == want.tobytes()
    pool.close(sid)
    # a grid loaded or declared whole counts as the slot's symbols, not as the 14 rows: no sample run is accepted behind it
    sid = pool.open(slot_index)
    assert pool.load_grid(sid, want) == abi.OK
    for f in (nsymb - 1, nsymb, 13, 14):
        for n in (1, 3):
            assert pool.samples(sid, f, n, span(f, n)) == abi.ERR_ARGUMENT, (f, n)
    assert pool.read_grid(sid).tobytes() == want.tobytes()
    pool.close(sid)
    sid = pool.open(slot_index)
    assert pool.symbols_written(sid, nsymb) == abi.OK
    assert pool.symbols_written(sid, nsymb + 1) == abi.ERR_ARGUMENT
    assert pool.samples(sid, nsymb, 1, span(nsymb, 1)) == abi.ERR_ARGUMENT
    assert not pool.read_grid(sid).any()
    pool.close(sid)
    pool.destroy()
