"""UL-SCH demultiplexer (nrphy_ulsch_demux_*): the descrambled soft bits of a PUSCH codeword with UCI to its UL-SCH, HARQ-ACK, CSI
part 1 and CSI part 2 streams, and the chain demultiplexer -> UCI decoder + PUSCH decoder on one stream.

The reference's answers were recorded once by tests/golden/record_ulsch_demultiplex_reference.cpp, which drives srsRAN-5G-ER's own
ulsch_demultiplex_impl over the 150 configurations of its unit test (tests/golden/ulsch_demultiplex_configs.json) with seeded soft
bits that this file regenerates: tests/golden/ulsch_reference_{cases,uci,sch}.npy hold the three UCI streams of every case, the
UL-SCH stream of the cases of at most 20000 soft bits and a checksum of the UL-SCH stream of every case.  Everything is a copy, a
zero or a sign change, so every comparison is exact: the NumPy restatement (tests/uci_model.py) against the recording on the CPU,
the device against the recording and against the restatement on the GPU.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import backends
import uci_model as model

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
REFERENCE = os.environ.get("SRSRAN_ROOT", "/root/reference/srsRAN-5G-ER")
GUARD = 64
SENTINEL = 0xA5
FIELDS = [f[0] for f in abi.UlschDemuxCfg._fields_]
STORED_LIMIT = 20000  # record_ulsch_demultiplex_reference.cpp stores the UL-SCH stream of codewords up to this size


def mix(h):
    """The recorder's 32-bit finaliser, on uint32 arrays."""
    h = np.asarray(h, np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def checksum(sch):
    w = mix(np.arange(sch.size)) | 1
    return int(((sch.astype(np.int64) + 129).astype(np.uint64) * w).sum(dtype=np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF))


class Recording:
    def __init__(self):
        self.configs = json.load(open(os.path.join(GOLDEN, "ulsch_demultiplex_configs.json")))
        self.cases = np.load(os.path.join(GOLDEN, "ulsch_reference_cases.npy"))
        self.uci = np.load(os.path.join(GOLDEN, "ulsch_reference_uci.npy"))
        self.sch = np.load(os.path.join(GOLDEN, "ulsch_reference_sch.npy"))
        self._cache = {}

    def __len__(self):
        return len(self.cases)

    def case(self, i):
        """(cfg dict with rnti and n_id, llr, (harq, csi1, csi2), sch or None, nof_sch_bits, checksum of sch)"""
        if i not in self._cache:
            rnti, n_id, total, nof_sch, uo, so, sch_sum, _ = (int(v) for v in self.cases[i])
            cfg = dict(self.configs[i], rnti=rnti, n_id=n_id)
            seed = (0x9E3779B9 * (i + 1)) & 0xFFFFFFFF
            assert (rnti, n_id) == (int(mix(seed ^ 0xAAAA)) % 65535 + 1, int(mix(seed ^ 0x5555)) % 1024)
            llr = ((mix(seed + np.arange(total, dtype=np.uint64)) % 255).astype(np.int64) - 127).astype(np.int8)
            parts = []
            for k in ("nof_enc_harq_ack_bits", "nof_enc_csi_part1_bits", "nof_enc_csi_part2_bits"):
                parts.append(self.uci[uo:uo + cfg[k]])
                uo += cfg[k]
            self._cache[i] = (cfg, llr, tuple(parts), self.sch[so:so + nof_sch] if so >= 0 else None, nof_sch, sch_sum)
        return self._cache[i]


@pytest.fixture(scope="module")
def recording():
    return Recording()


def make(cfg):
    return abi.make_ulsch_demux(**cfg)


BASE = dict(modulation=4, nof_layers=2, nof_prb=10, start_symbol_index=0, nof_symbols=14, dmrs_type=0, dmrs_symbol_mask=1 << 2,
            nof_cdm_groups_without_data=2, nof_harq_ack_rvd=64, nof_harq_ack_bits=1, nof_enc_harq_ack_bits=32, nof_csi_part1_bits=40,
            nof_enc_csi_part1_bits=240, nof_csi_part2_bits=2, nof_enc_csi_part2_bits=80, rnti=17, n_id=3)


def random_config(rng, max_prb=10):
    """A configuration drawn without looking at whether it is valid."""
    qm = int(rng.choice([0, 1, 2, 4, 6, 8]))
    layers = int(rng.integers(1, 5))
    nbre = model.bits_per_symbol(qm) * layers
    start = int(rng.integers(0, 4))
    nsym = int(rng.integers(3, 15 - start))
    mask = 0
    for l in rng.choice(np.arange(start, start + nsym), int(rng.integers(1, 4)), replace=False):
        mask |= 1 << int(l)
    if rng.integers(0, 3) == 0:  # consecutive DM-RS symbols
        mask |= (mask << 1) & ((1 << (start + nsym)) - 1)
    dmrs_type = int(rng.integers(0, 2))
    cfg = dict(modulation=qm, nof_layers=layers, nof_prb=int(rng.integers(1, max_prb + 1)), start_symbol_index=start, nof_symbols=nsym,
               dmrs_type=dmrs_type, dmrs_symbol_mask=mask, nof_cdm_groups_without_data=int(rng.integers(1, 3 + dmrs_type)),
               rnti=int(rng.integers(1, 65536)), n_id=int(rng.integers(0, 1024)))
    harq = int(rng.choice([0, 0, 1, 2, 7, 20]))
    exact = rng.integers(0, 10) != 0  # one in ten: soft bits that are no multiple of the RE
    enc = lambda lo, hi: int(rng.integers(lo, hi)) * nbre + (0 if exact else int(rng.integers(1, nbre + 1)) % nbre)
    cfg.update(nof_harq_ack_bits=harq, nof_enc_harq_ack_bits=enc(1, 60) if harq else 0,
               nof_harq_ack_rvd=int(rng.integers(0, 80)) * nbre if harq <= 2 and rng.integers(0, 4) else 0)
    for part in ("csi_part1", "csi_part2"):
        bits = int(rng.choice([0, 0, 1, 2, 5, 30]))
        cfg.update({"nof_%s_bits" % part: bits, "nof_enc_%s_bits" % part: enc(1, 120) if bits else 0})
    return cfg


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_ulsch_demux_pods_match_header():
    names = ", ".join("offsetof(nrphy_ulsch_demux_cfg_t, %s)" % f for f in FIELDS)
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){size_t v[] = {sizeof(nrphy_ulsch_demux_cfg_t), sizeof(nrphy_ulsch_demux_sizes_t), offsetof(nrphy_ulsch_demux_sizes_t, nof_sch_bits),
 offsetof(nrphy_ulsch_demux_sizes_t, nof_codeword_bits), %s}; for (size_t i = 0; i != sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]); return 0;}''' % names
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()]
    P, S = abi.UlschDemuxCfg, abi.UlschDemuxSizes
    assert out == [C.sizeof(P), C.sizeof(S), S.nof_sch_bits.offset, S.nof_codeword_bits.offset] + [getattr(P, f).offset for f in FIELDS]
    names = [s for s in abi.ABI_SYMBOLS if "_ulsch_" in s]
    assert len(names) == 6 and not [s for s in names if not hasattr(lib.load(), s)]
    assert not [s for s in names if "pucch" in s]


@pytest.mark.parametrize("name,change,want", [
    ("the base case", {}, True),
    ("unknown modulation", dict(modulation=3), False), ("no layer", dict(nof_layers=0), False), ("5 layers", dict(nof_layers=5), False),
    ("no PRB", dict(nof_prb=0), False), ("276 PRB", dict(nof_prb=276), False), ("275 PRB", dict(nof_prb=275), True),
    ("symbols beyond the slot", dict(start_symbol_index=2, nof_symbols=13), False), ("no symbol", dict(nof_symbols=0), False),
    ("DM-RS type 3", dict(dmrs_type=2), False), ("no CDM group", dict(nof_cdm_groups_without_data=0), False),
    ("3 CDM groups, type 1", dict(nof_cdm_groups_without_data=3), False),
    ("3 CDM groups, type 2", dict(nof_cdm_groups_without_data=3, dmrs_type=1), True),
    ("no DM-RS symbol", dict(dmrs_symbol_mask=0), False), ("DM-RS up to the last symbol", dict(dmrs_symbol_mask=0x3000), False),
    ("a DM-RS bit above the slot", dict(dmrs_symbol_mask=(1 << 2) | (1 << 14)), False),
    ("HARQ-ACK bits without soft bits", dict(nof_enc_harq_ack_bits=0), False),
    ("HARQ-ACK soft bits without bits", dict(nof_harq_ack_bits=0), False),
    ("CSI part 1 bits without soft bits", dict(nof_enc_csi_part1_bits=0), False),
    ("CSI part 2 soft bits without bits", dict(nof_csi_part2_bits=0), False),
    ("soft bits that are no multiple of the RE", dict(nof_enc_csi_part1_bits=244), False),
    ("more HARQ-ACK than the reserved set holds", dict(nof_enc_harq_ack_bits=72), False),
    ("a reserved set next to 3 HARQ-ACK bits", dict(nof_harq_ack_bits=3), False),
    ("3 HARQ-ACK bits", dict(nof_harq_ack_bits=3, nof_harq_ack_rvd=0), True),
    ("more CSI part 1 than the symbols hold", dict(nof_enc_csi_part1_bits=8 * 120 * 13), False),
    ("no UCI at all", dict(nof_harq_ack_rvd=0, nof_harq_ack_bits=0, nof_enc_harq_ack_bits=0, nof_csi_part1_bits=0,
                           nof_enc_csi_part1_bits=0, nof_csi_part2_bits=0, nof_enc_csi_part2_bits=0), True),
])
def test_ulsch_demux_validator(name, change, want):
    cfg = dict(BASE, **change)
    assert model.ulsch_validate(cfg) == want, name
    assert (lib.ulsch_demux_validate(make(cfg)) == abi.OK) == want, name
    assert (lib.ulsch_demux_sizes(make(cfg)) is not None) == want, name


def test_ulsch_demux_validator_and_sizes_over_the_reference_configurations_and_a_sweep(recording):
    for i, c in enumerate(recording.configs):
        assert lib.ulsch_demux_validate(make(c)) == abi.OK, c
        assert lib.ulsch_demux_sizes(make(c)) == model.ulsch_sizes(c) == (int(recording.cases[i][3]), int(recording.cases[i][2])), c
    rng = np.random.default_rng(7)
    accepted = 0
    for _ in range(1500):
        cfg = random_config(rng)
        want = model.ulsch_validate(cfg)
        assert (lib.ulsch_demux_validate(make(cfg)) == abi.OK) == want, cfg
        if want:
            accepted += 1
            assert lib.ulsch_demux_sizes(make(cfg)) == model.ulsch_sizes(cfg), cfg
    assert 300 < accepted < 1400


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_ulsch_extractor_reproduces_the_committed_fixture():
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([sys.executable, os.path.join(GOLDEN, "extract_ulsch_demultiplex_configs.py"), REFERENCE, d], check=True, timeout=120)
        name = "ulsch_demultiplex_configs.json"
        assert open(os.path.join(d, name)).read() == open(os.path.join(GOLDEN, name)).read()


def test_restatement_gold_bits_equal_the_oracle_generator(oracle):
    ones = np.ones(70000, np.int8)
    for c_init in (0, 1, 0x7FFFFFFF, (0x1234 << 15) + 935, (65535 << 15) + 1023):
        want = (oracle.prg_apply_xor_llr(c_init, 0, ones) < 0).astype(np.uint8)
        assert np.array_equal(model.gold_bits(c_init, ones.size), want), c_init


def test_restatement_equals_the_recording(recording):
    assert len(recording) == len(recording.configs) == 150
    stored = 0
    for i in range(len(recording)):
        cfg, llr, parts, sch, nof_sch, sch_sum = recording.case(i)
        got = model.ulsch_demultiplex(cfg, llr)
        for want, have in zip(parts, got[1:]):
            assert have.tobytes() == want.tobytes(), (i, cfg)
        assert got[0].size == nof_sch and checksum(got[0]) == sch_sum, (i, cfg)
        assert (sch is not None) == (llr.size <= STORED_LIMIT)
        if sch is not None:
            stored += 1
            assert got[0].tobytes() == sch.tobytes(), (i, cfg)
    assert stored > 60


def test_recording_is_not_vacuous(recording):
    """Every kind of part occurs, placeholder corrections change signs, and puncturing leaves zeros."""
    seen = set()
    for i in range(len(recording)):
        cfg, llr, parts, sch, nof_sch, _ = recording.case(i)
        qm = model.bits_per_symbol(cfg["modulation"])
        for name, part in zip(("harq", "csi1", "csi2"), parts):
            bits = cfg["nof_%s_bits" % {"harq": "harq_ack", "csi1": "csi_part1", "csi2": "csi_part2"}[name]]
            if part.size:
                seen.add((name, min(bits, 3), qm > 1))
        if sch is not None and cfg["nof_harq_ack_bits"] in (1, 2) and cfg["nof_enc_harq_ack_bits"]:
            assert (sch == 0).sum() >= cfg["nof_enc_harq_ack_bits"] - (parts[2] == 0).sum()
            seen.add("punctured")
        if cfg["nof_enc_harq_ack_bits"] == cfg["nof_enc_csi_part1_bits"] == cfg["nof_enc_csi_part2_bits"] == 0:
            assert sch is None or sch.tobytes() == llr.tobytes()
            seen.add("no UCI")
    # 1 bit (placeholders) and more than 2 bits (none) on a modulation that has placeholders; the 2-bit correction is the sweep's
    for kind in (("harq", 1, True), ("harq", 3, True), ("csi1", 1, True), ("csi1", 3, True), ("csi2", 1, True)):
        assert kind in seen, (kind, seen)
    assert "punctured" in seen and "no UCI" in seen


def test_multiplexer_and_demultiplexer_loop_back(recording):
    rng = np.random.default_rng(11)
    for i in range(len(recording)):
        cfg = recording.case(i)[0]
        nof_sch, total = model.ulsch_sizes(cfg)
        # Values the placeholder corrections leave alone (soft bits 0 and 1 of every symbol; the rest must survive a sign change:
        # checked on magnitudes), and HARQ-ACK of 1 or 2 bits overwrites: the UL-SCH and CSI part 2 come back with zeros there.
        streams = [rng.integers(1, 128, n).astype(np.int8) for n in (nof_sch, cfg["nof_enc_harq_ack_bits"], cfg["nof_enc_csi_part1_bits"],
                                                                     cfg["nof_enc_csi_part2_bits"])]
        codeword = model.ulsch_multiplex(cfg, *streams)
        assert codeword.size == total
        back = model.ulsch_demultiplex(cfg, codeword)
        assert np.array_equal(np.abs(back[1]), streams[1]) and np.array_equal(np.abs(back[2]), streams[2])
        punctured = cfg["nof_enc_harq_ack_bits"] if cfg["nof_harq_ack_bits"] in (1, 2) else 0
        for k in (0, 3):
            keep = back[k] != 0
            assert np.array_equal(np.abs(back[k][keep]), streams[k][keep])
        assert (back[0] == 0).sum() + (back[3] == 0).sum() == punctured, (i, cfg)


# =======================================================================================================================
# GPU
# =======================================================================================================================
def guarded(nbytes):
    import torch
    whole = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes].view(torch.int8)


def guards_intact(whole):
    a = whole.cpu().numpy()
    return bool((a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all())


class Batch:
    """Codewords (cfg, llr) back to back, every stream's pieces back to back, offsets rounded up to `align` bytes (+ `skew`)."""

    def __init__(self, ctx, codewords, align=16, skew=0):
        import torch
        self.codewords = codewords
        self.sizes = []  # per codeword: (codeword, sch, harq, csi1, csi2) soft bits
        for cfg, llr in codewords:
            nof_sch, total = lib.ulsch_demux_sizes(make(cfg))
            assert total == llr.size
            self.sizes.append((total, nof_sch, cfg.get("nof_enc_harq_ack_bits", 0), cfg.get("nof_enc_csi_part1_bits", 0),
                               cfg.get("nof_enc_csi_part2_bits", 0)))
        self.offsets = np.zeros((len(codewords) + 1, 5), np.int64)
        self.offsets[0] = skew
        for i, s in enumerate(self.sizes):
            self.offsets[i + 1] = (self.offsets[i] + np.array(s) + align - 1) // align * align + skew
        flat = np.zeros(int(self.offsets[-1][0]), np.int8)
        for i, (cfg, llr) in enumerate(codewords):
            flat[self.offsets[i][0]:self.offsets[i][0] + llr.size] = llr
        self.d_in = torch.from_numpy(flat).cuda()
        column = lambda k: [int(v) for v in self.offsets[:-1, k]]
        self.plan = lib.UlschDemuxPlan(ctx, [make(c) for c, _ in codewords], column(0), column(1), column(2), column(3), column(4))
        self.ctx = ctx

    def outputs(self):
        return [guarded(int(self.offsets[-1][k])) for k in range(1, 5)]

    def run(self, outputs=None, stream=None):
        """-> the four streams' buffers as int8 arrays, after checking the guards."""
        outputs = outputs or self.outputs()
        self.plan.run(self.d_in, *[o[1] for o in outputs], stream=stream)
        self.ctx.synchronize()
        assert all(guards_intact(o[0]) for o in outputs)
        return [o[1].cpu().numpy() for o in outputs]

    def split(self, flats, i):
        """The four streams of codeword i."""
        return [flats[k][self.offsets[i][k + 1]:self.offsets[i][k + 1] + self.sizes[i][k + 1]] for k in range(4)]

    def gaps_untouched(self, flats):
        """The bytes between the pieces still hold the sentinel."""
        for k in range(4):
            used = np.zeros(flats[k].size, bool)
            for i in range(len(self.codewords)):
                used[self.offsets[i][k + 1]:self.offsets[i][k + 1] + self.sizes[i][k + 1]] = True
            if not (flats[k].view(np.uint8)[~used] == SENTINEL).all():
                return False
        return True

    def close(self):
        self.plan.close()


def assert_case(recording, i, got):
    cfg, llr, parts, sch, nof_sch, sch_sum = recording.case(i)
    for want, have in zip(parts, got[1:]):
        assert have.tobytes() == want.tobytes(), (i, cfg)
    assert got[0].size == nof_sch and checksum(got[0]) == sch_sum, (i, cfg)
    if sch is not None:
        assert got[0].tobytes() == sch.tobytes(), (i, cfg)


@pytest.mark.gpu
def test_every_recorded_case_in_one_run(gpu_ctx, recording):
    batch = Batch(gpu_ctx, [recording.case(i)[:2] for i in range(len(recording))])
    flats = batch.run()
    batch.close()
    assert batch.gaps_untouched(flats)
    for i in range(len(recording)):
        assert_case(recording, i, batch.split(flats, i))


@pytest.mark.gpu
def test_every_recorded_case_through_the_host_call(gpu_ctx, recording):
    for i in range(len(recording)):
        cfg, llr = recording.case(i)[:2]
        assert_case(recording, i, gpu_ctx.ulsch_demultiplex_host(make(cfg), llr, fill=0x5A))


@pytest.fixture(scope="module")
def sweep():
    """220 random valid codewords of mixed configurations with the restatement's answers, computed once."""
    rng = np.random.default_rng(20241018)
    codewords = []
    while len(codewords) < 220:
        cfg = random_config(rng, max_prb=6)
        if model.ulsch_validate(cfg):
            codewords.append((cfg, rng.integers(-127, 128, model.ulsch_sizes(cfg)[1]).astype(np.int8)))
    assert len(set(c["modulation"] * 10 + c["nof_layers"] for c, _ in codewords)) > 18
    return codewords, [model.ulsch_demultiplex(c, l) for c, l in codewords]


@pytest.mark.gpu
@pytest.mark.parametrize("align,skew", [(16, 0), (4, 0), (1, 0), (16, 3)])
def test_randomised_sweep_against_the_restatement(gpu_ctx, sweep, align, skew):
    """Every copy unit: offsets that allow 16 bytes per thread, 4, 1, and buffers that are themselves unaligned."""
    codewords, want = sweep
    batch = Batch(gpu_ctx, codewords, align=align, skew=skew)
    flats = batch.run()
    batch.close()
    assert batch.gaps_untouched(flats)
    for i in range(len(codewords)):
        got = batch.split(flats, i)
        for k in range(4):
            assert got[k].tobytes() == want[i][k].tobytes(), (i, k, codewords[i][0])


@pytest.mark.gpu
def test_without_uci_the_ulsch_stream_is_the_input(gpu_ctx):
    rng = np.random.default_rng(5)
    codewords = []
    for qm, layers, nprb in ((0, 1, 1), (2, 1, 7), (4, 3, 25), (6, 2, 52), (8, 4, 273)):
        cfg = dict(modulation=qm, nof_layers=layers, nof_prb=nprb, start_symbol_index=0, nof_symbols=14, dmrs_type=0,
                   dmrs_symbol_mask=(1 << 2) | (1 << 11), nof_cdm_groups_without_data=1, rnti=1, n_id=1)
        nof_sch, total = lib.ulsch_demux_sizes(make(cfg))
        assert nof_sch == total == (12 * 12 + 2 * 6) * nprb * layers * model.bits_per_symbol(qm)  # the lengths nrphy_ulsch_demux_sizes gives
        codewords.append((cfg, rng.integers(-127, 128, total).astype(np.int8)))
    batch = Batch(gpu_ctx, codewords)
    import torch
    sch = guarded(int(batch.offsets[-1][1]))
    batch.plan.run(batch.d_in, sch[1])  # no UCI in the plan: the three other streams may be absent
    gpu_ctx.synchronize()
    assert guards_intact(sch[0])
    flat = sch[1].cpu().numpy()
    for i, (cfg, llr) in enumerate(codewords):
        assert flat[batch.offsets[i][1]:batch.offsets[i][1] + llr.size].tobytes() == llr.tobytes(), cfg
    batch.close()


@pytest.mark.gpu
def test_output_lengths_and_punctured_positions(gpu_ctx):
    """HARQ-ACK of 1 or 2 bits: the streams have the lengths nrphy_ulsch_demux_sizes gives, the UL-SCH stream keeps every position
    of the codeword that no CSI took, and exactly the HARQ-ACK REs are zero in it."""
    rng = np.random.default_rng(6)
    for bits, qm, layers in ((1, 2, 1), (2, 4, 2), (1, 8, 4), (2, 1, 1)):
        nbre = model.bits_per_symbol(qm) * layers
        cfg = dict(modulation=qm, nof_layers=layers, nof_prb=9, start_symbol_index=1, nof_symbols=12, dmrs_type=1,
                   dmrs_symbol_mask=1 << 3, nof_cdm_groups_without_data=2, nof_harq_ack_rvd=50 * nbre, nof_harq_ack_bits=bits,
                   nof_enc_harq_ack_bits=23 * nbre, nof_csi_part1_bits=9, nof_enc_csi_part1_bits=31 * nbre, rnti=4660, n_id=99)
        nof_sch, total = lib.ulsch_demux_sizes(make(cfg))
        assert total - nof_sch == cfg["nof_enc_csi_part1_bits"]  # HARQ-ACK took nothing away
        llr = rng.choice(np.concatenate([np.arange(-127, 0), np.arange(1, 128)]), total).astype(np.int8)  # no zero in the input
        batch = Batch(gpu_ctx, [(cfg, llr)])
        flats = batch.run()
        batch.close()
        sch, harq, csi1, csi2 = batch.split(flats, 0)
        assert (sch.size, harq.size, csi1.size, csi2.size) == (nof_sch, 23 * nbre, 31 * nbre, 0)
        zero_re = (sch.reshape(-1, nbre) == 0).all(axis=1)
        assert zero_re.sum() == 23 and (sch == 0).sum() == 23 * nbre
        assert (harq != 0).all() and (csi1 != 0).all()
        want = model.ulsch_demultiplex(cfg, llr)
        assert all(g.tobytes() == w.tobytes() for g, w in zip((sch, harq, csi1, csi2), want))


@pytest.mark.gpu
def test_two_runs_and_a_graph_replay_give_identical_bytes(gpu_ctx, recording):
    import torch
    picks = [i for i in range(0, len(recording), 3) if recording.case(i)[1].size <= 60000]
    batch = Batch(gpu_ctx, [recording.case(i)[:2] for i in picks])
    first = batch.run()
    second = batch.run()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    outputs = batch.outputs()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            batch.plan.run(batch.d_in, *[o[1] for o in outputs], stream=C.c_void_p(stream.cuda_stream))
    for _ in range(2):
        for o in outputs:
            o[1].fill_(0x33)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o[1].cpu().numpy() for o in outputs]
        for i in range(len(picks)):  # (the padding between the pieces holds the fill, not the first run's sentinel)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(batch.split(replayed, i), batch.split(first, i))), picks[i]
        assert all(guards_intact(o[0]) for o in outputs)
    batch.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,harq_bits,csi1_bits,csi2_bits", [("1 HARQ-ACK bit", 1, 0, 0), ("20 + 40 + 13 bits", 20, 40, 13)])
def test_chain_demultiplexer_uci_decoder_and_pusch_decoder_on_one_stream(gpu_ctx, name, harq_bits, csi1_bits, csi2_bits):
    """A codeword built here -- a transport block through nrphy_pdsch_encode_host, UCI through the restatement's encoder,
    multiplexed by the restatement, sent at +-20 with the scrambling placeholders applied -- goes through nrphy_ulsch_demux_run,
    nrphy_uci_decoder_run and nrphy_pusch_decode_batch on one stream with no host step in between."""
    import torch
    rng = np.random.default_rng(100 + harq_bits)
    qm, layers, nprb, bg, tb_size = 4, 1, 20, 2, 300
    enc = {1: (harq_bits, 32 if harq_bits == 1 else 160), 2: (csi1_bits, 240 if csi1_bits else 0), 3: (csi2_bits, 120 if csi2_bits else 0)}
    cfg = dict(modulation=qm, nof_layers=layers, nof_prb=nprb, start_symbol_index=0, nof_symbols=14, dmrs_type=0, dmrs_symbol_mask=1 << 2,
               nof_cdm_groups_without_data=2, nof_harq_ack_rvd=64 if harq_bits <= 2 else 0, nof_harq_ack_bits=harq_bits,
               nof_enc_harq_ack_bits=enc[1][1], nof_csi_part1_bits=csi1_bits, nof_enc_csi_part1_bits=enc[2][1],
               nof_csi_part2_bits=csi2_bits, nof_enc_csi_part2_bits=enc[3][1], rnti=0x4601, n_id=77)
    nof_sch, total = lib.ulsch_demux_sizes(make(cfg))
    tb = rng.integers(0, 256, tb_size, dtype=np.uint8)
    sch_bits, _ = gpu_ctx.pdsch_encode_host(bg, 0, qm, 0, layers, nof_sch // qm, tb)
    messages = {k: rng.integers(0, 2, bits, dtype=np.uint8) for k, (bits, _) in enc.items() if bits}
    coded = {k: model.encode(messages[k], enc[k][1], qm) for k in messages}
    codeword = model.ulsch_multiplex(cfg, sch_bits, *[coded.get(k, np.zeros(0, np.uint8)) for k in (1, 2, 3)])
    assert codeword.size == total
    llr = model.ulsch_received_llr(cfg, codeword)
    if harq_bits == 1:
        assert (codeword == model.PLACEHOLDER_ONE).any() and (codeword == model.PLACEHOLDER_REPEAT).any()

    # device buffers: the codeword, the UL-SCH stream, one buffer for the UCI streams (each at a 256-byte offset), the outputs
    order = sorted(messages)
    uci_offset = {k: 256 * i * 4 for i, k in enumerate(order)}
    msg_offset = {k: 64 * i for i, k in enumerate(order)}
    d_in = torch.from_numpy(llr).cuda()
    d_sch = torch.zeros(nof_sch, dtype=torch.int8, device="cuda")
    d_uci = torch.zeros(256 * 4 * 3, dtype=torch.int8, device="cuda")
    d_msg = torch.full((64 * 3,), 2, dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(3, dtype=torch.int32, device="cuda")
    cfg_dec = abi.PuschDecoderCfg(bg, qm, 0, layers, 0, tb_size, nof_sch // qm, 10, 1, 1)
    soft_bytes, state_bytes, _ = gpu_ctx.pusch_decoder_sizes(cfg_dec, 1)
    d_soft = torch.zeros(soft_bytes, dtype=torch.int8, device="cuda")
    d_state = torch.zeros(state_bytes, dtype=torch.uint8, device="cuda")
    d_tb = torch.zeros(tb_size + 4, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(4, dtype=torch.int32, device="cuda")
    part = lambda k: d_uci[uci_offset[k]:] if k in messages else None
    demux = lib.UlschDemuxPlan(gpu_ctx, [make(cfg)], [0], [0], [0], [0], [0])
    decoder = lib.UciDecoderPlan(gpu_ctx, [abi.make_uci_decoder(enc[k][0], enc[k][1], qm) for k in order], [uci_offset[k] for k in order],
                                 [msg_offset[k] for k in order])
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize()
    demux.run(d_in, d_sch, part(1), part(2), part(3), stream=sp)
    decoder.run(d_uci, d_msg, d_status, stream=sp)
    gpu_ctx.pusch_decode_batch(cfg_dec, 1, d_sch, nof_sch, d_soft, d_state, d_tb, tb_size + 4, d_res, stream=sp)
    stream.synchronize()
    demux.close()
    decoder.close()
    res = d_res.cpu().numpy()
    assert res[0] == 1 and d_tb.cpu().numpy()[:tb_size].tobytes() == tb.tobytes(), (name, res)
    status, msg = d_status.cpu().numpy(), d_msg.cpu().numpy()
    for i, k in enumerate(order):
        assert status[i] == abi.UCI_STATUS_VALID, (name, k, status)
        assert np.array_equal(msg[msg_offset[k]:msg_offset[k] + enc[k][0]], messages[k]), (name, k)
    if harq_bits == 1:  # the punctured positions reach the decoder as zeros
        assert (d_sch.cpu().numpy() == 0).sum() == enc[1][1]
