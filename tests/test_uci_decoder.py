"""UCI decoder (nrphy_uci_decoder_*): short blocks of 1 to 11 bits and polar messages of 12 to 1706 bits.

The reference's answers were recorded once by tests/golden/record_uci_reference.cpp, which drives srsRAN-5G-ER's own
uci_decoder_impl: tests/golden/uci_reference_{cases,llr,sent,decoded}.npy hold the 160 configurations of the reference's unit test
and the edge sizes, each with a noiseless, two noisy, an all-zero and an extreme-valued input.  Everything is integer arithmetic, so
every comparison here is exact: the NumPy restatement (tests/uci_model.py) against the recording on the CPU, the device against the
recording and against the restatement on the GPU.
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
FILL = 2       # what record_uci_reference.cpp put into the message buffer before decode()
GUARD = 64     # sentinel bytes on either side of every output
SENTINEL = 0xA5
MODULATIONS = {"PI_2_BPSK": 0, "BPSK": 1, "QPSK": 2, "QAM16": 4, "QAM64": 6, "QAM256": 8}
KIND_NOISELESS, KIND_LOW_NOISE, KIND_HIGH_NOISE, KIND_ZERO, KIND_EXTREME = range(5)


def configs():
    return json.load(open(os.path.join(GOLDEN, "uci_decoder_configs.json")))


class Recording:
    def __init__(self):
        self.cases = np.load(os.path.join(GOLDEN, "uci_reference_cases.npy"))
        self.llr = np.load(os.path.join(GOLDEN, "uci_reference_llr.npy"))
        self.sent = np.load(os.path.join(GOLDEN, "uci_reference_sent.npy"))
        self.decoded = np.load(os.path.join(GOLDEN, "uci_reference_decoded.npy"))

    def __len__(self):
        return len(self.cases)

    def case(self, i):
        """(A, E, modulation, kind, llr, sent, decoded, status)"""
        A, E, mod, kind, lo, mo, status, _ = (int(v) for v in self.cases[i])
        return A, E, mod, kind, self.llr[lo:lo + E], self.sent[mo:mo + A], self.decoded[mo:mo + A], status


@pytest.fixture(scope="module")
def recording():
    return Recording()


def size_class(A, E):
    return "1" if A == 1 else "2" if A == 2 else "3-11" if A <= 11 else "two blocks" if model.nof_codeblocks(A, E) == 2 else \
        "12-19" if A <= 19 else "20+"


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_uci_decoder_pods_match_header():
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %u %u %u\n", sizeof(nrphy_uci_decoder_cfg_t), offsetof(nrphy_uci_decoder_cfg_t, message_length),
 offsetof(nrphy_uci_decoder_cfg_t, llr_length), offsetof(nrphy_uci_decoder_cfg_t, modulation), NRPHY_UCI_STATUS_UNKNOWN,
 NRPHY_UCI_STATUS_VALID, NRPHY_UCI_STATUS_INVALID);return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()
    P = abi.UciDecoderCfg
    assert [int(x) for x in out] == [C.sizeof(P), P.message_length.offset, P.llr_length.offset, P.modulation.offset,
                                     abi.UCI_STATUS_UNKNOWN, abi.UCI_STATUS_VALID, abi.UCI_STATUS_INVALID]
    assert (abi.UCI_STATUS_UNKNOWN, abi.UCI_STATUS_VALID, abi.UCI_STATUS_INVALID) == \
        (model.STATUS_UNKNOWN, model.STATUS_VALID, model.STATUS_INVALID) == \
        (abi.PUCCH_STATUS_UNKNOWN, abi.PUCCH_STATUS_VALID, abi.PUCCH_STATUS_INVALID)
    names = [s for s in abi.ABI_SYMBOLS if "_uci_" in s]
    assert len(names) == 5 and not [s for s in names if not hasattr(lib.load(), s)]
    assert not [s for s in names if "pucch" in s]


@pytest.mark.parametrize("name,A,E,mod,want", [
    ("no bit", 0, 10, 2, False), ("1707 bits", 1707, 8192, 2, False), ("1706 bits", 1706, 16384, 2, True),
    ("1 bit, unknown modulation", 1, 10, 3, False), ("1 bit, E below the symbol", 1, 3, 4, False), ("1 bit, one symbol", 1, 4, 4, True),
    ("2 bits, E below the symbol", 2, 7, 8, False), ("2 bits, one symbol", 2, 8, 8, True), ("2 bits, pi/2-BPSK", 2, 1, 0, True),
    ("3 bits, E = A", 3, 3, 2, False), ("3 bits, E = A + 1", 3, 4, 2, True), ("11 bits, E = 11", 11, 11, 2, False),
    ("11 bits, any modulation code", 11, 12, 77, True),
    ("12 bits, E = K + 3", 12, 21, 2, False), ("12 bits, E = K + 4", 12, 22, 2, True),
    ("20 bits, E = K", 20, 31, 2, False), ("20 bits, E = K + 1", 20, 32, 2, True),
    ("one block of more than 8192 soft bits", 300, 8193, 2, False), ("8192 soft bits", 300, 8192, 2, True),
    ("K = 1023, E = K", 1012, 1023, 2, False), ("K = 1023, E = K + 1", 1012, 1024, 2, True), ("the last single block", 1012, 8192, 2, True),
    ("two blocks of more than 8192", 1706, 16386, 2, False), ("two blocks, E odd", 1706, 16385, 2, True),
    ("two blocks, K not below E / 2", 1013, 1036, 2, False),
])
def test_uci_decoder_validator(name, A, E, mod, want):
    assert model.validate(A, E, mod) == want, name
    assert (lib.uci_decoder_validate(abi.make_uci_decoder(A, E, mod)) == abi.OK) == want, name


def test_uci_decoder_validator_over_the_reference_configurations_and_a_sweep():
    for c in configs():
        cfg = abi.make_uci_decoder(c["message_length"], c["llr_length"], MODULATIONS[c["modulation"]])
        assert lib.uci_decoder_validate(cfg) == abi.OK, c
    # The validator and the restatement refuse the same sizes: every A up to 40 with every E up to 600 (all parity-check cases,
    # E - K on both sides of 189, every code length up to 512), and a coarser grid up to the largest sizes.
    sizes = [(A, E) for A in range(1, 41) for E in range(1, 601)]
    sizes += [(A, E) for A in list(range(41, 1720, 37)) + [359, 360, 1012, 1013, 1706] for E in list(range(40, 16500, 211)) + [1087, 1088]]
    for A, E in sizes:
        assert (lib.uci_decoder_validate(abi.make_uci_decoder(A, E, 2)) == abi.OK) == model.validate(A, E, 2), (A, E)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_uci_extractor_reproduces_the_committed_fixtures():
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([sys.executable, os.path.join(GOLDEN, "extract_uci_configs.py"), REFERENCE, d], check=True, timeout=120)
        for name in ("uci_decoder_configs.json", "uci_tables.json"):
            assert open(os.path.join(d, name)).read() == open(os.path.join(GOLDEN, name)).read(), name
    assert len(configs()) == 160


def test_uci_generator_script_reproduces_the_tables():
    committed = open(os.path.join(backends.PKG_DIR, "csrc", "uci_tables.inc")).read()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "uci_tables.inc")
        subprocess.run([sys.executable, os.path.join(backends.ROOT, "profiles", "gen_uci_tables.py"), out], check=True, timeout=120,
                       stdout=subprocess.DEVNULL)
        assert open(out).read() == committed


def test_recording_holds_every_configuration_and_the_edge_sizes(recording):
    sizes = set((int(c[0]), int(c[1]), int(c[2])) for c in recording.cases)
    for c in configs():
        assert (c["message_length"], c["llr_length"], MODULATIONS[c["modulation"]]) in sizes, c
    for A in range(12, 26):
        assert sum(1 for s in sizes if s[0] == A) >= 5, A
    for edge in [(359, 1088), (360, 1087), (360, 1088), (1706, 16384)]:
        assert edge + (2,) in sizes
    assert any(s[0] == 1012 for s in sizes) and any(s[0] == 1013 for s in sizes)
    # Repetition, puncturing and shortening for every code length.
    seen = set()
    for A, E, _ in sizes:
        if A >= 12:
            C_ = model.nof_codeblocks(A, E)
            code = model.PolarCode.get((A + C_ - 1) // C_ + model.crc_size(A), E // C_)
            seen.add((code.N, code.mode))
    # (A block of 32 cannot be punctured: puncturing needs 16 K <= 7 E with E < 32, and K is 18 at least.)
    assert seen >= set((N, mode) for N in (32, 64, 128, 256, 512, 1024) for mode in (0, 1, 2)) - {(32, 1)}
    # Parity-check bits with and without the fixed position (E - K above and below 189).
    pcs = [model.PolarCode.get(A + 6, E) for A, E, _ in sizes if 12 <= A <= 19]
    assert any(252 in c.pc or 248 in c.pc for c in pcs) and any(not (252 in c.pc or 248 in c.pc) for c in pcs)


def test_recording_is_not_vacuous(recording):
    valid, invalid = set(), set()
    for i in range(len(recording)):
        A, E, mod, kind, llr, sent, decoded, status = recording.case(i)
        assert status in (model.STATUS_VALID, model.STATUS_INVALID)
        (valid if status == model.STATUS_VALID else invalid).add(size_class(A, E))
        if kind == KIND_NOISELESS:
            assert status == model.STATUS_VALID and np.array_equal(sent, decoded), (i, A, E)
        if kind == KIND_ZERO:
            assert not llr.any()
    classes = {"1", "2", "3-11", "12-19", "20+", "two blocks"}
    assert valid == classes and invalid == classes
    # A second block that was not decoded keeps the recorder's fill.
    assert any(FILL in recording.case(i)[6] for i in range(len(recording)))


def test_restatement_equals_the_recording(recording):
    saturated_cases = 0
    for i in range(len(recording)):
        A, E, mod, kind, llr, sent, decoded, status = recording.case(i)
        model.STATS["saturated"] = 0
        message, got = model.decode(llr, A, mod, fill=FILL)
        assert got == status and message.tobytes() == decoded.tobytes(), (i, A, E, mod, kind)
        saturated_cases += model.STATS["saturated"] != 0
    assert saturated_cases > 0  # the order of the saturating sums is exercised


def test_restatement_encoder_reproduces_the_recorded_codewords_and_loops_back(recording):
    for i in range(len(recording)):
        A, E, mod, kind, llr, sent, decoded, status = recording.case(i)
        if kind == KIND_NOISELESS:
            assert model.codeword_llr(model.encode(sent, E, mod)).tobytes() == llr.tobytes(), (i, A, E, mod)
    rng = np.random.default_rng(5)
    for c in configs():
        A, E, mod = c["message_length"], c["llr_length"], MODULATIONS[c["modulation"]]
        sent = rng.integers(0, 2, A, dtype=np.uint8)
        message, status = model.decode(model.codeword_llr(model.encode(sent, E, mod)), A, mod)
        assert status == model.STATUS_VALID and np.array_equal(message, sent), c


# =======================================================================================================================
# GPU
# =======================================================================================================================
def guarded(nbytes, fill):
    """A device byte buffer between two guards of sentinel bytes: (whole tensor, the view to hand over)."""
    import torch
    whole = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    whole[GUARD:GUARD + nbytes] = fill
    return whole, whole[GUARD:GUARD + nbytes]


def guards_intact(whole):
    a = whole.cpu().numpy()
    return bool((a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all())


class Batch:
    """Messages (A, E, modulation, llr) laid out back to back, with a plan over them."""

    def __init__(self, ctx, messages):
        import torch
        self.ctx, self.messages = ctx, messages
        self.llr_offsets = np.cumsum([0] + [m[1] for m in messages])
        self.msg_offsets = np.cumsum([0] + [m[0] for m in messages])
        self.plan = lib.UciDecoderPlan(ctx, [abi.make_uci_decoder(A, E, mod) for A, E, mod, _ in messages],
                                       [int(v) for v in self.llr_offsets[:-1]], [int(v) for v in self.msg_offsets[:-1]])
        self.d_llr = torch.from_numpy(np.concatenate([np.asarray(m[3], np.int8) for m in messages])).cuda()

    def outputs(self):
        return guarded(int(self.msg_offsets[-1]), FILL), guarded(4 * len(self.messages), SENTINEL)

    def run(self, outputs=None, stream=None):
        """-> (message bytes of the whole batch, statuses [n]) after checking the guards."""
        (msg_w, msg), (st_w, st) = outputs or self.outputs()
        self.plan.run(self.d_llr, msg, st, stream=stream)
        self.ctx.synchronize()
        assert guards_intact(msg_w) and guards_intact(st_w)
        return msg.cpu().numpy().copy(), st.cpu().numpy().view(np.uint32).copy()

    def split(self, flat):
        return [flat[self.msg_offsets[i]:self.msg_offsets[i + 1]] for i in range(len(self.messages))]

    def close(self):
        self.plan.close()


def recorded_messages(recording):
    return [recording.case(i)[:3] + (recording.case(i)[4],) for i in range(len(recording))]


@pytest.mark.gpu
def test_every_recorded_case_in_one_run(gpu_ctx, recording):
    batch = Batch(gpu_ctx, recorded_messages(recording))
    flat, status = batch.run()
    batch.close()
    for i, message in enumerate(batch.split(flat)):
        A, E, mod, kind, _, _, decoded, want = recording.case(i)
        assert status[i] == want and message.tobytes() == decoded.tobytes(), (i, A, E, mod, kind)


@pytest.mark.gpu
def test_every_recorded_case_through_the_host_call(gpu_ctx, recording):
    for i in range(len(recording)):
        A, E, mod, kind, llr, _, decoded, want = recording.case(i)
        message, status = gpu_ctx.uci_decode_host(abi.make_uci_decoder(A, E, mod), llr, fill=FILL)
        assert status == want and message.tobytes() == decoded.tobytes(), (i, A, E, mod, kind)


def random_size(rng):
    while True:
        kind = rng.integers(0, 6)
        mod = int(rng.choice([0, 1, 2, 4, 6, 8]))
        if kind == 0:
            A, E = int(rng.integers(1, 3)), int(rng.integers(1, 80))
        elif kind == 1:
            A, E = int(rng.integers(3, 12)), int(rng.integers(4, 200))
        elif kind == 2:
            A, E = int(rng.integers(12, 26)), int(rng.integers(20, 700))
        elif kind == 3:
            A = int(rng.integers(26, 400))
            E = int(A * rng.uniform(1.05, 8.0)) + 12
        elif kind == 4:
            A = int(rng.integers(360, 1707))
            E = int(A * rng.uniform(1.05, 4.0)) + 24
        else:
            A, E = int(rng.integers(12, 200)), int(rng.integers(1000, 8193))
        if model.validate(A, E, mod):
            return A, E, mod


def random_input(rng, A, E, mod):
    """-> (sent, llr): a codeword through noise of a random level, or soft bits drawn from the whole domain."""
    sent = rng.integers(0, 2, A, dtype=np.uint8)
    clean = model.codeword_llr(model.encode(sent, E, mod)).astype(np.float64)
    style = rng.integers(0, 4)
    if style == 3:
        llr = rng.choice(np.concatenate([np.arange(-120, 121), [-127, 127] * 20]), E)
    else:
        sigma = [3.0, 15.0, 45.0][style]
        llr = np.clip(np.rint(clean * rng.choice([1.0, 4.0]) + sigma * rng.standard_normal(E)), -120, 120)
    return sent, llr.astype(np.int8)


@pytest.mark.gpu
def test_randomised_sweep_against_the_restatement(gpu_ctx, recording):
    rng = np.random.default_rng(20241017)
    recorded = set((int(c[0]), int(c[1])) for c in recording.cases)
    messages = []
    while len(messages) < 2200:
        A, E, mod = random_size(rng)
        messages.append((A, E, mod, random_input(rng, A, E, mod)[1]))
    assert sum((m[0], m[1]) not in recorded for m in messages) > 1500
    batch = Batch(gpu_ctx, messages)
    flat, status = batch.run()
    batch.close()
    nof_valid = 0
    for i, got in enumerate(batch.split(flat)):
        A, E, mod, llr = messages[i]
        want, want_status = model.decode(llr, A, mod, fill=FILL)
        assert status[i] == want_status and got.tobytes() == want.tobytes(), (i, A, E, mod)
        nof_valid += want_status == model.STATUS_VALID
    assert 400 < nof_valid < 2000


@pytest.mark.gpu
def test_all_zero_input_is_invalid(gpu_ctx):
    sizes = [(1, 8, 8), (2, 12, 4), (5, 40, 2), (11, 32, 2), (14, 60, 2), (40, 200, 2), (400, 2000, 2)]
    batch = Batch(gpu_ctx, [(A, E, mod, np.zeros(E, np.int8)) for A, E, mod in sizes])
    flat, status = batch.run()
    batch.close()
    assert (status == abi.UCI_STATUS_INVALID).all()
    for (A, E, mod), message in zip(sizes, batch.split(flat)):
        if A <= 11:
            assert (message == 1).all()  # the short-block detector's answer to silence
        else:
            # Silence decodes to hard decisions of 1 on every unfrozen position; the CRC refuses it.
            assert message.tobytes() == model.decode(np.zeros(E, np.int8), A, mod, fill=FILL)[0].tobytes()


@pytest.mark.gpu
def test_sign_flipped_codewords_give_another_message(gpu_ctx):
    rng = np.random.default_rng(3)
    sizes = [(1, 8, 2), (2, 24, 4), (3, 32, 2), (7, 64, 2), (11, 32, 2), (16, 80, 2), (30, 128, 2), (200, 700, 2)]
    sent = [rng.integers(0, 2, A, dtype=np.uint8) for A, _, _ in sizes]
    clean = [model.codeword_llr(model.encode(s, E, mod)) for s, (A, E, mod) in zip(sent, sizes)]
    batch = Batch(gpu_ctx, [(A, E, mod, l) for (A, E, mod), l in zip(sizes, clean)] +
                  [(A, E, mod, -l) for (A, E, mod), l in zip(sizes, clean)])
    flat, status = batch.run()
    batch.close()
    messages = batch.split(flat)
    n = len(sizes)
    for i, (A, E, mod) in enumerate(sizes):
        assert status[i] == abi.UCI_STATUS_VALID and np.array_equal(messages[i], sent[i])
        flipped = messages[n + i]
        if A == 1:
            assert flipped[0] == 1 - sent[i][0]
        elif A == 2:
            assert not np.array_equal(flipped, sent[i])
        elif A <= 11:
            # The all-ones codeword is basis sequence 0: flipping every sign flips bit 0 and nothing else.
            assert flipped[0] == 1 - sent[i][0] and np.array_equal(flipped[1:], sent[i][1:])
            assert status[n + i] == abi.UCI_STATUS_VALID
        else:
            # The all-ones codeword is the last row of the polar transform, whose input carries the last CRC bit: the message
            # bits come back and the CRC refuses them.
            assert status[n + i] == abi.UCI_STATUS_INVALID and np.array_equal(flipped, sent[i])


@pytest.mark.gpu
def test_low_noise_returns_the_sent_messages(gpu_ctx, recording):
    """Noise of standard deviation 8 on +-20: the reference decodes every recorded case of this kind (asserted), so must the device."""
    low = [i for i in range(len(recording)) if recording.case(i)[3] == KIND_LOW_NOISE]
    assert len(low) > 300 and all(recording.case(i)[7] == model.STATUS_VALID for i in low)
    batch = Batch(gpu_ctx, [recording.case(i)[:3] + (recording.case(i)[4],) for i in low])
    flat, status = batch.run()
    batch.close()
    assert (status == abi.UCI_STATUS_VALID).all()
    for i, message in zip(low, batch.split(flat)):
        assert np.array_equal(message, recording.case(i)[5]), i


@pytest.mark.gpu
def test_two_runs_and_a_graph_replay_give_identical_bytes(gpu_ctx, recording):
    import torch
    picks = list(range(0, len(recording), 7))
    batch = Batch(gpu_ctx, [recording.case(i)[:3] + (recording.case(i)[4],) for i in picks])
    first = batch.run()
    second = batch.run()
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    (msg_w, msg), (st_w, st) = batch.outputs()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            batch.plan.run(batch.d_llr, msg, st, stream=C.c_void_p(stream.cuda_stream))
    for _ in range(2):
        msg.fill_(FILL)
        st.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert msg.cpu().numpy().tobytes() == first[0].tobytes()
        assert st.cpu().numpy().view(np.uint32).tobytes() == first[1].tobytes()
        assert guards_intact(msg_w) and guards_intact(st_w)
    batch.close()
