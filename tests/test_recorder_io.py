"""Host checks of tests/golden/recorder_io.h (no GPU, no reference): what the golden recorders share for .npy files, seeded
inputs, bf16 rounding and the flat JSON of the *_configs.json files, driven through the stand-alone program
tests/recorder_io_check.cpp.  Every test runs against the program built plainly and built with -fsanitize=address,undefined
(skipped only where g++ has no sanitizer runtime).

The JSON readers meet the first object of the committed srs_configs.json and pusch_chest_configs.json.  Neither holds a negative
integer, a null or a boolean, so a third object, EXTRA below, adds those and a list with line breaks.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import backends

SRC = os.path.join(backends.ROOT, "tests", "recorder_io_check.cpp")
GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
FLAVOURS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
DTYPES = ["int8", "uint8", "int32", "int64", "uint32", "float32", "float64"]
EXTRA = '{"dc_position": -17, "second_hop_prb": null, "intra_slot": true, "sr": false, "prbs": [3, 4,\n 5, 60],\n "snr_db": -2.5e+00}'


@pytest.fixture(scope="module", params=list(FLAVOURS))
def check(request, tmp_path_factory):
    """run(*args) -> stdout of the check program of one flavour, which must exit with 0."""
    d = tmp_path_factory.mktemp("recorder_io_" + request.param)
    if request.param == "sanitized":
        probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(d / "probe")],
                               input="int main(){return 0;}", capture_output=True, text=True)
        if probe.returncode != 0:
            pytest.skip("this g++ has no sanitizer runtimes")
    exe = str(d / "recorder_io_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + FLAVOURS[request.param] + [SRC, "-o", exe], check=True, timeout=300)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    return run


def expected(dtype, n):
    """Value i of recorder_io_check.cpp's values<T>()."""
    dt = np.dtype(dtype)
    i = np.arange(n)
    v = (i * 37 % 251 - (0 if dt.kind == "u" else 125)).astype(dt)
    return v + ((i % 4) / 4).astype(dt) if dt.kind == "f" else v


def header_block(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x93NUMPY\x01\x00"
    return 10 + int.from_bytes(raw[8:10], "little")


def test_write_npy_loads_with_dtype_shape_and_values_and_read_npy_u32_reads_it_back(check, tmp_path):
    assert check("npy", tmp_path) == "ok: npy\n"  # the program compared read_npy_u32 with what it wrote
    for dtype in DTYPES:
        for name, shape in ((dtype + "_1d", (37,)), (dtype + "_2d", (5, 7))):
            path = tmp_path / (name + ".npy")
            got = np.load(path)
            assert got.dtype == np.dtype(dtype) and got.shape == shape, name
            assert np.array_equal(got, expected(dtype, got.size).reshape(shape)), name
            assert header_block(path) % 64 == 0, name
    only = np.load(tmp_path / "uint8_only.npy")
    assert only.dtype == np.uint8 and np.array_equal(only, expected("uint8", 37))
    empty = np.load(tmp_path / "empty.npy")
    assert empty.dtype == np.float32 and empty.shape == (0,)
    assert header_block(tmp_path / "uint8_only.npy") % 64 == 0 and header_block(tmp_path / "empty.npy") % 64 == 0


def first_object(name, start):
    """The text of the first object of a fixture that begins with `start`, and what json makes of it."""
    text = open(os.path.join(GOLDEN, name)).read()
    a = text.index(start)
    obj = text[a:text.index("}", a) + 1]
    return obj, json.loads(obj)


@pytest.mark.parametrize("name, start, ints, floats, lists", [
    ("srs_configs.json", '{"numerology"',
     ["numerology", "nof_antenna_ports", "start_symbol", "configuration_index", "sequence_id", "comb_offset", "freq_hopping"],
     ["expected_time_alignment_s"], ["rx_ports"]),
    ("pusch_chest_configs.json", '{"label"',
     ["numerology", "slot_index", "dmrs_type", "scrambling_id", "n_scid", "nof_rb", "first_symbol", "nof_symbols", "nof_tx_layers"],
     ["scaling", "est_noise_var"], ["dmrs_symbols", "rb_mask", "rx_ports", "slot"]),
])
def test_json_readers_agree_with_python_on_the_first_object_of_a_fixture(check, tmp_path, name, start, ints, floats, lists):
    obj, want = first_object(name, start)
    (tmp_path / "object.json").write_text(obj)
    queries = ["int:" + k for k in ints] + ["float:" + k for k in floats] + ["list:" + k for k in lists] + ["lines:" + k for k in lists]
    out = check("json", tmp_path / "object.json", *queries, "opt:no_such_key:-7", "opt:numerology:-7", "list:no_such_key").splitlines()
    assert [int(v) for v in out[:len(ints)]] == [want[k] for k in ints]
    out = out[len(ints):]
    assert [float(v) for v in out[:len(floats)]] == [want[k] for k in floats]
    out = out[len(floats):]
    assert [json.loads(v) for v in out[:2 * len(lists)]] == [want[k] for k in lists] * 2
    assert out[2 * len(lists):] == ["-7", str(want["numerology"]), "[]"]
    if name.startswith("pusch_chest"):
        assert check("json", tmp_path / "object.json", "field:label", "field:cyclic_prefix", "field:nof_rb").split() == \
            [want["label"], want["cyclic_prefix"], str(want["nof_rb"])]


def test_json_readers_on_negative_null_boolean_and_a_list_with_line_breaks(check, tmp_path):
    want = json.loads(EXTRA)
    (tmp_path / "object.json").write_text(EXTRA)
    out = check("json", tmp_path / "object.json", "int:dc_position", "opt:dc_position:0", "opt:second_hop_prb:-1", "opt:intra_slot:5",
                "opt:sr:5", "opt:missing:-1", "float:snr_db", "lines:prbs", "list:prbs", "field:dc_position").splitlines()
    assert out[:6] == ["-17", "-17", "-1", "1", "0", "-1"]
    assert float(out[6]) == want["snr_db"] and json.loads(out[7]) == want["prbs"]
    assert out[8] == "[]"  # the plain character class holds no line break: no match, as for a missing key
    assert out[9] == "-17"
    assert check("text") == "[] [7] [-2, -1, 0, 1, 2]\n"


def test_a_missing_required_key_stops_the_program(check, tmp_path):
    (tmp_path / "object.json").write_text(EXTRA)
    for query in ("int:missing", "float:missing", "field:missing", "int:second_hop_prb"):
        with pytest.raises(AssertionError, match="no "):
            check("json", tmp_path / "object.json", query)


def bf16_nearest_even(x):
    """bf16 bits of float32 x, nearest with ties to even, without the recorder's add-and-shift: the two neighbours and the
    remainder, compared."""
    u = x.view(np.uint32).astype(np.uint64)
    down, rest = u >> 16, u & 0xFFFF
    up = (rest > 0x8000) | ((rest == 0x8000) & (down & 1 == 1))
    return (down + up).astype(np.uint32)


def test_bf16_bits_rounds_to_nearest_even_and_bf16_value_round_trips(check, tmp_path):
    rng = np.random.default_rng(20241021)
    edges = np.array([0x3F808000, 0x3F818000,  # exact ties above an even and above an odd mantissa
                      0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000,
                      0x7F7F0000, 0xFF7F0000,  # the largest finite bf16, both signs
                      0x7F7E8001,              # just above the tie below it: rounds up to it
                      0x00000000, 0x80000000,  # both zeros
                      0x00008000, 0x00018000, 0x00000001], np.uint32)
    seeded = np.concatenate([rng.standard_normal(3000).astype(np.float32) * np.float32(10.0) ** rng.integers(-20, 20, 3000).astype(np.float32),
                             rng.integers(0, 0x7F7F0000, 1000, dtype=np.uint32).view(np.float32)]).view(np.uint32)
    every_bf16 = (np.arange(65536, dtype=np.uint32) << 16)
    words = np.concatenate([edges, seeded, every_bf16])
    np.save(tmp_path / "words.npy", words)
    check("words", tmp_path / "words.npy", tmp_path)
    bits = np.load(tmp_path / "bits.npy")
    assert bits.dtype == np.uint32 and np.array_equal(bits[:edges.size + seeded.size], bf16_nearest_even(words[:edges.size + seeded.size].view(np.float32)))
    assert list(bits[:2]) == [0x3F80, 0x3F82] and list(bits[6:9]) == [0x7F7F, 0xFF7F, 0x7F7F] and list(bits[9:11]) == [0, 0x8000]
    # every bf16 value, NaN patterns included, keeps its bits through bf16_bits and comes back through bf16_value
    assert np.array_equal(bits[-65536:], np.arange(65536, dtype=np.uint32))
    assert np.array_equal(np.load(tmp_path / "values.npy").view(np.uint32)[-65536:], every_bf16)


def test_mix_reproduces_the_first_soft_bits_of_the_ulsch_recording(check, tmp_path):
    """Case 0 of ulsch_reference_*: its input is not stored; record_ulsch_demultiplex_reference.cpp states soft bit k as
    (mix(seed_0 + k) mod 255) - 127 with seed_0 = 0x9E3779B9, rnti = mix(seed_0 ^ 0xAAAA) mod 65535 + 1 and
    n_id = mix(seed_0 ^ 0x5555) mod 1024.  The stored rnti and n_id of case 0 and the finaliser tests/test_ulsch_demultiplex.py
    restates in Python pin the C++ one."""
    from test_ulsch_demultiplex import mix
    seed = 0x9E3779B9
    words = np.concatenate([seed + np.arange(8, dtype=np.uint64), [seed ^ 0xAAAA, seed ^ 0x5555, 0, 0xFFFFFFFF]]).astype(np.uint32)
    np.save(tmp_path / "words.npy", words)
    check("words", tmp_path / "words.npy", tmp_path)
    got = np.load(tmp_path / "mix.npy")
    assert np.array_equal(got, mix(words).astype(np.uint32))
    soft = (got[:8] % 255).astype(np.int64) - 127
    assert np.array_equal(soft, (mix(words[:8]) % 255).astype(np.int64) - 127) and np.all(np.abs(soft) <= 127)
    rnti, n_id = (int(v) for v in np.load(os.path.join(GOLDEN, "ulsch_reference_cases.npy"))[0, :2])
    assert (int(got[8]) % 65535 + 1, int(got[9]) % 1024) == (rnti, n_id)
