"""SRS channel estimator (nrphy_srs_*): grid to channel matrix and time alignment.

CPU: the PODs against the header; the seven names; nrphy_srs_info against the restatement's mapping over the whole bandwidth
table; the validator over the reference's 72 configurations (tests/golden/srs_configs.json), over every refusal one by one and
over the cases of the reference's validator test; the extractor and the table generator against what is committed; the restatement
(tests/srs_model.py) against a recording of the reference (tests/golden/record_srs_reference.cpp -> srs_reference_*.npy); no
near-tied path in any grid the GPU parity tests use; the adaptor header against the reference's headers.

GPU: the device generator against the recorded sequences; parity with the restatement on the recorded and on seeded synthetic
grids; physics; batching; repeatability and graph replay; guards; one grid buffer shared with a PUCCH format 2 and a PUSCH
estimator plan.

T_REF: the largest |restatement - reference| / rms|mean LS estimate| over the 85 recorded cases is 9.1e-7 (measured; the
summation orders of the products and of the mean differ, nothing else does).  The tests assert four times that, 3.64e-6, for the
restatement against the recording and for the device against the restatement.  One wrong phase index at M = 12 moves a coefficient
by 2 pi / 1024 / 12 = 5.1e-4, far above it."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import backends
import srs_model as model
from pusch_chest_model import as_i32, dev

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
REFERENCE = "/root/reference/srsRAN-5G-ER"
NAMES = ("nrphy_srs_validate", "nrphy_srs_info", "nrphy_srs_plan_create", "nrphy_srs_plan_destroy", "nrphy_srs_run", "nrphy_srs_host",
         "nrphy_srs_sequence_host")
RESULT_DTYPE = np.dtype([("h_re", "<f4", (4, 4)), ("h_im", "<f4", (4, 4)), ("ta_bins", "<i4", (4, 4)), ("time_alignment_s", "<f8"),
                         ("reserved_", "<u4", (2,))])
T_REF = 9.1e-7
BOUND = 4 * T_REF
assert BOUND <= 2e-4  # one wrong phase index at M = 12 cannot hide
SENTINEL = 0x5A5AA5A5
GUARD = 16  # sentinel words on either side of the results
NOF_PORTS, NOF_SUBC = 4, 12 * 52
FIELDS = ("numerology", "nof_antenna_ports", "nof_symbols", "start_symbol", "configuration_index", "sequence_id", "bandwidth_index",
          "comb_size", "comb_offset", "cyclic_shift", "freq_position", "freq_shift", "freq_hopping")


def to_abi(cfg):
    c = abi.make_srs(**{k: cfg[k] for k in FIELDS}, hopping=cfg.get("hopping", 0), rx_ports=cfg["rx_ports"])
    c.nof_rx_ports = cfg.get("nof_rx_ports", len(cfg["rx_ports"]))
    return c


def make_cfg(c_srs, comb, **kw):
    cfg = dict(numerology=0, nof_antenna_ports=1, nof_symbols=1, start_symbol=13, configuration_index=c_srs, sequence_id=0,
               bandwidth_index=0, comb_size=comb, comb_offset=0, cyclic_shift=0, freq_position=0, freq_shift=0, freq_hopping=3, hopping=0,
               rx_ports=[0])
    cfg.update(kw)
    cfg["rx_ports"] = list(cfg["rx_ports"])
    return cfg


def last_subcarrier(cfg):
    return max(model.info(cfg, p)["initial_subcarrier"] + cfg["comb_size"] * (model.info(cfg, p)["sequence_length"] - 1)
               for p in range(cfg["nof_antenna_ports"]))


@functools.lru_cache(maxsize=None)
def fixtures():
    return json.load(open(os.path.join(GOLDEN, "srs_configs.json")))


@functools.lru_cache(maxsize=None)
def recording():
    """[(cfg, grid [ports][14][subc] words, result row, delay)] of the recorded cases."""
    cases, grids, results = (np.load(os.path.join(GOLDEN, "srs_reference_%s.npy" % k)) for k in ("cases", "grids", "results"))
    out = []
    for r, res in zip(cases, results):
        cfg = dict(zip(FIELDS, (int(v) for v in r[:13])), hopping=0, rx_ports=[int(v) for v in r[14:14 + r[13]]])
        ports, subc, k_lo, stride, count, offset = (int(r[j]) for j in (18, 19, 22, 23, 24, 25))
        ns, l0 = cfg["nof_symbols"], cfg["start_symbol"]
        grid = np.zeros((ports, 14, subc), np.uint32)
        grid[:, l0:l0 + ns, k_lo:k_lo + stride * count:stride] = grids[offset:offset + ports * ns * count].reshape(ports, ns, count)
        out.append((cfg, grid, res, int(r[20])))
    return out


@functools.lru_cache(maxsize=None)
def recorded_sequences():
    flat = np.load(os.path.join(GOLDEN, "srs_reference_sequences.npy"))
    out, i = [], 0
    while i < flat.size:
        u, M, n_cs, n_cs_max = (int(v) for v in flat[i:i + 4])
        out.append(((u, M, n_cs, n_cs_max), flat[i + 4:i + 4 + 2 * M].view(np.complex64)))
        i += 4 + 2 * M
    return out


# Seeded synthetic SRS on two grids of 52 PRB x 4 ports: (grid, configuration, delay in bins).  Each sits on symbols of its own.
SYNTHETIC = [
    (0, make_cfg(0, 4, comb_offset=3, sequence_id=11, rx_ports=[2], start_symbol=0), 0),                                     # M 12
    (0, make_cfg(0, 2, nof_antenna_ports=2, nof_symbols=2, start_symbol=1, numerology=1, cyclic_shift=3, sequence_id=59,
                 freq_shift=2, rx_ports=[1, 0]), 3),                                                                         # M 24
    (0, make_cfg(2, 4, nof_antenna_ports=4, nof_symbols=4, start_symbol=3, cyclic_shift=7, comb_offset=1, sequence_id=700,
                 rx_ports=[0, 1, 2, 3]), -3),                                                                                # M 36, swap
    (0, make_cfg(1, 2, nof_antenna_ports=4, start_symbol=7, cyclic_shift=1, sequence_id=1000, freq_shift=5,
                 rx_ports=[3, 1, 0, 2]), 3),                                                                                 # M 48
    (1, make_cfg(14, 2, nof_antenna_ports=2, nof_symbols=2, start_symbol=0, comb_offset=1, cyclic_shift=6, sequence_id=123,
                 rx_ports=[0, 2, 1]), 255),                                                                                  # M 312, W - 1
    (1, make_cfg(14, 4, start_symbol=2, numerology=1, comb_offset=2, sequence_id=30, rx_ports=[3]), -85),                    # M 156, -W
    (1, make_cfg(14, 2, bandwidth_index=1, freq_position=5, freq_shift=3, start_symbol=3, sequence_id=5, rx_ports=[1, 3]), -3),
    (1, make_cfg(9, 4, bandwidth_index=2, freq_position=3, freq_shift=2, freq_hopping=2, nof_symbols=4, start_symbol=10,
                 nof_antenna_ports=2, cyclic_shift=10, comb_offset=1, sequence_id=444, rx_ports=[0, 1, 2, 3]), 3),
]


@functools.lru_cache(maxsize=None)
def synthetic_grids():
    """The two grids [2][4][14][624]: every SRS of SYNTHETIC sent through seeded gains and its delay, with noise of standard
    deviation 0.05, on its own symbols.  Short sequences have flat peaks, which the other antenna ports tilt, so a channel that
    leaves a path near a tie between two bins is drawn again, as the recorder does;
    test_no_path_of_a_gpu_parity_grid_is_near_a_tie holds the result to that."""
    rng = np.random.default_rng(20241018)
    grids = model.transmit(make_cfg(0, 4), NOF_PORTS, NOF_SUBC, [[0]], noise_std=0.05, rng=rng)[None].repeat(2, axis=0).copy()
    for g, cfg, delay in SYNTHETIC:
        nrx, ntx = len(cfg["rx_ports"]), cfg["nof_antenna_ports"]
        for _ in range(1000):
            gains = (0.5 + rng.random((nrx, ntx))) * np.exp(2j * np.pi * rng.random((nrx, ntx)))
            words = model.transmit(cfg, NOF_PORTS, NOF_SUBC, gains, delay, 0.05, rng)
            if not model.estimate(cfg, words)["ta_near_tie"].any():
                break
        else:
            raise AssertionError("every channel of %r near a tie" % (cfg,))
        rows = slice(cfg["start_symbol"], cfg["start_symbol"] + cfg["nof_symbols"])
        grids[g][:, rows] = words[:, rows]
    return grids


@functools.lru_cache(maxsize=None)
def model_results():
    """The restatement's answers, computed once: (recorded cases, synthetic cases)."""
    grids = synthetic_grids()
    return [model.estimate(cfg, grid) for cfg, grid, _, _ in recording()], [model.estimate(cfg, grids[g]) for g, cfg, _ in SYNTHETIC]


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_srs_pods_match_header():
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(nrphy_srs_cfg_t),
 offsetof(nrphy_srs_cfg_t, nof_symbols), offsetof(nrphy_srs_cfg_t, configuration_index), offsetof(nrphy_srs_cfg_t, comb_size),
 offsetof(nrphy_srs_cfg_t, cyclic_shift), offsetof(nrphy_srs_cfg_t, freq_shift), offsetof(nrphy_srs_cfg_t, hopping),
 offsetof(nrphy_srs_cfg_t, nof_rx_ports), offsetof(nrphy_srs_cfg_t, rx_ports), sizeof(nrphy_srs_result_t),
 offsetof(nrphy_srs_result_t, h_im), offsetof(nrphy_srs_result_t, ta_bins), offsetof(nrphy_srs_result_t, time_alignment_s));return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()
    P, R = abi.SrsCfg, abi.SrsResult
    assert [int(x) for x in out] == [C.sizeof(P), P.nof_symbols.offset, P.configuration_index.offset, P.comb_size.offset,
                                     P.cyclic_shift.offset, P.freq_shift.offset, P.hopping.offset, P.nof_rx_ports.offset, P.rx_ports.offset,
                                     C.sizeof(R), R.h_im.offset, R.ta_bins.offset, R.time_alignment_s.offset]
    assert C.sizeof(R) == RESULT_DTYPE.itemsize == 208 and C.sizeof(R) % 16 == 0
    assert [RESULT_DTYPE.fields[k][1] for k in ("h_im", "ta_bins", "time_alignment_s")] == [R.h_im.offset, R.ta_bins.offset, R.time_alignment_s.offset]


def test_srs_names_are_declared_listed_and_exported():
    header = open(os.path.join(backends.ROOT, "include", "mi355_nrphy.h")).read()
    for name in NAMES:
        assert "int %s(" % name in header, name
        assert name in abi.ABI_SYMBOLS and hasattr(lib.load(), name), name
    assert sorted(s for s in abi.ABI_SYMBOLS if "_srs_" in s) == sorted(NAMES)


def test_info_equals_the_restatement_over_the_bandwidth_table():
    n = 0
    for c_srs in range(64):
        for b_srs in range(4):
            for comb in (2, 4):
                for ntx, port in ((1, 0), (2, 1), (4, 1), (4, 2), (4, 3)):
                    for cs in (1, (12 if comb == 4 else 8) // 2 + 1):  # below and above n_cs_max / 2: the comb-offset swap
                        cfg = make_cfg(c_srs, comb, bandwidth_index=b_srs, nof_antenna_ports=ntx, cyclic_shift=cs, comb_offset=(c_srs + b_srs) % comb,
                                       freq_position=(7 * c_srs + 3 * b_srs) % 68, freq_shift=(5 * c_srs + b_srs) % 269, sequence_id=(37 * c_srs + b_srs) % 1024)
                        assert lib.srs_info(to_abi(cfg), port) == model.info(cfg, port), cfg
                        n += 1
    assert n == 64 * 4 * 2 * 5 * 2
    assert lib.srs_info(to_abi(make_cfg(0, 2)), 1) is None  # a port the SRS does not have
    assert lib.srs_info(to_abi(make_cfg(64, 2)), 0) is None


def test_search_window_is_256_and_85_bins_at_every_numerology():
    for mu in range(5):
        assert model.window(make_cfg(0, 2, numerology=mu)) == 256 and model.window(make_cfg(0, 4, numerology=mu)) == 85


def test_validator_accepts_the_reference_configurations():
    est = fixtures()["estimator"]
    assert len(est) == 72
    for cfg in est:
        subc = 12 * (last_subcarrier(cfg) // 12 + 1)
        assert lib.srs_validate(to_abi(cfg), max(cfg["rx_ports"]) + 1, subc) == abi.OK, cfg
        assert lib.srs_validate(to_abi(cfg), max(cfg["rx_ports"]) + 1, last_subcarrier(cfg)) == abi.ERR_ARGUMENT, cfg
        assert lib.srs_validate(to_abi(cfg), max(cfg["rx_ports"]), subc) == abi.ERR_ARGUMENT, cfg


def test_validator_refuses_the_cases_of_the_reference_validator_test():
    v = fixtures()["validator"]
    assert lib.srs_validate(to_abi(v["base"]), 1, 12 * 275) == abi.OK
    assert [c["message"] for c in v["cases"]] == ["Invalid SRS resource.", "Frequency hopping is not supported.",
                                                  "No sequence nor group hopping supported.", "Receive port list is empty."]
    for case in v["cases"]:
        cfg = dict(v["base"], **case["sets"])
        assert lib.srs_validate(to_abi(cfg), 1, 12 * 275) == abi.ERR_ARGUMENT, case


BASE = dict(nof_antenna_ports=4, cyclic_shift=4, rx_ports=[0, 1])  # C_SRS 14, comb 2: M 312 on 52 PRB; ports 1 and 3 on comb 1


@pytest.mark.parametrize("name,sets,ports,subc", [
    ("comb offset not below the comb size", dict(comb_offset=2), 4, 624),
    ("cyclic shift above 7 with comb 2", dict(cyclic_shift=8), 4, 624),
    ("frequency hopping", dict(bandwidth_index=1, freq_hopping=0), 4, 624),
    ("group hopping", dict(hopping=1), 4, 624),
    ("sequence hopping", dict(hopping=2), 4, 624),
    ("no receive port", dict(rx_ports=[]), 4, 624),
    ("symbols beyond the slot", dict(nof_symbols=2, start_symbol=13), 4, 624),
    ("start symbol 14", dict(start_symbol=14), 4, 624),
    ("numerology 5", dict(numerology=5), 4, 624),
    ("C_SRS 64", dict(configuration_index=64), 4, 624),
    ("sequence id 1024", dict(sequence_id=1024), 4, 624),
    ("B_SRS 4", dict(bandwidth_index=4, freq_hopping=4), 4, 624),
    ("comb 3", dict(comb_size=3), 4, 624),
    ("comb 8", dict(comb_size=8), 4, 624),
    ("cyclic shift 12 with comb 4", dict(comb_size=4, cyclic_shift=12), 4, 624),
    ("n_RRC 68", dict(freq_position=68), 4, 624),
    ("n_shift 269", dict(freq_shift=269), 4, 12 * 275 * 2),
    ("b_hop 4", dict(freq_hopping=4), 4, 624),
    ("three antenna ports", dict(nof_antenna_ports=3), 4, 624),
    ("no antenna port", dict(nof_antenna_ports=0), 4, 624),
    ("three symbols", dict(nof_symbols=3, start_symbol=0), 4, 624),
    ("no symbol", dict(nof_symbols=0), 4, 624),
    ("five receive ports", dict(rx_ports=[0, 1, 2, 3], nof_rx_ports=5), 8, 624),
    ("a repeated receive port", dict(rx_ports=[0, 1, 0]), 4, 624),
    ("a receive port outside the grid", dict(rx_ports=[0, 2]), 2, 624),
    ("last subcarrier of antenna port 0 beyond the grid", dict(comb_offset=1, cyclic_shift=0), 4, 623),
    ("last subcarrier of antenna ports 1 and 3 alone beyond the grid", dict(), 4, 623),
    ("n_shift past the grid", dict(freq_shift=1), 4, 624),
])
def test_validator_refuses(name, sets, ports, subc):
    assert lib.srs_validate(to_abi(make_cfg(14, 2, **BASE)), 4, 624) == abi.OK
    assert lib.srs_validate(to_abi(make_cfg(14, 2, **dict(BASE, **sets))), ports, subc) == abi.ERR_ARGUMENT, name


def test_validator_accepts_the_edges_and_refuses_null():
    assert lib.srs_validate(to_abi(make_cfg(14, 2, **dict(BASE, cyclic_shift=0))), 4, 623) == abi.OK  # every port on comb 0: last is 622
    assert lib.srs_validate(to_abi(make_cfg(63, 2, numerology=4, sequence_id=1023, freq_position=67, cyclic_shift=7, comb_offset=1)), 1, 3264) == abi.OK
    assert lib.srs_validate(to_abi(make_cfg(0, 4, cyclic_shift=11, comb_offset=3, freq_shift=268, nof_symbols=4, start_symbol=10,
                                            rx_ports=[3, 2, 1, 0])), 4, 12 * 272) == abi.OK
    assert int(lib.load().nrphy_srs_validate(None, 4, 624)) == abi.ERR_ARGUMENT


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_extractor_reproduces_the_committed_fixtures():
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([sys.executable, os.path.join(GOLDEN, "extract_srs_configs.py"), REFERENCE, d], check=True, timeout=120, capture_output=True)
        for name in ("srs_configs.json", "srs_tables.json"):
            assert open(os.path.join(d, name)).read() == open(os.path.join(GOLDEN, name)).read(), name


def test_generated_tables_are_current():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "srs_tables.inc")
        subprocess.run([sys.executable, os.path.join(backends.ROOT, "profiles", "gen_srs_tables.py"), out], check=True, timeout=120, capture_output=True)
        assert open(out).read() == open(os.path.join(backends.PKG_DIR, "csrc", "srs_tables.inc")).read()
    assert all(m % 4 == 0 for row in model.BANDWIDTH for m, _ in row)  # lengths 6 and 18 cannot occur


def test_recording_covers_the_reference_configurations_and_the_small_shapes():
    rec = recording()
    est = fixtures()["estimator"]
    assert len(rec) == 85
    for (cfg, grid, _, _), want in zip(rec, est):
        assert all(cfg[k] == want[k] for k in FIELDS) and cfg["rx_ports"] == want["rx_ports"]
    small = rec[len(est):]
    assert {model.info(c, 0)["sequence_length"] for c, _, _, _ in small} >= {12, 24, 36, 48, 312, 1632}
    assert {d for _, _, _, d in small} >= {0, 3, -3, 255, -256, 84, -85}
    assert all(g.shape == (4, 14, 624) for _, g, _, _ in small[:-1]) and small[-1][1].shape == (4, 14, 3264)
    assert all(c["start_symbol"] + c["nof_symbols"] == 14 for c, _, _, _ in small)
    assert {(c["nof_antenna_ports"], c["nof_symbols"], c["numerology"], c["comb_size"]) for c, _, _, _ in small} >= {
        (1, 1, 0, 4), (2, 2, 1, 2), (4, 4, 0, 4), (4, 1, 1, 4), (4, 2, 0, 2)}
    assert any(c["bandwidth_index"] > 0 and c["freq_position"] > 0 and c["freq_shift"] > 0 for c, _, _, _ in small)
    for name in ("cases", "grids", "results", "sequences"):
        assert os.path.getsize(os.path.join(GOLDEN, "srs_reference_%s.npy" % name)) < 1 << 20


def test_restatement_generates_the_recorded_sequences():
    seqs = recorded_sequences()
    assert len(seqs) > 200 and {M for (_, M, _, _), _ in seqs} >= {12, 24, 36, 48, 312, 1632}
    for (u, M, n_cs, n_cs_max), want in seqs:
        assert np.abs(model.sequence(u, M, n_cs, n_cs_max) - want).max() <= 1e-6, (u, M, n_cs, n_cs_max)


def test_restatement_against_the_recording():
    """Per-path bins and the time alignment equal the reference's; the coefficients within 4 T_REF of rms|mean LS estimate| (the
    largest figure over the recording, 9.1e-7, is T_REF: see the module's docstring)."""
    worst = 0.0
    for (cfg, grid, res, delay), got in zip(recording(), model_results()[0]):
        scs = 15000 << cfg["numerology"]
        want_h = (res[:16] + 1j * res[16:32]).reshape(4, 4)
        want_bins = np.rint(res[32:48] * 4096 * scs).astype(np.int64).reshape(4, 4)
        assert np.array_equal(got["ta_bins"], want_bins), cfg
        assert abs(got["time_alignment_s"] - res[48]) <= 1e-12, cfg
        worst = max(worst, float(np.abs(got["h"] - want_h).max()) / got["lse_rms"])
        # What the adaptor computes on the host: the reference's min stays at numeric_limits<double>::min().
        W = model.window(cfg)
        assert res[49] == sys.float_info.min and res[50] == W / (4096.0 * scs) and res[51] == 1 / (4096.0 * scs)
    print("largest |restatement - reference| / rms|LSE| = %.3e" % worst)
    assert worst <= BOUND


def test_no_path_of_a_gpu_parity_grid_is_near_a_tie():
    """Every grid the GPU parity tests use -- all recorded ones, all synthetic ones --, every path, no exclusion.  (The all-zero grid
    of the physics test is all ties by construction; what it must give is fixed by the tie rules, not by a comparison.)"""
    recorded, synthetic = model_results()
    assert len(recorded) == 85 and len(synthetic) == len(SYNTHETIC)
    assert not any(r["ta_near_tie"].any() for r in recorded)
    assert not any(r["ta_near_tie"].any() for r in synthetic)


def test_restatement_recovers_gains_and_delays():
    cfg = make_cfg(14, 2, nof_antenna_ports=2, cyclic_shift=3, rx_ports=[0, 1, 2])
    gains = np.array([[1.0, 0.5j], [-0.8, 0.6 - 0.3j], [0.7j, -1.1]])
    flat = model.estimate(cfg, model.transmit(cfg, NOF_PORTS, NOF_SUBC, gains))
    assert np.abs(flat["h"][:3, :2] - gains).max() <= 0.01 and flat["time_alignment_s"] == 0
    for d in (7, -11):
        got = model.estimate(cfg, model.transmit(cfg, NOF_PORTS, NOF_SUBC, gains, delay_bins=d))
        assert (got["ta_bins"][:3, :2] == d).all() and abs(got["time_alignment_s"] - d / (4096.0 * 15000)) <= 1e-15


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_adaptor_header_compiles_against_the_reference():
    src = r'''#include "mi355_nrphy_srsran.h"
srsran::srs_estimator_result estimate_through_the_adaptor(std::shared_ptr<mi355::context> ctx, const srsran::resource_grid_reader& grid,
                                                          const srsran::srs_estimator_configuration& config)
{
  mi355::srs_estimator_adaptor adaptor(std::move(ctx));
  srsran::srs_estimator&       base = adaptor;
  mi355::srs_estimator_validator_adaptor           validator;
  srsran::srs_estimator_configuration_validator&   vbase = validator;
  return vbase.is_valid(config) ? base.estimate(grid, config) : srsran::srs_estimator_result();
}
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-DNDEBUG", "-w", "-I", os.path.join(REFERENCE, "include"),
                        "-I", os.path.join(REFERENCE, "external", "fmt", "include"), "-I", os.path.join(REFERENCE, "external"), "-I", REFERENCE,
                        "-I", os.path.join(backends.ROOT, "include"), "-I", os.path.join(backends.PKG_DIR, "adaptors"),
                        os.path.join(d, "t.cpp")], check=True, timeout=300)


# =======================================================================================================================
# GPU
# =======================================================================================================================
def guarded(nbytes):
    """A device buffer of `nbytes` (a multiple of 8) between two guards of sentinel words: (whole tensor, the view to hand over)."""
    import torch
    words = nbytes // 4
    whole = torch.full((words + 2 * GUARD,), int(np.uint32(SENTINEL).view(np.int32)), dtype=torch.int32, device="cuda")
    return whole, whole[GUARD:GUARD + words]


def guards_intact(whole):
    a = whole.cpu().numpy().view(np.uint32)
    return bool((a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all())


def run_plan(ctx, cfgs, grid_indices, d_grid, nof_grids, nof_ports, nof_subc, stream=None, plan=None):
    """[n] of RESULT_DTYPE after a run into a guarded buffer of sentinel words (every byte of a result is written)."""
    own = plan is None
    if own:
        plan = lib.SrsPlan(ctx, [to_abi(c) for c in cfgs], grid_indices, nof_grids, nof_ports, nof_subc)
    whole, view = guarded(len(cfgs) * RESULT_DTYPE.itemsize)
    plan.run(d_grid, view, stream=stream)
    ctx.synchronize()
    if own:
        plan.close()
    assert guards_intact(whole), "sentinel words around d_result"
    return view.cpu().numpy().view(RESULT_DTYPE).copy()


def as_record(result):
    """An abi.SrsResult as a RESULT_DTYPE record."""
    return np.frombuffer(bytes(result), RESULT_DTYPE)[0]


def check_against_restatement(cfg, got, want, what):
    nrx, ntx = len(cfg["rx_ports"]), cfg["nof_antenna_ports"]
    assert np.array_equal(got["ta_bins"], want["ta_bins"]), what
    assert abs(float(got["time_alignment_s"]) - want["time_alignment_s"]) <= 1e-12, what
    h = got["h_re"] + 1j * got["h_im"]
    err = float(np.abs(h - want["h"]).max()) / want["lse_rms"]
    outside = np.ones((4, 4), bool)
    outside[:nrx, :ntx] = False
    assert not h[outside].any() and not got["ta_bins"][outside].any() and not got["reserved_"].any(), what
    return err


_SYNTHETIC_RUN = {}


def synthetic_run(ctx):
    """One batch run over SYNTHETIC, shared by the tests that read its results (nothing modifies them)."""
    if "out" not in _SYNTHETIC_RUN:
        _SYNTHETIC_RUN["out"] = run_plan(ctx, [c for _, c, _ in SYNTHETIC], [g for g, _, _ in SYNTHETIC], dev(as_i32(synthetic_grids())), 2,
                                         NOF_PORTS, NOF_SUBC)
    return _SYNTHETIC_RUN["out"]


@pytest.mark.gpu
def test_device_generator_gives_the_recorded_sequences(gpu_ctx):
    wanted = dict(recorded_sequences())
    seen = set()
    for cfg, _, _, _ in recording():
        for port in range(cfg["nof_antenna_ports"]):
            i = model.info(cfg, port)
            key = (i["u"], i["sequence_length"], i["n_cs"], i["n_cs_max"])
            if key in seen:
                continue
            seen.add(key)
            got = gpu_ctx.srs_sequence_host(to_abi(cfg), port)
            assert got.shape == (key[1],) and np.abs(got - wanted[key]).max() <= 1e-6, key
    assert seen == set(wanted)


@pytest.mark.gpu
def test_parity_with_the_restatement_on_the_recorded_grids(gpu_ctx):
    worst = 0.0
    for (cfg, grid, _, _), want in zip(recording(), model_results()[0]):
        got = as_record(gpu_ctx.srs_host(to_abi(cfg), grid))
        worst = max(worst, check_against_restatement(cfg, got, want, cfg))
    print("largest |device - restatement| / rms|LSE| on the recorded grids = %.3e" % worst)
    assert worst <= BOUND


@pytest.mark.gpu
def test_parity_with_the_restatement_on_synthetic_grids(gpu_ctx):
    worst = 0.0
    for (_, cfg, delay), got, want in zip(SYNTHETIC, synthetic_run(gpu_ctx), model_results()[1]):
        worst = max(worst, check_against_restatement(cfg, got, want, cfg))
    print("largest |device - restatement| / rms|LSE| on the synthetic grids = %.3e" % worst)
    assert worst <= BOUND


@pytest.mark.gpu
def test_physics(gpu_ctx):
    """A flat unit channel gives h = g[rx][tx] within 1 %; a delay of d bins gives ta_bins = d on every path; an all-zero grid gives
    ta = 0, h = 0 and no NaN."""
    gains = np.array([[1.0, 0.5j, -0.7, 0.9j], [-0.8, 0.6 - 0.3j, 1.2, 0.4 + 0.4j], [0.7j, -1.1, 0.3 - 0.9j, 1.0]])
    for cfg in (make_cfg(14, 2, nof_antenna_ports=2, cyclic_shift=3, rx_ports=[0, 1, 2]),
                make_cfg(14, 4, nof_antenna_ports=4, cyclic_shift=8, comb_offset=1, nof_symbols=2, start_symbol=12, numerology=1, rx_ports=[2, 0, 3])):
        ntx = cfg["nof_antenna_ports"]
        flat = as_record(gpu_ctx.srs_host(to_abi(cfg), model.transmit(cfg, NOF_PORTS, NOF_SUBC, gains)))
        assert np.abs((flat["h_re"] + 1j * flat["h_im"])[:3, :ntx] - gains[:, :ntx]).max() <= 0.01
        assert flat["time_alignment_s"] == 0 and not flat["ta_bins"].any()
        W = model.window(cfg)
        for d in (7, -11, W - 1, -W):
            got = as_record(gpu_ctx.srs_host(to_abi(cfg), model.transmit(cfg, NOF_PORTS, NOF_SUBC, gains, delay_bins=d)))
            assert (got["ta_bins"][:3, :ntx] == d).all(), (cfg, d)
            assert abs(got["time_alignment_s"] - d / (4096.0 * (15000 << cfg["numerology"]))) <= 1e-15
        zero = as_record(gpu_ctx.srs_host(to_abi(cfg), np.zeros((NOF_PORTS, 14, NOF_SUBC), np.uint32)))
        assert zero.tobytes() == np.zeros(1, RESULT_DTYPE).tobytes()


@pytest.mark.gpu
def test_batch_equals_per_srs_host_calls(gpu_ctx):
    grids = synthetic_grids()
    for (g, cfg, _), got in zip(SYNTHETIC, synthetic_run(gpu_ctx)):
        assert bytes(gpu_ctx.srs_host(to_abi(cfg), grids[g])) == got.tobytes(), cfg


@pytest.mark.gpu
def test_graph_replay_and_two_runs_give_identical_bytes(gpu_ctx):
    import torch
    cfgs, index = [c for _, c, _ in SYNTHETIC], [g for g, _, _ in SYNTHETIC]
    d_grid = dev(as_i32(synthetic_grids()))
    plan = lib.SrsPlan(gpu_ctx, [to_abi(c) for c in cfgs], index, 2, NOF_PORTS, NOF_SUBC)
    runs = [run_plan(gpu_ctx, cfgs, index, d_grid, 2, NOF_PORTS, NOF_SUBC, plan=plan).tobytes() for _ in range(2)]
    assert runs[0] == runs[1] == synthetic_run(gpu_ctx).tobytes()
    whole, view = guarded(len(cfgs) * RESULT_DTYPE.itemsize)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.run(d_grid, view, stream=C.c_void_p(stream.cuda_stream))
    for _ in range(2):
        view.fill_(int(np.uint32(SENTINEL).view(np.int32)))
        graph.replay()
        torch.cuda.synchronize()
        assert view.cpu().numpy().tobytes() == runs[0] and guards_intact(whole)
    plan.close()


@pytest.mark.gpu
def test_run_refuses_null_and_misaligned_pointers(gpu_ctx):
    cfg = SYNTHETIC[0][1]
    plan = lib.SrsPlan(gpu_ctx, [to_abi(cfg)], [0], 2, NOF_PORTS, NOF_SUBC)
    d_grid = dev(as_i32(synthetic_grids()))
    whole, view = guarded(2 * RESULT_DTYPE.itemsize)
    for grid, result in ((None, view), (d_grid, None), (d_grid, whole[GUARD + 1:GUARD + 1 + RESULT_DTYPE.itemsize // 4])):
        with pytest.raises(lib.NrphyError):
            plan.run(grid, result)
    plan.close()
    with pytest.raises(lib.NrphyError):
        lib.SrsPlan(gpu_ctx, [to_abi(cfg)], [2], 2, NOF_PORTS, NOF_SUBC)  # a grid the buffer does not have
    with pytest.raises(lib.NrphyError):
        lib.SrsPlan(gpu_ctx, [to_abi(make_cfg(63, 2))], [0], 2, NOF_PORTS, NOF_SUBC)  # 272 PRB on a 52 PRB grid
    gpu_ctx.synchronize()
    assert (whole.cpu().numpy().view(np.uint32) == SENTINEL).all()


@pytest.mark.gpu
def test_srs_shares_one_grid_buffer_and_stream_with_pucch_format_2_and_pusch(gpu_ctx):
    """A slot whose grid feeds a PUSCH estimator (PRBs 10..29), a PUCCH format 2 receiver (PRBs 40..42 of symbols 12-13) and an SRS on
    symbol 13: three plans read the same device grid on the same stream, and each gives exactly what its host call gives alone."""
    import torch
    g, srs, _ = SYNTHETIC[4]
    srs = dict(srs, start_symbol=12)
    words = synthetic_grids()[g].copy()
    words[:, 12:14] = words[:, 0:2]
    f2 = abi.make_pf2(starting_prb=40, nof_prb=3, nof_symbols=2, start_symbol=12, bwp_size_rb=52, n_id=40, n_id_0=40, rnti=4097, slot_index=6,
                      nof_harq_ack=4, nof_csi_part1=16, rx_ports=(0, 1, 2, 3))
    pusch = abi.make_pusch_chest(prbs=range(10, 30), slot_index=6, scrambling_id=40, dmrs_symbols=(2, 11), rx_ports=(0, 1, 2, 3))
    d_grid = dev(as_i32(words[None]))
    chest = lib.PuschChestPlan(gpu_ctx, [pusch], [0], 1, NOF_PORTS, NOF_SUBC, [0])
    pf2 = lib.Pf2Plan(gpu_ctx, [f2], [0], 1, NOF_PORTS, NOF_SUBC, [0], [0])
    plan = lib.SrsPlan(gpu_ctx, [to_abi(srs)], [0], 1, NOF_PORTS, NOF_SUBC)
    E, A = lib.pf2_sizes(f2)
    buffers = {"ce": guarded(4 * NOF_PORTS * 14 * NOF_SUBC), "nv": guarded(4 * NOF_PORTS), "llr": guarded(E), "message": guarded((A + 7) // 8 * 8),
               "status": guarded(8), "csi": guarded(C.sizeof(abi.Pf2Csi)), "srs": guarded(RESULT_DTYPE.itemsize)}
    o = {k: v for k, (_, v) in buffers.items()}
    o["ce"].zero_()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    handle = C.c_void_p(stream.cuda_stream)
    chest.run(d_grid, o["ce"], o["nv"], stream=handle)
    pf2.run(d_grid, o["llr"], o["message"], o["status"], o["csi"], stream=handle)
    plan.run(d_grid, o["srs"], stream=handle)
    stream.synchronize()
    assert all(guards_intact(w) for w, _ in buffers.values())
    want_ce, want_nv, _ = gpu_ctx.pusch_chest_host(pusch, words)
    assert o["ce"].cpu().numpy().view(np.uint32).tobytes() == want_ce.tobytes()
    assert o["nv"].cpu().numpy().view(np.float32).tobytes() == want_nv.tobytes()
    want = gpu_ctx.pf2_host(f2, words)
    assert o["llr"].cpu().numpy().view(np.int8)[:E].tobytes() == want["llr"].tobytes()
    assert int(o["status"].cpu().numpy().view(np.uint32)[0]) == want["status"] and o["csi"].cpu().numpy().tobytes() == bytes(want["csi"])
    got = o["srs"].cpu().numpy().view(RESULT_DTYPE)[0]
    assert got.tobytes() == bytes(gpu_ctx.srs_host(to_abi(srs), words))
    assert (got["ta_bins"][:3, :2] == 255).all()
    for p in (chest, pf2, plan):
        p.close()
