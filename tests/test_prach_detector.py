"""PRACH generator and detector (nrphy_prach_*).

The reference's own arithmetic is in tests/golden/prach_detector_reference_*.npy: what srsRAN-5G-ER's prach_detector_generic_impl
and prach_generator_impl answered on 74 occasions (tests/golden/record_prach_detector_reference.cpp wrote them and states every
layout).  No recorded decision is fragile, so nothing is set aside when the restatement or the device is compared with it.

CPU: the POD mirrors, nrphy_prach_threshold over the whole cross product against tests/golden/prach_thresholds.json, the validator
over each refused case and over the reference unit test's 60 configurations (tests/golden/prach_detector_configs.json), the
extractor that wrote both fixtures, the recording's own consistency, and the restatement (tests/prach_model.py): its generator
against the definition of the sequence and against the recorded sequences, its detect() in float64 and float32 against the
recording, decision for decision.
GPU: the device's generator against the restatement's and the recorded sequences; every recorded occasion through nrphy_prach_run
and a handful through nrphy_prach_detect_host against the recording; the reference configurations on buffers built here; parity of
every output with the float64 restatement on seeded random occasions; physics (zero buffer, noise only, adjacent shifts,
unmonitored preambles, caller's thresholds); batches against per-occasion host calls, strided input, graph replay, sentinels.
"""
import ctypes as C
import json
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import backends
import prach_model as model
from pusch_chest_model import dev

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
REFERENCE = "/root/reference/srsRAN-5G-ER"
RESULT_DTYPE = np.dtype([("rssi_dB", "<f4"), ("time_resolution_s", "<f4"), ("time_advance_max_s", "<f4"), ("nof_detected", "<u4"),
                         ("detected_mask", "<u8")])
PREAMBLE_DTYPE = np.dtype([("detected", "<u4"), ("delay_samples", "<u4"), ("time_advance_s", "<f4"), ("peak", "<f4"),
                           ("detection_metric", "<f4")])
SENTINEL = 0x5A5AA5A5
GUARD = 16  # sentinel words on either side of every output

# Largest |float32 restatement - float64 restatement| of a metric sample relative to max(|metric|, 1e-3), measured on the
# occasions of test_parity_with_the_restatement (the test prints it again on every run): 3.73e-4.  It is what single precision
# costs the whole metric row of an occasion, the samples far below the peak included, in NumPy's order of operations.  The device
# may differ from the float64 restatement by 8 x that: its radix-16 transform and window sums order their additions differently
# from the restatement's FFT and pairwise sums, and both errors grow with log N.
MODEL_SPREAD = 3.73e-4
METRIC_TOL = 8 * MODEL_SPREAD
# The reference's own error, measured against the recording by test_restatement_equals_the_recording (which prints both again on
# every run): the largest |recorded - float64 restatement| of a detection metric relative to the metric, 2.77e-4, and of rssi_dB,
# 8.79e-6 dB (at -388 dB, where float32 resolves 3.1e-5 dB; where |rssi_dB| < 64 it is 2.4e-6 dB).
REF_SPREAD = 2.8e-4
REF_RSSI_SPREAD_DB = 9e-6
# The same for the generator: the largest |recorded - restatement| of a component relative to sqrt(L), measured by
# test_restatement_generator_equals_the_recording: 8.09e-8 (the two build the same float32 table with two libms).
REF_GENERATOR_SPREAD = 1e-7
# The recording admits no occasion with a monitored peak within this of the threshold, or with the two largest samples of a
# detected window within this of the larger.
RECORDING_MARGIN = 0.02
# rssi_dB = 10 log10f(rssi): two ulp of log10f and the product's rounding, at |dB| < 64 (ulp 3.8e-6), rounded up.
RSSI_TOL_DB = 2e-5


def thresholds_fixture():
    return json.load(open(os.path.join(GOLDEN, "prach_thresholds.json")))


def configs_fixture():
    return json.load(open(os.path.join(GOLDEN, "prach_detector_configs.json")))


def to_abi(cfg):
    return abi.make_prach(format=cfg["format"], ra_scs=cfg["ra_scs"], root_sequence_index=cfg["root_sequence_index"],
                          zero_correlation_zone=cfg["zero_correlation_zone"], start_preamble_index=cfg["start_preamble_index"],
                          nof_preamble_indices=cfg["nof_preamble_indices"], nof_rx_ports=cfg["nof_rx_ports"],
                          threshold=cfg.get("threshold", 0.0), win_margin=cfg.get("win_margin", 0))


def make_cfg(fmt, zcz=0, ports=1, root=0, scs=None, start=0, nof=64, **kw):
    cfg = dict(format=fmt, ra_scs=scs or model.default_scs(fmt), root_sequence_index=root, zero_correlation_zone=zcz,
               start_preamble_index=start, nof_preamble_indices=nof, nof_rx_ports=ports)
    cfg.update(kw)
    return cfg


def reference_cfg(f):
    """A fixture entry as a configuration.  The reference's generator takes the root sequence index modulo the table's length
    (lut[index % size]); the library refuses an index outside the table, so the reduction happens here."""
    return make_cfg(f["format"], f["zero_correlation_zone"], f["nof_rx_ports"],
                    f["root_sequence_index"] % (model.seq_len(f["format"]) - 1), f["ra_scs"], f["start_preamble_index"],
                    f["nof_preamble_indices"])


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_prach_pods_match_header():
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\n", sizeof(nrphy_prach_cfg_t),
 offsetof(nrphy_prach_cfg_t, root_sequence_index), offsetof(nrphy_prach_cfg_t, nof_rx_ports), offsetof(nrphy_prach_cfg_t, threshold),
 offsetof(nrphy_prach_cfg_t, win_margin), sizeof(nrphy_prach_result_t), offsetof(nrphy_prach_result_t, nof_detected),
 offsetof(nrphy_prach_result_t, detected_mask), sizeof(nrphy_prach_preamble_t), offsetof(nrphy_prach_preamble_t, time_advance_s),
 offsetof(nrphy_prach_preamble_t, detection_metric), NRPHY_PRACH_FORMAT_B4, NRPHY_PRACH_FORMAT_A3_B3, NRPHY_PRACH_SCS_1_25,
 NRPHY_PRACH_SCS_5, NRPHY_PRACH_MAX_PREAMBLES);return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()
    P, R, M = abi.PrachCfg, abi.PrachResult, abi.PrachPreamble
    assert [int(x) for x in out] == [C.sizeof(P), P.root_sequence_index.offset, P.nof_rx_ports.offset, P.threshold.offset,
                                     P.win_margin.offset, C.sizeof(R), R.nof_detected.offset, R.detected_mask.offset, C.sizeof(M),
                                     M.time_advance_s.offset, M.detection_metric.offset, abi.PRACH_FORMATS.index("B4"),
                                     abi.PRACH_FORMATS.index("A3/B3"), abi.PRACH_SPACINGS.index("1.25"),
                                     abi.PRACH_SPACINGS.index("5"), abi.PRACH_MAX_PREAMBLES]
    assert C.sizeof(R) == RESULT_DTYPE.itemsize and C.sizeof(M) == PREAMBLE_DTYPE.itemsize
    assert abi.PRACH_FORMATS == model.FORMATS and abi.PRACH_SPACINGS == model.SPACINGS


def test_threshold_table_over_the_whole_cross_product():
    rows = {(r["ports"], r["scs"], r["format"], r["zcz"]): r for r in thresholds_fixture()}
    assert len(rows) == 432
    flags = [r["flag"] for r in rows.values()]
    assert (flags.count("red"), flags.count("orange"), flags.count("green")) == (82, 256, 94)
    found = 0
    for ports in (1, 2, 3, 4):
        for scs in model.SPACINGS:
            for fmt in model.FORMATS:
                for zcz in range(16):
                    c = abi.make_prach(format=fmt, ra_scs=scs, zero_correlation_zone=zcz, nof_rx_ports=ports)
                    got, want = lib.prach_threshold(c), rows.get((ports, scs, fmt, zcz))
                    if want is None:
                        assert got is None, (ports, scs, fmt, zcz)
                    else:
                        found += 1
                        assert got is not None, (ports, scs, fmt, zcz)
                        assert np.float32(got[0]) == np.float32(float(want["threshold"])), (ports, scs, fmt, zcz)
                        assert got[1:] == (want["margin"], model.FLAGS.index(want["flag"])), (ports, scs, fmt, zcz)
    assert found == 432


def _base(**kw):
    args = dict(format="0", ra_scs="1.25", root_sequence_index=100, zero_correlation_zone=1, start_preamble_index=0,
                nof_preamble_indices=64, nof_rx_ports=2)
    args.update(kw)
    return abi.make_prach(**args)


@pytest.mark.parametrize("name,cfg,want", [
    ("base", _base(), abi.OK),
    ("part of the preambles", _base(start_preamble_index=60, nof_preamble_indices=4), abi.OK),
    ("last root", _base(root_sequence_index=837), abi.OK),
    ("short", _base(format="B4", ra_scs="30", root_sequence_index=137, zero_correlation_zone=11), abi.OK),
    ("restricted set A", _base(restricted_set=1), abi.ERR_ARGUMENT),
    ("restricted set B", _base(restricted_set=2), abi.ERR_ARGUMENT),
    ("reserved N_CS", _base(zero_correlation_zone=16), abi.ERR_ARGUMENT),
    ("start + nof above 64", _base(start_preamble_index=1), abi.ERR_ARGUMENT),
    ("start above 64", _base(start_preamble_index=65, nof_preamble_indices=1), abi.ERR_ARGUMENT),
    ("nof wraps", _base(start_preamble_index=2, nof_preamble_indices=0xFFFFFFFF), abi.ERR_ARGUMENT),
    ("no preamble", _base(nof_preamble_indices=0), abi.ERR_ARGUMENT),
    ("no port", _base(nof_rx_ports=0), abi.ERR_ARGUMENT),
    ("5 ports", _base(nof_rx_ports=5, threshold=0.3, win_margin=5), abi.ERR_ARGUMENT),
    ("3 ports have no row", _base(nof_rx_ports=3), abi.ERR_ARGUMENT),
    ("3 ports with the caller's threshold", _base(nof_rx_ports=3, threshold=0.3, win_margin=5), abi.OK),
    ("long root index", _base(root_sequence_index=838), abi.ERR_ARGUMENT),
    ("short root index", _base(format="A1", ra_scs="15", root_sequence_index=138), abi.ERR_ARGUMENT),
    ("unknown format", _base(format=14), abi.ERR_ARGUMENT),
    ("unknown spacing", _base(ra_scs=6), abi.ERR_ARGUMENT),
    ("long format at 15 kHz", _base(ra_scs="15"), abi.ERR_ARGUMENT),
    ("long format at 5 kHz", _base(ra_scs="5"), abi.ERR_ARGUMENT),
    ("format 3 at 1.25 kHz", _base(format="3", ra_scs="1.25", threshold=0.3, win_margin=5), abi.ERR_ARGUMENT),
    ("short format at 1.25 kHz", _base(format="A1", ra_scs="1.25"), abi.ERR_ARGUMENT),
    ("red row", _base(format="2", zero_correlation_zone=0, nof_rx_ports=1), abi.ERR_ARGUMENT),
    ("red row with the caller's threshold", _base(format="2", zero_correlation_zone=0, nof_rx_ports=1, threshold=0.5, win_margin=5),
     abi.OK),
    ("format 3 has no row", _base(format="3", ra_scs="5"), abi.ERR_ARGUMENT),
    ("format 3 with the caller's threshold", _base(format="3", ra_scs="5", threshold=0.3, win_margin=5), abi.OK),
    ("C2 at 60 kHz with the caller's threshold", _base(format="C2", ra_scs="60", threshold=0.3, win_margin=12), abi.OK),
    ("mixed format with the caller's threshold", _base(format="A1/B1", ra_scs="15", threshold=0.3, win_margin=12), abi.OK),
    ("threshold without margin", _base(threshold=0.3), abi.ERR_ARGUMENT),
    ("margin without threshold", _base(win_margin=5), abi.ERR_ARGUMENT),
    ("negative threshold", _base(threshold=-0.3, win_margin=5), abi.ERR_ARGUMENT),
    ("NaN threshold", _base(threshold=float("nan"), win_margin=5), abi.ERR_ARGUMENT),
    ("infinite threshold", _base(threshold=float("inf"), win_margin=5), abi.ERR_ARGUMENT),
    ("margin longer than the transform", _base(threshold=0.3, win_margin=600), abi.ERR_ARGUMENT),
])
def test_prach_validator(name, cfg, want):
    assert lib.prach_validate(cfg) == want, name
    assert (lib.prach_window_width(cfg) != 0) == (want == abi.OK), name


def accepted_reference_configurations():
    rows = {(r["ports"], r["scs"], r["format"], r["zcz"]): r["flag"] for r in thresholds_fixture()}
    out = []
    for f in configs_fixture():
        flag = rows.get((f["nof_rx_ports"], f["ra_scs"], f["format"], f["zero_correlation_zone"]))
        if flag is not None and flag != "red":
            out.append(f)
    return out


def test_prach_validator_over_the_reference_configurations():
    fixtures = configs_fixture()
    assert len(fixtures) == 60
    accepted = accepted_reference_configurations()
    got = [f for f in fixtures if lib.prach_validate(to_abi(reference_cfg(f))) == abi.OK]
    assert got == accepted
    assert (len(got), len(fixtures) - len(got)) == (48, 12)
    for f in got:  # what the plan derives is what the restatement derives
        assert lib.prach_window_width(to_abi(reference_cfg(f))) == model.derive(reference_cfg(f))["win_width"]


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_extractor_reproduces_the_committed_fixtures():
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([os.environ.get("PYTHON", "python3"), os.path.join(GOLDEN, "extract_prach_configs.py"), REFERENCE, d], check=True,
                       timeout=120)
        for name in ("prach_thresholds.json", "prach_detector_configs.json"):
            assert open(os.path.join(d, name)).read() == open(os.path.join(GOLDEN, name)).read(), name
    # The root table the library and the restatement share is the reference's, entry for entry.
    text = open(os.path.join(REFERENCE, "lib", "phy", "upper", "channel_processors", "prach_generator_impl.cpp")).read()
    luts = re.findall(r"lut = \{([^}]*)\}", text)
    assert [int(x) for x in re.findall(r"\d+", luts[0])] == model.root_table(839)
    assert [int(x) for x in re.findall(r"\d+", luts[1])] == model.root_table(139)


def test_restatement_generator_equals_the_definition():
    """The table-driven float32 generator against the DFT of the Zadoff-Chu sequence in double.  Bound 2e-6 relative to the
    amplitude sqrt(L): float32 table entries at that amplitude, three ulp.  Measured: 6.4e-7."""
    worst = 0.0
    for fmt, root, pre, zcz in (("0", 834, 63, 1), ("0", 0, 0, 0), ("B4", 137, 63, 11), ("A1", 50, 17, 5), ("2", 400, 33, 9),
                                ("3", 22, 40, 7), ("1", 837, 63, 0)):
        err = np.abs(model.generate(fmt, root, zcz, pre) - model.generate_by_definition(fmt, root, zcz, pre)).max()
        worst = max(worst, err / np.sqrt(model.seq_len(fmt)))
    print("worst relative error %.3g" % worst)
    assert worst < 2e-6


RECORDED_FORMATS = ("0", "1", "2", "3", "A1", "A2", "A3", "B1", "B4", "C0", "C2")
_recording = {}


def recording():
    """The recorded occasions, read once: a list of dicts with cfg, x ([ports][symbols][L] complex64: the int16 pairs times
    2^-e), words, e, rssi_dB, time_resolution, time_advance_max, detections (rows of preamble index, time advance in seconds,
    detection_metric), group, origin and nof_tx."""
    if "cases" not in _recording:
        load = lambda name: np.load(os.path.join(GOLDEN, "prach_detector_reference_%s.npy" % name))
        rows, results, detections = load("cases"), load("results"), load("detections")
        inputs = [load("in%d" % k) for k in range(int(rows[:, 8].max()) + 1)]
        assert rows.shape[1] == 16 and results.shape == (len(rows), 3) and detections.shape[1] == 3
        out = []
        for r, res in zip(rows.tolist(), results):
            cfg = make_cfg(RECORDED_FORMATS[r[0]], r[3], r[6], r[2], model.SPACINGS[r[1]], r[4], r[5])
            words = inputs[r[8]][r[9]:r[9] + r[10]]
            value = np.ldexp(words.astype(np.float32), -r[7])
            assert value.dtype == np.float32
            x = (value[:, 0] + 1j * value[:, 1]).astype(np.complex64).reshape(r[6], model.NOF_SYMBOLS[cfg["format"]], -1)
            out.append(dict(cfg=cfg, x=x, words=words, e=r[7], rssi_dB=float(res[0]), time_resolution=float(res[1]),
                            time_advance_max=float(res[2]), detections=detections[r[11]:r[11] + r[12]], group=r[13], origin=r[14],
                            nof_tx=r[15]))
        _recording["cases"] = out
    return _recording["cases"]


def recorded_models():
    """model.detect(cfg, x, float64) of every recorded occasion, computed once and shared."""
    if "models" not in _recording:
        _recording["models"] = [model.detect(k["cfg"], k["x"], np.float64) for k in recording()]
    return _recording["models"]


def recorded_sequences():
    """[(format, root_sequence_index, zcz, preamble_index, sequence complex64 [L])] of the recording."""
    pairs = np.load(os.path.join(GOLDEN, "prach_detector_reference_sequences.npy"))
    out, at = [], 0
    while at != len(pairs):
        fmt = RECORDED_FORMATS[int(pairs[at, 0])]
        L = model.seq_len(fmt)
        y = pairs[at + 2:at + 2 + L]
        out.append((fmt, int(pairs[at, 1]), int(pairs[at + 1, 0]), int(pairs[at + 1, 1]), (y[:, 0] + 1j * y[:, 1]).astype(np.complex64)))
        at += 2 + L
    return out


def is_early_return(case):
    """The reference left before the search: the RSSI it reported is not a normal float32."""
    with np.errstate(under="ignore"):
        return not model.is_normal(np.asarray(np.float32(10.0) ** (np.float32(case["rssi_dB"]) / np.float32(10.0))))


def test_recording_is_what_its_header_states():
    """The files' sizes, the inputs recomputed from the int16 values and the scales, the case table against
    prach_detector_configs.json, the ground the edge shapes have to cover, and the two conditions under which no recorded decision
    is fragile, asserted with the float64 restatement."""
    names = [n for n in os.listdir(GOLDEN) if n.startswith("prach_detector_reference_")]
    sizes = [os.path.getsize(os.path.join(GOLDEN, n)) for n in names]
    assert max(sizes) < 900000 and sum(sizes) < 2000000, dict(zip(names, sizes))
    cases = recording()
    rows = {(r["ports"], r["scs"], r["format"], r["zcz"]): r["flag"] for r in thresholds_fixture()}
    for i, k in enumerate(cases):
        cfg = k["cfg"]
        assert k["words"].dtype == np.int16 and k["words"].shape == (cfg["nof_rx_ports"] * model.NOF_SYMBOLS[cfg["format"]] *
                                                                     model.seq_len(cfg["format"]), 2), i
        # Every input is its int16 times 2^-e exactly, in float32.
        back = np.ldexp(np.stack([k["x"].real, k["x"].imag], -1).astype(np.float64).reshape(-1, 2), k["e"])
        assert (back == k["words"]).all(), i
        assert rows[(cfg["nof_rx_ports"], cfg["ra_scs"], cfg["format"], cfg["zero_correlation_zone"])] != "red", i
        assert lib.prach_validate(to_abi(cfg)) == abi.OK, i
    # The first group is the accepted configurations of the reference's unit test, each reporting its preamble at its delay.
    fixtures = configs_fixture()
    accepted = accepted_reference_configurations()
    first = [k for k in cases if k["group"] == 0]
    assert len(first) == len(accepted) == 48 and all(k["group"] == 0 for k in cases[:48])
    for k, f in zip(first, accepted):
        assert fixtures[k["origin"]] == f and k["cfg"] == reference_cfg(f) and k["nof_tx"] == 1
        assert [int(v) for v in k["detections"][:, 0]] == [f["preamble_index"]]
        delay = f["true_delay"] * model.dft_size(f["format"]) * model.SCS_HZ[f["ra_scs"]]
        assert abs(k["detections"][0, 1] / k["time_resolution"] - delay) <= 2.0, f
    # The ground of the edge shapes.
    edges = cases[48:]
    assert all(k["group"] == 1 for k in edges) and [k["origin"] for k in edges] == list(range(len(edges)))
    derived = [model.derive(k["cfg"]) for k in edges]
    assert {k["cfg"]["format"] for k in edges} == {"0", "1", "A1", "A2", "B4"}
    assert {(k["cfg"]["format"], k["cfg"]["ra_scs"]) for k in edges} >= {("A1", "15"), ("A1", "30"), ("A2", "15"), ("A2", "30"),
                                                                       ("B4", "15"), ("B4", "30")}
    assert {k["cfg"]["nof_rx_ports"] for k in edges} == {1, 2, 4}
    assert any(d["n_cs"] == 0 for d in derived) and any(64 % d["nof_shifts"] for d in derived)
    assert any(k["cfg"]["nof_preamble_indices"] == 1 for k in edges)
    assert any(k["cfg"]["start_preamble_index"] % d["nof_shifts"] and
               (k["cfg"]["start_preamble_index"] + k["cfg"]["nof_preamble_indices"]) % d["nof_shifts"] for k, d in zip(edges, derived))
    assert any(k["cfg"]["root_sequence_index"] + d["nof_sequences"] > d["L"] - 1 for k, d in zip(edges, derived))
    reported = [(k, d, int(row[0]), int(round(row[1] / k["time_resolution"]))) for k, d in zip(edges, derived) for row in k["detections"]]
    assert any(p % d["nof_shifts"] == 0 for k, d, p, _ in reported if d["nof_shifts"] > 1)                     # window 0
    assert any(p % d["nof_shifts"] == d["nof_shifts"] - 1 for k, d, p, _ in reported if d["nof_shifts"] > 1)  # a root's last
    assert any(delay == math.ceil(0.8 * d["max_delay"]) - 1 for k, d, p, delay in reported)  # the last delay that is reported
    assert any(len(k["detections"]) >= 4 for k in edges)
    assert any(np.diff(k["detections"][:, 0]).min(initial=64) == 1 for k in edges)
    assert any(k["nof_tx"] > len(k["detections"]) and not is_early_return(k) for k in edges)  # transmitted, not reported
    assert any(k["nof_tx"] == 0 and not is_early_return(k) and len(k["detections"]) == 0 for k in edges)  # noise only
    assert any(k["rssi_dB"] == -np.inf and not k["words"].any() for k in edges)
    assert any(np.isfinite(k["rssi_dB"]) and is_early_return(k) and k["nof_tx"] > 0 for k in edges)  # subnormal RSSI
    assert any(k["words"].any() and not k["x"][-1].any() and len(k["detections"]) for k in edges)  # a port that is all zero
    assert all(is_early_return(k) == (k["rssi_dB"] < -300) and (not is_early_return(k) or len(k["detections"]) == 0) for k in cases)
    metrics = np.concatenate([k["detections"][:, 2] for k in cases])
    assert len(metrics) > 80 and metrics.min() >= 1.05 and metrics.max() <= 50.0
    # No fragile decision.
    windows = 0
    for i, (k, m) in enumerate(zip(cases, recorded_models())):
        th = m["derived"]["threshold"]
        for row in m["metric"]:
            if row is not None:
                top = np.sort(row)[-2:]
                windows += 1
                assert abs(top[1] / th - 1.0) >= RECORDING_MARGIN, (i, k["cfg"], float(top[1]), th)
                assert top[1] <= th or top[1] - top[0] > RECORDING_MARGIN * top[1], (i, k["cfg"], top)
    print("%d cases, %d monitored windows, %d detections with metrics %.2f ... %.2f" % (len(cases), windows, len(metrics),
                                                                                      metrics.min(), metrics.max()))


def compare_detections(case, m, what):
    """The decisions of a restatement result `m` against the recording, exactly; returns the largest relative difference of a
    detection metric."""
    assert m["time_resolution"] == case["time_resolution"] and m["time_advance_max"] == case["time_advance_max"], what
    want = case["detections"]
    assert [i for i in range(64) if m["detected"][i]] == [int(v) for v in want[:, 0]], what
    assert m["nof_detected"] == len(want), what
    worst = 0.0
    for index, advance, metric in want:
        assert m["delay"][int(index)] == int(round(advance / case["time_resolution"])), (what, index)
        assert m["time_advance"][int(index)] == advance, (what, index)
        worst = max(worst, abs(m["detection_metric"][int(index)] - metric) / metric)
    return worst


def test_restatement_equals_the_recording():
    """detect() of the restatement against the reference's on every recorded occasion: the detected set, every delay and both
    times exactly, in float64 and in float32.  The float64 restatement's distance from the recorded detection_metric and rssi_dB
    is the reference's own single-precision error: REF_SPREAD and REF_RSSI_SPREAD_DB, measured here.  The float32 restatement
    adds its own: MODEL_SPREAD for a metric, and for rssi_dB the rounding of log10f and of the product, two ulp of the value."""
    spread = rssi_spread = rssi_spread_audible = spread32 = 0.0
    for i, (case, m64) in enumerate(zip(recording(), recorded_models())):
        m32 = model.detect(case["cfg"], case["x"], np.float32)
        spread = max(spread, compare_detections(case, m64, (i, case["cfg"], "float64")))
        worst32 = compare_detections(case, m32, (i, case["cfg"], "float32"))
        spread32 = max(spread32, worst32)
        assert worst32 <= REF_SPREAD + MODEL_SPREAD, (i, case["cfg"], worst32)
        if np.isfinite(case["rssi_dB"]):
            err = abs(m64["rssi_dB"] - case["rssi_dB"])
            rssi_spread = max(rssi_spread, err)
            if abs(case["rssi_dB"]) < 64:
                rssi_spread_audible = max(rssi_spread_audible, err)
            assert abs(m32["rssi_dB"] - case["rssi_dB"]) <= REF_RSSI_SPREAD_DB + 2 * float(np.spacing(np.float32(abs(case["rssi_dB"])))), i
        else:
            assert m64["rssi_dB"] == case["rssi_dB"] == m32["rssi_dB"], i
    print("recorded - float64 restatement: detection metric %.3g relative (constant %.3g), rssi_dB %.3g dB (constant %.3g; %.3g dB "
          "where |rssi_dB| < 64); recorded - float32 restatement: detection metric %.3g"
          % (spread, REF_SPREAD, rssi_spread, REF_RSSI_SPREAD_DB, rssi_spread_audible, spread32))
    assert spread <= REF_SPREAD and rssi_spread <= REF_RSSI_SPREAD_DB
    # What the device is granted against the recording stays well inside the margin the recording keeps around every decision.
    assert 8 * REF_SPREAD < RECORDING_MARGIN / 4


def test_restatement_generator_equals_the_recording():
    """model.generate against prach_generator_impl::generate on the recorded tuples: both lengths, roots 0 and L - 2, zcz 0 and
    15, preamble 63, root indices that wrap.  A wrong table index moves a sample by at least 2 pi / 4L x sqrt(L), 1.9e-3 sqrt(L)
    on 839 elements; the measured difference is far below it."""
    tuples = recorded_sequences()
    assert len(tuples) == 12 and {len(y) for *_, y in tuples} == {839, 139}
    assert {(model.seq_len(f), r) for f, r, _, _, _ in tuples} >= {(839, 0), (839, 837), (139, 0), (139, 137)}
    assert {z for _, _, z, _, _ in tuples} >= {0, 15} and any(p == 63 for _, _, _, p, _ in tuples)
    assert any(r + (p if model.n_cs(model.default_scs(f), z) == 0 else p // (model.seq_len(f) // model.n_cs(model.default_scs(f), z)))
               >= model.seq_len(f) - 1 for f, r, z, p, _ in tuples)
    worst = 0.0
    for fmt, root, zcz, pre, want in tuples:
        got = model.generate(fmt, root, zcz, pre)
        err = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max()) / np.sqrt(model.seq_len(fmt))
        worst = max(worst, float(err))
    print("recorded - restatement generator: %.3g sqrt(L) (constant %.3g)" % (worst, REF_GENERATOR_SPREAD))
    assert worst <= REF_GENERATOR_SPREAD
    assert REF_GENERATOR_SPREAD < 1e-3 * 2 * np.pi / (4 * 839)


# =======================================================================================================================
# GPU
# =======================================================================================================================
def guarded(words):
    """A device buffer of `words` 32-bit words between two guards of sentinel words: (whole tensor, the view to hand over)."""
    import torch
    whole = torch.full((words + 2 * GUARD,), np.int32(np.uint32(SENTINEL).view(np.int32)), dtype=torch.int32, device="cuda")
    return whole, whole[GUARD:GUARD + words]


def guards_intact(whole):
    a = whole.cpu().numpy().view(np.uint32)
    return bool((a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all())


def pack(cfgs, buffers):
    """Occasions of mixed formats in one buffer: [occasion][port 0..3][symbol 0..11][839], zeros where an occasion has less."""
    x = np.zeros((len(cfgs), 4, 12, 839), np.complex64)
    for i, b in enumerate(buffers):
        x[i, :b.shape[0], :b.shape[1], :b.shape[2]] = b
    return x, [i * 4 * 12 * 839 for i in range(len(cfgs))], 12 * 839, 839


def run_plan(ctx, cfgs, x, offsets, port_stride, symbol_stride, with_metric=True, stream=None, outputs=None, plan=None):
    """nrphy_prach_run on a plan of cfgs over the device copy of x; returns (results, preambles [n][64], metric [n][64][stride] or
    None) as NumPy arrays, after checking the guards around every output."""
    own = plan is None
    if own:
        plan = lib.PrachPlan(ctx, [to_abi(c) for c in cfgs], offsets, port_stride, symbol_stride)
    n, stride = len(cfgs), plan.metric_stride
    d_x = dev(np.ascontiguousarray(x).view(np.float32)) if not hasattr(x, "data_ptr") else x
    res_w, res = guarded(n * RESULT_DTYPE.itemsize // 4)
    pre_w, pre = guarded(n * 64 * PREAMBLE_DTYPE.itemsize // 4)
    met_w, met = guarded(n * 64 * stride) if with_metric else (None, None)
    plan.run(d_x, res, pre, met, stream=stream)
    ctx.synchronize()
    assert guards_intact(res_w) and guards_intact(pre_w) and (met_w is None or guards_intact(met_w))
    out = (res.cpu().numpy().view(RESULT_DTYPE), pre.cpu().numpy().view(PREAMBLE_DTYPE).reshape(n, 64),
           met.cpu().numpy().view(np.float32).reshape(n, 64, stride) if with_metric else None)
    if own:
        plan.close()
    return out


def detected_indices(pre_row):
    return [int(i) for i in np.nonzero(pre_row["detected"])[0]]


def check_header(res, pre_row, m, what):
    assert abs(float(res["rssi_dB"]) - m["rssi_dB"]) <= RSSI_TOL_DB, (what, float(res["rssi_dB"]), m["rssi_dB"])
    assert res["time_resolution_s"] == np.float32(m["time_resolution"]), what
    assert res["time_advance_max_s"] == np.float32(m["time_advance_max"]), what
    found = detected_indices(pre_row)
    assert int(res["nof_detected"]) == len(found) and int(res["detected_mask"]) == sum(1 << i for i in found), what


def compare_with_model(cfg, res, pre_row, metric_rows, m, what, stats):
    """One occasion against the float64 restatement `m`; decisions near the threshold and exact ties are set aside (counted)."""
    check_header(res, pre_row, m, what)
    win = m["derived"]["win_width"]
    th = m["derived"]["threshold"]
    start, end = cfg["start_preamble_index"], cfg["start_preamble_index"] + cfg["nof_preamble_indices"]
    for i in range(64):
        if not (start <= i < end):
            assert pre_row[i].tobytes() == bytes(PREAMBLE_DTYPE.itemsize), (what, i)
            assert not metric_rows[i].any(), (what, i)
            continue
        want = m["metric"][i]
        got = metric_rows[i, :win]
        err = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-3)
        stats["metric"] = max(stats["metric"], float(err.max()))
        assert err.max() <= METRIC_TOL, (what, i, float(err.max()))
        assert not metric_rows[i, win:].any(), (what, i)
        perr = abs(float(pre_row[i]["peak"]) - m["peak"][i]) / max(abs(m["peak"][i]), 1e-3)
        assert perr <= METRIC_TOL, (what, i, perr)
        assert abs(float(pre_row[i]["detection_metric"]) - m["peak"][i] / th) <= METRIC_TOL * max(m["peak"][i], 1e-3) / th * 1.001, (what, i)
        stats["pairs"] += 1
        if m["tie"][i] or abs(m["peak"][i] / th - 1.0) < 0.01:
            stats["set_aside"] += 1
            continue
        assert bool(pre_row[i]["detected"]) == m["detected"][i], (what, i, float(pre_row[i]["peak"]), m["peak"][i], th)
        assert int(pre_row[i]["delay_samples"]) == m["delay"][i], (what, i)
        assert abs(float(pre_row[i]["time_advance_s"]) - m["time_advance"][i]) <= model.T_C, (what, i)


@pytest.mark.gpu
def test_generator_equals_the_restatement(gpu_ctx):
    """Every sample within 4e-7 sqrt(L) of the restatement's table-driven float32 generator: the table entries come from two
    libms that may differ by an ulp, while a wrong table index moves a sample by at least 2 pi / 4L x sqrt(L)."""
    rng = np.random.default_rng(11)
    for fmt, scs in (("0", "1.25"), ("B4", "15")):
        L = model.seq_len(fmt)
        cases = [(L - 2, 63, 1), (L - 2, 63, 0), (0, 0, 0), (L - 2, 0, 15), (L - 40, 63, 3)]
        cases += [(int(rng.integers(0, L - 1)), int(rng.integers(0, 64)), int(rng.integers(0, 16))) for _ in range(32)]
        worst = 0.0
        for root, pre, zcz in cases:
            got = gpu_ctx.prach_generate_host(abi.make_prach(format=fmt, ra_scs=scs, root_sequence_index=root, zero_correlation_zone=zcz),
                                              pre)
            want = model.generate(fmt, root, zcz, pre, scs)
            err = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max()) / np.sqrt(L)
            worst = max(worst, float(err))
            assert err <= 4e-7, (fmt, root, pre, zcz, float(err))
        print("format %s: worst error %.3g sqrt(L) over %d cases" % (fmt, worst, len(cases)))
    assert gpu_ctx.lib.nrphy_prach_generate_host(gpu_ctx.handle, C.byref(abi.make_prach(format="0", root_sequence_index=838)), 0,
                                                 np.zeros(839, np.complex64).ctypes.data) == abi.ERR_ARGUMENT


@pytest.mark.gpu
def test_reference_configurations_are_detected(gpu_ctx):
    """Each accepted configuration of the reference's unit test, on a buffer that carries its expected preamble at unit power,
    delayed by true_delay, with a phase per port and noise at -20 dB: exactly that preamble, within 2 correlation samples (the
    floored window start biases the delay by less than one sample, quantisation adds at most half)."""
    rng = np.random.default_rng(21)
    fixtures = accepted_reference_configurations()
    assert len(fixtures) == 48
    cfgs, buffers, delays = [], [], []
    for f in fixtures:
        cfg = reference_cfg(f)
        delay = f["true_delay"] * model.dft_size(f["format"]) * model.SCS_HZ[f["ra_scs"]]
        cfgs.append(cfg)
        delays.append(delay)
        buffers.append(model.transmit(cfg, [(f["preamble_index"], delay, 1.0)], rng, noise_std=0.1))
    res, pre, _ = run_plan(gpu_ctx, cfgs, *pack(cfgs, buffers), with_metric=False)
    worst = 0.0
    for i, f in enumerate(fixtures):
        assert detected_indices(pre[i]) == [f["preamble_index"]], (i, f)
        assert int(res[i]["nof_detected"]) == 1 and int(res[i]["detected_mask"]) == 1 << f["preamble_index"]
        err = abs(float(pre[i][f["preamble_index"]]["delay_samples"]) - delays[i])
        worst = max(worst, err)
        assert err <= 2.0, (i, f, err)
    print("48 of 48 detected, worst delay error %.3f samples" % worst)


def check_against_recording(case, res, pre_row, what, stats):
    """One occasion's result header and preamble slots (NumPy records) against the recording."""
    found = detected_indices(pre_row)
    want = case["detections"]
    assert found == [int(v) for v in want[:, 0]], (what, found)
    assert int(res["nof_detected"]) == len(found) and int(res["detected_mask"]) == sum(1 << i for i in found), what
    assert res["time_resolution_s"] == np.float32(case["time_resolution"]), what
    assert res["time_advance_max_s"] == np.float32(case["time_advance_max"]), what
    if np.isfinite(case["rssi_dB"]):
        err = abs(float(res["rssi_dB"]) - case["rssi_dB"])
        stats["rssi"] = max(stats["rssi"], err)
        assert err <= RSSI_TOL_DB + REF_RSSI_SPREAD_DB, (what, float(res["rssi_dB"]), case["rssi_dB"])
    else:
        assert float(res["rssi_dB"]) == case["rssi_dB"], what
    for index, advance, metric in want:
        slot = pre_row[int(index)]
        assert int(slot["delay_samples"]) == int(round(advance / case["time_resolution"])), (what, index)
        assert abs(float(slot["time_advance_s"]) - advance) <= model.T_C, (what, index)
        err = abs(float(slot["detection_metric"]) - metric) / metric
        stats["ref_metric"] = max(stats["ref_metric"], err)
        assert err <= 8 * REF_SPREAD, (what, index, float(slot["detection_metric"]), metric)
    start, end = case["cfg"]["start_preamble_index"], case["cfg"]["start_preamble_index"] + case["cfg"]["nof_preamble_indices"]
    for i in range(64):
        if not (start <= i < end) or is_early_return(case):
            assert pre_row[i].tobytes() == bytes(PREAMBLE_DTYPE.itemsize), (what, i)


def check_recorded_occasion(case, m64, res, pre_row, metric_rows, what, stats):
    """Against the recording, and, for what the reference does not expose (the metric rows, the slots it does not report),
    against the float64 restatement as test_parity_with_the_restatement does."""
    check_against_recording(case, res, pre_row, what, stats)
    if is_early_return(case):
        assert not metric_rows.any(), what
    else:
        compare_with_model(case["cfg"], res, pre_row, metric_rows, m64, what, stats)


@pytest.mark.gpu
def test_recorded_occasions_on_the_device(gpu_ctx):
    """Every recorded occasion through nrphy_prach_run, formats mixed in one plan, against the reference's answers: the detected
    set, nof_detected, the mask and every delay identical, the times to float32 and T_c, detection_metric within 8 REF_SPREAD
    (the factor this file grants the device for its order of summation), rssi_dB within RSSI_TOL_DB + REF_RSSI_SPREAD_DB.  Nothing
    is set aside."""
    cases, models = recording(), recorded_models()
    stats = dict(metric=0.0, pairs=0, set_aside=0, ref_metric=0.0, rssi=0.0)
    for first in range(0, len(cases), 100):
        part = cases[first:first + 100]
        cfgs = [k["cfg"] for k in part]
        res, pre, met = run_plan(gpu_ctx, cfgs, *pack(cfgs, [k["x"] for k in part]))
        for i, case in enumerate(part):
            check_recorded_occasion(case, models[first + i], res[i], pre[i], met[i], (first + i, case["cfg"]), stats)
    print("%d occasions: device - recorded detection metric %.3g relative (allowed %.3g), rssi_dB %.3g dB (allowed %.3g); device - "
          "float64 restatement metric rows %.3g (allowed %.3g); %d pairs, %d set aside"
          % (len(cases), stats["ref_metric"], 8 * REF_SPREAD, stats["rssi"], RSSI_TOL_DB + REF_RSSI_SPREAD_DB, stats["metric"], METRIC_TOL,
             stats["pairs"], stats["set_aside"]))
    assert stats["set_aside"] == 0


@pytest.mark.gpu
def test_recorded_occasions_through_the_host_entry_point(gpu_ctx):
    """nrphy_prach_detect_host on recorded occasions of each shape: long and short, 1, 2 and 4 ports, 1, 2, 4 and 12 symbols, zcz
    0, part of the preambles monitored, and both early returns."""
    cases, models = recording(), recorded_models()
    picked, seen = [], set()
    for i, k in enumerate(cases[48:], 48):  # the first edge shape of each kind
        cfg = k["cfg"]
        kind = (cfg["format"], cfg["nof_rx_ports"], cfg["zero_correlation_zone"] == 0, cfg["nof_preamble_indices"] == 64,
                is_early_return(k), np.isfinite(k["rssi_dB"]))
        if (kind[0], kind[1]) not in seen or kind[2:] not in seen:
            picked.append(i)
        seen.update([(kind[0], kind[1]), kind[2:]])
    assert 8 <= len(picked) <= 16
    assert {cases[i]["cfg"]["format"] for i in picked} == {"0", "1", "A1", "A2", "B4"}
    assert {cases[i]["cfg"]["nof_rx_ports"] for i in picked} == {1, 2, 4}
    stats = dict(metric=0.0, pairs=0, set_aside=0, ref_metric=0.0, rssi=0.0)
    for i in picked:
        case = cases[i]
        r, p, met = gpu_ctx.prach_detect_host(to_abi(case["cfg"]), case["x"], with_metric=True)
        check_recorded_occasion(case, models[i], np.frombuffer(bytes(r), RESULT_DTYPE)[0], np.frombuffer(bytes(p), PREAMBLE_DTYPE), met,
                                (i, case["cfg"]), stats)
    print("%d occasions: device - recorded detection metric %.3g relative, rssi_dB %.3g dB" % (len(picked), stats["ref_metric"], stats["rssi"]))
    assert stats["set_aside"] == 0


@pytest.mark.gpu
def test_generator_equals_the_recording(gpu_ctx):
    """nrphy_prach_generate_host against prach_generator_impl::generate on the recorded tuples, within the 4e-7 sqrt(L) of
    test_generator_equals_the_restatement plus the restatement's measured distance from the recording."""
    worst = 0.0
    for fmt, root, zcz, pre, want in recorded_sequences():
        got = gpu_ctx.prach_generate_host(abi.make_prach(format=fmt, ra_scs=model.default_scs(fmt), root_sequence_index=root,
                                                         zero_correlation_zone=zcz), pre)
        err = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max()) / np.sqrt(model.seq_len(fmt))
        worst = max(worst, float(err))
        assert err <= 4e-7 + REF_GENERATOR_SPREAD, (fmt, root, zcz, pre, float(err))
    print("device - recorded generator: %.3g sqrt(L) (allowed %.3g)" % (worst, 4e-7 + REF_GENERATOR_SPREAD))


def parity_occasions(rng, count):
    """Seeded occasions over formats 0, 1, 2, A1, A2, B4 with 1 / 2 / 4 ports: every non-red row of the table once, then rows
    drawn at random.  Three in four carry one or two preambles at -5 ... +15 dB over unit-variance noise, delayed by up to half
    the usable window; one in four is noise only."""
    rows = [r for r in thresholds_fixture() if r["flag"] != "red"]
    picks = rows + [rows[int(i)] for i in rng.integers(0, len(rows), max(0, count - len(rows)))]
    out = []
    for k, r in enumerate(picks):
        L = model.seq_len(r["format"])
        cfg = make_cfg(r["format"], r["zcz"], r["ports"], int(rng.integers(0, L - 1)), r["scs"])
        if k % 5 == 4:  # a part of the preambles only
            start = int(rng.integers(0, 60))
            cfg.update(start_preamble_index=start, nof_preamble_indices=int(rng.integers(1, 65 - start)))
        d = model.derive(cfg)
        usable = 0.5 * min(d["win_width"], 0.8 * d["max_delay"])
        tx = []
        if k % 4 != 3:
            for index in rng.choice(64, 1 + int(rng.integers(0, 2)), replace=False):
                tx.append((int(index), float(rng.uniform(0, usable)), 10 ** (float(rng.uniform(-5, 15)) / 20)))
        out.append((cfg, model.transmit(cfg, tx, rng, noise_std=1.0)))
    return out


@pytest.mark.gpu
def test_parity_with_the_restatement(gpu_ctx):
    """Every output against the float64 restatement on 600 seeded occasions (38,400 slots).  A (occasion, preamble) pair is left
    out of the decision comparison only if the restatement puts its peak within 1 % of the threshold or the two largest samples of
    its window are equal; the share left out must not exceed 0.1 %."""
    rng = np.random.default_rng(31)
    occasions = parity_occasions(rng, 600)
    assert len(occasions) >= 600
    stats = dict(metric=0.0, pairs=0, set_aside=0)
    spread = 0.0
    for first in range(0, len(occasions), 100):
        part = occasions[first:first + 100]
        cfgs = [c for c, _ in part]
        res, pre, met = run_plan(gpu_ctx, cfgs, *pack(cfgs, [b for _, b in part]))
        for i, (cfg, x) in enumerate(part):
            m64 = model.detect(cfg, x, np.float64)
            m32 = model.detect(cfg, x, np.float32)
            for a, b in zip(m32["metric"], m64["metric"]):
                if b is not None:
                    spread = max(spread, float((np.abs(a.astype(np.float64) - b) / np.maximum(np.abs(b), 1e-3)).max()))
            compare_with_model(cfg, res[i], pre[i], met[i], m64, (first + i, cfg), stats)
    print("float32 - float64 restatement spread %.3g (constant %.3g); device - float64 worst %.3g (allowed %.3g); "
          "%d pairs, %d set aside" % (spread, MODEL_SPREAD, stats["metric"], METRIC_TOL, stats["pairs"], stats["set_aside"]))
    assert stats["set_aside"] <= 0.001 * stats["pairs"]


@pytest.mark.gpu
def test_zero_buffer_gives_the_header_and_no_detection(gpu_ctx):
    cfg = make_cfg("0", 1, 2, 5)
    x = np.zeros((2, 1, 839), np.complex64)
    res, pre, met = gpu_ctx.prach_detect_host(to_abi(cfg), x, with_metric=True)
    d = model.derive(cfg)
    assert res.rssi_dB == -np.inf and res.nof_detected == 0 and res.detected_mask == 0
    assert np.float32(res.time_resolution_s) == np.float32(d["time_resolution"])
    assert np.float32(res.time_advance_max_s) == np.float32(d["time_advance_max"])
    assert bytes(pre) == bytes(64 * PREAMBLE_DTYPE.itemsize) and not met.any()


@pytest.mark.gpu
def test_noise_only_occasions_give_no_detection(gpu_ctx):
    """200 seeded noise-only occasions at the table's thresholds.  The restatement is asked first, so that a false alarm of the
    algorithm itself is not blamed on the device."""
    rng = np.random.default_rng(41)
    rows = [r for r in thresholds_fixture() if r["flag"] != "red"]
    occasions = []
    for k in range(200):
        r = rows[int(rng.integers(0, len(rows)))]
        cfg = make_cfg(r["format"], r["zcz"], r["ports"], int(rng.integers(0, model.seq_len(r["format"]) - 1)), r["scs"])
        occasions.append((cfg, model.transmit(cfg, [], rng, noise_std=float(rng.uniform(0.1, 10.0)))))
    for cfg, x in occasions:
        assert model.detect(cfg, x, np.float64)["nof_detected"] == 0, cfg
    cfgs = [c for c, _ in occasions]
    res, pre, _ = run_plan(gpu_ctx, cfgs, *pack(cfgs, [b for _, b in occasions]), with_metric=False)
    assert not pre["detected"].any() and not res["nof_detected"].any() and not res["detected_mask"].any()


@pytest.mark.gpu
def test_adjacent_shifts_and_unmonitored_preambles(gpu_ctx):
    rng = np.random.default_rng(51)
    # Preambles 20 and 21 share a root (N_CS = 13: 64 shifts per root) in adjacent windows.
    cfg = make_cfg("0", 1, 2, 77)
    x = model.transmit(cfg, [(20, 3.0, 1.0), (21, 5.0, 1.0)], rng, noise_std=0.1)
    res, pre, _ = gpu_ctx.prach_detect_host(to_abi(cfg), x)
    pre = np.frombuffer(bytes(pre), PREAMBLE_DTYPE)
    assert detected_indices(pre) == [20, 21] and res.nof_detected == 2 and res.detected_mask == (1 << 20) | (1 << 21)
    assert abs(int(pre[20]["delay_samples"]) - 3) <= 2 and abs(int(pre[21]["delay_samples"]) - 5) <= 2
    # The same buffer with only [0, 21) monitored: 21 is not reported and its slot is zero.
    part = dict(cfg, start_preamble_index=0, nof_preamble_indices=21)
    res, pre, _ = gpu_ctx.prach_detect_host(to_abi(part), x)
    pre = np.frombuffer(bytes(pre), PREAMBLE_DTYPE)
    assert detected_indices(pre) == [20] and res.nof_detected == 1
    assert pre[21:].tobytes() == bytes(43 * PREAMBLE_DTYPE.itemsize)
    # A preamble of another root (B4, N_CS = 23: 6 shifts per root), outside [12, 18).
    cfg = make_cfg("B4", 11, 4, 130, "30", start=12, nof=6)
    x = model.transmit(cfg, [(13, 2.0, 1.0), (40, 2.0, 1.0)], rng, noise_std=0.1)
    res, pre, _ = gpu_ctx.prach_detect_host(to_abi(cfg), x)
    assert detected_indices(np.frombuffer(bytes(pre), PREAMBLE_DTYPE)) == [13] and res.detected_mask == 1 << 13


@pytest.mark.gpu
def test_formats_without_a_row_run_with_the_callers_threshold(gpu_ctx):
    rng = np.random.default_rng(61)
    stats = dict(metric=0.0, pairs=0, set_aside=0)
    for fmt, scs, zcz, ports, margin in (("3", "5", 4, 2, 5), ("3", "5", 0, 1, 5), ("C2", "15", 9, 4, 12), ("C2", "60", 3, 2, 12),
                                         ("A3/B3", "30", 12, 1, 12)):
        cfg = make_cfg(fmt, zcz, ports, 17, scs, threshold=0.35, win_margin=margin)
        assert lib.prach_validate(to_abi(dict(cfg, threshold=0.0, win_margin=0))) == abi.ERR_ARGUMENT
        d = model.derive(cfg)
        x = model.transmit(cfg, [(33, 0.3 * d["max_delay"], 1.0)], rng, noise_std=0.3)
        res, pre, met = run_plan(gpu_ctx, [cfg], *pack([cfg], [x]))
        m = model.detect(cfg, x, np.float64)
        assert m["detected"][33]
        compare_with_model(cfg, res[0], pre[0], met[0], m, cfg, stats)
        assert detected_indices(pre[0]) == [i for i in range(64) if m["detected"][i]]
    assert stats["set_aside"] <= 2


def mixed_batch(rng):
    cfgs = [make_cfg("0", 0, 4, 830), make_cfg("B4", 11, 2, 100, "15"), make_cfg("1", 6, 1, 3), make_cfg("A1", 0, 4, 137, "30"),
            make_cfg("2", 9, 2, 500, start=10, nof=30, threshold=0.145, win_margin=5), make_cfg("A2", 14, 1, 7, "15"), make_cfg("0", 12, 2, 400),
            make_cfg("C0", 5, 3, 9, "120", threshold=0.4, win_margin=12)]
    buffers = []
    for k, cfg in enumerate(cfgs):
        d = model.derive(cfg)
        tx = [(int(rng.integers(cfg["start_preamble_index"], cfg["start_preamble_index"] + cfg["nof_preamble_indices"])),
               0.3 * d["max_delay"], 1.0)] if k != 2 else []
        buffers.append(model.transmit(cfg, tx, rng, noise_std=0.5))
    return cfgs, buffers


@pytest.mark.gpu
def test_mixed_batch_equals_per_occasion_host_calls(gpu_ctx):
    rng = np.random.default_rng(71)
    cfgs, buffers = mixed_batch(rng)
    res, pre, met = run_plan(gpu_ctx, cfgs, *pack(cfgs, buffers))
    assert np.count_nonzero(pre["detected"]) >= 6
    for i, (cfg, x) in enumerate(zip(cfgs, buffers)):
        r, p, m = gpu_ctx.prach_detect_host(to_abi(cfg), x, with_metric=True)
        assert bytes(r) == res[i].tobytes(), i
        assert bytes(p) == pre[i].tobytes(), i
        assert m.shape[1] == model.derive(cfg)["win_width"]
        assert m.tobytes() == met[i, :, :m.shape[1]].tobytes() and not met[i, :, m.shape[1]:].any(), i


@pytest.mark.gpu
def test_strided_input_equals_packed_input(gpu_ctx):
    """A prach_buffer tensor (re, symbol, td occasion, fd occasion, port; re fastest) with 3 x 2 occasions read in place."""
    rng = np.random.default_rng(81)
    cfg = make_cfg("A2", 8, 4, 60, "30")
    nsym, L, ntd, nfd, ports = 4, 139, 3, 2, 4
    occ = [model.transmit(cfg, [(int(rng.integers(0, 64)), 1.5, 1.0)], rng, noise_std=0.3) for _ in range(ntd * nfd)]
    tensor = np.zeros((ports, nfd, ntd, nsym, L), np.complex64)
    for i, x in enumerate(occ):
        tensor[:, i // ntd, i % ntd] = x
    offsets = [((i // ntd) * ntd + i % ntd) * nsym * L for i in range(ntd * nfd)]
    cfgs = [cfg] * len(occ)
    strided = run_plan(gpu_ctx, cfgs, tensor, offsets, nfd * ntd * nsym * L, L)
    packed = run_plan(gpu_ctx, cfgs, *pack(cfgs, occ))
    for a, b in zip(strided, packed):
        assert a.tobytes() == b.tobytes()
    assert all(len(detected_indices(row)) == 1 for row in strided[1])


@pytest.mark.gpu
def test_graph_replay_and_two_runs_give_identical_bytes(gpu_ctx):
    import torch
    rng = np.random.default_rng(91)
    cfgs, buffers = mixed_batch(rng)
    x, offsets, port_stride, symbol_stride = pack(cfgs, buffers)
    plan = lib.PrachPlan(gpu_ctx, [to_abi(c) for c in cfgs], offsets, port_stride, symbol_stride)
    d_x = dev(x.view(np.float32))
    first = run_plan(gpu_ctx, cfgs, d_x, offsets, port_stride, symbol_stride, plan=plan)
    second = run_plan(gpu_ctx, cfgs, d_x, offsets, port_stride, symbol_stride, plan=plan)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    n, stride = len(cfgs), plan.metric_stride
    res_w, res = guarded(n * RESULT_DTYPE.itemsize // 4)
    pre_w, pre = guarded(n * 64 * PREAMBLE_DTYPE.itemsize // 4)
    met_w, met = guarded(n * 64 * stride)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plan.run(d_x, res, pre, met, stream=C.c_void_p(stream.cuda_stream))
    for _ in range(2):
        res.zero_()
        pre.zero_()
        met.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert res.cpu().numpy().tobytes() == first[0].tobytes()
        assert pre.cpu().numpy().tobytes() == first[1].tobytes()
        assert met.cpu().numpy().tobytes() == first[2].tobytes()
        assert guards_intact(res_w) and guards_intact(pre_w) and guards_intact(met_w)
    plan.close()
