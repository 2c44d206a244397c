"""PRACH generator and detector (nrphy_prach_*).

CPU: the POD mirrors, nrphy_prach_threshold over the whole cross product against tests/golden/prach_thresholds.json, the validator
over each refused case and over the reference unit test's 60 configurations (tests/golden/prach_detector_configs.json), the
extractor that wrote both fixtures, and the restatement's generator (tests/prach_model.py) against the definition of the sequence.
GPU: the device's generator against the restatement's; the reference configurations on buffers built here; parity of every
output with the float64 restatement on seeded random occasions; physics (zero buffer, noise only, adjacent shifts, unmonitored
preambles, caller's thresholds); batches against per-occasion host calls, strided input, graph replay, sentinels.
"""
import ctypes as C
import json
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
# occasions of test_parity_with_the_restatement (the test prints it again on every run): 3.73e-4.  The device may differ from the
# float64 restatement by 8 x that: its radix-16 transform and window sums order their additions differently from the
# restatement's FFT and pairwise sums, and both errors grow with log N.  (The reference binary cannot be built for this block,
# so the float32 restatement stands in for the reference's own error.)
MODEL_SPREAD = 3.73e-4
METRIC_TOL = 8 * MODEL_SPREAD
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
