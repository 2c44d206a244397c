"""OFDM PRACH demodulator (nrphy_prach_demod_*): baseband samples to the prach_buffer.

CPU: the POD mirrors and the exported symbols, the validator over each refused case, over the reference unit test's 112
configurations (tests/golden/prach_demod_configs.json) and against the restatement on a seeded sweep, nrphy_prach_demod_sizes, the
generated tables against their fixture, the extractor, and the float64 restatement (tests/prach_demod_model.py) against the
reference's own answers (tests/golden/prach_demod_reference_*.npy, recorded by tests/golden/record_prach_demod_reference.cpp on
inputs both sides generate from one integer sequence).
GPU: every recorded case against the recording and the restatement; sentinels around and inside an oversized buffer; a mixed batch
against per-item host calls, two runs and a graph replay; samples to detected preambles on one stream; zero input; refused plans.

The measure is test_dft_vs_oracle's: the largest |a - b| of a case over its largest |b|.  The limit is the project's 1e-5 for IQ.
"""
import ctypes as C
import functools
import importlib.util
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import backends
import prach_demod_model as model
from pusch_chest_model import dev

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
REFERENCE = "/root/reference/srsRAN-5G-ER"
TOL = 1e-5
SENTINEL = np.complex64(complex(-7.25e8, 3.5e-9))  # no transform of inputs below 1 in magnitude comes near it
GUARD = 64
RESULT_DTYPE = np.dtype([("rssi_dB", "<f4"), ("time_resolution_s", "<f4"), ("time_advance_max_s", "<f4"), ("nof_detected", "<u4"),
                         ("detected_mask", "<u8")])
PREAMBLE_DTYPE = np.dtype([("detected", "<u4"), ("delay_samples", "<u4"), ("time_advance_s", "<f4"), ("peak", "<f4"),
                           ("detection_metric", "<f4")])


def to_abi(cfg):
    return abi.make_prach_demod(**cfg)


def make_cfg(srate_hz=30720000, format="0", ntd=1, nfd=2, start=0, rb=0, nprb=79, mu=0, ports=1):
    return dict(srate_hz=srate_hz, format=format, nof_td_occasions=ntd, nof_fd_occasions=nfd, start_symbol=start, rb_offset=rb,
                nof_prb_ul_grid=nprb, pusch_numerology=mu, nof_rx_ports=ports)


def configs_fixture():
    return json.load(open(os.path.join(GOLDEN, "prach_demod_configs.json")))


def fixture_cfg(f):
    return make_cfg(f["srate_hz"], f["format"], f["nof_td_occasions"], f["nof_fd_occasions"], f["start_symbol"], f["rb_offset"],
                    f["nof_prb_ul_grid"], {15: 0, 30: 1, 60: 2, 120: 3}[f["pusch_scs_kHz"]])


@functools.lru_cache(maxsize=None)
def recording():
    """[(configuration, input samples, the reference's [td][fd][symbol][L_RA])] of every recorded case."""
    cases = np.load(os.path.join(GOLDEN, "prach_demod_reference_cases.npy"))
    files, out = {}, []
    for row in cases:
        srate, fmt, ntd, nfd, start, rb, nprb, mu, n_in, shard, offset, count = (int(v) for v in row)
        if shard not in files:
            files[shard] = np.load(os.path.join(GOLDEN, "prach_demod_reference_out%d.npy" % shard))
        cfg = make_cfg(srate, model.FORMATS[fmt], ntd, nfd, start, rb, nprb, mu)
        d = model.derive(cfg)
        out.append((cfg, n_in, files[shard][offset:offset + count].reshape(ntd, nfd, d["nof_symbols"], d["L"])))
    return out


@functools.lru_cache(maxsize=None)
def restated():
    """The float64 restatement of every recorded case, computed once and shared."""
    out = []
    for index, (cfg, n_in, _) in enumerate(recording()):
        x = model.lcg_samples(index, n_in)
        out.append((x, model.demodulate(cfg, x)))
    return out


def distance(a, b):
    return float(np.abs(np.asarray(a, np.complex128) - b).max() / np.abs(b).max())


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_prach_demod_pods_match_header():
    src = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(nrphy_prach_demod_cfg_t),
 offsetof(nrphy_prach_demod_cfg_t, srate_hz), offsetof(nrphy_prach_demod_cfg_t, format), offsetof(nrphy_prach_demod_cfg_t, nof_td_occasions),
 offsetof(nrphy_prach_demod_cfg_t, nof_fd_occasions), offsetof(nrphy_prach_demod_cfg_t, start_symbol),
 offsetof(nrphy_prach_demod_cfg_t, rb_offset), offsetof(nrphy_prach_demod_cfg_t, nof_prb_ul_grid),
 offsetof(nrphy_prach_demod_cfg_t, pusch_numerology), offsetof(nrphy_prach_demod_cfg_t, nof_rx_ports),
 sizeof(nrphy_prach_demod_sizes_t), offsetof(nrphy_prach_demod_sizes_t, sequence_length),
 offsetof(nrphy_prach_demod_sizes_t, nof_symbols), offsetof(nrphy_prach_demod_sizes_t, window_samples));return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(backends.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True, timeout=120)
        out = subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()
    P, S = abi.PrachDemodCfg, abi.PrachDemodSizes
    assert [int(x) for x in out] == [C.sizeof(P), P.srate_hz.offset, P.format.offset, P.nof_td_occasions.offset,
                                     P.nof_fd_occasions.offset, P.start_symbol.offset, P.rb_offset.offset, P.nof_prb_ul_grid.offset,
                                     P.pusch_numerology.offset, P.nof_rx_ports.offset, C.sizeof(S), S.sequence_length.offset,
                                     S.nof_symbols.offset, S.window_samples.offset]
    assert abi.PRACH_FORMATS == model.FORMATS


def test_prach_demod_symbols_are_declared_and_exported():
    names = ["nrphy_prach_demod_validate", "nrphy_prach_demod_sizes", "nrphy_prach_demod_plan_create",
             "nrphy_prach_demod_plan_destroy", "nrphy_prach_demod_run", "nrphy_prach_demodulate_host"]
    header = open(os.path.join(backends.ROOT, "include", "mi355_nrphy.h")).read()
    handle = lib.load()
    for name in names:
        assert name in abi.ABI_SYMBOLS and name + "(" in header
        assert getattr(handle, name) is not None
    assert sorted(n for n in abi.ABI_SYMBOLS if "prach_demod" in n) == sorted(names)


@pytest.mark.parametrize("name,cfg,want", [
    ("format 0", make_cfg(), abi.OK),
    ("format 0, 8 fd occasions up to the grid's edge", make_cfg(nfd=8, rb=31), abi.OK),
    ("format 3 at 30 kHz", make_cfg(61440000, "3", nprb=106, mu=1), abi.OK),
    ("format 0 at 60 kHz", make_cfg(61440000, "0", nprb=60, mu=2, nfd=1), abi.OK),
    ("7 two-symbol occasions", make_cfg(format="A1/B1", ntd=7, nprb=106), abi.OK),
    ("B4 from symbol 2", make_cfg(format="B4", start=2, nprb=106), abi.OK),
    ("A1 at 5.76 MHz", make_cfg(5760000, "A1", ntd=2, nfd=1, start=6, rb=9, nprb=25), abi.OK),
    ("4 ports, 275 PRB at 92.16 MHz", make_cfg(92160000, "B4", nfd=4, start=2, rb=110, nprb=275, ports=4), abi.OK),
    ("C2 at 120 kHz", make_cfg(61440000, "C2", ntd=2, nfd=1, start=1, rb=5, nprb=40, mu=3), abi.OK),
    ("unknown format", make_cfg(format=14), abi.ERR_ARGUMENT),
    ("unknown numerology", make_cfg(mu=4), abi.ERR_ARGUMENT),
    ("no td occasion", make_cfg(ntd=0), abi.ERR_ARGUMENT),
    ("two td occasions on a long format", make_cfg(ntd=2), abi.ERR_ARGUMENT),
    ("no td occasion on a short format", make_cfg(format="A1", ntd=0, nprb=106), abi.ERR_ARGUMENT),
    ("8 two-symbol occasions", make_cfg(format="A1", ntd=8, nprb=106), abi.ERR_ARGUMENT),
    ("an occasion past the slot", make_cfg(format="A1", start=13, nprb=106), abi.ERR_ARGUMENT),
    ("B4 from symbol 3", make_cfg(format="B4", start=3, nprb=106), abi.ERR_ARGUMENT),
    ("td occasions that wrap", make_cfg(format="A1", ntd=0x80000000, nprb=106), abi.ERR_ARGUMENT),
    ("start symbol 14", make_cfg(start=14), abi.ERR_ARGUMENT),
    ("no fd occasion", make_cfg(nfd=0), abi.ERR_ARGUMENT),
    ("9 fd occasions", make_cfg(nfd=9), abi.ERR_ARGUMENT),
    ("reserved row: 1.25 kHz with 120 kHz", make_cfg(61440000, "0", nprb=4, mu=3, nfd=1), abi.ERR_ARGUMENT),
    ("reserved row: 5 kHz with 120 kHz", make_cfg(61440000, "3", nprb=20, mu=3, nfd=1), abi.ERR_ARGUMENT),
    ("a rate that is no multiple of the spacing", make_cfg(30720001), abi.ERR_ARGUMENT),
    ("24577 points", make_cfg(30721250), abi.ERR_ARGUMENT),
    ("8192 points", make_cfg(122880000, "A1", nprb=106), abi.ERR_ARGUMENT),
    ("64 points", make_cfg(7680000, "A1", nprb=20, mu=3, nfd=1), abi.ERR_ARGUMENT),
    ("no sampling rate", make_cfg(0), abi.ERR_ARGUMENT),
    ("12288 points below a grid of 15264", make_cfg(15360000, nprb=106), abi.ERR_ARGUMENT),
    ("1536 points on a grid of 1536", make_cfg(23040000, "A1", nprb=128), abi.ERR_ARGUMENT),
    ("the last fd occasion leaves the grid", make_cfg(nfd=8, rb=32), abi.ERR_ARGUMENT),
    ("the only fd occasion leaves the grid", make_cfg(nfd=1, rb=74), abi.ERR_ARGUMENT),
    ("RB offset 275", make_cfg(92160000, "B4", nfd=1, rb=275, nprb=275), abi.ERR_ARGUMENT),
    ("a prefix of 40.5 samples", make_cfg(5760000, "B1", ntd=2, nfd=1, start=6, rb=9, nprb=25), abi.ERR_ARGUMENT),
    ("a prefix of 40.5 samples at 120 kHz", make_cfg(46080000, "B1", nfd=1, start=2, rb=2, nprb=20, mu=3), abi.ERR_ARGUMENT),
    ("the same with A1", make_cfg(46080000, "A1", nfd=1, start=2, rb=2, nprb=20, mu=3), abi.OK),
    ("no port", make_cfg(ports=0), abi.ERR_ARGUMENT),
    ("5 ports", make_cfg(ports=5), abi.ERR_ARGUMENT),
    ("no PRB", make_cfg(nprb=0), abi.ERR_ARGUMENT),
    ("276 PRB", make_cfg(92160000, "B4", nfd=1, nprb=276), abi.ERR_ARGUMENT),
])
def test_prach_demod_validator(name, cfg, want):
    assert lib.prach_demod_validate(to_abi(cfg)) == want, name
    assert (lib.prach_demod_sizes(to_abi(cfg)) is not None) == (want == abi.OK), name
    assert model.validate(cfg) == (want == abi.OK), name


def test_prach_demod_validator_takes_null():
    handle = lib.load()
    assert handle.nrphy_prach_demod_validate(None) == abi.ERR_ARGUMENT
    assert handle.nrphy_prach_demod_sizes(C.byref(to_abi(make_cfg())), None) == abi.ERR_ARGUMENT


def sizes_tuple(cfg):
    s = lib.prach_demod_sizes(to_abi(cfg))
    return None if s is None else (s.dft_size, s.sequence_length, s.nof_symbols, s.window_samples)


def test_prach_demod_validator_and_sizes_over_the_reference_configurations():
    fixtures = configs_fixture()
    assert len(fixtures) == 112
    for f in fixtures:
        cfg = fixture_cfg(f)
        assert lib.prach_demod_validate(to_abi(cfg)) == abi.OK, f
        assert sizes_tuple(cfg) == model.sizes(cfg), f
    # what the header leaves out, and an input no shorter than the reference's window
    for cfg, n_in, _ in recording():
        assert sizes_tuple(cfg) == model.sizes(cfg), cfg
        assert model.sizes(cfg)[3] <= n_in, cfg
    assert [c for c, _, _ in recording()[:112]] == [fixture_cfg(f) for f in fixtures]


def test_prach_demod_validator_equals_the_restatement_on_a_seeded_sweep():
    """4000 configurations around the accepted ones: each starts from a recorded case and has up to three fields redrawn."""
    rng = np.random.default_rng(7)
    base = [c for c, _, _ in recording()]
    draw = dict(srate_hz=lambda: int(rng.choice([1920000, 5760000, 7680000, 11520000, 15360000, 23040000, 30720000, 46080000, 61440000,
                                                 69120000, 92160000, 122880000, 30721250, 245760000])),
                format=lambda: int(rng.integers(0, 15)), nof_td_occasions=lambda: int(rng.integers(0, 9)),
                nof_fd_occasions=lambda: int(rng.integers(0, 10)), start_symbol=lambda: int(rng.integers(0, 15)),
                rb_offset=lambda: int(rng.integers(0, 280)), nof_prb_ul_grid=lambda: int(rng.integers(0, 278)),
                pusch_numerology=lambda: int(rng.integers(0, 5)), nof_rx_ports=lambda: int(rng.integers(0, 6)))
    accepted = 0
    for _ in range(4000):
        cfg = dict(base[int(rng.integers(0, len(base)))])
        for key in rng.choice(list(draw), int(rng.integers(0, 4)), replace=False):
            cfg[key] = draw[key]()
        named = dict(cfg, format=model.FORMATS[cfg["format"]] if isinstance(cfg["format"], int) and cfg["format"] < 14 else cfg["format"])
        want = model.sizes(named)
        assert sizes_tuple(cfg) == want, cfg
        assert lib.prach_demod_validate(to_abi(cfg)) == (abi.OK if want is not None else abi.ERR_ARGUMENT), cfg
        accepted += want is not None
    assert 800 < accepted < 3200, accepted


def test_generated_tables_equal_the_fixture_and_the_restatement():
    spec = importlib.util.spec_from_file_location("gen_prach_demod_tables", os.path.join(backends.ROOT, "profiles", "gen_prach_demod_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.render() == open(os.path.join(backends.PKG_DIR, "csrc", "prach_demod_tables.inc")).read()
    tables = json.load(open(os.path.join(GOLDEN, "prach_demod_tables.json")))
    hz = [15000, 30000, 60000, 120000, 1250, 5000]
    assert len(tables["preamble"]) == 4 + 10 * 4 * 2
    for r in tables["preamble"]:
        i = model.preamble_info(r["format"], r["mu"], bool(r["last"]))
        assert (i["L"], i["ra_scs_hz"], i["nof_symbols"], i["cp_kappa"], i["symbols_kappa"], i["duration"]) == \
            (r["sequence_length"], hz[r["ra_scs"]], r["nof_symbols"], r["cp_kappa"], r["symbols_kappa"], r["duration"]), r
    assert len(tables["window"]) == 1332
    for fmt, mu, start, ntd, kappa in tables["window"]:
        assert model.window_kappa(fmt, mu, start, ntd) == kappa, (fmt, mu, start, ntd)
    assert len(tables["mapping"]) == 24
    for ra, mu, nof_rb_ra, k_bar in tables["mapping"]:
        assert model.MAPPING.get((hz[ra], mu), (0, 0)) == (nof_rb_ra, k_bar), (ra, mu)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_prach_demod_extractor_reproduces_the_committed_fixture():
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([os.environ.get("PYTHON", "python3"), os.path.join(GOLDEN, "extract_prach_demod_configs.py"), REFERENCE, d],
                       check=True, timeout=120)
        assert open(os.path.join(d, "prach_demod_configs.json")).read() == open(os.path.join(GOLDEN, "prach_demod_configs.json")).read()


def test_recorded_inputs_are_the_stated_sequence():
    """The vectorised generator against the recurrence written out, and exact in float32."""
    x, want = ((5 + 1) * 0x9E3779B97F4A7C15) & model.MASK, []
    for _ in range(64):
        x = (x * model.LCG_A + model.LCG_C) & model.MASK
        want.append(((x >> 40) - (1 << 23)) / float(1 << 23))
    got = model.lcg_values(5, 64)
    assert got.dtype == np.float32 and [float(v) for v in got] == want
    s = model.lcg_samples(5, 32)
    assert s.dtype == np.complex64 and [float(v) for v in s.real] == want[0::2] and [float(v) for v in s.imag] == want[1::2]


def test_restatement_equals_the_reference_on_every_recorded_case():
    """The float64 restatement against ofdm_prach_demodulator_impl with dft_processor_generic_impl, on all 138 cases: the 112 of
    the unit test's header and 26 more (sequences across and above the grid centre, 1 to 8 fd occasions, every transform size,
    every spacing, occasions across 0.5 ms, mixed formats).  Largest distance measured: 7.9e-7."""
    cases = recording()
    assert len(cases) == 138
    sizes = {model.derive(c)["dft_size"] for c, _, _ in cases}
    assert sizes == set(model.DFT_SIZES) - {128}
    assert {c["nof_fd_occasions"] for c, _, _ in cases} >= {1, 4, 8} and {c["pusch_numerology"] for c, _, _ in cases} == {0, 1, 2, 3}
    assert {c["format"] for c, _, _ in cases} == set(model.FORMATS)
    worst = 0.0
    for (cfg, _, ref), (_, got) in zip(cases, restated()):
        d = distance(ref, got)
        worst = max(worst, d)
        assert d <= TOL, (cfg, d)
    print("reference - float64 restatement: worst distance %.3g over %d cases" % (worst, len(cases)))


# =======================================================================================================================
# GPU
# =======================================================================================================================
def buffer_strides(shape):
    """Element strides (port, fd, td, symbol) of a C-contiguous [ports][td][fd][symbols][row] buffer."""
    _, ntd, nfd, nsym, row = shape
    return dict(port_stride=ntd * nfd * nsym * row, fd_stride=nsym * row, td_stride=nfd * nsym * row, symbol_stride=row)


def run_items(ctx, items, one_plan=False, stream=None, state=None):
    """items: [(cfg, samples [ports][n])] -> the device's [ports][td][fd][symbols][L_RA] of every item, with the items back to back
    in one input and one output buffer.  The strides belong to a plan, so items share a plan where their input rows and buffers have
    one shape; one_plan gives every item the largest row and buffer of the batch.  state: (plans, d_in, d_out) of an earlier call to
    run again; returns (outputs, state)."""
    import torch
    shapes = []
    for cfg, x in items:
        d = model.derive(cfg)
        shapes.append((cfg["nof_rx_ports"], cfg["nof_td_occasions"], cfg["nof_fd_occasions"], d["nof_symbols"], d["L"]))
    rows = [x.shape[1] for _, x in items]
    alloc = list(shapes)
    if one_plan:
        alloc = [tuple(max(s[k] for s in shapes) for k in range(5))] * len(items)
        rows = [max(rows)] * len(items)
    in_off = np.concatenate([[0], np.cumsum([a[0] * r for a, r in zip(alloc, rows)])]).astype(int)
    out_off = np.concatenate([[0], np.cumsum([int(np.prod(a)) for a in alloc])]).astype(int)
    if state is None:
        flat = np.zeros(in_off[-1], np.complex64)
        for i, (cfg, x) in enumerate(items):
            for p in range(x.shape[0]):
                flat[in_off[i] + p * rows[i]:in_off[i] + p * rows[i] + x.shape[1]] = x[p]
        groups = {}
        for i in range(len(items)):
            groups.setdefault((rows[i], alloc[i][1:]), []).append(i)
        plans = [lib.PrachDemodPlan(ctx, [to_abi(items[i][0]) for i in idx], [int(in_off[i]) for i in idx], key[0],
                                    [int(out_off[i]) for i in idx], **buffer_strides((0,) + key[1])) for key, idx in groups.items()]
        assert not one_plan or len(plans) == 1
        state = (plans, dev(flat.view(np.float32)), torch.zeros(2 * int(out_off[-1]), dtype=torch.float32, device="cuda"))
    plans, d_in, d_out = state
    for p in plans:
        p.run(d_in, d_out, stream=stream)
    ctx.synchronize() if stream is None else torch.cuda.synchronize()
    host = d_out.cpu().numpy().view(np.complex64)
    outs = []
    for i, s in enumerate(shapes):
        whole = host[out_off[i]:out_off[i + 1]].reshape(alloc[i])
        outs.append(np.ascontiguousarray(whole[:s[0], :s[1], :s[2], :s[3], :s[4]]))
    return outs, state


def close(state):
    for p in state[0]:
        p.close()


@pytest.mark.gpu
def test_every_recorded_case_on_the_device(gpu_ctx):
    """One port, the recorded occasions; against the reference's answers and the float64 restatement, both within 1e-5.
    Measured on MI355X: 8.7e-7 from the reference, 4.4e-7 from the restatement (the reference itself: 7.9e-7 from the restatement)."""
    cases, models = recording(), restated()
    items = [(cfg, x[None, :]) for (cfg, _, _), (x, _) in zip(cases, models)]
    worst_ref, worst_model = 0.0, 0.0
    for first in range(0, len(items), 46):
        outs, state = run_items(gpu_ctx, items[first:first + 46])
        close(state)
        for k, got in enumerate(outs):
            cfg, _, ref = cases[first + k]
            d_ref, d_model = distance(got[0], ref), distance(got[0], models[first + k][1])
            print("case %3d %s: device - reference %.3g, device - restatement %.3g" % (first + k, cfg, d_ref, d_model))
            worst_ref, worst_model = max(worst_ref, d_ref), max(worst_model, d_model)
    print("device - reference worst %.3g, device - float64 restatement worst %.3g" % (worst_ref, worst_model))
    assert worst_ref <= TOL and worst_model <= TOL


def sentinel_case(ctx, cfg, seed):
    """An oversized buffer [ports + 1][td + 1][fd + 1][symbols + 1][L_RA + 5] between guards, inputs at an offset with a port
    stride above the window: the item's elements equal the restatement, every other element is the sentinel."""
    import torch
    d = model.derive(cfg)
    P, ntd, nfd, nsym, L = cfg["nof_rx_ports"], cfg["nof_td_occasions"], cfg["nof_fd_occasions"], d["nof_symbols"], d["L"]
    rng = np.random.default_rng(seed)
    in_off, in_stride = 7, d["window_samples"] + 13
    flat = np.zeros(in_off + P * in_stride, np.complex64)
    x = (rng.uniform(-1, 1, (P, d["window_samples"])) + 1j * rng.uniform(-1, 1, (P, d["window_samples"]))).astype(np.complex64)
    for p in range(P):
        flat[in_off + p * in_stride:in_off + p * in_stride + d["window_samples"]] = x[p]
    shape = (P + 1, ntd + 1, nfd + 1, nsym + 1, L + 5)
    whole = torch.from_numpy(np.full(GUARD + int(np.prod(shape)) + GUARD, SENTINEL, np.complex64).view(np.float32)).cuda()
    plan = lib.PrachDemodPlan(ctx, [to_abi(cfg)], [in_off], in_stride, [GUARD], **buffer_strides(shape))
    plan.run(dev(flat.view(np.float32)), whole)
    ctx.synchronize()
    plan.close()
    host = whole.cpu().numpy().view(np.complex64)
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all()
    body = host[GUARD:-GUARD].reshape(shape)
    written = np.zeros(shape, bool)
    written[:P, :ntd, :nfd, :nsym, :L] = True
    assert (body[~written] == SENTINEL).all()
    assert not (body[written] == SENTINEL).any()
    for p in range(P):
        want = model.demodulate(cfg, x[p])
        dist = distance(body[p, :ntd, :nfd, :nsym, :L], want)
        print("%s port %d: device - restatement %.3g" % (cfg, p, dist))
        assert dist <= TOL, (cfg, p, dist)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [
    make_cfg(format="A1/B1", ntd=2, nfd=2, start=5, rb=46, nprb=106, ports=2),           # one LDS transform, across 0.5 ms and the centre
    make_cfg(format="0", nfd=2, rb=33, nprb=79, ports=2),                                # 6 x 4096, the second occasion across the centre
    make_cfg(46080000, "3", nfd=3, rb=2, nprb=51, mu=1, ports=3),                        # 3 x 3072, four symbols
    make_cfg(61440000, "0", nfd=1, rb=75, nprb=160, mu=1, ports=1),                      # 12 x 4096
], ids=["A1/B1", "format 0", "format 3", "49152"])
def test_nothing_outside_the_items_elements_is_written(gpu_ctx, cfg):
    sentinel_case(gpu_ctx, cfg, 3)


def mixed_items(rng):
    cfgs = [make_cfg(format="0", nfd=2, rb=10, nprb=79, ports=4),
            make_cfg(61440000, "A1/B1", ntd=3, nfd=2, start=2, rb=20, nprb=106, mu=1, ports=1),
            make_cfg(format="B4", nfd=1, rb=50, nprb=106, ports=4),
            make_cfg(61440000, "3", nfd=2, rb=0, nprb=106, mu=1, ports=2),
            make_cfg(7680000, "0", nfd=1, rb=12, nprb=25, ports=1)]
    items = []
    for cfg in cfgs:
        n = model.derive(cfg)["window_samples"]
        items.append((cfg, (rng.uniform(-1, 1, (cfg["nof_rx_ports"], n)) + 1j * rng.uniform(-1, 1, (cfg["nof_rx_ports"], n))).astype(np.complex64)))
    return items


@pytest.mark.gpu
def test_mixed_batch_equals_host_calls_twice_and_in_a_graph(gpu_ctx):
    """Long and short formats, several td occasions, 1 to 4 ports, three sampling rates in one set of plans: item by item the bytes
    of nrphy_prach_demodulate_host; a second run and a graph replay give the same bytes."""
    import torch
    items = mixed_items(np.random.default_rng(5))
    first, state = run_items(gpu_ctx, items, one_plan=True)
    for (cfg, x), got in zip(items, first):
        single = gpu_ctx.prach_demodulate_host(to_abi(cfg), x)
        assert single.shape == got.shape and single.tobytes() == got.tobytes(), cfg
        assert distance(got[-1], model.demodulate(cfg, x[-1])) <= TOL, cfg
    plans, d_in, d_out = state
    untouched = d_out.cpu().numpy().copy()
    d_out.zero_()
    second, _ = run_items(gpu_ctx, items, one_plan=True, state=state)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            plans[0].run(d_in, d_out, stream=C.c_void_p(stream.cuda_stream))
    d_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == untouched.tobytes()  # the buffer started as zeros: the elements no item owns still are
    close(state)


def samples_to_detections(ctx, demod_cfg, det_cfg, preamble, td_with_preamble, delay, seed):
    """The generator's sequence on the subcarriers of (td_with_preamble, fd 0), delayed by `delay` samples, a phase per port and a
    little noise; nrphy_prach_demod_run then nrphy_prach_run on one stream with nothing between.  Returns, per (td, fd) occasion, the
    result header and the 64 preamble slots."""
    import torch
    d = model.derive(demod_cfg)
    P, ntd, nfd = demod_cfg["nof_rx_ports"], demod_cfg["nof_td_occasions"], demod_cfg["nof_fd_occasions"]
    rng = np.random.default_rng(seed)
    sequence = ctx.prach_generate_host(abi.make_prach(**det_cfg), preamble)
    start, occasion = model.modulate(demod_cfg, td_with_preamble, 0, sequence, delay)
    n = d["window_samples"]
    sigma = 0.05 * np.sqrt(np.mean(np.abs(occasion) ** 2))
    x = sigma * (rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n)))
    for p in range(P):
        x[p, start:start + len(occasion)] += occasion * np.exp(1j * 0.7 * p)
    shape = (P, ntd, nfd, d["nof_symbols"], d["L"])
    st = buffer_strides(shape)
    demod = lib.PrachDemodPlan(ctx, [to_abi(demod_cfg)], [0], n, [0], **st)
    occasions = [(td, fd) for td in range(ntd) for fd in range(nfd)]
    detect = lib.PrachPlan(ctx, [abi.make_prach(**det_cfg)] * len(occasions), [td * st["td_stride"] + fd * st["fd_stride"] for td, fd in occasions],
                           st["port_stride"], st["symbol_stride"])
    d_x = dev(x.astype(np.complex64).view(np.float32))
    d_buf = torch.zeros(2 * int(np.prod(shape)), dtype=torch.float32, device="cuda")
    d_res = torch.zeros(len(occasions) * RESULT_DTYPE.itemsize // 4, dtype=torch.int32, device="cuda")
    d_pre = torch.zeros(len(occasions) * 64 * PREAMBLE_DTYPE.itemsize // 4, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = C.c_void_p(stream.cuda_stream)
    demod.run(d_x, d_buf, stream=sp)
    detect.run(d_buf, d_res, d_pre, None, stream=sp)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(RESULT_DTYPE)
    pre = d_pre.cpu().numpy().view(PREAMBLE_DTYPE).reshape(len(occasions), 64)
    demod.close()
    detect.close()
    return {occ: (res[i], pre[i]) for i, occ in enumerate(occasions)}


@pytest.mark.gpu
@pytest.mark.parametrize("name,demod_cfg,det_cfg,preamble,td,delay", [
    # format 0 at 30.72 MHz: 24 samples per correlation sample; N_CS = 26, preamble 32 is the second root at shift 0
    ("format 0", make_cfg(format="0", nfd=1, rb=12, nprb=79, ports=2),
     dict(format="0", ra_scs="1.25", root_sequence_index=40, zero_correlation_zone=5, start_preamble_index=0,
          nof_preamble_indices=64, nof_rx_ports=2), 32, 0, 240),
    # B4 at 30 kHz and 61.44 MHz: 8 samples per correlation sample; N_CS = 23, preamble 12 is the third root at shift 0
    ("B4", make_cfg(61440000, "B4", nfd=1, start=2, rb=30, nprb=106, mu=1, ports=1),
     dict(format="B4", ra_scs="30", root_sequence_index=9, zero_correlation_zone=11, start_preamble_index=0, nof_preamble_indices=64,
          nof_rx_ports=1), 12, 0, 40),
    # A1 at 15 kHz with two td occasions: the preamble is in the second only
    ("A1", make_cfg(format="A1", ntd=2, nfd=1, start=4, rb=3, nprb=106, ports=1),
     dict(format="A1", ra_scs="15", root_sequence_index=77, zero_correlation_zone=11, start_preamble_index=0, nof_preamble_indices=64,
          nof_rx_ports=1), 6, 1, 24),
])
def test_samples_to_detections_on_one_stream(gpu_ctx, name, demod_cfg, det_cfg, preamble, td, delay):
    out = samples_to_detections(gpu_ctx, demod_cfg, det_cfg, preamble, td, delay, 17)
    for (i_td, i_fd), (res, pre) in out.items():
        found = [int(i) for i in np.nonzero(pre["detected"])[0]]
        if i_td != td:
            assert found == [] and int(res["nof_detected"]) == 0, (name, i_td, found)
            continue
        assert found == [preamble] and int(res["nof_detected"]) == 1, (name, i_td, found)
        ta, resolution = float(pre[preamble]["time_advance_s"]), float(res["time_resolution_s"])
        print("%s: time advance %.4g s for a delay of %.4g s (resolution %.4g s)" % (name, ta, delay / demod_cfg["srate_hz"], resolution))
        assert abs(ta - delay / demod_cfg["srate_hz"]) <= resolution, (name, ta, delay / demod_cfg["srate_hz"], resolution)


@pytest.mark.gpu
def test_zero_input_gives_zero_output_and_refused_plans_stay_null(gpu_ctx):
    for cfg in (make_cfg(format="0", nfd=2, ports=2), make_cfg(format="C2", ntd=2, nfd=2, nprb=106, ports=1)):
        d = model.derive(cfg)
        before = np.full((cfg["nof_rx_ports"], cfg["nof_td_occasions"], 2, d["nof_symbols"], d["L"]), SENTINEL, np.complex64)
        out = gpu_ctx.prach_demodulate_host(to_abi(cfg), np.zeros((cfg["nof_rx_ports"], d["window_samples"]), np.complex64), symbols=before)
        assert out.shape == before.shape and not out.view(np.uint32).any()
    good, bad = to_abi(make_cfg()), to_abi(make_cfg(nfd=9))
    zero = (C.c_uint64 * 2)(0, 0)
    handle = C.c_void_p(0x1234)
    rc = gpu_ctx.lib.nrphy_prach_demod_plan_create(gpu_ctx.handle, 2, (abi.PrachDemodCfg * 2)(good, bad), zero, 1 << 20, zero, 1 << 20, 839,
                                                   1 << 16, 1 << 12, C.byref(handle))
    assert rc == abi.ERR_ARGUMENT and not handle.value
    handle = C.c_void_p(0x1234)
    rc = gpu_ctx.lib.nrphy_prach_demod_plan_create(gpu_ctx.handle, 0, (abi.PrachDemodCfg * 2)(good, bad), zero, 1 << 20, zero, 1 << 20, 839,
                                                   1 << 16, 1 << 12, C.byref(handle))
    assert rc == abi.ERR_ARGUMENT and not handle.value
    assert gpu_ctx.lib.nrphy_prach_demod_run(None, None, None, None) == abi.ERR_ARGUMENT
    assert gpu_ctx.lib.nrphy_prach_demod_plan_destroy(None) == abi.OK
