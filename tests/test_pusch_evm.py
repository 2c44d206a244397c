"""PUSCH EVM and the EVM-based SINR: nrphy_pusch_demod_run_evm / nrphy_pusch_demodulate_host_evm, nrphy_pusch_evm_* and
nrphy_pusch_evm_slot.

The recording (tests/golden/pusch_evm_reference_*, written by tests/golden/record_pusch_evm_reference.cpp) holds what the
reference's pusch_demodulator_impl reports when it is constructed with evm_calculator_generic_impl over
modulation_mapper_lut_impl: per case the inputs, the equalised (deprecoded) symbols, the soft bits before descrambling, every
provisional stats.evm and the final one, and the mapper's tables.

CPU: the ABI's additions and the POD; the validator; tests/pusch_evm_model.py, the NumPy restatement of the reference's
arithmetic, against every recorded value bit for bit.
GPU: the fused kernel's EVM on every recorded case against the recording, within the derived allowance of the model's
docstring (transform-precoded cases with the additional 2 d of the deprecoder's bound), and against the model run on the
device's own stand-alone equaliser, deprecoder and demapper; one plan with four of the cases; the processor and the slot pool.

Largest deviations observed (MI355X), relative to the recorded EVM:
  fused kernel against the recording, plain cases        1.5e-07 (allowed 3.9e-06 .. 1.9e-05)
  fused kernel against the recording, transform precoded 2.7e-07 (allowed, with the 2 d, 9.2e-06 .. 8.4e-05)
  fused kernel against the model on the stand-alone path 1.5e-07 (0 on every transform-precoded case)
"""
import ctypes as C
import functools
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import backends
import pusch_evm_model as model
import pusch_tp_model as tp_model
import test_pusch_processor as proc
from pusch_chest_model import as_i32, dev, gold, to_cbf16
from test_pusch_transform_precoding import dft_bounds

abi = backends.abi
lib = backends.pkg.lib

GOLDEN = os.path.join(backends.ROOT, "tests", "golden")
BOTH = abi.PUSCH_DEMOD_TRANSFORM_PRECODING | abi.PUSCH_DEMOD_PI2_BPSK
MIXED = (0, 1, 2, 6)               # the cases of the plan that holds several: 1, 2, 3a and 5a of the issue's list
MIX_PORTS, MIX_SUBC = 4, 12 * 52
f32 = np.float32


def bits_to_f32(u):
    return np.array(u, np.uint32).view(np.float32)


class Recorded:
    """One case: its configuration, its inputs laid out as the library reads them, and per OFDM symbol with data the equaliser's
    output, the symbols the EVM calculator saw and the soft bits before descrambling."""

    def __init__(self, row, blobs, nports=None, nsubc=None):
        self.row = row
        self.cfg = abi.make_pusch_demod(prbs=row["prbs"], qm=row["qm"], rnti=row["rnti"], n_id=row["n_id"],
                                        start_symbol=row["start_symbol_index"], nof_symbols=row["nof_symbols"],
                                        dmrs_symbols=row["dmrs_symbols"], dmrs_type=row["dmrs_type"],
                                        nof_cdm_groups_without_data=row["nof_cdm_groups_without_data"],
                                        nof_layers=row["nof_tx_layers"], rx_ports=row["rx_ports"], equalizer=row["equalizer"],
                                        transform_precoding=row["transform_precoding"])
        self.tp = bool(row["transform_precoding"])
        self.qm = row["qm"]
        self.nports = nports or max(row["rx_ports"]) + 1
        self.nsubc = nsubc or 12 * (max(row["prbs"]) + 1)
        P, L, nsym, nsc = len(row["rx_ports"]), row["nof_tx_layers"], row["nof_symbols"], 12 * len(row["prbs"])
        subc = np.array([12 * p + k for p in row["prbs"] for k in range(12)])
        syms = np.arange(row["start_symbol_index"], row["start_symbol_index"] + nsym)
        g = blobs["grids"][row["grid_off"]: row["grid_off"] + P * nsym * nsc].reshape(P, nsym, nsc)
        c = blobs["ce"][row["ce_off"]: row["ce_off"] + L * P * nsc].reshape(L, P, nsc)
        self.grid = np.zeros((self.nports, 14, self.nsubc), np.uint32)
        self.ce = np.zeros((L, P, 14, self.nsubc), np.uint32)
        for i, port in enumerate(row["rx_ports"]):
            self.grid[port][np.ix_(syms, subc)] = g[i]
        self.ce[:, :, syms[:, None], subc[None, :]] = c[:, :, None, :]
        self.noise_vars = np.zeros(abi.MAX_PORTS, np.float32)
        self.noise_vars[:P] = row["noise_vars"]
        self.llr = blobs["llr"][row["llr_off"]: row["llr_off"] + row["nof_bits"]]
        self.soft_all = blobs["soft"][row["llr_off"]: row["llr_off"] + row["nof_bits"]]
        self.evm = bits_to_f32(row["evm_bits"])[()]
        self.provisional = bits_to_f32(row["provisional_evm_bits"])
        self.eq, self.x, self.soft = [], [], []
        at, zat, bat = row["eq_off"], row["z_off"], 0
        for l in range(14):
            n = tp_model.data_subcarriers(self.cfg, l).size * L
            if n == 0:
                continue
            self.eq.append(blobs["eq"][at: at + n])
            self.x.append(blobs["z"][zat: zat + n] if self.tp else self.eq[-1])
            self.soft.append(self.soft_all[bat: bat + n * self.qm])
            at, zat, bat = at + n, zat + n, bat + n * self.qm
        assert bat == row["nof_bits"]
        self.n_max = max(x.size for x in self.x)

    def two_d(self):
        """2 d of a transform-precoded case (0 otherwise): d = 4 x the size's bound x the RMS of a symbol's equalised input, as
        tests/test_pusch_transform_precoding.py defines it; the largest over the symbols."""
        if not self.tp:
            return 0.0
        bound = dft_bounds()[len(self.row["prbs"])]
        return 2 * max(float(f32(4 * bound * np.sqrt(np.mean(np.abs(eq.astype(np.complex128)) ** 2)))) for eq in self.eq)


@functools.lru_cache(maxsize=None)
def recording():
    load = lambda name: np.load(os.path.join(GOLDEN, "pusch_evm_reference_%s.npy" % name))
    blobs = {k: load(k) for k in ("grids", "ce", "llr", "soft")}
    for k in ("eq", "z", "tables"):
        blobs[k] = load(k).view(np.complex64).reshape(-1)
    rows = json.load(open(os.path.join(GOLDEN, "pusch_evm_reference_cases.json")))
    return rows, blobs


@functools.lru_cache(maxsize=None)
def cases():
    rows, blobs = recording()
    return [Recorded(r, blobs) for r in rows]


def tables():
    return recording()[1]["tables"]


# =======================================================================================================================
# CPU
# =======================================================================================================================
NEW_SYMBOLS = ["nrphy_pusch_demod_run_evm", "nrphy_pusch_demodulate_host_evm", "nrphy_pusch_evm_validate",
               "nrphy_pusch_evm_plan_create", "nrphy_pusch_evm_host", "nrphy_pusch_evm_slot"]
PINNED_SUBSTRINGS = ["_pusch_proc_", "_pusch_csi2_", "_ul_slot", "_uci_", "_ulsch_", "pucch", "_srs_", "_pf2_", "prach_demod",
                     "prach_window", "_ofh_"]


def test_abi_additions_and_the_pod():
    assert set(abi.ABI_SYMBOLS) >= set(NEW_SYMBOLS)
    handle = lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name
        assert not [s for s in PINNED_SUBSTRINGS if s in name], name  # the counts other tests pin stay what they are
    protos = r'''#include "mi355_nrphy.h"
int (*a)(nrphy_pusch_demod_plan_t*, const void*, const void*, const float*, int8_t*, uint64_t, float*, float*, void*) =
    nrphy_pusch_demod_run_evm;
int (*b)(nrphy_ctx_t*, const nrphy_pusch_demod_cfg_t*, const void*, uint32_t, uint32_t, const void*, const float*, uint32_t, int8_t*,
         float*, float*) = nrphy_pusch_demodulate_host_evm;
int (*c)(const nrphy_pusch_pdu_t*, const nrphy_pusch_evm_options_t*, uint32_t, uint32_t) = nrphy_pusch_evm_validate;
int (*d)(nrphy_ctx_t*, uint32_t, const nrphy_pusch_pdu_t*, const nrphy_pusch_evm_options_t*, const uint32_t*, uint32_t, uint32_t,
         uint32_t, const uint64_t*, const uint64_t*, const uint64_t*, const uint64_t*, nrphy_pusch_proc_plan_t**) =
    nrphy_pusch_evm_plan_create;
int (*e)(nrphy_ctx_t*, const nrphy_pusch_pdu_t*, const nrphy_pusch_evm_options_t*, const void*, uint32_t, uint32_t, int8_t*, uint8_t*,
         uint8_t*, uint8_t*, nrphy_pusch_result_t*) = nrphy_pusch_evm_host;
int (*f)(nrphy_ul_slots_t*, uint32_t, uint32_t, const nrphy_pusch_pdu_t*, const nrphy_pusch_evm_options_t*, const uint64_t*,
         const uint64_t*) = nrphy_pusch_evm_slot;
'''
    sizes = r'''#include "mi355_nrphy.h"
#include <stdio.h>
#include <stddef.h>
int main(void){printf("%zu %zu %zu %zu %zu %zu\n", sizeof(nrphy_pusch_evm_options_t), offsetof(nrphy_pusch_evm_options_t, proc),
 offsetof(nrphy_pusch_evm_options_t, enable_evm), offsetof(nrphy_pusch_evm_options_t, reserved_), sizeof(nrphy_pusch_result_t),
 sizeof(nrphy_pusch_proc_options_t)); return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        include = ["-I", os.path.join(backends.ROOT, "include")]
        open(os.path.join(d, "p.c"), "w").write(protos)  # compiled, not linked: the prototypes are the ones stated here
        subprocess.run(["gcc", "-Werror", "-c", os.path.join(d, "p.c"), "-o", os.path.join(d, "p.o")] + include, check=True, timeout=120)
        open(os.path.join(d, "t.c"), "w").write(sizes)
        subprocess.run(["gcc", os.path.join(d, "t.c"), "-o", os.path.join(d, "t")] + include, check=True, timeout=120)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, timeout=60).stdout.split()]
    E = abi.PuschEvmOptions
    assert out == [C.sizeof(E), E.proc.offset, E.enable_evm.offset, E.reserved_.offset, C.sizeof(abi.PuschResult),
                   C.sizeof(abi.PuschProcOptions)] == [24, 0, 16, 20, 96, 16]
    o = abi.make_pusch_evm_options(csi_sinr_calc_method=abi.PUSCH_SINR_EVM)
    assert (o.enable_evm, o.reserved_, o.proc.csi_sinr_calc_method, o.proc.dec_nof_iterations) == (1, 0, abi.PUSCH_SINR_EVM, 10)


METHODS = (abi.PUSCH_SINR_CHANNEL_ESTIMATOR, abi.PUSCH_SINR_POST_EQUALIZATION, abi.PUSCH_SINR_EVM)


@pytest.mark.parametrize("enable,method,reserved,want", [
    (0, abi.PUSCH_SINR_CHANNEL_ESTIMATOR, 0, True), (0, abi.PUSCH_SINR_POST_EQUALIZATION, 0, True),
    (0, abi.PUSCH_SINR_EVM, 0, False),  # the EVM-based SINR without the EVM
    (1, abi.PUSCH_SINR_CHANNEL_ESTIMATOR, 0, True), (1, abi.PUSCH_SINR_POST_EQUALIZATION, 0, True), (1, abi.PUSCH_SINR_EVM, 0, True),
    (2, abi.PUSCH_SINR_CHANNEL_ESTIMATOR, 0, False), (2, abi.PUSCH_SINR_EVM, 0, False),
    (1, abi.PUSCH_SINR_EVM, 1, False), (0, abi.PUSCH_SINR_CHANNEL_ESTIMATOR, 7, False),
    (1, 3, 0, False),
])
def test_evm_validator(enable, method, reserved, want):
    for name in "abcdef":
        pdu = proc.make_pdus(name)[0]
        o = abi.make_pusch_evm_options(enable_evm=enable, reserved_=reserved, csi_sinr_calc_method=method)
        assert (lib.pusch_evm_validate(pdu, o, proc.NPORTS, proc.NSUBC) == abi.OK) == want, name
    # the calls without the EVM keep their verdicts
    assert (lib.pusch_proc_validate(pdu, o.proc, proc.NPORTS, proc.NSUBC) == abi.OK) == (method != abi.PUSCH_SINR_EVM and method < 3)


def test_evm_validator_without_evm_is_the_processor_validator():
    """Every row of the processor's validator table, through nrphy_pusch_evm_validate with enable_evm = 0."""
    rows = [m for m in proc.test_pusch_proc_validator.pytestmark if m.name == "parametrize"][0].args[1]
    assert len(rows) >= 40
    for name, case, pdu_change, opt_change, want in rows:
        pdu = abi.make_pusch_pdu(**dict(proc.pdu_args()[case], **pdu_change))
        o = abi.PuschEvmOptions(proc._opts(**opt_change), 0, 0)
        assert (lib.pusch_evm_validate(pdu, o, proc.NPORTS, proc.NSUBC) == abi.OK) == want, name
        assert lib.pusch_evm_validate(pdu, o, proc.NPORTS, proc.NSUBC) == lib.pusch_proc_validate(pdu, o.proc, proc.NPORTS, proc.NSUBC)


def test_recording_covers_the_shapes():
    rows, blobs = recording()
    cs = cases()
    assert len(cs) == 14
    assert (rows[0]["qm"], len(rows[0]["prbs"]), rows[0]["nof_symbols"], len(cs[0].x)) == (2, 1, 14, 13)
    assert sorted({x.size for x in cs[1].x}) == [132, 264] and rows[1]["start_symbol_index"] == 2 and rows[1]["nof_symbols"] == 10
    assert [(r["nof_tx_layers"], len(r["rx_ports"]), r["qm"]) for r in rows[2:4]] == [(2, 2, 6), (2, 4, 8)]
    assert rows[2]["prbs"] == [3, 7, 40]
    for k, layers in ((4, 1), (5, 2)):  # the RE without estimate: every soft bit 0, every hard bit 1, and it counts
        r, c = rows[k], cs[k]
        assert r["nof_tx_layers"] == layers and r["zero_subc"] >= 0
        j = [12 * p + i for p in r["prbs"] for i in range(12)].index(r["zero_subc"])
        for soft, x in zip(c.soft, c.x):
            assert (soft.reshape(-1, layers * c.qm)[j] == 0).all() and x.size == 24 * layers
    assert [(r["transform_precoding"], len(r["prbs"]), r["qm"]) for r in rows[6:13]] == [
        (1, 1, 1), (1, 1, 2), (1, 1, 6), (1, 25, 1), (1, 25, 2), (1, 25, 6), (0, 3, 1)]
    assert cs[13].n_max == 4104 and len(cs[13].x) == 1
    for r, c in zip(rows, cs):
        assert lib.pusch_demod_validate_ex(c.cfg, c.nports, c.nsubc, BOTH) == abi.OK
        assert len(c.provisional) == len(c.x) and c.provisional[-1].view(np.uint32) == c.evm.view(np.uint32)
        # the soft bits before descrambling are the codeword with the sequence applied again
        flip = gold(r["rnti"] * 2 ** 15 + r["n_id"], c.llr.size).astype(bool)
        assert np.array_equal(np.where(flip, -c.llr.astype(np.int16), c.llr), c.soft_all)


def test_model_tables_are_the_recorded_ones():
    for qm in (2, 4, 6, 8):
        at = model.TABLE_OFFSET[qm]
        assert np.array_equal(model.formula_table(qm).view(np.uint32), tables()[at: at + (1 << qm)].view(np.uint32)), qm
    assert tables().size == 340


def test_model_gives_every_recorded_value_bit_for_bit():
    for n, c in enumerate(cases()):
        provisional, final = model.evm(c.qm, c.x, c.soft, tables())
        assert np.array_equal(np.array(provisional, f32).view(np.uint32), c.provisional.view(np.uint32)), n
        assert final.view(np.uint32) == c.evm.view(np.uint32), n


# =======================================================================================================================
# GPU: the demodulator
# =======================================================================================================================
def standalone_evm(ctx, c):
    """The model on the device's own nrphy_channel_equalize (-> nrphy_transform_deprecode) -> nrphy_demodulate_soft outputs."""
    cfg = c.cfg
    P = cfg.nof_rx_ports
    ports = [cfg.rx_ports[i] for i in range(P)]
    modulation = 0 if cfg.qm == 1 else cfg.qm
    xs, softs = [], []
    for l in range(14):
        ks = tp_model.data_subcarriers(cfg, l)
        if ks.size == 0:
            continue
        eq, ev = ctx.channel_equalize_host(cfg.equalizer, c.grid[ports][:, l, ks], c.ce[:, :, l, ks], c.noise_vars[:P], 1.0)
        eq, ev = eq.reshape(-1), ev.reshape(-1)
        z = ctx.transform_deprecode_host(ks.size // 12, eq) if cfg.transform_precoding else eq
        xs.append(np.asarray(z, np.complex64))
        softs.append(ctx.demodulate_soft_host(modulation, z, ev))
    return model.evm(c.qm, xs, softs)[1]


@pytest.mark.gpu
def test_host_form_against_the_recording_and_the_standalone_chain(gpu_ctx):
    worst = {"plain": 0.0, "tp": 0.0, "chain": 0.0}
    for n, c in enumerate(cases()):
        nv = c.noise_vars[:c.cfg.nof_rx_ports]
        want_llr, want_sinr = gpu_ctx.pusch_demodulate_host_ex(c.cfg, c.grid, c.ce, nv, BOTH)
        llr, sinr, evm = gpu_ctx.pusch_demodulate_host_evm(c.cfg, c.grid, c.ce, nv, BOTH)
        assert np.array_equal(llr, want_llr), n
        assert f32(sinr).view(np.uint32) == f32(want_sinr).view(np.uint32), n
        dev_rec = abs(float(evm) - float(c.evm))
        tol = model.allowance(c.n_max) * float(c.evm) + c.two_d()
        chain = standalone_evm(gpu_ctx, c)
        dev_chain = abs(float(evm) - float(chain))
        print("case %2d: evm %.9g recorded %.9g (off %.3g relative, allowed %.3g) stand-alone chain %.9g (off %.3g relative)" % (
            n, evm, c.evm, dev_rec / float(c.evm), tol / float(c.evm), chain, dev_chain / float(chain)))
        key = "tp" if c.tp else "plain"
        worst[key] = max(worst[key], dev_rec / float(c.evm))
        worst["chain"] = max(worst["chain"], dev_chain / float(chain))
        assert dev_rec <= tol, (n, evm, c.evm, tol)
        assert dev_chain <= model.allowance(c.n_max) * float(chain), (n, evm, chain)
    print("largest relative deviations:", worst)


def mixed_cases():
    rows, blobs = recording()
    return [Recorded(rows[k], blobs, MIX_PORTS, MIX_SUBC) for k in MIXED]


class MixedRun:
    """One plan over the MIXED cases, each on a grid of its own, and its device buffers."""

    def __init__(self, ctx):
        import torch
        self.cases = mixed_cases()
        n = len(self.cases)
        ce_offsets = np.cumsum([0] + [c.ce.size for c in self.cases])[:-1]
        self.plan = lib.PuschDemodPlan(ctx, [c.cfg for c in self.cases], list(range(n)), n, MIX_PORTS, MIX_SUBC,
                                       [int(o) for o in ce_offsets], features=BOTH)
        self.G = [self.plan.codeword_bits(i) for i in range(n)]
        self.stride = max(self.G) + 13
        self.d_grids = dev(as_i32(np.stack([c.grid for c in self.cases])))
        self.d_ces = dev(as_i32(np.concatenate([c.ce.reshape(-1) for c in self.cases])))
        self.d_nv = dev(np.stack([c.noise_vars for c in self.cases]))
        self.n = n
        self.torch = torch

    def run(self, ctx, sinr=True, evm=True, stream=None, out=None):
        torch = self.torch
        d_llr, d_sinr, d_evm = out or (torch.full((self.n * self.stride,), 77, dtype=torch.int8, device="cuda"),
                                       torch.full((self.n,), -1.0, dtype=torch.float32, device="cuda"),
                                       torch.full((self.n,), -1.0, dtype=torch.float32, device="cuda"))
        self.plan.run(self.d_grids, self.d_ces, self.d_nv, d_llr, self.stride, d_sinr if sinr else None, stream=stream,
                      d_evm=d_evm if evm else None)
        if out is None:
            ctx.synchronize()
            return d_llr.cpu().numpy(), d_sinr.cpu().numpy(), d_evm.cpu().numpy()


@pytest.mark.gpu
def test_one_plan_with_four_cases(gpu_ctx):
    import torch
    m = MixedRun(gpu_ctx)
    llr, sinr, evm = m.run(gpu_ctx)
    for i, c in enumerate(m.cases):  # each PUSCH's EVM is its single-PUSCH value bit for bit
        nv = c.noise_vars[:c.cfg.nof_rx_ports]
        one_llr, one_sinr, one_evm = gpu_ctx.pusch_demodulate_host_evm(c.cfg, c.grid, c.ce, nv, BOTH)
        assert evm[i].view(np.uint32) == one_evm.view(np.uint32), (i, evm[i], one_evm)
        assert sinr[i].view(np.uint32) == f32(one_sinr).view(np.uint32), i
        assert np.array_equal(llr[i * m.stride: i * m.stride + m.G[i]], one_llr), i
        assert (llr[i * m.stride + m.G[i]: (i + 1) * m.stride] == 77).all(), i
    # either output alone; the one left out is not written
    llr_e, sinr_e, evm_e = m.run(gpu_ctx, sinr=False)
    assert np.array_equal(llr_e, llr) and (sinr_e == -1.0).all() and np.array_equal(evm_e.view(np.uint32), evm.view(np.uint32))
    llr_s, sinr_s, evm_s = m.run(gpu_ctx, evm=False)
    assert np.array_equal(llr_s, llr) and (evm_s == -1.0).all() and np.array_equal(sinr_s.view(np.uint32), sinr.view(np.uint32))
    # two runs give identical bytes
    again = m.run(gpu_ctx)
    for a, b in zip(again, (llr, sinr, evm)):
        assert a.tobytes() == b.tobytes()
    # one graph replay
    out = (torch.zeros(m.n * m.stride, dtype=torch.int8, device="cuda"), torch.zeros(m.n, dtype=torch.float32, device="cuda"),
           torch.zeros(m.n, dtype=torch.float32, device="cuda"))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            m.run(gpu_ctx, stream=C.c_void_p(stream.cuda_stream), out=out)
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = out[0].cpu().numpy()
        for i in range(m.n):
            assert np.array_equal(got[i * m.stride: i * m.stride + m.G[i]], llr[i * m.stride: i * m.stride + m.G[i]]), i
        assert np.array_equal(out[1].cpu().numpy().view(np.uint32), sinr.view(np.uint32))
        assert np.array_equal(out[2].cpu().numpy().view(np.uint32), evm.view(np.uint32))
    m.plan.close()


# =======================================================================================================================
# GPU: the processor and the slot pool
# =======================================================================================================================
FIELDS = [f for f, _ in abi.PuschResult._fields_]


def field_bytes(r, f):
    return np.array(getattr(r, f), proc.RESULT_DTYPE[f]).tobytes()


@pytest.mark.gpu
def test_processor_with_the_evm(gpu_ctx):
    sc = proc.Scenario.get(gpu_ctx, "abcdef", abi.EQ_ZF)
    grids = sc.grids(True)
    opts = sc.opts
    for i, (name, p, d) in enumerate(zip(sc.names, sc.pdus, sc.derived)):
        base, base_tb, base_uci = gpu_ctx.pusch_proc_host(p, opts, grids[i])
        assert (base.has_evm, base.evm) == (0, 0.0), name
        # enable_evm = 0: the bytes of nrphy_pusch_proc_host
        off, off_tb, off_uci = gpu_ctx.pusch_evm_host(p, abi.PuschEvmOptions(opts, 0, 0), grids[i])
        assert bytes(off) == bytes(base) and off_tb.tobytes() == base_tb.tobytes() and off_uci.tobytes() == base_uci.tobytes(), name
        # the demodulator's EVM on what nrphy_pusch_chest_host gives for the derived configuration
        ce, nv, _ = gpu_ctx.pusch_chest_host(d.chest, grids[i])
        _, _, want_evm = gpu_ctx.pusch_demodulate_host_evm(d.demod, grids[i], ce, nv, 0)
        for method in METHODS:
            o = abi.PuschEvmOptions(proc._opts(csi_sinr_calc_method=method), 1, 0)
            # what the calls without the EVM give for the method; for the EVM method sinr_dB is left out, and nothing else
            # depends on the method
            same = method in (opts.csi_sinr_calc_method, abi.PUSCH_SINR_EVM)
            ref = base if same else gpu_ctx.pusch_proc_host(p, o.proc, grids[i])[0]
            on, on_tb, on_uci = gpu_ctx.pusch_evm_host(p, o, grids[i])
            skip = ("has_evm", "evm") + (("sinr_dB",) if method == abi.PUSCH_SINR_EVM else ())
            for f in FIELDS:
                if f not in skip:
                    assert field_bytes(on, f) == field_bytes(ref, f), (name, method, f)
            assert on_tb.tobytes() == base_tb.tobytes() and on_uci.tobytes() == base_uci.tobytes(), (name, method)
            assert on.has_evm == 1 and f32(on.evm).view(np.uint32) == want_evm.view(np.uint32), (name, method, on.evm, want_evm)
            assert on.evm > 0, name  # (e), without codeword, has one too
            if method == abi.PUSCH_SINR_EVM:
                want = f32(f32(-20.0) * np.log10(f32(on.evm)) - f32(3.7))
                assert abs(float(on.sinr_dB) - float(want)) <= 1e-4, (name, on.sinr_dB, want)
        print("(%s) evm %.6g, EVM-based SINR %.4f dB, post-equalisation %.4f dB" % (name, on.evm, on.sinr_dB, on.sinr_post_eq_dB))


@pytest.mark.gpu
def test_plan_form_with_the_evm_equals_the_host_form(gpu_ctx):
    """nrphy_pusch_evm_plan_create over (a)-(f) in one plan, run by nrphy_pusch_proc_run: every record's EVM fields are the host
    form's."""
    sc = proc.Scenario.get(gpu_ctx, "abcdef", abi.EQ_ZF)
    grids = sc.grids(True)
    o = abi.PuschEvmOptions(proc._opts(csi_sinr_calc_method=abi.PUSCH_SINR_EVM), 1, 0)
    L = sc.layout
    plan = lib.PuschProcPlan(gpu_ctx, sc.pdus, o, sc.gidx, len(sc.names), proc.NPORTS, proc.NSUBC, L.soft, L.state, L.tb, L.uci)
    B = proc.Buffers(L, len(sc.names), None)
    plan.run(dev(as_i32(grids)), B.harq, B.tb, B.uci, B.result)
    gpu_ctx.synchronize()
    got = B.read()
    plan.close()
    for i, p in enumerate(sc.pdus):
        one = gpu_ctx.pusch_evm_host(p, o, grids[i])[0]
        r = got["result"][i]
        for f in ("has_evm", "evm", "sinr_dB", "sinr_post_eq_dB", "sinr_ch_estimator_dB", "tb_crc_ok"):
            assert np.array(r[f]).tobytes() == field_bytes(one, f), (sc.names[i], f)
        assert r["has_evm"] == 1


@pytest.mark.gpu
def test_slot_pool_mixes_both_calls(gpu_ctx):
    import torch
    nports, nprb = 2, proc.NSUBC // 12
    ofdm = abi.OfdmConfig(0, nprb, 384, 0, 1.0 / np.sqrt(384), 2.0e9)
    rng = np.random.default_rng(31)
    pdus = [proc.make_pdus("a", rx_ports=(0,))[0], proc.make_pdus("b", rx_ports=(0, 1))[0]]
    derived = [lib.pusch_proc_derive(p, proc.OPTIONS, nports, proc.NSUBC) for p in pdus]
    sent = [proc.transmit(gpu_ctx, p, d, rng) for p, d in zip(pdus, derived)]
    clean = sum(s.clean[:nports] for s in sent)
    noise = (rng.standard_normal(clean.shape) + 1j * rng.standard_normal(clean.shape)) * np.sqrt(0.5 * 10 ** -2.0)
    words = to_cbf16((clean + noise).astype(np.complex64)).view(np.uint32).reshape(nports, 14, proc.NSUBC)
    layout = proc.Layout(pdus, proc.OPTIONS)
    d_harq = torch.zeros(layout.harq_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pool = lib.UlSlots(gpu_ctx, ofdm, nports, 1, d_harq=d_harq, max_pusch=2, max_uci_bits=64,
                       max_tb_bytes=sum(p.tb_size_bytes for p in pdus))
    o = abi.make_pusch_evm_options(csi_sinr_calc_method=abi.PUSCH_SINR_EVM)
    sid = pool.open(0)
    assert pool.load_grid(sid, words.view(np.uint16).reshape(nports, 14, proc.NSUBC, 2)) == abi.OK
    assert pool.pusch_evm(sid, pdus[1:], abi.make_pusch_evm_options(enable_evm=2), layout.soft[1:], layout.state[1:]) == abi.ERR_ARGUMENT
    assert pool.pusch(sid, pdus[:1], proc.OPTIONS, layout.soft[:1], layout.state[:1]) == abi.OK
    assert pool.pusch_evm(sid, pdus[1:], o, layout.soft[1:], layout.state[1:]) == abi.OK
    assert pool.finish(sid) == abi.OK and pool.wait(sid) == abi.OK
    got = pool.pusch_results(sid)
    want0, tb0, _ = gpu_ctx.pusch_proc_host(pdus[0], proc.OPTIONS, words)
    want1, tb1, uci1 = gpu_ctx.pusch_evm_host(pdus[1], o, words)
    assert len(got) == 2 and got[0].has_evm == 0 and bytes(got[0]) == bytes(want0)
    assert got[1].has_evm == 1 and got[1].evm > 0 and bytes(got[1]) == bytes(want1)
    assert pool.tb(sid, 0).tobytes() == tb0.tobytes() and pool.tb(sid, 1).tobytes() == tb1.tobytes()
    assert pool.uci_bits(sid, 1).tobytes() == uci1.tobytes()
    assert want0.tb_crc_ok == 1 and want1.tb_crc_ok == 1
    pool.close(sid)
    pool.destroy()
