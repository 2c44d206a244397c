"""nrphy_ofdm_demod_symbols on the GPU: the OFDM demodulator over a run of symbols, from complex float or complex int16 samples
(puxch_processor_impl::process_symbol, R/lib/phy/lower/processors/uplink/puxch/puxch_processor_impl.cpp:30-81, with the radio's
srsvec::convert in front, R/lib/srsvec/conversion.cpp:67-129).

The reference of every comparison is the whole-slot launch nrphy_ofdm_demod_run, which test_gpu_parity.py pins to the oracle and to
the reference's own output: a run of symbols must give that launch's rows bit for bit, touch no other row and read no other
sample; int16 samples must give what the float path gives for float32(x) * float32(1 / scale) formed in numpy, bit for bit, which a
multiply fused into the first butterfly would miss for the gains that are not powers of two.
"""
import numpy as np
import pytest

import backends

abi = backends.pkg.abi
lib = backends.pkg.lib

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC17FC2  # a cbf16 word no demodulation writes (two NaN payloads)

# name -> (numerology, bw_rb, dft_size, extended CP, window offset, the slot of each of the two grids)
CASES = {
    "d128": (2, 6, 128, 0, 0, (0, 1)),
    "d384": (2, 25, 384, 0, 0, (3, 2)),
    "d512w": (2, 25, 512, 0, 5, (1, 2)),
    "d1536": (2, 106, 1536, 0, 0, (0, 3)),
    "d4096": (2, 273, 4096, 0, 0, (2, 1)),
    "dx1024w": (2, 51, 1024, 1, 3, (0, 1)),
}
NOF_PORTS = 2


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_cfg(name):
    mu, bw, n, ext, wo, slots = CASES[name]
    return abi.OfdmConfig(mu, bw, n, ext, 1.0 / np.sqrt(n), 3.5e9), wo, slots


def symbol_offsets(cfg, slot):
    nsymb = 12 if cfg.cp else 14
    off = [0]
    for l in range(nsymb):
        off.append(off[-1] + lib.symbol_size(cfg, nsymb * slot + l))
    return off


def whole_slot(ctx, plan, cfg, iq, slots, wo):
    """nrphy_ofdm_demod_run over both grids into a sentinel-filled buffer: [2][ports][14][subc] uint32."""
    import torch
    d_grid = torch.full((2, NOF_PORTS, 14, 12 * cfg.bw_rb), SENTINEL, dtype=torch.int32, device="cuda")
    d_slot = dev(np.array(slots, np.uint32).view(np.int32))
    torch.cuda.synchronize()
    plan.demod_run(2, dev(iq.view(np.float32)), d_grid, d_slot_index=d_slot, window_offset=wo)
    ctx.synchronize()
    return d_grid.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", list(CASES))
def test_cf32_symbol_range_equals_the_whole_slot_launch(gpu_ctx, name):
    import torch
    cfg, wo, slots = make_cfg(name)
    nsymb = 12 if cfg.cp else 14
    plan = lib.OfdmPlan(gpu_ctx, cfg, NOF_PORTS)
    rng = np.random.default_rng(cfg.dft_size)
    iq = (rng.standard_normal((2, NOF_PORTS, plan.slot_stride)) + 1j * rng.standard_normal((2, NOF_PORTS, plan.slot_stride))).astype(np.complex64)
    want = whole_slot(gpu_ctx, plan, cfg, iq, slots, wo)
    assert np.all(want[:, :, nsymb:] == SENTINEL) and not np.any(want[:, :, :nsymb] == SENTINEL)
    d_slot = dev(np.array(slots, np.uint32).view(np.int32))
    ranges = [(0, 1), (1, 3), (4, nsymb - 4)]

    def only(first, n):
        """The samples with everything outside symbols [first, first + n) of each grid made NaN."""
        out = np.full_like(iq, np.nan + 1j * np.nan)
        for g, slot in enumerate(slots):
            off = symbol_offsets(cfg, slot)
            out[g, :, off[first]: off[first + n]] = iq[g, :, off[first]: off[first + n]]
        return dev(out.view(np.float32))

    together = torch.full((2, NOF_PORTS, 14, 12 * cfg.bw_rb), SENTINEL, dtype=torch.int32, device="cuda")
    for first, n in ranges:
        d_grid = torch.full_like(together, SENTINEL)
        d_iq = only(first, n)
        torch.cuda.synchronize()
        for target in (d_grid, together):
            assert plan.demod_symbols(2, d_iq, target, first, n, d_slot_index=d_slot, window_offset=wo) == abi.OK
        gpu_ctx.synchronize()
        got = d_grid.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:, :, first: first + n], want[:, :, first: first + n]), (first, n)
        assert np.all(got[:, :, :first] == SENTINEL) and np.all(got[:, :, first + n:] == SENTINEL), (first, n)
    assert np.array_equal(together.cpu().numpy().view(np.uint32), want)
    plan.close()


def bf16_to_f32(raw):
    return (raw.astype(np.uint32) << 16).view(np.float32)


def assert_bf16_grids_close(got, want, min_exact=0.99):
    """The closeness rule of test_gpu_parity.py for cbf16 grids out of different float FFTs."""
    a, b = bf16_to_f32(got), bf16_to_f32(want)
    scale = np.abs(b).max()
    assert np.all(np.abs(a - b) <= np.maximum(np.abs(b), 1e-3 * scale) * 2.0 ** -7)
    assert np.mean(got == want) >= min_exact


@pytest.mark.parametrize("name", list(CASES))
def test_ci16_equals_the_float_path_on_converted_samples(gpu_ctx, oracle, name):
    import torch
    cfg, wo, slots = make_cfg(name)
    nsymb = 12 if cfg.cp else 14
    plan = lib.OfdmPlan(gpu_ctx, cfg, NOF_PORTS)
    rng = np.random.default_rng(7 * cfg.dft_size)
    x = rng.integers(-32768, 32768, (2, NOF_PORTS, plan.slot_stride, 2)).astype(np.int16)
    flat = x.reshape(-1)
    for value in (-32768, 32767, 0):
        flat[rng.choice(flat.size, flat.size // 16, replace=False)] = value
    x[:, :, -3:] = [[-32768, 32767], [32767, -32768], [0, -32768]]
    assert (x == -32768).any() and (x == 32767).any() and (x == 0).any()
    d_x = dev(x)
    d_slot = dev(np.array(slots, np.uint32).view(np.int32))
    for scale in (32768.0, 32767.0, 10000.0):
        gain = np.float32(1.0) / np.float32(scale)
        conv = x.astype(np.float32) * gain
        assert conv.dtype == np.float32
        conv = np.ascontiguousarray(conv).view(np.complex64).reshape(2, NOF_PORTS, plan.slot_stride)
        want = whole_slot(gpu_ctx, plan, cfg, conv, slots, wo)
        d_grid = torch.full((2, NOF_PORTS, 14, 12 * cfg.bw_rb), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert plan.demod_symbols(2, d_x, d_grid, 0, nsymb, iq_format=abi.IQ_CI16, iq_scale=scale, d_slot_index=d_slot,
                                  window_offset=wo) == abi.OK
        gpu_ctx.synchronize()
        got = d_grid.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want), scale
        if name == "d512w" and scale == 10000.0:
            for g, slot in enumerate(slots):
                size = lib.slot_size(cfg, slot)
                ref = oracle.ofdm_demod_slot(cfg, conv[g, :, :size], slot, wo)
                assert_bf16_grids_close(got[g].view(np.uint16).reshape(ref.shape)[:, :nsymb], ref[:, :nsymb])
    plan.close()


def test_arguments_are_refused_without_a_launch(gpu_ctx):
    import torch
    for ext in (0, 1):
        cfg = abi.OfdmConfig(2, 6, 128, ext, 1.0, 0.0)
        nsymb = 12 if ext else 14
        plan = lib.OfdmPlan(gpu_ctx, cfg, NOF_PORTS)
        d_grid = torch.full((1, NOF_PORTS, 14, 72), SENTINEL, dtype=torch.int32, device="cuda")
        d_iq = torch.ones((1, NOF_PORTS, plan.slot_stride, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        shortest_cp = (144 * 128) // 2048
        refused = [dict(first_symbol=0, nof_symbols=0), dict(first_symbol=nsymb, nof_symbols=1),
                   dict(first_symbol=nsymb - 1, nof_symbols=2), dict(first_symbol=0, nof_symbols=nsymb + 1),
                   dict(first_symbol=3, nof_symbols=0xFFFFFFFE), dict(first_symbol=0, nof_symbols=1, iq_format=2),
                   dict(first_symbol=0, nof_symbols=1, window_offset=shortest_cp)]
        refused += [dict(first_symbol=0, nof_symbols=1, iq_format=abi.IQ_CI16, iq_scale=s)
                    for s in (0.0, -1.0, float("inf"), float("nan"))]
        for kw in refused:
            assert plan.demod_symbols(1, d_iq, d_grid, **kw) == abi.ERR_ARGUMENT, kw
        # iq_scale is not looked at for float samples, and no grid is no work
        assert plan.demod_symbols(0, d_iq, d_grid, 0, nsymb) == abi.OK
        assert plan.demod_symbols(0, d_iq, d_grid, 0, nsymb, iq_format=abi.IQ_CI16, iq_scale=32768.0) == abi.OK
        gpu_ctx.synchronize()
        assert np.all(d_grid.cpu().numpy().view(np.uint32) == SENTINEL)
        assert plan.demod_symbols(1, d_iq, d_grid, nsymb - 1, 1, iq_scale=float("nan")) == abi.OK
        gpu_ctx.synchronize()
        got = d_grid.cpu().numpy().view(np.uint32)
        assert np.all(got[:, :, : nsymb - 1] == SENTINEL) and np.all(got[:, :, nsymb:] == SENTINEL) and not np.any(got[:, :, nsymb - 1] == SENTINEL)
        plan.close()
