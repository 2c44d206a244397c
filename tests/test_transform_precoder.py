"""Transform deprecoder (nrphy_transform_deprecode, nrphy_transform_precoding_nof_prb_valid).

CPU: the valid sizes.  GPU: every one of the 53 sizes against numpy.fft.ifft in float64, within 4 x the error an independent
single-precision transform makes on the same inputs (tests/golden/pusch_tp_dft_bounds.json, measured by
tests/golden/make_pusch_tp_dft_bounds.py with scipy.fft on complex64; a different factorisation and twiddle order may cost a few
ulp per stage, a wrong twiddle, stage or scale is off by O(1)); the calling forms.
"""
import json
import os

import numpy as np
import pytest

import backends
import pusch_tp_model as model
from pusch_chest_model import dev

abi = backends.abi
lib = backends.pkg.lib

BOUNDS = os.path.join(backends.ROOT, "tests", "golden", "pusch_tp_dft_bounds.json")


def test_valid_sizes_are_the_2_3_5_smooth_ones():
    got = [n for n in range(276) if lib.transform_precoding_nof_prb_valid(n)]
    assert got == model.VALID_NOF_PRB
    assert len(got) == 53 and got[0] == 1 and got[-1] == 270
    assert not lib.transform_precoding_nof_prb_valid(276) and not lib.transform_precoding_nof_prb_valid(300)


def test_bounds_fixture_covers_every_size():
    bounds = json.load(open(BOUNDS))
    assert sorted(int(k) for k in bounds) == model.VALID_NOF_PRB
    assert all(1e-8 < v < 5e-6 for v in bounds.values()), bounds  # float32 rounding errors of unit-variance data


def deprecode(ctx, nof_prb, x, in_place=False):
    import torch
    d_in = dev(np.ascontiguousarray(x).view(np.float32))
    d_out = d_in if in_place else torch.zeros_like(d_in)
    ctx.transform_deprecode(nof_prb, x.shape[0], d_in, d_out)
    ctx.synchronize()
    return d_out.cpu().numpy().view(np.complex64).reshape(x.shape)


@pytest.mark.gpu
def test_every_size_against_float64(gpu_ctx):
    bounds = json.load(open(BOUNDS))
    bad = []
    for nof_prb in model.VALID_NOF_PRB:
        x = model.dft_inputs(nof_prb)
        got = deprecode(gpu_ctx, nof_prb, x)
        err = float(np.abs(got.astype(np.complex128) - model.dft_exact(x)).max())
        ratio = err / bounds[str(nof_prb)]
        print("nof_prb %3d  N %4d  device error %.3e  bound %.3e  ratio %.2f" % (nof_prb, 12 * nof_prb, err, bounds[str(nof_prb)],
                                                                                 ratio))
        if not err <= 4 * bounds[str(nof_prb)]:
            bad.append((nof_prb, err, bounds[str(nof_prb)]))
    assert not bad, bad


@pytest.mark.gpu
def test_calling_forms(gpu_ctx):
    import torch
    for nof_prb in (1, 5, 25, 27, 270):
        x = model.dft_inputs(nof_prb)
        out = deprecode(gpu_ctx, nof_prb, x)
        assert np.array_equal(deprecode(gpu_ctx, nof_prb, x, in_place=True).view(np.uint64), out.view(np.uint64)), nof_prb
        for b in range(x.shape[0]):
            assert np.array_equal(gpu_ctx.transform_deprecode_host(nof_prb, x[b]).view(np.uint64), out[b].view(np.uint64)), nof_prb
    # batch = 0 does nothing, whatever the pointers; an invalid size is an argument error
    d = torch.full((24,), 7.0, dtype=torch.float32, device="cuda")
    gpu_ctx.transform_deprecode(1, 0, d, d)
    gpu_ctx.transform_deprecode(1, 0, None, None)
    gpu_ctx.synchronize()
    assert (d.cpu().numpy() == 7.0).all()
    for nof_prb in (0, 7, 11, 271, 276):
        rc = gpu_ctx.lib.nrphy_transform_deprecode(gpu_ctx.handle, nof_prb, 1, d.data_ptr(), d.data_ptr(), None)
        assert rc == abi.ERR_ARGUMENT, nof_prb
        rc = gpu_ctx.lib.nrphy_transform_deprecode_host(gpu_ctx.handle, nof_prb, None, None)
        assert rc == abi.ERR_ARGUMENT, nof_prb
    assert (d.cpu().numpy() == 7.0).all()
