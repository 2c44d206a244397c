"""Writes tests/golden/pusch_tp_dft_bounds.json: per transform-precoding size, the largest absolute error of an independent
single-precision transform (scipy.fft.ifft on complex64, pocketfft) against float64 on the inputs of
tests/test_transform_precoder.py (pusch_tp_model.dft_inputs).  The test allows the device 4 x this figure, so SciPy is needed
here only.

    python tests/golden/make_pusch_tp_dft_bounds.py tests/golden/pusch_tp_dft_bounds.json
"""
import json
import os
import sys

import numpy as np
import scipy.fft

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pusch_tp_model as model  # noqa: E402


def main(out):
    bounds = {}
    for nof_prb in model.VALID_NOF_PRB:
        x = model.dft_inputs(nof_prb)
        single = scipy.fft.ifft(x, axis=-1)
        assert single.dtype == np.complex64
        single = single * np.float32(np.sqrt(np.float32(x.shape[-1])))
        assert single.dtype == np.complex64
        bounds[str(nof_prb)] = float(np.abs(single.astype(np.complex128) - model.dft_exact(x)).max())
    with open(out, "w") as f:
        json.dump(bounds, f, indent=0, sort_keys=False)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
