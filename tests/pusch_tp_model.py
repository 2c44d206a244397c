"""What the transform-precoding tests share (tests/test_transform_precoder.py, tests/test_pusch_transform_precoding.py) and what
tests/golden/make_pusch_tp_dft_bounds.py measures its bounds on: the valid sizes, the seeded transform inputs, and the composed
path of a transform-precoded PUSCH through the stand-alone device calls."""
import numpy as np


def nof_prb_valid(n):
    """transform_precoding::is_nof_prbs_valid: 2^a 3^b 5^c within 1..275."""
    if not 1 <= n <= 275:
        return False
    for f in (2, 3, 5):
        while n % f == 0:
            n //= f
    return n == 1


VALID_NOF_PRB = [n for n in range(276) if nof_prb_valid(n)]


def dft_inputs(nof_prb):
    """Three symbols of 12 * nof_prb complex64: two of unit-variance complex Gaussian noise, one with a single nonzero element."""
    n = 12 * nof_prb
    rng = np.random.default_rng(5000 + nof_prb)
    x = ((rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))) / np.sqrt(2)).astype(np.complex64)
    k = int(rng.integers(0, n))
    one = x[2, k]
    x[2] = 0
    x[2, k] = one
    return x


def dft_exact(x):
    """The deprecoder in float64: the unnormalised inverse DFT divided by sqrt(N)."""
    x = np.asarray(x, np.complex128)
    return np.fft.ifft(x, axis=-1) * np.sqrt(x.shape[-1])


def data_subcarriers(cfg, l):
    """Ascending grid subcarriers of the data RE of OFDM symbol l (empty outside the allocation): on a DM-RS symbol what
    dmrs_type::get_dmrs_prb_mask leaves."""
    if not cfg.start_symbol_index <= l < cfg.start_symbol_index + cfg.nof_symbols:
        return np.zeros(0, np.int64)
    prbs = [b for b in range(320) if (cfg.prb_mask[b // 64] >> (b % 64)) & 1]
    ks = range(12)
    if (cfg.dmrs_symbol_mask >> l) & 1:
        cdm = cfg.nof_cdm_groups_without_data
        if cfg.dmrs_type == 1:
            removed = set(range(0, 12, 2)) if cdm == 1 else set(range(12))
        else:
            removed = {k for g in range(cdm) for k in (2 * g, 2 * g + 1, 2 * g + 6, 2 * g + 7)}
        ks = [k for k in range(12) if k not in removed]
    return np.array([12 * p + k for p in prbs for k in ks], np.int64)


def composed(ctx, cfg, grid, ce, noise_vars):
    """RE taken in NumPy -> nrphy_channel_equalize -> nrphy_transform_deprecode per symbol (a transform-precoded PUSCH) ->
    nrphy_demodulate_soft per symbol -> nrphy_llr_descramble.  Returns the soft bits, the float64 SINR, and per OFDM symbol the
    equalised RE, their noise variances and the symbols handed to the demapper."""
    P = cfg.nof_rx_ports
    ports = [cfg.rx_ports[i] for i in range(P)]
    modulation = 0 if cfg.qm == 1 else cfg.qm  # NRPHY_MOD_PI2_BPSK
    llr, eqs, nvs, zs = [], [], [], []
    for l in range(14):
        ks = data_subcarriers(cfg, l)
        if ks.size == 0:
            continue
        eq, ev = ctx.channel_equalize_host(cfg.equalizer, grid[ports][:, l, ks], ce[:, :, l, ks], noise_vars[:P], 1.0)
        eq, ev = eq.reshape(-1), ev.reshape(-1)
        z = ctx.transform_deprecode_host(ks.size // 12, eq) if cfg.transform_precoding else eq
        llr.append(ctx.demodulate_soft_host(modulation, z, ev))
        eqs.append(eq)
        nvs.append(ev)
        zs.append(z)
    llr = ctx.llr_descramble_host(cfg.rnti * 2 ** 15 + cfg.n_id, np.concatenate(llr))
    v = np.concatenate(nvs).astype(np.float64)
    v = v[~np.isinf(v)]
    sinr = float(-10 * np.log10(v.sum() / v.size)) if v.size and v.sum() > 0 else float("inf")
    return llr, sinr, eqs, nvs, zs
