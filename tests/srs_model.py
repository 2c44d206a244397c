"""NumPy restatement of the SRS channel estimator (srs_estimator_generic_impl::estimate with low_papr_sequence_generator_impl,
time_alignment_estimator_dft_impl and get_srs_information), for tests/test_srs_estimator.py.

Four parts: info() (the mapping), sequence() (the generator), transmit() (ports on their combs and cyclic shifts, a channel with
per-path gains, a delay in bins of the 4096-point transform, AWGN, cbf16 quantisation) and estimate().  The arithmetic that
decides a result is restated in np.float32 step by step: the Zadoff-Chu root, the unit circles' angles, the products, and the
compensation's phase index (a float64 index rounds differently at half-way points, and one wrong index moves a coefficient by
about 2 pi / 1024 / M).  The inverse DFT is evaluated in float64; ta_near_tie says where that could matter.

A configuration is anything with the fields of nrphy_srs_cfg_t as attributes or keys (rx_ports a sequence, nof_rx_ports
optional for a mapping)."""
import json
import os

import numpy as np

from pusch_chest_model import from_cbf16, to_cbf16

f32 = np.float32
TWOPI = f32(2.0) * f32(np.pi)  # 2.0F * static_cast<float>(M_PI)
DFT_SIZE = 4096
CEXP_SIZE = 1024
CS_SIZE = 24
NSYMB = 14

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_T = json.load(open(os.path.join(_GOLDEN, "srs_tables.json")))
BANDWIDTH = _T["bandwidth"]  # [C_SRS][B_SRS] = (m_SRS, N)
PHI = {12: json.load(open(os.path.join(_GOLDEN, "pucch_tables.json")))["phi_12"], 24: _T["phi_24"]}


def field(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def rx_ports(cfg):
    ports = list(field(cfg, "rx_ports"))
    return ports if isinstance(cfg, dict) else ports[:cfg.nof_rx_ports]


# ---- the mapping (get_srs_information) ----------------------------------------------------------------------------------------
def info(cfg, port):
    comb, c_srs, b_srs = field(cfg, "comb_size"), field(cfg, "configuration_index"), field(cfg, "bandwidth_index")
    ntx, cs = field(cfg, "nof_antenna_ports"), field(cfg, "cyclic_shift")
    n_cs_max = 12 if comb == 4 else 8
    k_tc = field(cfg, "comb_offset")
    if n_cs_max // 2 <= cs < n_cs_max and ntx == 4 and port in (1, 3):
        k_tc = (k_tc + comb // 2) % comb
    total = 0
    for b in range(b_srs + 1):
        m_srs, N = BANDWIDTH[c_srs][b]
        total += comb * (m_srs * 12 // comb) * (((4 * field(cfg, "freq_position")) // m_srs) % N)
    return {"sequence_length": BANDWIDTH[c_srs][b_srs][0] * 12 // comb, "initial_subcarrier": field(cfg, "freq_shift") * 12 + k_tc + total,
            "n_cs": (cs + (n_cs_max * port) // ntx) % n_cs_max, "n_cs_max": n_cs_max, "u": field(cfg, "sequence_id") % 30}


def window(cfg):
    """time_alignment_estimator_dft_impl's max_ta_samples for the estimator's max_ta, in double as the reference evaluates it."""
    scs_khz = 15 << field(cfg, "numerology")
    comb = field(cfg, "comb_size")
    max_ta = 1.0 / float((12 if comb == 4 else 8) * scs_khz * 1000 * comb)
    return int(np.floor(max_ta * float(scs_khz * 1000 * DFT_SIZE)))


# ---- the generator (low_papr_sequence_generator_impl) -------------------------------------------------------------------------
def unit_circle(size):
    """complex_exponential_table(size, 1): polar(1, float(2 pi) float(n) / float(size)), the angle in single precision."""
    a = ((f32(2 * np.pi) * np.arange(size, dtype=np.float32)).astype(np.float32) / f32(size)).astype(np.float32)
    a = a.astype(np.float64)
    return (np.cos(a).astype(np.float32) + 1j * np.sin(a).astype(np.float32)).astype(np.complex64)


def cmul(a, b):
    """srsvec::prod on complex values, every product and sum rounded to single precision."""
    ar, ai, br, bi = a.real.astype(np.float32), a.imag.astype(np.float32), b.real.astype(np.float32), b.imag.astype(np.float32)
    re = ((ar * br).astype(np.float32) - (ai * bi).astype(np.float32)).astype(np.float32)
    im = ((ar * bi).astype(np.float32) + (ai * br).astype(np.float32)).astype(np.float32)
    return (re + 1j * im).astype(np.complex64)


def conj_prod(a, b):
    """srsvec::prod_conj: a conj(b) = (a.re b.re + a.im b.im, a.im b.re - a.re b.im)."""
    ar, ai, br, bi = a.real.astype(np.float32), a.imag.astype(np.float32), b.real.astype(np.float32), b.imag.astype(np.float32)
    re = ((ar * br).astype(np.float32) + (ai * bi).astype(np.float32)).astype(np.float32)
    im = ((ai * br).astype(np.float32) - (ar * bi).astype(np.float32)).astype(np.float32)
    return (re + 1j * im).astype(np.complex64)


def prime_lower_than(n):
    for v in range(n - 1, 2, -1):
        if all(v % f for f in range(2, int(v ** 0.5) + 1)):
            return v
    return 2


def zc_root(u, n_zc):
    """zc_sequence_q(u, 0, N_zc): single precision, the half added in double."""
    q_hat = f32(f32(f32(n_zc) * f32(u + 1)) / f32(31))
    return int(f32(np.float64(q_hat) + 0.5))


def sequence(u, M, n_cs, n_cs_max):
    n = np.arange(M)
    if M in PHI:
        r = unit_circle(8)[(8 + np.array(PHI[M][u])) % 8]
    else:
        n_zc = prime_lower_than(M)
        q = zc_root(u, n_zc)
        m = n % n_zc
        arg = -((q * m * (m + 1)) % (2 * n_zc))
        r = unit_circle(2 * n_zc)[(2 * n_zc + arg) % (2 * n_zc)]
    if n_cs != 0:
        r = cmul(r, unit_circle(CS_SIZE)[(n * (n_cs * CS_SIZE // n_cs_max)) % CS_SIZE])
    return r


def port_sequence(cfg, port):
    i = info(cfg, port)
    return sequence(i["u"], i["sequence_length"], i["n_cs"], i["n_cs_max"])


# ---- a transmitter and a channel -----------------------------------------------------------------------------------------------
def transmit(cfg, nof_ports, nof_subc, gains, delay_bins=0, noise_std=0.0, rng=None):
    """grid [nof_ports][14][nof_subc] cbf16 words: antenna port p sends its sequence on its comb, receive port i (grid port
    rx_ports[i]) sees it through gains[i][p] and a delay of delay_bins / (4096 scs) seconds (the phase exp(-j 2 pi k d / 4096) on
    subcarrier k), plus complex Gaussian noise of standard deviation noise_std on every element of the grid."""
    ports = rx_ports(cfg)
    ns, l0, comb = field(cfg, "nof_symbols"), field(cfg, "start_symbol"), field(cfg, "comb_size")
    g = np.zeros((nof_ports, NSYMB, nof_subc), np.complex128)
    for p in range(field(cfg, "nof_antenna_ports")):
        i = info(cfg, p)
        k = i["initial_subcarrier"] + comb * np.arange(i["sequence_length"])
        x = port_sequence(cfg, p).astype(np.complex128) * np.exp(-2j * np.pi * k * delay_bins / DFT_SIZE)
        for irx, q in enumerate(ports):
            for l in range(l0, l0 + ns):
                g[q, l, k] += gains[irx][p] * x
    if noise_std:
        g += noise_std * np.sqrt(0.5) * (rng.standard_normal(g.shape) + 1j * rng.standard_normal(g.shape))
    return to_cbf16(g.astype(np.complex64))


# ---- the estimator --------------------------------------------------------------------------------------------------------------
def mean_lse(cfg, grid, irx, port):
    i = info(cfg, port)
    ns, l0, comb = field(cfg, "nof_symbols"), field(cfg, "start_symbol"), field(cfg, "comb_size")
    k = i["initial_subcarrier"] + comb * np.arange(i["sequence_length"])
    r = port_sequence(cfg, port)
    acc = None
    for l in range(l0, l0 + ns):
        e = conj_prod(from_cbf16(grid[rx_ports(cfg)[irx], l, k]), r)
        acc = e if acc is None else ((acc.real + e.real).astype(np.float32) + 1j * (acc.imag + e.imag).astype(np.float32)).astype(np.complex64)
    if ns > 1:
        s = f32(1.0 / float(f32(ns)))
        acc = ((acc.real * s).astype(np.float32) + 1j * (acc.imag * s).astype(np.float32)).astype(np.complex64)
    return acc


def phase_indices(M, ps, off):
    """static_cast<int>(std::round(float(1024) * (float(n) * ps + offset) / TWOPI)), every step in single precision."""
    n = np.arange(M, dtype=np.float32)
    x = ((f32(CEXP_SIZE) * ((n * f32(ps)).astype(np.float32) + f32(off)).astype(np.float32)).astype(np.float32) / TWOPI).astype(np.float32)
    x = x.astype(np.float64)
    return np.where(x >= 0, np.floor(x + 0.5), -np.floor(-x + 0.5)).astype(np.int64) % CEXP_SIZE


def estimate(cfg, grid):
    """grid [ports][14][subc] cbf16 words -> dict: h complex64 [4][4] ([rx][tx]), ta_bins int [4][4], time_alignment_s (double),
    ta_near_tie bool [4][4] (the two largest searched magnitudes of the path within 1e-4 of each other, as
    pusch_chest_model.estimate_port defines it) and lse_rms, the root mean square of all mean LS estimates."""
    nrx, ntx, comb = len(rx_ports(cfg)), field(cfg, "nof_antenna_ports"), field(cfg, "comb_size")
    scs_khz = 15 << field(cfg, "numerology")
    W = window(cfg)
    lse = {}
    ta_bins = np.zeros((4, 4), np.int64)
    near = np.zeros((4, 4), bool)
    ta, power, count = 0.0, 0.0, 0
    for p in range(ntx):
        for i in range(nrx):
            e = lse[i, p] = mean_lse(cfg, grid, i, p)
            power += float(np.sum(np.abs(e.astype(np.complex128)) ** 2))
            count += e.size
            x = np.zeros(DFT_SIZE, np.complex128)
            x[comb * np.arange(e.size)] = e
            mag = np.abs(np.fft.ifft(x) * DFT_SIZE) ** 2
            mag = np.concatenate([mag[:W], mag[DFT_SIZE - W:]])
            i_d, i_a = int(np.argmax(mag[:W])), int(np.argmax(mag[W:]))
            ta_bins[i, p] = i_d if mag[i_d] >= mag[W + i_a] else i_a - W
            top = np.sort(mag)[-2:]
            near[i, p] = bool(top[1] - top[0] <= 1e-4 * top[1])
            ta += float(ta_bins[i, p]) / float(DFT_SIZE * scs_khz * 1000)
    ta /= float(ntx * nrx)
    ps = f32(np.float64(TWOPI) * ta * float(scs_khz) * 1000.0 * float(comb))
    cexp = unit_circle(CEXP_SIZE)
    h = np.zeros((4, 4), np.complex64)
    for p in range(ntx):
        k0 = info(cfg, p)["initial_subcarrier"]
        off = f32(f32(ps * f32(k0 % comb)) / f32(comb))
        for i in range(nrx):
            c = cmul(lse[i, p], cexp[phase_indices(lse[i, p].size, ps, off)])
            h[i, p] = np.complex64(np.sum(c, dtype=np.complex64)) / f32(c.size)
    return {"h": h, "ta_bins": ta_bins, "time_alignment_s": ta, "ta_near_tie": near, "lse_rms": float(np.sqrt(power / max(count, 1)))}
