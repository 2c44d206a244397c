"""NumPy restatement of the PRACH generator and detector the library replaces: prach_generator_impl::generate
(R/lib/phy/upper/channel_processors/prach_generator_impl.cpp:97-287) and prach_detector_generic_impl::detect
(prach_detector_generic_impl.cpp:89-359, symbols combined), in float32 or float64 (`dtype`).  The integer arithmetic follows the
reference's order of operations; the order of the floating-point sums is NumPy's, which is what the tolerances of
tests/test_prach_detector.py are measured against.  That file holds generate() and detect() against a recording of the
reference's own classes (tests/golden/prach_detector_reference_*.npy), decision for decision.

The closed form's constants are derived here (f = u^-1 mod L, the offset from the Gauss sum), not read from the library; the
logical-to-physical root table (TS 38.211 Table 6.3.3.1-3) is read from csrc/prach_tables.inc, and the thresholds from
tests/golden/prach_thresholds.json.
"""
import json
import math
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORMATS = ("0", "1", "2", "3", "A1", "A2", "A3", "B1", "B4", "C0", "C2", "A1/B1", "A2/B2", "A3/B3")
SPACINGS = ("15", "30", "60", "120", "1.25", "5")
FLAGS = ("red", "orange", "green")
SCS_HZ = {"15": 15000, "30": 30000, "60": 60000, "120": 120000, "1.25": 1250, "5": 5000}
NOF_SYMBOLS = dict(zip(FORMATS, (1, 2, 4, 4, 2, 4, 6, 2, 12, 1, 4, 2, 4, 6)))
CP_KAPPA = dict(zip(FORMATS, (3168, 21024, 4688, 3168, 288, 576, 864, 216, 936, 1240, 2048, 288, 576, 864)))
N_CS = {"1.25": (0, 13, 15, 18, 22, 26, 32, 38, 46, 59, 76, 93, 119, 167, 279, 419),
        "5": (0, 13, 26, 33, 38, 41, 49, 55, 64, 76, 93, 119, 139, 209, 279, 419),
        "short": (0, 2, 4, 6, 8, 10, 12, 13, 15, 17, 19, 23, 27, 34, 46, 69)}
T_C = 1.0 / (480000.0 * 4096.0)
MAX_PREAMBLES = 64


def is_long(fmt):
    return FORMATS.index(fmt) < 4


def seq_len(fmt):
    return 839 if is_long(fmt) else 139


def dft_size(fmt):
    return 1024 if is_long(fmt) else 256


def default_scs(fmt):
    return "5" if fmt == "3" else "1.25" if is_long(fmt) else "15"


def n_cs(scs, zcz):
    return N_CS[scs if scs in ("1.25", "5") else "short"][zcz]


_cache = {}


def root_table(L):
    key = ("root", L)
    if key not in _cache:
        text = open(os.path.join(ROOT, "srsran-edgeric-5g_amd", "csrc", "prach_tables.inc")).read()
        body = re.search(r"PRACH_ROOT_%s\[\d+\] = \{([^}]*)\}" % ("LONG" if L == 839 else "SHORT"), text).group(1)
        _cache[key] = [int(x) for x in re.findall(r"\d+", body)]
        assert len(_cache[key]) == L - 1
    return _cache[key]


def thresholds():
    if "th" not in _cache:
        rows = json.load(open(os.path.join(HERE, "golden", "prach_thresholds.json")))
        _cache["th"] = {(r["ports"], r["scs"], r["format"], r["zcz"]): (r["threshold"], r["margin"], r["flag"]) for r in rows}
    return _cache["th"]


def closed_form(L, u):
    """(f, offset) of sequence number u: f = u^-1 mod L; offset = the phase of sum_i x_u(i) on the grid of 4L steps."""
    key = ("cf", L, u)
    if key not in _cache:
        i = np.arange(L, dtype=np.int64)
        y0 = np.exp(-1j * np.pi * ((u * i * (i + 1)) % (2 * L)) / L).sum()
        _cache[key] = (pow(u, -1, L), int(round(np.angle(y0) * 4 * L / (2 * np.pi))) % (4 * L))
    return _cache[key]


def cexp_table(L, dtype):
    key = ("cexp", L, np.dtype(dtype).name)
    if key not in _cache:
        i = np.arange(4 * L)
        if np.dtype(dtype) == np.float32:  # complex_exponential_table: polar(sqrtf(L), float(2 pi) * float(i) / float(4 L))
            f32 = np.float32
            phase = f32(2.0 * np.pi) * i.astype(f32) / f32(4 * L)
            amp = np.sqrt(f32(L))
            _cache[key] = (amp * np.cos(phase) + 1j * (amp * np.sin(phase))).astype(np.complex64)
        else:
            _cache[key] = np.sqrt(float(L)) * np.exp(2j * np.pi * i / (4 * L))
    return _cache[key]


def sequence_of(fmt, scs, root_sequence_index, zcz, preamble_index):
    """(u, C_v) of a preamble, as prach_generator_impl::generate selects them."""
    L = seq_len(fmt)
    ncs = n_cs(scs if is_long(fmt) else "15", zcz)
    root, shift = root_sequence_index + preamble_index, 0
    if ncs != 0:
        per_root = L // ncs
        root = root_sequence_index + preamble_index // per_root
        shift = (preamble_index % per_root) * ncs
    lut = root_table(L)
    return lut[root % len(lut)], shift


def generate_u(L, u, shift, dtype=np.float32):
    """y_{u,v}[n] from the table: index (2 (u f n (f n + 1) + 2 C_v n) + offset) mod 4L."""
    key = ("y", L, u, shift, np.dtype(dtype).name)
    if key not in _cache:
        f, offset = closed_form(L, u)
        n = np.arange(L, dtype=np.int64)  # the largest product is below 2^49
        idx = (2 * (u * f * n * (f * n + 1) + 2 * shift * n) + offset) % (4 * L)
        _cache[key] = cexp_table(L, dtype)[idx]
    return _cache[key]


def generate(fmt, root_sequence_index, zcz, preamble_index, scs=None, dtype=np.float32):
    u, shift = sequence_of(fmt, scs or default_scs(fmt), root_sequence_index, zcz, preamble_index)
    return generate_u(seq_len(fmt), u, shift, dtype)


def generate_by_definition(fmt, root_sequence_index, zcz, preamble_index, scs=None):
    """TS 38.211 6.3.3.1 in double: y = DFT of x_u((i + C_v) mod L), x_u(i) = exp(-j pi u i (i + 1) / L)."""
    L = seq_len(fmt)
    u, shift = sequence_of(fmt, scs or default_scs(fmt), root_sequence_index, zcz, preamble_index)
    i = (np.arange(L, dtype=np.int64) + shift) % L
    x = np.exp(-1j * np.pi * ((u * i * (i + 1)) % (2 * L)) / L)
    return np.fft.fft(x)


def round_to_tc(seconds):
    tc_units = int(seconds / T_C * 10.0)
    return (tc_units // 10 + (tc_units % 10) // 5) * T_C


def derive(cfg):
    """The constants detect() derives (prach_detector_generic_impl.cpp:97-172).  cfg: a dict with format, ra_scs (names),
    root_sequence_index, zero_correlation_zone, start_preamble_index, nof_preamble_indices, nof_rx_ports and, optionally,
    threshold and win_margin (both, or neither: the table's)."""
    fmt, scs = cfg["format"], cfg["ra_scs"]
    L, N, hz = seq_len(fmt), dft_size(fmt), SCS_HZ[scs]
    d = dict(L=L, N=N, nof_symbols=NOF_SYMBOLS[fmt], n_cs=n_cs(scs, cfg["zero_correlation_zone"]))
    d["nof_shifts"], d["nof_sequences"] = 1, 64
    if d["n_cs"] != 0:
        d["nof_shifts"] = min(MAX_PREAMBLES, L // d["n_cs"])
        d["nof_sequences"] = -(-64 // d["nof_shifts"])
    d["sample_rate"] = float(N * hz)
    cp_kappa = CP_KAPPA[fmt] if is_long(fmt) else CP_KAPPA[fmt] >> SPACINGS.index(scs)
    cp_duration = float(cp_kappa * 64) * T_C
    cp_prach = int(math.floor(cp_duration * L * hz))
    win = cp_prach if d["n_cs"] == 0 else min(d["n_cs"], cp_prach)
    d["win_width"] = (win * N) // L
    max_delay = cp_prach if d["n_cs"] == 0 else min(max(d["n_cs"], 1) - 1, cp_prach)
    d["max_delay"] = (max_delay * N) // L
    if cfg.get("win_margin"):
        d["threshold"], d["win_margin"] = float(np.float32(cfg["threshold"])), cfg["win_margin"]
    else:
        th, margin, _ = thresholds()[(cfg["nof_rx_ports"], scs, fmt, cfg["zero_correlation_zone"])]
        d["threshold"], d["win_margin"] = float(np.float32(float(th))), margin
    d["time_resolution"] = round_to_tc(1.0 / d["sample_rate"])
    d["time_advance_max"] = round_to_tc(d["max_delay"] * 0.8 / d["sample_rate"])
    d["window_start"] = [(N - (d["n_cs"] * w * N) // L) % N for w in range(d["nof_shifts"])]
    return d


def is_normal(x):
    return np.isfinite(x) & (np.abs(x) >= np.finfo(x.dtype).tiny)


def detect(cfg, symbols, dtype=np.float64):
    """detect() on symbols [ports][symbols][L].  Returns a dict: rssi_dB, time_resolution, time_advance_max, nof_detected and,
    per preamble index (64 entries; unmonitored ones zero): detected, delay, time_advance, peak, detection_metric, tie (the two
    largest samples of the window are equal), metric (a list of 64 arrays of win_width samples, or None)."""
    import scipy.fft
    d = derive(cfg)
    L, N, ports, nsym = d["L"], d["N"], cfg["nof_rx_ports"], d["nof_symbols"]
    rdt = np.dtype(dtype)
    cdt = np.complex64 if rdt == np.float32 else np.complex128
    x = np.asarray(symbols)[:ports, :nsym, :L].astype(cdt)
    power = (x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2).sum()
    # average_power divides by L, detect() by ports x symbols x L once more.
    rssi = rdt.type(power / L / (ports * nsym * L))
    out = dict(time_resolution=d["time_resolution"], time_advance_max=d["time_advance_max"], nof_detected=0,
               detected=[False] * 64, delay=[0] * 64, time_advance=[0.0] * 64, peak=[0.0] * 64, detection_metric=[0.0] * 64,
               tie=[False] * 64, metric=[None] * 64, derived=d)
    with np.errstate(divide="ignore"):
        out["rssi_dB"] = float(rdt.type(10) * np.log10(rssi))
    # The reference's RSSI is a float whatever `dtype` is, and its early return asks whether that float is normal: an occasion
    # whose RSSI is subnormal in float32 is not searched, although the metric, a ratio, would not mind.
    if not is_normal(np.asarray(np.float32(rssi))):
        return out
    start, end = cfg["start_preamble_index"], cfg["start_preamble_index"] + cfg["nof_preamble_indices"]
    shifts, win, margin = d["nof_shifts"], d["win_width"], d["win_margin"]
    seqs = [s for s in range(d["nof_sequences"]) if s * shifts < end and (s + 1) * shifts > start]
    lut = root_table(L)
    roots = np.stack([generate_u(L, lut[(cfg["root_sequence_index"] + s) % len(lut)], 0, rdt) for s in seqs]).astype(cdt)
    combined = x[:, 0, :].copy()
    for s in range(1, nsym):
        combined = combined + x[:, s, :]
    no_root = combined[None, :, :] * np.conj(roots)[:, None, :]  # [sequence][port][L]
    idft_in = np.zeros(no_root.shape[:2] + (N,), cdt)
    idft_in[..., :L // 2 + 1] = no_root[..., L - (L // 2 + 1):]
    idft_in[..., N - L // 2:] = no_root[..., :L // 2]
    corr = (scipy.fft.ifft(idft_in, axis=-1) * rdt.type(N)).astype(cdt)
    modsq = (corr.real ** 2 + corr.imag ** 2) * (rdt.type(1) / rdt.type(N * L * L))
    ws = np.array(d["window_start"])
    ref_idx = ((ws[:, None] + N - margin) % N + np.arange(2 * margin + win)[None, :]) % N  # [shift][2 margin + win]
    win_idx = ws[:, None] + np.arange(win)[None, :]                                      # [shift][win]
    reference = modsq[:, :, ref_idx].sum(axis=-1, dtype=rdt)                              # [sequence][port][shift]
    window = modsq[:, :, win_idx] * (rdt.type(N) / rdt.type(L))                           # [sequence][port][shift][win]
    num = np.zeros((len(seqs), shifts, win), rdt)
    den = np.zeros((len(seqs), shifts, win), rdt)
    for p in range(ports):
        num = num + window[:, p]
        diff = reference[:, p, :, None] - window[:, p]
        den = den + np.where(is_normal(diff), diff, rdt.type(1e-9))
    with np.errstate(divide="ignore", invalid="ignore"):
        metric = num / np.abs(den)
    th = rdt.type(np.float32(d["threshold"]))
    for si, s in enumerate(seqs):
        for w in range(shifts):
            pre = s * shifts + w
            if pre < start or pre >= end:
                continue
            m = metric[si, w]
            delay = int(np.argmax(m))
            peak = m[delay]
            top = np.sort(m)[-2:] if win > 1 else [peak, -1]
            out["metric"][pre] = m
            out["delay"][pre], out["peak"][pre], out["tie"][pre] = delay, float(peak), bool(top[0] == top[-1]) and win > 1
            out["time_advance"][pre] = round_to_tc(delay / d["sample_rate"])
            out["detection_metric"][pre] = float(peak / th)
            out["detected"][pre] = bool(peak > th and delay < float(np.float32(d["max_delay"])) * 0.8)
    out["nof_detected"] = sum(out["detected"])
    return out


def transmit(cfg, preambles, rng, noise_std=0.0, port_phases=None):
    """A buffer [ports][symbols][L] complex64 for cfg: every (preamble_index, delay in correlation samples, amplitude) of
    `preambles` at `amplitude` per resource element, delayed by the phase ramp exp(-j 2 pi k delay / N), with an independent phase
    per port (random when port_phases is None), the same in every symbol, plus complex noise of standard deviation noise_std."""
    fmt = cfg["format"]
    L, N, ports, nsym = seq_len(fmt), dft_size(fmt), cfg["nof_rx_ports"], NOF_SYMBOLS[fmt]
    k = np.arange(L)
    x = np.zeros((ports, nsym, L), np.complex128)
    for index, delay, amplitude in preambles:
        y = generate(fmt, cfg["root_sequence_index"], cfg["zero_correlation_zone"], index, cfg["ra_scs"], np.float64) / np.sqrt(L)
        ph = rng.uniform(0, 2 * np.pi, ports) if port_phases is None else np.asarray(port_phases)
        x += amplitude * (y * np.exp(-2j * np.pi * k * delay / N))[None, None, :] * np.exp(1j * ph)[:, None, None]
    if noise_std:
        x += noise_std * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)) / np.sqrt(2)
    return x.astype(np.complex64)
