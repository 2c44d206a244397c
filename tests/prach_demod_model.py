"""NumPy restatement of the OFDM PRACH demodulator (ofdm_prach_demodulator_impl::demodulate): window arithmetic in integer units
of kappa (64 T_c, one sample at 30.72 MHz), np.fft.fft in float64, bin selection.  A configuration is a dict with srate_hz,
format (name), nof_td_occasions, nof_fd_occasions, start_symbol, rb_offset, nof_prb_ul_grid, pusch_numerology and nof_rx_ports.
Also the integer generator of the recorded inputs (tests/golden/record_prach_demod_reference.cpp states the same one)."""
import numpy as np

FORMATS = ("0", "1", "2", "3", "A1", "A2", "A3", "B1", "B4", "C0", "C2", "A1/B1", "A2/B2", "A3/B3")
KAPPA_HZ = 30720000  # kappa units per second
HALF_MS = 15360      # 0.5 ms in kappa
DFT_SIZES = (128, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096, 4608, 6144, 9216, 12288, 18432, 24576, 36864, 49152)
# TS 38.211 Table 6.3.3.1-1: symbols, cyclic prefix in kappa, spacing in Hz.
LONG = {"0": (1, 3168, 1250), "1": (2, 21024, 1250), "2": (4, 4688, 1250), "3": (4, 3168, 5000)}
# Table 6.3.3.1-2 at 15 kHz: symbols, cyclic prefix in kappa (of the last occasion too), duration in PUSCH symbols.
SHORT = {"A1": (2, 288, 288, 2), "A2": (4, 576, 576, 4), "A3": (6, 864, 864, 6), "B1": (2, 216, 216, 2), "B4": (12, 936, 936, 12),
         "C0": (1, 1240, 1240, 2), "C2": (4, 2048, 2048, 6), "A1/B1": (2, 288, 216, 2), "A2/B2": (4, 576, 360, 4),
         "A3/B3": (6, 864, 504, 6)}
# Table 6.3.3.2-1: (PRACH spacing in Hz, PUSCH numerology) -> (N_RB^RA, k_bar); what is missing is reserved.
MAPPING = {(1250, 0): (6, 7), (1250, 1): (3, 1), (1250, 2): (2, 133), (5000, 0): (24, 12), (5000, 1): (12, 10), (5000, 2): (6, 7),
           (15000, 0): (12, 2), (15000, 1): (6, 2), (15000, 2): (3, 2), (30000, 0): (24, 2), (30000, 1): (12, 2), (30000, 2): (6, 2),
           (60000, 2): (12, 2), (60000, 3): (6, 2), (120000, 2): (24, 2), (120000, 3): (12, 2)}


def is_long(fmt):
    return fmt in LONG


def preamble_info(fmt, mu, last):
    """L_RA, spacing in Hz, symbols, cyclic prefix and length of the symbols in kappa, duration in PUSCH symbols."""
    if is_long(fmt):
        nsym, cp, hz = LONG[fmt]
        return dict(L=839, ra_scs_hz=hz, nof_symbols=nsym, cp_kappa=cp, symbols_kappa=nsym * KAPPA_HZ // hz, duration=0)
    nsym, cp, cp_last, duration = SHORT[fmt]
    return dict(L=139, ra_scs_hz=15000 << mu, nof_symbols=nsym, cp_kappa=(cp_last if last else cp) >> mu,
                symbols_kappa=nsym * (2048 >> mu), duration=duration)


def slot_start(kappa):
    """Sixteen kappa more after time 0, and again after 0.5 ms."""
    if kappa > 0:
        kappa += 16
    if kappa > HALF_MS:
        kappa += 16
    return kappa


def window_kappa(fmt, mu, start_symbol, nof_td_occasions):
    """get_prach_window_duration."""
    if is_long(fmt):
        info = preamble_info(fmt, 0, False)
        end = slot_start(2192 * start_symbol) + info["cp_kappa"] + info["symbols_kappa"]
        return (end + 30719) // 30720 * 30720  # up to a whole millisecond
    symbol = 2192 >> mu
    start = slot_start(symbol * start_symbol)
    end = start + symbol * preamble_info(fmt, mu, False)["duration"] * nof_td_occasions
    if start <= 0 <= end:
        end += 16
    if start <= HALF_MS < end:
        end += 16
    return end


def occasions(cfg):
    """Per time-domain occasion: start, cyclic prefix and length in kappa, as the reference derives them."""
    fmt, mu, out = cfg["format"], cfg["pusch_numerology"], []
    for td in range(cfg["nof_td_occasions"]):
        info = preamble_info(fmt, mu, td == cfg["nof_td_occasions"] - 1)
        start = slot_start((2192 >> mu) * (cfg["start_symbol"] + info["duration"] * td))
        cp, end = info["cp_kappa"], start + info["cp_kappa"] + info["symbols_kappa"]
        if not is_long(fmt):
            if start <= 0 <= end:
                cp += 16
            if start <= HALF_MS <= end:
                cp += 16
        out.append(dict(start=start, cp=cp, length=cp + info["symbols_kappa"]))
    return out


def derive(cfg):
    """Everything the plan precomputes, or None where the configuration is refused."""
    fmt, mu, srate = cfg["format"], cfg["pusch_numerology"], cfg["srate_hz"]
    if fmt not in FORMATS or not 0 <= mu <= 3 or not 1 <= cfg["nof_rx_ports"] <= 4 or not 1 <= cfg["nof_prb_ul_grid"] <= 275:
        return None
    ntd, nfd = cfg["nof_td_occasions"], cfg["nof_fd_occasions"]
    if not 1 <= nfd <= 8 or ntd < 1 or cfg["start_symbol"] > 13 or cfg["rb_offset"] >= 275:
        return None
    info = preamble_info(fmt, mu, False)
    if is_long(fmt) and ntd != 1:
        return None
    if not is_long(fmt) and cfg["start_symbol"] + info["duration"] * ntd > 14:
        return None
    if (info["ra_scs_hz"], mu) not in MAPPING:
        return None
    nof_rb_ra, k_bar = MAPPING[(info["ra_scs_hz"], mu)]
    if srate <= 0 or srate % info["ra_scs_hz"] != 0 or srate // info["ra_scs_hz"] not in DFT_SIZES:
        return None
    dft_size = srate // info["ra_scs_hz"]
    K = (15000 << mu) // info["ra_scs_hz"]
    grid = cfg["nof_prb_ul_grid"] * K * 12
    if dft_size <= grid:
        return None
    k_start = [K * 12 * (cfg["rb_offset"] + nof_rb_ra * fd) + k_bar for fd in range(nfd)]
    if k_start[-1] + info["L"] >= grid:
        return None
    occ = occasions(cfg)
    times = [v for o in occ for v in (o["start"], o["cp"], o["length"])]
    if not is_long(fmt):
        times.append(window_kappa(fmt, mu, cfg["start_symbol"], ntd))
    if any((t * srate) % KAPPA_HZ != 0 for t in times):
        return None

    def samples(kappa):
        return kappa * srate // KAPPA_HZ

    window = max(samples(o["start"] + o["length"]) for o in occ)
    if not is_long(fmt):
        window = max(window, samples(window_kappa(fmt, mu, cfg["start_symbol"], ntd)))
    return dict(L=info["L"], nof_symbols=info["nof_symbols"], dft_size=dft_size, grid=grid, k_start=k_start,
                first_bin=[(k - grid // 2) % dft_size for k in k_start],
                symbol_offset=[samples(o["start"]) + samples(o["cp"]) for o in occ], window_samples=window)


def validate(cfg):
    return derive(cfg) is not None


def sizes(cfg):
    d = derive(cfg)
    return None if d is None else (d["dft_size"], d["L"], d["nof_symbols"], d["window_samples"])


def demodulate(cfg, x):
    """x: the samples of one port -> [td][fd][symbol][L_RA] complex128 (an unnormalised direct transform, no correction)."""
    d = derive(cfg)
    N, L = d["dft_size"], d["L"]
    out = np.zeros((cfg["nof_td_occasions"], cfg["nof_fd_occasions"], d["nof_symbols"], L), np.complex128)
    for td, offset in enumerate(d["symbol_offset"]):
        for s in range(d["nof_symbols"]):
            X = np.fft.fft(np.asarray(x[offset + N * s:offset + N * (s + 1)], np.complex128))
            for fd, b in enumerate(d["first_bin"]):
                out[td, fd, s] = X[(b + np.arange(L)) % N]
    return out


def modulate(cfg, td, fd, sequence, delay=0):
    """The reverse, for the tests: `sequence` [L_RA] on the subcarriers of occasion (td, fd), an inverse transform scaled to unit
    gain through demodulate(), repeated over the occasion's symbols behind its cyclic prefix and delayed by `delay` samples (the
    prefix covers the delay).  Returns (first sample of the occasion, the occasion's samples)."""
    d = derive(cfg)
    N, L = d["dft_size"], d["L"]
    occ = occasions(cfg)[td]
    start, cp = (v * cfg["srate_hz"] // KAPPA_HZ for v in (occ["start"], occ["cp"]))
    X = np.zeros(N, np.complex128)
    X[(d["first_bin"][fd] + np.arange(L)) % N] = sequence
    symbol = np.fft.ifft(X)
    return start, symbol[(np.arange(cp + d["nof_symbols"] * N) - cp - delay) % N]


# ---- the recorded inputs ------------------------------------------------------------------------------------------------------
LCG_A, LCG_C = 6364136223846793005, 1442695040888963407
MASK = (1 << 64) - 1


def lcg_values(case_index, n):
    """n float32 values of case `case_index`: x <- A x + C mod 2^64 from x0 = (case + 1) * 0x9E3779B97F4A7C15; bits 40..63 of every
    step, v, as (v - 2^23) / 2^23.  x_i = A^i x0 + C (1 + A + ... + A^(i-1)), with uint64 wrap-around for the modulus."""
    x0 = ((case_index + 1) * 0x9E3779B97F4A7C15) & MASK
    with np.errstate(over="ignore"):
        powers = np.cumprod(np.full(n, LCG_A, np.uint64))              # A^1 ... A^n
        sums = np.cumsum(np.concatenate([[np.uint64(1)], powers[:-1]]), dtype=np.uint64)  # 1 + ... + A^(i-1), i = 1 ... n
        x = powers * np.uint64(x0) + np.uint64(LCG_C) * sums
    v = (x >> np.uint64(40)).astype(np.int64)
    return ((v - (1 << 23)) / float(1 << 23)).astype(np.float32)


def lcg_samples(case_index, n):
    v = lcg_values(case_index, 2 * n)
    return (v[0::2] + 1j * v[1::2]).astype(np.complex64)
