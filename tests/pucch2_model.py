"""NumPy restatement of the PUCCH format 2 receiver (pucch_processor_impl::process for format2_configuration): the DM-RS of
dmrs_pucch_processor_format2_impl, port_channel_estimator_average_impl::compute with filter smoothing and CFO compensation for
pilots on every third subcarrier, get_channel_state_information, pucch_demodulator_impl::demodulate and the UCI decoder -- in
float32 and in the reference's order of operations, written from reading the reference.  It generalises
pusch_chest_model.estimate_port_layer to stride 3 and offset 1 and shares that module's choices: every reduction is summed in
float64 and rounded once; atan2, hypot, cos, sin and log10 are evaluated in float64 and rounded once.  A float64 variant of the
estimator (dt=np.float64) gives the spectrum the time-alignment checks compare against.  The transmitter at the end builds the
grids the tests receive.

A configuration is a dict with the fields of nrphy_pf2_cfg_t (rx_ports a tuple).  Grids and estimates are raw cbf16 words.
"""
import numpy as np

import uci_model
from pusch_chest_model import RC_FILTER, TA_WINDOW, epochs, from_words, gold, to_words, virtual_pilots

f32 = np.float32
VALID, INVALID = uci_model.STATUS_VALID, uci_model.STATUS_INVALID
QPSK = 2
MAX_CODE_RATE = f32(0.80)
CSI_DTYPE = np.dtype([("sinr_dB", "<f4"), ("rsrp_dB", "<f4"), ("epre_dB", "<f4"), ("time_alignment_s", "<f4"), ("cfo_hz", "<f4"),
                      ("reserved_", "<u4", (3,))])
FIELDS = ("numerology", "slot_index", "bwp_size_rb", "bwp_start_rb", "starting_prb", "nof_prb", "start_symbol_index", "nof_symbols",
          "rnti", "n_id", "n_id_0", "nof_harq_ack", "nof_sr", "nof_csi_part1", "nof_csi_part2")


def make_cfg(starting_prb, nof_prb, nof_symbols, start_symbol_index=0, bwp_start_rb=0, bwp_size_rb=None, numerology=0, slot_index=0,
             rnti=1, n_id=0, n_id_0=0, nof_harq_ack=0, nof_sr=0, nof_csi_part1=0, nof_csi_part2=0, rx_ports=(0,)):
    return dict(numerology=numerology, slot_index=slot_index, bwp_size_rb=275 - bwp_start_rb if bwp_size_rb is None else bwp_size_rb,
                bwp_start_rb=bwp_start_rb, starting_prb=starting_prb, nof_prb=nof_prb, start_symbol_index=start_symbol_index,
                nof_symbols=nof_symbols, rnti=rnti, n_id=n_id, n_id_0=n_id_0, nof_harq_ack=nof_harq_ack, nof_sr=nof_sr,
                nof_csi_part1=nof_csi_part1, nof_csi_part2=nof_csi_part2, rx_ports=tuple(rx_ports))


def from_fixture(f):
    """A configuration of tests/golden/pf2_configs.json (fields the entry does not have keep make_cfg's defaults)."""
    cfg = make_cfg(f["starting_prb"], f["nof_prb"], f["nof_symbols"])
    for k in FIELDS:
        if k in f:
            cfg[k] = f[k]
    cfg["rx_ports"] = tuple(f.get("rx_ports", (0,)))
    return cfg


def to_abi(abi, cfg):
    c = abi.Pf2Cfg()
    for k in FIELDS:
        setattr(c, k, cfg[k])
    c.nof_rx_ports = len(cfg["rx_ports"])
    for i, q in enumerate(cfg["rx_ports"]):
        c.rx_ports[i] = q
    return c


def payload_bits(cfg):
    return cfg["nof_harq_ack"] + cfg["nof_sr"] + cfg["nof_csi_part1"] + cfg["nof_csi_part2"]


def nof_llr(cfg):
    return 16 * cfg["nof_prb"] * cfg["nof_symbols"]


def code_rate(cfg):
    """pucch_format2_code_rate, in float32."""
    A, E = payload_bits(cfg), nof_llr(cfg)
    crc = uci_model.nof_codeblocks(A, E) * uci_model.crc_size(A)
    return f32(f32(A + crc) / f32(E))


def validate(cfg, grid_nof_ports, grid_nof_subc):
    """What nrphy_pf2_validate accepts."""
    ports = cfg["rx_ports"]
    A = payload_bits(cfg)
    return bool(cfg["numerology"] <= 4 and cfg["slot_index"] < (10 << cfg["numerology"]) and cfg["rnti"] <= 65535 and
                cfg["n_id"] <= 1023 and cfg["n_id_0"] <= 65535 and
                cfg["bwp_start_rb"] + cfg["bwp_size_rb"] <= min(grid_nof_subc // 12, 275) and
                1 <= cfg["nof_prb"] <= 16 and cfg["starting_prb"] + cfg["nof_prb"] <= cfg["bwp_size_rb"] and
                1 <= cfg["nof_symbols"] <= 2 and cfg["start_symbol_index"] + cfg["nof_symbols"] <= 14 and
                cfg["nof_csi_part2"] == 0 and 3 <= A <= 1706 and not code_rate(cfg) > MAX_CODE_RATE and
                uci_model.validate(A, nof_llr(cfg), QPSK) and 1 <= len(ports) <= 4 and len(set(ports)) == len(ports) and
                all(q < grid_nof_ports for q in ports))


# ---- DM-RS, data positions, constants ---------------------------------------------------------------------------------------
def dmrs_c_init(cfg, symbol):
    """dmrs_pucch_processor_format2_impl::c_init (a product beyond 32 bits: Python integers)."""
    n_id = cfg["n_id_0"]
    return ((14 * cfg["slot_index"] + symbol + 1) * (2 * n_id + 1) * 2 ** 17 + 2 * n_id) % 2 ** 31


def first_prb(cfg):
    return cfg["bwp_start_rb"] + cfg["starting_prb"]


def pilot_subcarriers(cfg):
    """Grid subcarriers of the pilots: 1, 4, 7 and 10 of every PRB."""
    return 12 * first_prb(cfg) + 3 * np.arange(4 * cfg["nof_prb"]) + 1


def data_subcarriers(cfg):
    """Grid subcarriers of the data REs of one symbol, ascending: those with k mod 3 != 1."""
    k = np.arange(12 * cfg["nof_prb"])
    return 12 * first_prb(cfg) + k[k % 3 != 1]


def pilots(cfg, symbol, dt=np.float32):
    """The DM-RS of one symbol: the sequence advanced by 2 x 4 x first PRB bits, QPSK of amplitude sqrt(1/2), real part first."""
    n = 4 * cfg["nof_prb"]
    skip = 8 * first_prb(cfg)
    c = gold(dmrs_c_init(cfg, symbol), skip + 2 * n)[skip:]
    a = dt(f32(np.sqrt(0.5))) if dt == np.float32 else dt(np.sqrt(0.5))
    return np.where(c[0::2] == 1, -a, a).astype(dt), np.where(c[1::2] == 1, -a, a).astype(dt)


def filter_taps(nof_rb, stride=3):
    """filter_type(nof_rb, stride)."""
    nof_rb = min(nof_rb, 3)
    nof_out = (nof_rb * 10 + 1) // 2 // stride
    n = 31 // 2 - nof_out * stride
    nof_out = 2 * nof_out + 1
    taps = np.zeros(nof_out, np.float32)
    total = f32(0)
    for i in range(nof_out):
        taps[i] = RC_FILTER[n]
        total = f32(total + taps[i])
        n += stride
    return (taps * f32(f32(1) / total)).astype(np.float32)


def nof_virtual_pilots(nof_rb, ntaps):
    return 4 if nof_rb == 1 else min(12, ntaps // 2)


def _twopi(dt):
    return f32(2.0) * f32(np.pi) if dt == np.float32 else dt(2 * np.pi)


def _phasor(x, dt):
    x = np.float64(x)
    return dt(np.cos(x)), dt(np.sin(x))


def _cmul(ar, ai, br, bi, dt):
    return (ar * br - ai * bi).astype(dt), (ar * bi + ai * br).astype(dt)


def _virtual_pilots(abs_, arg, offset, dt):
    """compute_v_pilots; the float32 form is pusch_chest_model's."""
    if dt == np.float32:
        return virtual_pilots(abs_.astype(np.float32), arg.astype(np.float32), offset)
    n = len(abs_)
    arg = np.unwrap(np.asarray(arg, np.float64))
    x = np.arange(n, dtype=np.float64)
    sa, ia = np.polyfit(x, np.asarray(abs_, np.float64), 1)
    sg, ig = np.polyfit(x, arg, 1)
    return [((sa * (i + offset) + ia) * np.cos(sg * (i + offset) + ig), (sa * (i + offset) + ia) * np.sin(sg * (i + offset) + ig))
            for i in range(n)]


def _db(v, dt=np.float32):
    """convert_power_to_dB."""
    with np.errstate(all="ignore"):
        return dt(dt(10) * dt(np.log10(np.float64(v))))


# ---- one receive port ---------------------------------------------------------------------------------------------------------
def estimate_port(cfg, grid, port, dt=np.float32):
    """Returns (rows: the estimate of every symbol of the allocation as cbf16 words [nof_symbols][12 nof_prb], measurements)."""
    nprb, ns = cfg["nof_prb"], cfg["nof_symbols"]
    N = 4 * nprb
    ep = [dt(e) for e in epochs(cfg["numerology"])]
    syms = [cfg["start_symbol_index"] + l for l in range(ns)]
    rows = grid[cfg["rx_ports"][port]]
    k = pilot_subcarriers(cfg)
    twopi = _twopi(dt)
    pil = [pilots(cfg, l, dt) for l in syms]
    rx = []
    for l in syms:
        yr, yi = from_words(rows[l, k])
        rx.append((yr.astype(dt), yi.astype(dt)))
    epre = 0.0
    ls = []
    for (pr, pi), (yr, yi) in zip(pil, rx):
        epre += float(np.sum((yr * yr + yi * yi).astype(dt).astype(np.float64)))
        ls.append(((yr * pr + yi * pi).astype(dt), (yi * pr - yr * pi).astype(dt)))
    Ar, Ai = ls[0]
    cfo = None
    if ns == 2:
        lr, li = ls[1]
        dr = float(np.sum((lr * Ar + li * Ai).astype(dt).astype(np.float64)))
        di = float(np.sum((li * Ar - lr * Ai).astype(dt).astype(np.float64)))
        phase = dt(np.arctan2(np.float64(dt(di)), np.float64(dt(dr))))
        cfo = dt(dt(phase / twopi) / dt(ep[syms[1]] - ep[syms[0]]))
        ar, ai = _cmul(Ar, Ai, *_phasor(dt(dt(-twopi * ep[syms[0]]) * cfo), dt), dt)
        br, bi = _cmul(lr, li, *_phasor(dt(dt(-twopi * ep[syms[1]]) * cfo), dt), dt)
        Ar, Ai = (ar + br).astype(dt), (ai + bi).astype(dt)
    scale = dt(dt(1) / dt(dt(ns) * dt(1)))
    Ar, Ai = (Ar * scale).astype(dt), (Ai * scale).astype(dt)

    # virtual pilots and the FIR
    taps = filter_taps(nprb).astype(dt)
    T = taps.size
    mid = T // 2
    nv = nof_virtual_pilots(nprb, T)
    ends = []
    for side in range(2):
        sl = slice(0, nv) if side == 0 else slice(N - nv, N)
        re, im = Ar[sl].astype(np.float64), Ai[sl].astype(np.float64)
        ends.append(_virtual_pilots(np.sqrt(re * re + im * im).astype(dt), np.arctan2(im, re).astype(dt), -nv if side == 0 else nv, dt))
    Er = np.concatenate([np.array([v[0] for v in ends[0]], dt), Ar, np.array([v[0] for v in ends[1]], dt)])
    Ei = np.concatenate([np.array([v[1] for v in ends[0]], dt), Ai, np.array([v[1] for v in ends[1]], dt)])
    Fr = np.zeros(N, dt)
    Fi = np.zeros(N, dt)
    for i in range(T):
        h = taps[T - 1 - i]
        s = nv - mid + i
        Fr = (Fr + (Er[s:s + N] * h).astype(dt)).astype(dt)
        Fi = (Fi + (Ei[s:s + N] * h).astype(dt)).astype(dt)
    pw = float(np.sum((Fr * Fr + Fi * Fi).astype(dt).astype(np.float64)))
    rsrp = dt(pw / N)

    # noise
    ne = 0.0
    for (pr, pi), (yr, yi), l in zip(pil, rx, syms):
        er, ei = _cmul((Fr * dt(-1)).astype(dt), (Fi * dt(-1)).astype(dt), pr, pi, dt)
        if ns == 2:
            er, ei = _cmul(er, ei, *_phasor(dt(dt(twopi * ep[l]) * cfo), dt), dt)
        er, ei = (er + yr).astype(dt), (ei + yi).astype(dt)
        ne += float(np.sum((er * er + ei * ei).astype(dt).astype(np.float64)))

    # time alignment: the pilots at their grid subcarriers
    n = np.concatenate([np.arange(TA_WINDOW), 4096 - TA_WINDOW + np.arange(TA_WINDOW)])
    X = np.exp(2j * np.pi * np.outer(n, k) / 4096.0) @ (Fr.astype(np.float64) + 1j * Fi.astype(np.float64))
    mag = np.abs(X) ** 2
    i_d, i_a = int(np.argmax(mag[:TA_WINDOW])), int(np.argmax(mag[TA_WINDOW:]))
    ta_bins = i_d if mag[i_d] >= mag[TA_WINDOW + i_a] else i_a - TA_WINDOW

    # interpolation, offset 1 and stride 3: the first two outputs hold pilot 0, a running sum of (next - this) / 3 carries on from
    # the accumulated value, the last output holds the last pilot; then cbf16
    outs = []
    for F in (Fr, Fi):
        jump = ((F[1:] - F[:-1]).astype(dt) / dt(3)).astype(dt)
        o = np.cumsum(np.concatenate([F[:1], np.repeat(jump, 3)]).astype(dt), dtype=dt)
        outs.append(np.concatenate([F[:1], o, F[-1:]]).astype(dt))
    base = to_words(outs[0].astype(np.float32), outs[1].astype(np.float32))
    est = []
    for l in syms:
        w = base
        if cfo is not None:
            a, b = from_words(base)
            w = to_words(*[v.astype(np.float32) for v in _cmul(a.astype(dt), b.astype(dt), *_phasor(dt(dt(twopi * ep[l]) * cfo), dt), dt)])
        est.append(w)

    epre_f = dt(epre / (N * ns))
    nvar_raw = dt(ne / (N * ns - 1))
    min_noise = dt(rsrp / dt(1e10))
    noise_var = nvar_raw if nvar_raw > min_noise else min_noise
    with np.errstate(all="ignore"):
        snr = dt(rsrp / noise_var) if noise_var != 0 else dt(1000)
    scs = 15000 << cfg["numerology"]
    meas = {"noise_var": noise_var, "rsrp": rsrp, "epre": epre_f, "snr": snr, "ta_bins": ta_bins, "ta_s": dt(ta_bins / (4096.0 * scs)),
            "cfo_hz": dt(dt(cfo * dt(scs // 1000)) * dt(1000)) if ns == 2 else dt(np.nan), "ta_mag": mag, "smoothed": Fr + 1j * Fi}
    return np.stack(est), meas


def estimate(cfg, grid, dt=np.float32):
    """grid [ports][14][subc] words -> (est [rx][nof_symbols][12 nof_prb] words, meas [rx])."""
    out = [estimate_port(cfg, grid, p, dt) for p in range(len(cfg["rx_ports"]))]
    return np.stack([e for e, _ in out]), [m for _, m in out]


def ta_bin_index(ta_bins):
    """Index into ta_mag of a signed bin."""
    return ta_bins if ta_bins >= 0 else 2 * TA_WINDOW + ta_bins


def channel_state_information(meas, dt=np.float32):
    """channel_estimate::get_channel_state_information -> CSI_DTYPE record."""
    epre = rsrp = noise = dt(0)
    best, best_snr = 0, dt(0)
    for p, m in enumerate(meas):
        epre, rsrp, noise = dt(epre + m["epre"]), dt(rsrp + m["rsrp"]), dt(noise + m["noise_var"])
        if m["snr"] > best_snr:
            best, best_snr = p, m["snr"]
    n = dt(len(meas))
    tiny, big = np.finfo(np.float32).tiny, np.finfo(np.float32).max
    sinr = dt(rsrp / noise) if tiny <= abs(noise) <= big else dt(1e6)
    out = np.zeros((), CSI_DTYPE)
    out["sinr_dB"], out["rsrp_dB"], out["epre_dB"] = _db(sinr, dt), _db(dt(rsrp / n), dt), _db(dt(epre / n), dt)
    out["time_alignment_s"], out["cfo_hz"] = meas[best]["ta_s"], meas[best]["cfo_hz"]
    return out, best


# ---- demodulator ----------------------------------------------------------------------------------------------------------------
def isnormal(x):
    a = np.abs(x)
    return (a >= np.finfo(np.float32).tiny) & (a <= np.finfo(np.float32).max)


def ref_equalize(rx, ch, noise_vars, tx_scaling=1.0):
    """ZF over the ports for one layer: rx [port][re], ch [port][re] (cbf16 words), noise_vars [port] -> (eq [re] complex64, nv [re]
    f32).  equalize_zf_1xn.h after the port reduction of channel_equalizer_generic_impl.cpp, every operation rounded to float32 as
    written (the single-layer branch of test_pusch_demodulator.ref_equalize)."""
    s = f32(tx_scaling)
    P, N = rx.shape
    nv = np.asarray(noise_vars, np.float32)
    eq = np.zeros(N, np.complex64)
    ev = np.full(N, np.inf, np.float32)
    msq, nacc, ar, ai = (np.zeros(N, np.float32) for _ in range(4))
    with np.errstate(all="ignore"):
        for i in range(P):
            a, b = from_words(rx[i])
            c, d = from_words(ch[i])
            n = c * c + d * d
            ok = isnormal(n) & bool(isnormal(nv[i])) & bool(nv[i] > 0)
            msq = np.where(ok, msq + n, msq)
            nacc = np.where(ok, nacc + n * nv[i], nacc)
            ar = np.where(ok, ar + (a * c + b * d), ar)
            ai = np.where(ok, ai + (b * c - a * d), ai)
        dp = s * msq
        good = isnormal(dp) & isnormal(nacc)
        rcp = f32(1) / dp
        eq[good] = (ar * rcp + 1j * (ai * rcp))[good]
        ev[good] = ((nacc * rcp) * rcp)[good]
    return eq, ev


def data_res(cfg, grid, est):
    """(rx [port][re], ch [port][re]) of the data REs, symbol by symbol, subcarriers ascending."""
    k = data_subcarriers(cfg)
    kk = k - 12 * first_prb(cfg)
    rx = np.stack([np.concatenate([grid[q, cfg["start_symbol_index"] + l, k] for l in range(cfg["nof_symbols"])]) for q in cfg["rx_ports"]])
    ch = np.stack([np.concatenate([est[p, l, kk] for l in range(cfg["nof_symbols"])]) for p in range(len(cfg["rx_ports"]))])
    return rx, ch


def descramble(cfg, llr):
    c = gold((cfg["rnti"] << 15) + cfg["n_id"], llr.size)
    return np.where(c == 1, -llr.astype(np.int16), llr.astype(np.int16)).astype(np.int8)


def demodulate(cfg, grid, est, noise_vars, oracle):
    """pucch_demodulator_impl::demodulate from an estimate [rx][nof_symbols][12 nof_prb] and the ports' noise variances; the QPSK
    demapper is the C oracle's, which is pinned to the compiled reference."""
    rx, ch = data_res(cfg, grid, est)
    eq, ev = ref_equalize(rx, ch, noise_vars)
    return descramble(cfg, oracle.demodulate_soft(QPSK, eq, ev))


def process(cfg, grid, oracle, fill=0):
    """The whole receiver: dict of message, status, csi, meas, est, llr."""
    est, meas = estimate(cfg, grid)
    llr = demodulate(cfg, grid, est, [m["noise_var"] for m in meas], oracle)
    message, status = uci_model.decode(llr, payload_bits(cfg), QPSK, fill)
    csi, best = channel_state_information(meas)
    return {"message": message, "status": status, "csi": csi, "best_port": best, "meas": meas, "est": est, "llr": llr}


# ---- transmitter and channel ------------------------------------------------------------------------------------------------------
def transmit(cfg, message):
    """uci_model.encode -> scramble -> QPSK on the data REs, DM-RS on the pilots: [(symbol, grid subcarriers, values), ...]."""
    E = nof_llr(cfg)
    cw = np.asarray(uci_model.encode(np.asarray(message, np.uint8), E, QPSK), np.uint8)
    b = cw ^ gold((cfg["rnti"] << 15) + cfg["n_id"], E)
    a = np.sqrt(0.5)
    x = a * ((1 - 2.0 * b[0::2]) + 1j * (1 - 2.0 * b[1::2]))
    kd, kp = data_subcarriers(cfg), pilot_subcarriers(cfg)
    out = []
    for l in range(cfg["nof_symbols"]):
        s = cfg["start_symbol_index"] + l
        pr, pi = pilots(cfg, s, np.float64)
        out.append((s, kd, x[l * kd.size:(l + 1) * kd.size]))
        out.append((s, kp, pr + 1j * pi))
    return out


def add_to_grid(grid, res, gains, delay=0.0, cfo=0.0, numerology=0):
    """Adds the transmission to grid [ports][14][subc] (complex): per port a gain, a delay in samples of a 4096-point transform
    and a CFO normalised to the subcarrier spacing (a phase per symbol at its start epoch)."""
    ep = epochs(numerology)
    for s, k, v in res:
        for p, g in enumerate(gains):
            grid[p, s, k] += g * v * np.exp(-2j * np.pi * delay * k / 4096.0) * np.exp(2j * np.pi * cfo * float(ep[s]))
    return grid


def quantize(grid):
    """Complex grid -> cbf16 words."""
    return to_words(grid.real.astype(np.float32), grid.imag.astype(np.float32))


def received_grid(rng, cfg, message, nof_ports, nof_subc, snr_db=None, delay=0.0, cfo=0.0, taps=1, fill=None):
    """A seeded received grid: per grid port a random gain (and, with taps > 1, further delayed paths), delay, CFO and AWGN at
    snr_db relative to a unit-power transmission (None: no noise).  fill: a grid to add to (other users of the slot)."""
    grid = np.zeros((nof_ports, 14, nof_subc), complex) if fill is None else fill
    res = transmit(cfg, message)
    for t in range(taps):
        gains = [(0.6 + 0.8 * rng.random()) * np.exp(2j * np.pi * rng.random()) * (0.5 ** t) for _ in range(nof_ports)]
        add_to_grid(grid, res, gains, delay=delay + 2.5 * t, cfo=cfo, numerology=cfg["numerology"])
    if snr_db is not None:
        sigma = np.sqrt(0.5 * 10 ** (-snr_db / 10))
        grid = grid + sigma * (rng.standard_normal(grid.shape) + 1j * rng.standard_normal(grid.shape))
    return grid
