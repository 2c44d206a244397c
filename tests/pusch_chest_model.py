"""NumPy restatement of the PUSCH DM-RS channel estimator (dmrs_pusch_estimator_impl + port_channel_estimator_average_impl with
filter smoothing and CFO compensation, + the PUSCH processor's DC step), in float32 and in the reference's order of operations.

Choices shared with the library, where the reference leaves room: every reduction is summed in float64 and rounded once;
atan2, hypot, cos and sin are evaluated in float64 and rounded once to float32.  Complex products are written out per component
so that no step is fused.  Grids and estimates are raw cbf16 words (uint32, real part in the low half).
"""
import numpy as np

f32 = np.float32
TWOPI = f32(2.0) * f32(np.pi)
PI = f32(np.pi)
SQRT1_2 = f32(np.sqrt(0.5))
TA_WINDOW = 144
NO_DC = 0xFFFFFFFF
RC_FILTER = np.array([-0.0641253, -0.0660711, -0.0611526, -0.0485918, -0.0281126, 0.0000000, 0.0348830, 0.0751249,
                      0.1188406, 0.1637874, 0.2075139, 0.2475302, 0.2814857, 0.3073415, 0.3235207, 0.3290274,
                      0.3235207, 0.3073415, 0.2814857, 0.2475302, 0.2075139, 0.1637874, 0.1188406, 0.0751249,
                      0.0348830, 0.0000000, -0.0281126, -0.0485918, -0.0611526, -0.0660711, -0.0641253], np.float32)


# ---- cbf16 ---------------------------------------------------------------------------------------------------------------
def to_bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)


def to_words(re, im):
    return (to_bf16(re) | (to_bf16(im) << 16)).astype(np.uint32)


def from_words(w):
    w = np.asarray(w, np.uint32)
    return (w << 16).view(np.float32), (w & 0xFFFF0000).view(np.float32)


def to_cbf16(z):
    z = np.asarray(z, np.complex64)
    return to_words(z.real, z.imag)


def from_cbf16(w):
    re, im = from_words(w)
    return (re + 1j * im).astype(np.complex64)


# ---- what the GPU tests of the receive side hand to the library -----------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def as_i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


# ---- sequences and constants -----------------------------------------------------------------------------------------------
def gold(c_init, n):
    """c(0 .. n) of TS 38.211 Section 5.2.1."""
    total = 1600 + n
    x1 = np.zeros(total + 31, np.uint8)
    x2 = np.zeros(total + 31, np.uint8)
    x1[0] = 1
    x2[:31] = (c_init >> np.arange(31)) & 1
    for i in range(0, total, 28):
        k = min(28, total - i)
        x1[i + 31:i + 31 + k] = x1[i + 3:i + 3 + k] ^ x1[i:i + k]
        x2[i + 31:i + 31 + k] = x2[i + 3:i + 3 + k] ^ x2[i + 2:i + 2 + k] ^ x2[i + 1:i + 1 + k] ^ x2[i:i + k]
    return x1[1600:total] ^ x2[1600:total]


def c_init(slot_index, symbol, scrambling_id, n_scid):
    return ((14 * slot_index + symbol + 1) * (2 * scrambling_id + 1) * 2 ** 17 + 2 * scrambling_id + n_scid) % 2 ** 31


def epochs(numerology):
    """initialize_symbol_start_epochs, normal cyclic prefix: start of every symbol of the slot in symbols."""
    out, e = [], 0.0
    for l in range(14):
        cp = (144 >> numerology) + (16 if l == 0 or l == 7 * (1 << numerology) else 0)
        e += cp * (1 << numerology) / 2048.0 + (0.0 if l == 0 else 1.0)
        out.append(f32(e))
    return out


def filter_taps(nof_rb):
    """filter_type(nof_rb, 2)."""
    nof_rb = min(nof_rb, 3)
    nof_out = (nof_rb * 10 + 1) // 2 // 2
    n = 31 // 2 - nof_out * 2
    nof_out = 2 * nof_out + 1
    taps = np.zeros(nof_out, np.float32)
    total = f32(0)
    for i in range(nof_out):
        taps[i] = RC_FILTER[n]
        total = f32(total + taps[i])
        n += 2
    rcp = f32(f32(1) / total)
    return (taps * rcp).astype(np.float32)


def phasor(x):
    x = np.float64(x)
    return f32(np.cos(x)), f32(np.sin(x))


def cmul(ar, ai, br, bi):
    return (ar * br - ai * bi).astype(np.float32), (ar * bi + ai * br).astype(np.float32)


def prbs_of(cfg):
    return [b for b in range(5 * 64) if (cfg.prb_mask[b // 64] >> (b % 64)) & 1]


def pilots(cfg, dmrs_symbol, layer):
    """The DM-RS of one symbol on the allocation's pilot list (6 per PRB), layer 0 or 1."""
    prbs = np.array(prbs_of(cfg))
    c = gold(c_init(cfg.slot_index, dmrs_symbol, cfg.scrambling_id, cfg.n_scid), 12 * (prbs.max() + 1))
    b = (12 * prbs[:, None] + 2 * np.arange(6)).ravel()
    pr = np.where(c[b] == 1, -SQRT1_2, SQRT1_2).astype(np.float32)
    pi = np.where(c[b + 1] == 1, -SQRT1_2, SQRT1_2).astype(np.float32)
    if layer == 1:
        sign = np.where(np.arange(b.size) % 2 == 1, f32(-1), f32(1)).astype(np.float32)
        pr, pi = pr * sign, pi * sign
    return pr, pi, b


# ---- one (receive port, layer) ----------------------------------------------------------------------------------------------
def virtual_pilots(abs_, arg, offset):
    n = len(abs_)
    arg = [f32(a) for a in arg]
    k = f32(0)
    for i in range(n - 1):
        old_a, next_a = arg[i], arg[i + 1]
        arg[i] = f32(arg[i] + f32(f32(2) * k) * PI)
        jump = f32(next_a - old_a)
        if abs(jump) > PI:
            k = f32(k - (f32(-1) if jump < 0 else f32(1)))
    arg[n - 1] = f32(arg[n - 1] + f32(f32(2) * k) * PI)
    nf = f32(n)
    mean_x = f32(f32(f32(n * (n - 1)) / f32(2)) / nf)
    norm_x_sq = f32(f32((n - 1) * n * (2 * n - 1)) / f32(6))
    den = f32(norm_x_sq - f32(f32(nf * mean_x) * mean_x))
    sa = sg = da = dg = f32(0)
    for i in range(n):
        sa = f32(sa + abs_[i])
        sg = f32(sg + arg[i])
        da = f32(da + f32(abs_[i] * f32(i)))
        dg = f32(dg + f32(arg[i] * f32(i)))
    mean_abs, mean_arg = f32(sa / nf), f32(sg / nf)
    slope_abs = f32(f32(da - f32(f32(mean_x * mean_abs) * nf)) / den)
    slope_arg = f32(f32(dg - f32(f32(mean_x * mean_arg) * nf)) / den)
    icp_abs = f32(mean_abs - f32(slope_abs * mean_x))
    icp_arg = f32(mean_arg - f32(slope_arg * mean_x))
    out = []
    for i in range(n):
        x = f32(i + offset)
        r = f32(f32(slope_abs * x) + icp_abs)
        c, s = phasor(f32(f32(slope_arg * x) + icp_arg))
        out.append((f32(r * c), f32(r * s)))
    return out


def interpolate(Fr, Fi):
    """The smoothed pilots (float32) -> cbf16 words of the allocation [2 N]: the reference's running sum of half steps, the last
    element repeated, then cbf16."""
    outs = []
    for F in (Fr, Fi):
        hh = ((F[1:] - F[:-1]) * f32(0.5)).astype(np.float32)
        seq = np.concatenate([F[:1], np.repeat(hh, 2)]).astype(np.float32)
        o = np.cumsum(seq, dtype=np.float32)
        outs.append(np.concatenate([o, F[-1:]]).astype(np.float32))
    return to_words(outs[0], outs[1])


def rotate(row, cfo, epoch):
    """A row of cbf16 words at one symbol: rotated by the CFO's phase at the symbol's start and rounded again (cfo None: as is)."""
    if cfo is None:
        return row
    a, b = from_words(row)
    return to_words(*cmul(a, b, *phasor(f32(f32(TWOPI * epoch) * cfo))))


def estimate_port_layer(cfg, grid, port, layer):
    """Returns (row: interpolated cbf16 words of the allocation [12 nprb], cfo or None, measurements dict)."""
    prbs = prbs_of(cfg)
    nprb = len(prbs)
    N = 6 * nprb
    beta = f32(cfg.scaling)
    ep = epochs(cfg.numerology)
    dmrs = [l for l in range(14) if (cfg.dmrs_symbol_mask >> l) & 1]
    nd = len(dmrs)
    rows = grid[cfg.rx_ports[port]]
    pil = [pilots(cfg, l, layer) for l in dmrs]
    epre = 0.0
    cfo = None
    Ar = Ai = None
    for dd, l in enumerate(dmrs):
        pr, pi, k = pil[dd]
        yr, yi = from_words(rows[l, k])
        epre += float(np.sum((yr * yr + yi * yi).astype(np.float64)))
        lr = (yr * pr + yi * pi).astype(np.float32)
        li = (yi * pr - yr * pi).astype(np.float32)
        if dd == 0:
            Ar, Ai = lr, li
        elif dd == 1:
            dr = float(np.sum((lr * Ar + li * Ai).astype(np.float64)))
            di = float(np.sum((li * Ar - lr * Ai).astype(np.float64)))
            phase = f32(np.arctan2(np.float64(f32(di)), np.float64(f32(dr))))
            cfo = f32(f32(phase / TWOPI) / f32(ep[dmrs[1]] - ep[dmrs[0]]))
            r0 = phasor(f32(f32(-TWOPI * ep[dmrs[0]]) * cfo))
            r1 = phasor(f32(f32(-TWOPI * ep[dmrs[1]]) * cfo))
            ar, ai = cmul(Ar, Ai, *r0)
            br, bi = cmul(lr, li, *r1)
            Ar, Ai = (ar + br).astype(np.float32), (ai + bi).astype(np.float32)
        else:
            r = phasor(f32(f32(-TWOPI * ep[l]) * cfo))
            cr, ci = cmul(lr, li, *r)
            Ar, Ai = (Ar + cr).astype(np.float32), (Ai + ci).astype(np.float32)
    scale = f32(f32(1) / f32(f32(nd) * beta))
    Ar, Ai = (Ar * scale).astype(np.float32), (Ai * scale).astype(np.float32)

    # virtual pilots and the FIR
    taps = filter_taps(nprb)
    T = taps.size
    mid = T // 2
    nv = 6 if nprb == 1 else min(12, T // 2)
    ends = []
    for side in range(2):
        sl = slice(0, nv) if side == 0 else slice(N - nv, N)
        re, im = Ar[sl].astype(np.float64), Ai[sl].astype(np.float64)
        ends.append(virtual_pilots(np.sqrt(re * re + im * im).astype(np.float32), np.arctan2(im, re).astype(np.float32),
                                   -nv if side == 0 else nv))
    Er = np.concatenate([np.array([v[0] for v in ends[0]], np.float32), Ar, np.array([v[0] for v in ends[1]], np.float32)])
    Ei = np.concatenate([np.array([v[1] for v in ends[0]], np.float32), Ai, np.array([v[1] for v in ends[1]], np.float32)])
    Fr = np.zeros(N, np.float32)
    Fi = np.zeros(N, np.float32)
    for i in range(T):
        h = taps[T - 1 - i]
        s = nv - mid + i
        Fr = (Fr + Er[s:s + N] * h).astype(np.float32)
        Fi = (Fi + Ei[s:s + N] * h).astype(np.float32)
    pw = float(np.sum((Fr * Fr + Fi * Fi).astype(np.float64)))
    rsrp = f32(pw * float(beta) * float(beta) / N)

    # noise
    ne = 0.0
    for dd, l in enumerate(dmrs):
        pr, pi, k = pil[dd]
        yr, yi = from_words(rows[l, k])
        er, ei = cmul((Fr * -beta).astype(np.float32), (Fi * -beta).astype(np.float32), pr, pi)
        if nd >= 2:
            er, ei = cmul(er, ei, *phasor(f32(f32(TWOPI * ep[l]) * cfo)))
        er, ei = (er + yr).astype(np.float32), (ei + yi).astype(np.float32)
        ne += float(np.sum((er * er + ei * ei).astype(np.float64)))

    # time alignment
    k = pil[0][2]
    n = np.concatenate([np.arange(TA_WINDOW), 4096 - TA_WINDOW + np.arange(TA_WINDOW)])
    X = np.exp(2j * np.pi * np.outer(n, k) / 4096.0) @ (Fr.astype(np.float64) + 1j * Fi.astype(np.float64))
    mag = np.abs(X) ** 2
    i_d, i_a = int(np.argmax(mag[:TA_WINDOW])), int(np.argmax(mag[TA_WINDOW:]))
    ta_bins = i_d if mag[i_d] >= mag[TA_WINDOW + i_a] else i_a - TA_WINDOW
    top = np.sort(mag)[-2:]
    near_tie = bool(top[1] - top[0] <= 1e-4 * top[1])

    row = interpolate(Fr, Fi)

    epre_f = f32(epre / (N * nd))
    nvar_raw = f32(ne / (N * nd - 1))
    min_noise = f32(rsrp / f32(1e10))
    noise_var = nvar_raw if nvar_raw > min_noise else min_noise
    datarp = f32(f32(rsrp / beta) / beta)
    snr = f32(datarp / noise_var) if noise_var != 0 else f32(1000)
    scs = 15000 << cfg.numerology
    meas = {"noise_var": noise_var, "rsrp": rsrp, "epre": epre_f, "snr": snr, "ta_bins": ta_bins,
            "ta_s": f32(ta_bins / (4096.0 * scs)), "cfo_hz": f32(f32(cfo * f32(scs // 1000)) * f32(1000)) if nd >= 2 else f32(np.nan),
            "ta_near_tie": near_tie, "ta_mag": mag, "smoothed": (Fr + 1j * Fi).astype(np.complex64), "cfo": cfo}
    return row, cfo, meas


def estimate(cfg, grid, ce=None):
    """grid [ports][14][subc] cbf16 words -> (ce [layers][rx][14][subc] words (ce, or zeros, with the allocated region
    written), noise_vars [rx] (layer 0), meas [rx][layers])."""
    L, P = cfg.nof_tx_layers, cfg.nof_rx_ports
    nsubc = grid.shape[-1]
    ce = np.zeros((L, P, 14, nsubc), np.uint32) if ce is None else ce.copy()
    prbs = prbs_of(cfg)
    subc = (12 * np.array(prbs)[:, None] + np.arange(12)).ravel()
    ep = epochs(cfg.numerology)
    meas = [[None] * L for _ in range(P)]
    for p in range(P):
        for l in range(L):
            row, cfo, m = estimate_port_layer(cfg, grid, p, l)
            meas[p][l] = m
            for s in range(cfg.start_symbol_index, cfg.start_symbol_index + cfg.nof_symbols):
                w = rotate(row, cfo, ep[s]).copy()
                if cfg.dc_position != NO_DC:
                    w[subc == cfg.dc_position] = 0
                ce[l, p, s, subc] = w
    noise_vars = np.array([meas[p][0]["noise_var"] for p in range(P)], np.float32)
    return ce, noise_vars, meas
