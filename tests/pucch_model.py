"""NumPy restatement of the PUCCH format 0 and format 1 processors (pucch_processor_impl::process: pucch_detector_format0,
dmrs_pucch_processor_format1_impl on port_channel_estimator_average_impl with the `mean` smoothing strategy and CFO compensation
off, pucch_detector_format1, channel_estimate::get_channel_state_information), in the reference's order of operations, and a
format 0 / format 1 transmitter per TS 38.211 Sections 6.3.2.3 and 6.3.2.4 to build grids.

process(cfg, grid, np.float32) is the restatement in the reference's arithmetic; process(cfg, grid, np.float64) runs the same
steps in double precision (the cbf16 rounding of the estimate stays: it is a step of the algorithm, not an error of the arithmetic).
Choices shared with the library and with pusch_chest_model.py: every reduction is summed in float64 and rounded once; atan2,
log10, cos and sin are evaluated in float64 and rounded once.  Complex products are written out per component so that no step is
fused.  Grids and estimates are raw cbf16 words (uint32, real part in the low half).

A configuration is a dict: format, numerology, slot_index, bwp_start_rb, bwp_size_rb, starting_prb, second_hop_prb (None: no
hopping), start_symbol_index, nof_symbols, initial_cyclic_shift, time_domain_occ, n_id, nof_harq_ack, sr_opportunity, ports.
"""
import functools
import json
import os

import numpy as np

from pusch_chest_model import epochs, from_words, gold, to_words

UNKNOWN, VALID, INVALID = 0, 1, 2
THRESHOLD = 4.0
_TABLES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pucch_tables.json")))
PHI_12 = _TABLES["phi_12"]     # TS 38.211 Table 5.2.2.2-2
OCC_PHI = _TABLES["occ_phi"]   # TS 38.211 Table 6.3.2.4.1-2, [N - 1][i][m]

# pucch_detector_format0.cpp:42-64: (m_cs, sr, ack bits) in the order the detector walks them.
FORMAT0_TABLES = {
    (0, True): [(0, 1, [])],
    (1, False): [(0, None, [0]), (6, None, [1])],
    (2, False): [(0, None, [0, 0]), (3, None, [0, 1]), (6, None, [1, 1]), (9, None, [1, 0])],
    (1, True): [(0, 0, [0]), (6, 0, [1]), (3, 1, [0]), (9, 1, [1])],
    (2, True): [(0, 0, [0, 0]), (3, 0, [0, 1]), (6, 0, [1, 1]), (9, 0, [1, 0]), (1, 1, [0, 0]), (4, 1, [0, 1]), (7, 1, [1, 1]),
                (10, 1, [1, 0])],
}


def make_cfg(format, starting_prb, nof_symbols, start_symbol_index=0, second_hop_prb=None, bwp_start_rb=0, bwp_size_rb=None,
             numerology=0, slot_index=0, initial_cyclic_shift=0, time_domain_occ=0, n_id=0, nof_harq_ack=1, sr_opportunity=False,
             ports=(0,)):
    return dict(format=format, numerology=numerology, slot_index=slot_index, bwp_start_rb=bwp_start_rb,
                bwp_size_rb=275 - bwp_start_rb if bwp_size_rb is None else bwp_size_rb, starting_prb=starting_prb,
                second_hop_prb=second_hop_prb, start_symbol_index=start_symbol_index, nof_symbols=nof_symbols,
                initial_cyclic_shift=initial_cyclic_shift, time_domain_occ=time_domain_occ, n_id=n_id, nof_harq_ack=nof_harq_ack,
                sr_opportunity=bool(sr_opportunity), ports=list(ports))


def from_fixture(f):
    """An entry of tests/golden/pucch_configs.json as a configuration (slot_count = sfn * slots per frame + slot)."""
    return make_cfg(f["format"], f["starting_prb"], f["nof_symbols"], f["start_symbol_index"], f["second_hop_prb"], f["bwp_start_rb"],
                    f["bwp_size_rb"], f["numerology"], f["slot_count"] % (10 << f["numerology"]), f["initial_cyclic_shift"],
                    f.get("time_domain_occ", 0), f["n_id"], f["nof_harq_ack"], f.get("sr_opportunity", False), f["ports"])


# nrphy_pucch_result_t as a NumPy record (what the tests and profiles/pucch_bench.py read device results through).
RESULT_DTYPE = np.dtype([("status", "<u4"), ("harq_ack", "<u4", (2,)), ("sr", "<u4"), ("detection_metric", "<f4"), ("sinr_dB", "<f4"),
                         ("rsrp_dB", "<f4"), ("epre_dB", "<f4"), ("time_alignment_s", "<f4"), ("cfo_hz", "<f4")])


def to_abi(abi, cfg):
    """A configuration dict as the library's nrphy_pucch_cfg_t (abi: the package's abi module)."""
    return abi.make_pucch(format=cfg["format"], starting_prb=cfg["starting_prb"], nof_symbols=cfg["nof_symbols"],
                          start_symbol=cfg["start_symbol_index"], second_hop_prb=cfg["second_hop_prb"], bwp_size_rb=cfg["bwp_size_rb"],
                          bwp_start_rb=cfg["bwp_start_rb"], numerology=cfg["numerology"], slot_index=cfg["slot_index"],
                          initial_cyclic_shift=cfg["initial_cyclic_shift"], time_domain_occ=cfg["time_domain_occ"], n_id=cfg["n_id"],
                          nof_harq_ack=cfg["nof_harq_ack"], sr_opportunity=cfg["sr_opportunity"], rx_ports=cfg["ports"])


# ---- sequences -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def n_cs(n_id, slot_index):
    """n_cs(n_slot, l), l = 0 .. 13 (TS 38.211 Section 6.3.2.2.2): sum_m 2^m c(8 (14 n_slot + l) + m), c_init = n_id."""
    c = gold(n_id, 8 * 14 * (slot_index + 1))[8 * 14 * slot_index:].reshape(14, 8).astype(np.int64)
    return (c << np.arange(8)).sum(axis=1)


def alpha_index(cfg, symbol, m_cs=0):
    return int((cfg["initial_cyclic_shift"] + m_cs + n_cs(cfg["n_id"], cfg["slot_index"])[symbol]) % 12)


def _polar(phase, dt):
    x = np.float64(phase)
    return dt(np.cos(x)), dt(np.sin(x))


def _twopi(dt):
    return dt(2.0) * dt(np.float32(np.pi) if dt is np.float32 else np.pi)


def cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def low_papr(u, alpha, dt=np.float32):
    """r_uv^alpha(n), n < 12, as low_papr_sequence_generator_impl builds it: an 8-entry exponential table indexed by phi(n), times a
    24-entry table indexed by 2 alpha n."""
    pi2 = dt(2 * np.pi)
    e8 = [_polar(pi2 * dt(k) / dt(8), dt) for k in range(8)]
    e24 = [_polar(pi2 * dt(k) / dt(24), dt) for k in range(24)]
    br = np.array([e8[(8 + p) % 8][0] for p in PHI_12[u]], dt)
    bi = np.array([e8[(8 + p) % 8][1] for p in PHI_12[u]], dt)
    sr = np.array([e24[(2 * alpha * n) % 24][0] for n in range(12)], dt)
    si = np.array([e24[(2 * alpha * n) % 24][1] for n in range(12)], dt)
    return cmul(br, bi, sr, si)


def low_papr_by_definition(u, alpha):
    n = np.arange(12)
    return np.exp(1j * (np.array(PHI_12[u]) * np.pi / 4 + 2 * np.pi * alpha * n / 12))


def occ(length, index, dt=np.float32):
    """w_i(m), m < N (pucch_orthogonal_sequence: polar(1, TWOPI phi / N))."""
    tp = _twopi(dt)
    w = [_polar(tp * dt(phi) / dt(length), dt) for phi in OCC_PHI[length - 1][index]]
    return np.array([a for a, _ in w], dt), np.array([b for _, b in w], dt)


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def grid_prb(cfg, hop):
    second = cfg["second_hop_prb"]
    return cfg["bwp_start_rb"] + (second if hop and second is not None else cfg["starting_prb"])


def format1_layout(cfg):
    """Per symbol offset of the allocation: (hop, is DM-RS, index within the hop's DM-RS or data symbols, their number)."""
    ns = cfg["nof_symbols"]
    half = ns // 2 if cfg["second_hop_prb"] is not None else ns
    kinds = [(1 if off >= half else 0, off % 2 == 0) for off in range(ns)]
    out = []
    for off, (hop, dmrs) in enumerate(kinds):
        same = [o for o, k in enumerate(kinds) if k == (hop, dmrs)]
        out.append((hop, dmrs, same.index(off), len(same)))
    return out


# ---- transmitter ------------------------------------------------------------------------------------------------------------
def transmit(cfg, ack_bits=(), sr=None):
    """The resource elements one UE sends: {(symbol, grid PRB): 12 complex128}, unit amplitude."""
    u = cfg["n_id"] % 30
    s0 = cfg["start_symbol_index"]
    out = {}
    if cfg["format"] == 0:
        table = FORMAT0_TABLES[(cfg["nof_harq_ack"], cfg["sr_opportunity"])]
        want_sr = None if not cfg["sr_opportunity"] else int(sr or 0)
        (m_cs,) = [m for m, s, a in table if a == list(ack_bits) and (s == want_sr if cfg["nof_harq_ack"] else True)]
        for l in range(cfg["nof_symbols"]):
            out[(s0 + l, grid_prb(cfg, l != 0))] = low_papr_by_definition(u, alpha_index(cfg, s0 + l, m_cs))
        return out
    bits = list(ack_bits) if cfg["nof_harq_ack"] else [0]  # positive SR alone: one 0 bit
    if len(bits) == 1:
        d = ((1 - 2 * bits[0]) + 1j * (1 - 2 * bits[0])) / np.sqrt(2)
    else:
        d = ((1 - 2 * bits[0]) + 1j * (1 - 2 * bits[1])) / np.sqrt(2)
    for off, (hop, dmrs, m, count) in enumerate(format1_layout(cfg)):
        w = np.exp(2j * np.pi * OCC_PHI[count - 1][cfg["time_domain_occ"]][m] / count)
        r = low_papr_by_definition(u, alpha_index(cfg, s0 + off))
        out[(s0 + off, grid_prb(cfg, hop))] = w * r if dmrs else w * d * r
    return out


def add_to_grid(grid, res, gains, delay=0.0, cfo=0.0, numerology=0):
    """Adds one UE's resource elements to a complex grid [ports][14][subc]: per-port complex gain, a delay in units of 1 / (4096
    x spacing) (a phase ramp over the subcarriers) and a CFO normalised to the spacing (a phase per symbol start epoch)."""
    ep = epochs(numerology)
    for (symbol, prb), x in res.items():
        k = 12 * prb + np.arange(12)
        ramp = np.exp(-2j * np.pi * k * delay / 4096.0) * np.exp(2j * np.pi * cfo * float(ep[symbol]))
        for p, g in enumerate(gains):
            grid[p, symbol, k] += g * ramp * x


def quantize(grid):
    return to_words(grid.real.astype(np.float32), grid.imag.astype(np.float32))


# ---- receiver ---------------------------------------------------------------------------------------------------------------
def _rsum(x):
    return np.sum(np.asarray(x, np.float64))


def _db(v, dt):
    with np.errstate(divide="ignore"):
        return dt(dt(10) * dt(np.log10(np.float64(v))))


def _isnormal(x, dt):
    a = np.abs(x)
    return (a >= np.finfo(dt).tiny) & np.isfinite(a)


def _row(grid, cfg, port, symbol, prb, dt):
    re, im = from_words(grid[cfg["ports"][port], symbol, 12 * prb:12 * prb + 12])
    return re.astype(dt), im.astype(dt)


def process_format0(cfg, grid, dt=np.float32):
    u = cfg["n_id"] % 30
    P, ns, s0 = len(cfg["ports"]), cfg["nof_symbols"], cfg["start_symbol_index"]
    rows = [[_row(grid, cfg, p, s0 + l, grid_prb(cfg, l != 0), dt) for p in range(P)] for l in range(ns)]
    epre = dt(0)
    for l in range(ns):
        for p in range(P):
            yr, yi = rows[l][p]
            epre = dt(epre + dt(_rsum(yr * yr + yi * yi) / 12.0))
    epre = dt(epre / dt(ns * P))
    best, best_rsrp, message = dt(0), dt(0), None
    metrics = []
    for m_cs, sr, ack in FORMAT0_TABLES[(cfg["nof_harq_ack"], cfg["sr_opportunity"])]:
        sum_corr, sum_nv = dt(0), dt(0)
        for l in range(ns):
            sr_, si_ = low_papr(u, alpha_index(cfg, s0 + l, m_cs), dt)
            for p in range(P):
                yr, yi = rows[l][p]
                lr, li = yr * sr_ + yi * si_, yi * sr_ - yr * si_
                avg_pwr = dt(_rsum(lr * lr + li * li) / 12.0)
                mr, mi = dt(dt(_rsum(lr)) / dt(12)), dt(dt(_rsum(li)) / dt(12))
                corr = dt(mr * mr + mi * mi)
                diff = dt(avg_pwr - corr)
                noise_var = diff if diff > 0 else dt(0)
                sum_corr = dt(sum_corr + corr)
                sum_nv = dt(sum_nv + dt(noise_var * corr))
        metric = dt(dt(sum_corr * sum_corr) / sum_nv) if _isnormal(sum_nv, dt) else dt(0)
        metrics.append(float(metric))
        if metric > best:
            best, best_rsrp, message = metric, sum_corr, (sr, ack)
    sr, ack = message if message is not None else (0, [0] * cfg["nof_harq_ack"])
    return dict(status=VALID if best > THRESHOLD else INVALID, harq_ack=list(ack), sr=int(sr or 0), metric=best, raw_metric=float(best),
                sinr_dB=_db(best, dt), rsrp_dB=_db(best_rsrp, dt), epre_dB=_db(epre, dt), time_alignment_s=dt(0), cfo_hz=dt(np.nan),
                candidates=metrics, meas=None, ce=None)


def equalize_zf(yr, yi, hr, hi, nv, dt):
    """channel_equalizer (ZF, one layer, beta 1) per RE: y [ports][re], h [ports][re], nv [ports] -> (x re, x im, variance)."""
    n_re = yr.shape[1]
    msq, nacc, ar, ai = (np.zeros(n_re, dt) for _ in range(4))
    for p in range(yr.shape[0]):
        n = hr[p] * hr[p] + hi[p] * hi[p]
        ok = _isnormal(n, dt) & bool(_isnormal(nv[p], dt) and nv[p] > 0)
        msq = np.where(ok, msq + n, msq)
        nacc = np.where(ok, nacc + n * nv[p], nacc)
        ar = np.where(ok, ar + (yr[p] * hr[p] + yi[p] * hi[p]), ar)
        ai = np.where(ok, ai + (yi[p] * hr[p] - yr[p] * hi[p]), ai)
    d = dt(1) * msq
    ok = _isnormal(d, dt) & _isnormal(nacc, dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        rcp = dt(1) / d
        return (np.where(ok, ar * rcp, dt(0)).astype(dt), np.where(ok, ai * rcp, dt(0)).astype(dt),
                np.where(ok, nacc * rcp * rcp, dt(np.inf)).astype(dt))


def process_format1(cfg, grid, dt=np.float32):
    u = cfg["n_id"] % 30
    P, ns, s0 = len(cfg["ports"]), cfg["nof_symbols"], cfg["start_symbol_index"]
    layout = format1_layout(cfg)
    nof_hops = 2 if cfg["second_hop_prb"] is not None else 1
    ep = epochs(cfg["numerology"])
    twopi = _twopi(dt)
    nof_pilots = 12 * sum(1 for _, dmrs, _, _ in layout if dmrs)
    ce = np.zeros((P, 14, grid.shape[-1]), np.uint32)
    region = np.zeros((P, 14, grid.shape[-1]), bool)
    meas, h_words = [], []
    for p in range(P):
        rsrp = epre = noise = dt(0)
        cfo = None
        h_words.append([])
        for hop in range(nof_hops):
            dmrs = [off for off, (h, is_dmrs, _, _) in enumerate(layout) if h == hop and is_dmrs]
            nd = len(dmrs)
            prb = grid_prb(cfg, hop)
            wr, wi = occ(nd, cfg["time_domain_occ"], dt)
            rx, z = [], []
            lr = li = None
            epre_hop = dt(0)
            cfo_hop = None
            for j, off in enumerate(dmrs):
                rr, ri = low_papr(u, alpha_index(cfg, s0 + off), dt)
                zr, zi = cmul(rr, ri, wr[j], wi[j])
                yr, yi = _row(grid, cfg, p, s0 + off, prb, dt)
                rx.append((yr, yi))
                z.append((zr, zi))
                pr, pi = yr * zr + yi * zi, yi * zr - yr * zi
                epre_hop = dt(epre_hop + dt(dt(_rsum(yr * yr + yi * yi) / 12.0) * dt(12)))
                if j == 0:
                    lr, li = pr, pi
                    continue
                if j == 1:
                    dr, di = dt(_rsum(pr * lr + pi * li)), dt(_rsum(pi * lr - pr * li))
                    phase = dt(np.arctan2(np.float64(di), np.float64(dr)))
                    cfo_hop = dt(dt(phase / twopi) / dt(ep[s0 + dmrs[1]] - ep[s0 + dmrs[0]]))
                lr, li = lr + pr, li + pi
            epre = dt(epre + epre_hop)
            if cfo_hop is not None:
                cfo = cfo_hop if cfo is None else dt(dt(cfo + cfo_hop) / dt(2))
            scale = dt(dt(1) / dt(dt(nd) * dt(1)))
            hr, hi = dt(_rsum(lr * scale) / 12.0), dt(_rsum(li * scale) / 12.0)
            rsrp = dt(rsrp + dt(dt(dt(hr * hr + hi * hi) * dt(12)) * dt(nd)))
            noise_hop = dt(0)
            for (yr, yi), (zr, zi) in zip(rx, z):
                er, ei = cmul(-hr, -hi, zr, zi)
                er, ei = er + yr, ei + yi
                noise_hop = dt(noise_hop + dt(dt(_rsum(er * er + ei * ei) / 12.0) * dt(12)))
            noise = dt(noise + noise_hop)
            word = to_words(np.array([hr], np.float32), np.array([hi], np.float32))[0]
            h_words[p].append(word)
            for off, (h, _, _, _) in enumerate(layout):
                if h == hop:
                    ce[p, s0 + off, 12 * prb:12 * prb + 12] = word
                    region[p, s0 + off, 12 * prb:12 * prb + 12] = True
        rsrp = dt(rsrp / dt(nof_pilots))
        epre = dt(epre / dt(nof_pilots))
        noise = dt(noise / dt(nof_pilots - 1))
        min_noise = dt(rsrp / dt(1e10))
        noise_var = noise if min_noise < noise else min_noise
        snr = dt(rsrp / noise_var) if noise_var != 0 else dt(1000)
        scs_khz = 15 << cfg["numerology"]
        meas.append(dict(noise_var=noise_var, rsrp=rsrp, epre=epre, snr=snr, ta_s=dt(0), ta_bins=0,
                         cfo_hz=dt(dt(cfo * dt(scs_khz)) * dt(1000)) if cfo is not None else dt(np.nan)))
    # channel_estimate::get_channel_state_information
    epre_lin = rsrp_lin = noise_all = dt(0)
    best_port, best_snr = 0, dt(0)
    for p, m in enumerate(meas):
        epre_lin, rsrp_lin, noise_all = dt(epre_lin + m["epre"]), dt(rsrp_lin + m["rsrp"]), dt(noise_all + m["noise_var"])
        if m["snr"] > best_snr:
            best_port, best_snr = p, m["snr"]
    sinr = dt(rsrp_lin / noise_all) if _isnormal(noise_all, dt) else dt(1e6)
    # the detector
    data = [(off, hop, m, count) for off, (hop, dmrs, m, count) in enumerate(layout) if not dmrs]
    nv = [m["noise_var"] for m in meas]
    sr_ = si_ = sv = 0.0
    for off, hop, m, count in data:
        prb = grid_prb(cfg, hop)
        rows = [_row(grid, cfg, p, s0 + off, prb, dt) for p in range(P)]
        yr, yi = np.array([r[0] for r in rows], dt), np.array([r[1] for r in rows], dt)
        h = [from_words(np.full(12, h_words[p][hop], np.uint32)) for p in range(P)]
        hr, hi = np.array([a for a, _ in h]).astype(dt), np.array([b for _, b in h]).astype(dt)
        xr, xi, xv = equalize_zf(yr, yi, hr, hi, nv, dt)
        wr, wi = occ(count, cfg["time_domain_occ"], dt)
        rr, ri = low_papr(u, alpha_index(cfg, s0 + off), dt)
        tr, ti = cmul(xr, xi, wr[m], -wi[m])
        tr, ti = cmul(tr, ti, rr, -ri)
        sr_, si_, sv = sr_ + _rsum(tr), si_ + _rsum(ti), sv + _rsum(xv)
    nre = 12 * len(data)
    det_r, det_i = dt(dt(sr_) / dt(nre)), dt(dt(si_) / dt(nre))
    eq_noise_var = dt(dt(sv / float(nre)) / dt(nre))
    m1, m2 = dt(det_r + det_i), dt(det_r - det_i)
    bits = 0 if m1 > 0 else 3
    bits2 = 2 if m2 > 0 else 1
    m1, m2 = abs(m1), abs(m2)
    if cfg["nof_harq_ack"] > 1 and m2 > m1:
        bits = bits2
    with np.errstate(divide="ignore", invalid="ignore"):
        metric = dt(dt(det_r * det_r + det_i * det_i) / eq_noise_var)
    status = INVALID
    if metric > THRESHOLD:
        status = VALID if cfg["nof_harq_ack"] > 0 or (bits & 1) == 0 else UNKNOWN
    ack = [bits & 1, (bits >> 1) & 1][:cfg["nof_harq_ack"]]
    return dict(status=status, harq_ack=ack, sr=0, metric=dt(metric / dt(THRESHOLD)), raw_metric=float(metric),
                sinr_dB=_db(sinr, dt), rsrp_dB=_db(dt(rsrp_lin / dt(P)), dt), epre_dB=_db(dt(epre_lin / dt(P)), dt),
                time_alignment_s=dt(0), cfo_hz=meas[best_port]["cfo_hz"], statistics=(float(m1), float(m2)), meas=meas, ce=ce,
                region=region)


def process(cfg, grid, dt=np.float32):
    """grid [ports][14][subc] cbf16 words -> the result record as a dict (plus what the tests look inside for)."""
    return process_format0(cfg, grid, dt) if cfg["format"] == 0 else process_format1(cfg, grid, dt)
