"""NumPy restatement of the PUSCH DM-RS channel estimator on the low-PAPR DM-RS of a transform-precoded PUSCH: the restatement of
tests/pusch_chest_model.py with the pilot swapped.  The pilot is r_{u,0}(n), u = n_rs_id mod 30, of length M_zc = 6 M_rb
(TS 38.211 Sections 5.2.2 and 6.4.1.1.1.2, group and sequence hopping off), in the arithmetic of the reference's
low_papr_sequence_generator_impl: every element is an entry of complex_exponential_table(size, 1),
std::polar(1.0f, float(2 pi) * float(index) / float(size)), with cosf and sinf as the reference's build has them -- the C library's
single-precision routines, restated in libm_sincosf() below.  They are not correctly rounded: 1.3 % of the components of the
recorded sequences are one float32 step from cos and sin evaluated in float64 and rounded once (what srs_model.unit_circle gives).

  M_zc = 6, 12, 18, 24   entry (8 + phi(n)) mod 8 of the 8-point table; phi from tests/golden/pusch_lowpapr_tables.json (6, 18),
                         tests/golden/pucch_tables.json (12) and tests/golden/srs_tables.json (24)
  M_zc >= 36             N_zc the largest prime below M_zc, q = zc_sequence_q(u, 0, N_zc) in float32 (srs_model.zc_root),
                         m = n mod N_zc, entry (2 N_zc - (q m (m + 1) mod 2 N_zc)) mod 2 N_zc of the 2 N_zc-point table
  M_zc = 30              not a length of the reference's generator: exp(-j pi (u + 1)(n + 1)(n + 2) / 31), entry
                         (62 - ((u + 1)(n + 1)(n + 2) mod 62)) mod 62 of the 62-point table
"""
import contextlib
import functools
import json
import os

import numpy as np

import pusch_chest_model as base
import srs_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32 = np.float32


def nof_prb_valid(n):
    """transform_precoding_helpers.h: 2^a 3^b 5^c, up to 275."""
    if not 1 <= n <= 275:
        return False
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


VALID_NOF_PRB = [n for n in range(1, 276) if nof_prb_valid(n)]


@functools.lru_cache(maxsize=None)
def phi_tables():
    own = json.load(open(os.path.join(GOLDEN, "pusch_lowpapr_tables.json")))
    return {6: own["phi_6"], 18: own["phi_18"], 12: json.load(open(os.path.join(GOLDEN, "pucch_tables.json")))["phi_12"],
            24: json.load(open(os.path.join(GOLDEN, "srs_tables.json")))["phi_24"]}


_F = float.fromhex
_HPI_INV, _HPI = _F("0x1.45F306DC9C883p+23"), _F("0x1.921FB54442D18p0")
_C = [1.0, _F("-0x1.ffffffd0c621cp-2"), _F("0x1.55553e1068f19p-5"), _F("-0x1.6c087e89a359dp-10"), _F("0x1.99343027bf8c3p-16")]
_S = [_F("-0x1.555545995a603p-3"), _F("0x1.1107605230bc4p-7"), _F("-0x1.994eb3774cf24p-13")]


def libm_sincosf(y):
    """(sinf(y), cosf(y)) of glibc 2.28 and later (the Arm Optimized Routines' sincosf) for float32 0 <= y < 120: below 0.75 (the
    top 12 bits of pi / 4) no reduction, else n = round(y 2 / pi) from a 2^24-scaled product truncated to int32 and y - n pi / 2;
    two polynomials in float64, each rounded once to float32; the sine's sign from the quadrant, the cosine's coefficients negated
    in quadrants 2 and 3, the two swapped in odd quadrants.  Below 2^-12: (y, 1)."""
    y = np.asarray(y, np.float32)
    x = y.astype(np.float64)
    small = y < f32(0.75)
    n = np.where(small, 0, (((x * _HPI_INV).astype(np.int32).astype(np.int64) + 0x800000) >> 24)).astype(np.int64)
    x = np.where(small, x, x - n * _HPI)
    x2 = x * x
    xs = np.where(((n + 1) & 2) != 0, -x, x)
    x3, x4 = x2 * xs, x2 * x2
    c2, s1, c1 = _C[3] + x2 * _C[4], _S[1] + x2 * _S[2], _C[0] + x2 * _C[1]
    x5, x6 = x3 * x2, x4 * x2
    s, c = xs + x3 * _S[0], c1 + x4 * _C[2]
    sv, cv = (s + x5 * s1).astype(np.float32), (c + x6 * c2).astype(np.float32)
    cv = np.where((n & 2) != 0, -cv, cv)
    odd, tiny = (n & 1) == 1, y < f32(2.0 ** -12)
    return (np.where(tiny, y, np.where(odd, cv, sv)).astype(np.float32),
            np.where(tiny, f32(1), np.where(odd, sv, cv)).astype(np.float32))


def circle(index, size):
    """complex_exponential_table(size, 1)[index] with the reference's bits, complex64."""
    angle = ((base.TWOPI * np.asarray(index, np.float32)).astype(np.float32) / f32(size)).astype(np.float32)
    s, c = libm_sincosf(angle)
    return (c + 1j * s).astype(np.complex64)


def indices(u, nof_prb):
    """(entries [6 nof_prb], table size) of r_{u,0}."""
    M = 6 * nof_prb
    n = np.arange(M, dtype=np.int64)
    if M < 30:
        return (8 + np.array(phi_tables()[M][u], np.int64)) & 7, 8
    if M == 30:
        return (62 - ((u + 1) * (n + 1) * (n + 2)) % 62) % 62, 62
    n_zc = srs_model.prime_lower_than(M)
    q = srs_model.zc_root(u, n_zc)
    m = n % n_zc
    return (2 * n_zc - (q * m * (m + 1)) % (2 * n_zc)) % (2 * n_zc), 2 * n_zc


def sequence(n_rs_id, nof_prb):
    """low_papr_sequence_generator::generate(seq, n_rs_id % 30, 0, 0, 1), complex64 [6 nof_prb]."""
    idx, size = indices(n_rs_id % 30, nof_prb)
    return circle(idx, size)


def pilots(cfg, n_rs_id):
    """What pusch_chest_model.pilots returns, for the low-PAPR DM-RS: the same on every DM-RS symbol, layer 0 only."""
    prbs = np.array(base.prbs_of(cfg))
    s = sequence(n_rs_id, prbs.size)
    b = (12 * prbs[:, None] + 2 * np.arange(6)).ravel()
    return s.real.astype(np.float32), s.imag.astype(np.float32), b


@contextlib.contextmanager
def pilot_swapped(n_rs_id):
    """While inside, pusch_chest_model.pilots is the low-PAPR DM-RS of n_rs_id: for pusch_chest_model.estimate and for whatever
    else reads the pilots through that module (a test's transmitter, its parity check)."""
    saved = base.pilots
    base.pilots = lambda cfg, dmrs_symbol, layer: pilots(cfg, n_rs_id)
    try:
        yield
    finally:
        base.pilots = saved


def estimate(cfg, n_rs_id, grid, ce=None):
    """pusch_chest_model.estimate with the pilot swapped."""
    assert cfg.nof_tx_layers == 1
    with pilot_swapped(n_rs_id):
        return base.estimate(cfg, grid, ce)
