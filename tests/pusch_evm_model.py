"""The EVM of the reference's pusch_demodulator_impl, restated in NumPy for tests/test_pusch_evm.py.

evm_calculator_generic_impl::calculate is handed one OFDM symbol's n equalised (deprecoded) symbols x and the demapper's
n * qm soft bits before descrambling.  In sub-blocks of 4096 symbols it takes hard decisions (1 where the soft bit is <= 0), maps
them with modulation_mapper_lut_impl (a table per modulation; pi/2-BPSK alternates two by the parity of the position in the
sub-block), subtracts (srsvec::subtract: m - x per component in float32) and adds real(srsvec::dot_prod(d, d)) to a float32
power; the symbol's EVM is sqrt(power / float32(n)).  dot_prod, as an AVX2 build without contraction compiles it: 8 float32 lanes,
lane k accumulating the terms re * re + im * im (each operation rounded) of elements k, k + 8, ... in order, then the lanes
added in order starting from 0, then the remaining len % 8 terms one by one.  Fewer than 8 elements: the one-by-one loop alone.
pusch_demodulator_impl: over the symbols with data in ascending order acc += float32(n) * evm, cnt += n, and after every symbol
stats.evm = acc / float32(cnt).
"""
import numpy as np

F = np.float32
SUB_BLOCK = 4096
TABLE_OFFSET = {2: 0, 4: 4, 6: 20, 8: 84}  # into the recorded tables, QPSK first


def pi2_bpsk_tables():
    """modulator_table_pi_2_bpsk: (even, odd), entry b = the point of bit b; M_SQRT1_2 rounded to float32."""
    c = F(np.sqrt(0.5))
    return np.array([complex(c, c), complex(-c, -c)], np.complex64), np.array([complex(-c, c), complex(c, -c)], np.complex64)


def formula_table(qm):
    """The points of modulator_table_s<qm> from its constructor: integer levels (TS 38.211 Section 5.1) times the float32
    scaling = sqrt(1 / average power); entry i = the symbol of the bits of i, first bit highest."""
    i = np.arange(1 << qm)
    bit = lambda k: (i >> (qm - 1 - k)) & 1  # b(k)
    re, im = np.ones(i.size, np.int64), np.ones(i.size, np.int64)
    for k in range(qm - 2, 0, -2):  # 1 -> 2 - 1 s -> 4 - (...) s -> ...
        re = (1 << ((qm - k) // 2)) - (1 - 2 * bit(k)) * re
        im = (1 << ((qm - k) // 2)) - (1 - 2 * bit(k + 1)) * im
    re, im = (1 - 2 * bit(0)) * re, (1 - 2 * bit(1)) * im
    avg = F(np.mean(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2))
    scaling = np.sqrt(F(1) / avg, dtype=F)
    return (re.astype(F) * scaling + 1j * (im.astype(F) * scaling)).astype(np.complex64)


def hard_bits(soft):
    return (np.asarray(soft, np.int8) <= 0).astype(np.int64)


def map_points(qm, soft, tables):
    """The constellation points of one sub-block's hard decisions.  tables: the recorded [340] complex64, or None for the
    formula."""
    b = hard_bits(soft).reshape(-1, qm)
    if qm == 1:
        even, odd = pi2_bpsk_tables()
        j = np.arange(b.shape[0])
        return np.where(j & 1, odd[b[:, 0]], even[b[:, 0]]).astype(np.complex64)
    index = np.zeros(b.shape[0], np.int64)
    for k in range(qm):
        index = (index << 1) | b[:, k]
    table = formula_table(qm) if tables is None else tables[TABLE_OFFSET[qm]: TABLE_OFFSET[qm] + (1 << qm)]
    return table[index]


def dot_prod_real(d):
    """real(srsvec::dot_prod(d, d)) of complex64 d in the order of the AVX2 build."""
    re, im = d.real.astype(F), d.imag.astype(F)
    term = (re * re).astype(F) + (im * im).astype(F)  # float32 arrays: every operation rounds to float32
    n8 = term.size // 8 * 8
    result = F(0)
    if n8:
        lanes = np.zeros(8, F)
        for row in term[:n8].reshape(-1, 8):
            lanes = row + lanes
        for k in range(8):
            result = F(result + lanes[k])
    for t in term[n8:]:
        result = F(result + t)
    return result


def symbol_evm(qm, x, soft, tables=None):
    """evm_calculator_generic_impl::calculate for one block: float32."""
    x = np.asarray(x, np.complex64)
    soft = np.asarray(soft, np.int8)
    assert soft.size == x.size * qm
    power = F(0)
    for at in range(0, x.size, SUB_BLOCK):
        xs = x[at: at + SUB_BLOCK]
        m = map_points(qm, soft[at * qm: (at + xs.size) * qm], tables)
        d = ((m.real.astype(F) - xs.real.astype(F)) + 1j * (m.imag.astype(F) - xs.imag.astype(F))).astype(np.complex64)
        power = F(power + dot_prod_real(d))
    return np.sqrt(F(power / F(x.size)), dtype=F)


def evm(qm, xs, softs, tables=None):
    """pusch_demodulator_impl's accumulation over the OFDM symbols with data (xs, softs: one array per symbol, ascending):
    (every provisional stats.evm, the final one), float32."""
    acc, cnt, provisional = F(0), 0, []
    for x, soft in zip(xs, softs):
        acc = F(acc + F(F(x.size) * symbol_evm(qm, x, soft, tables)))
        cnt += x.size
        provisional.append(F(acc / F(cnt)))
    return provisional, provisional[-1]


def allowance(n_max):
    """Relative allowance between the library's EVM (a symbol's terms added in double, rounded once) and the reference's
    (an 8-lane float32 chain of n / 8 additions, off by at most (n / 8 + 16) 2^-24 of P_s, halved by the square root):
    (n_max / 16 + 64) 2^-24, the 64 for the products, the division, the root and the 14-term mean."""
    return (n_max / 16 + 64) * 2.0 ** -24
