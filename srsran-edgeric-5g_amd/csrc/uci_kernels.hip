// UCI decoder: short blocks (1 to 11 bits) and polar (12 to 1706 bits), one wavefront per message, every message of a plan in one
// launch.  Restates uci_decoder_impl::decode (R/lib/phy/upper/channel_processors/uci/uci_decoder_impl.cpp) on
// short_block_detector_impl::detect (R/lib/phy/upper/channel_coding/short/short_block_detector_impl.cpp) and on the polar receive
// chain (polar_rate_dematcher_impl, polar_decoder_impl, polar_deallocator_impl under R/lib/phy/upper/channel_coding/polar/), in
// integers on int8 soft bits: the result equals the reference's bit for bit.
//
// Short block: the 32 (or bits-per-symbol, or three times that) de-matched soft bits are one lane each, every lane adding its own
// repetitions in ascending order with the saturating sum; the 2^(A-1) even-valued codewords are spread over the lanes, each built
// from the basis sequences' columns, and the winner is the largest |correlation| at the smallest index.
//
// Polar: the stage soft bits (2N - 1 bytes), the partial sums and the decoder's output sit in LDS.  The walk over the tree does not
// depend on the soft bits, so the host flattens it per code into a list of operations (f, g, rate-1 leaf, partial-sum XOR; rate-0
// nodes need none) that the wavefront runs in order: uniform control flow, the vectors across the lanes.  The two blocks of a
// segmented message run one after the other on the same wavefront, because whether the second one runs depends on the first.
#include "nrphy_internal.h"

namespace nrphy {

namespace {

constexpr uint32_t WAVE          = 64;
constexpr uint32_t UCI_MAX_N     = 1024;
constexpr int      UCI_LLR_MAX   = 120;
constexpr int      UCI_LLR_INFTY = 127;

#include "uci_tables.inc"

// TS 38.212 Table 5.4.1.1-1.
__device__ const uint8_t UCI_SUBBLOCK_PATTERN[32] = NR_POLAR_SUBBLOCK_PATTERN;

// log_likelihood_ratio::operator+= and promotion_sum (R/lib/phy/upper/log_likelihood_ratio.cpp:38-88): opposite values give 0, an
// infinite summand wins (the left one first), otherwise the sum is clamped to +-120 or promoted to +-127.
__device__ __forceinline__ bool llr_isinf(int v)
{
  return v < -UCI_LLR_MAX || v > UCI_LLR_MAX;
}
template <int LIMIT>
__device__ __forceinline__ int llr_sum(int a, int b)
{
  if (a == -b) {
    return 0;
  }
  if (llr_isinf(a)) {
    return a;
  }
  if (llr_isinf(b)) {
    return b;
  }
  const int t = a + b;
  return t > UCI_LLR_MAX ? LIMIT : (t < -UCI_LLR_MAX ? -LIMIT : t);
}
__device__ __forceinline__ int llr_soft_xor(int x, int y)
{
  const int m = min(abs(x), abs(y));
  return x * y < 0 ? -m : m;
}

__device__ __forceinline__ uint32_t wave_reduce_xor(uint32_t v)
{
  for (uint32_t d = 32; d != 0; d >>= 1) {
    v ^= __shfl_xor(v, d);
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_reduce_max(uint32_t v)
{
  for (uint32_t d = 32; d != 0; d >>= 1) {
    v = max(v, (uint32_t)__shfl_xor(v, d));
  }
  return v;
}

struct UciShared {
  int8_t  llr[2 * UCI_MAX_N]; // stage s at [2^s - 1, 2^(s+1) - 1)
  uint8_t est[UCI_MAX_N];     // partial sums
  uint8_t u[UCI_MAX_N];       // decoder output
  int     tmp[32];            // the de-matched short block
};

// short_block_detector_impl::detect.  Returns the status; the message goes to `out`.
__device__ uint32_t short_block(const UciMsgDesc& m, const int8_t* llr, uint8_t* out, UciShared& sh, uint32_t lane)
{
  const uint32_t A = m.A, E = m.E;
  // An all-zero input: all ones, invalid.
  uint32_t any = 0;
  for (uint32_t i = lane; i < E; i += WAVE) {
    any |= (uint32_t)(llr[i] != 0);
  }
  if (__ballot(any != 0) == 0) {
    if (lane < A) {
      out[lane] = 1;
    }
    return NRPHY_UCI_STATUS_INVALID;
  }
  // rate_dematch: position j adds inputs j, j + M, ... in that order (the saturating sum does not commute with reordering).
  const uint32_t M = A == 1 ? m.bps : (A == 2 ? 3 * m.bps : 32);
  if (lane < 32) {
    int acc = 0;
    if (lane < M) {
      for (uint32_t i = lane; i < E; i += M) {
        acc = llr_sum<UCI_LLR_MAX>(acc, (int)llr[i]);
      }
    }
    sh.tmp[lane] = acc;
  }
  __syncthreads();
  if (A == 1) {
    if (lane == 0) {
      out[0] = sh.tmp[0] > 0 ? 0 : 1;
    }
    return NRPHY_UCI_STATUS_VALID; // metric 1 against threshold 0
  }
  int64_t m2 = 0, norm = 0, num = 0, den_scale = 0, threshold = 0;
  if (A == 2) {
    // detect_2: three soft bits, combined from the two copies when the symbol carries more than one bit.
    int l0, l1, l2;
    if (M == 3) {
      l0 = sh.tmp[0], l1 = sh.tmp[1], l2 = sh.tmp[2];
    } else {
      const uint32_t step = M / 3 - 2;
      l0                  = sh.tmp[0] + sh.tmp[step + 3];
      l1                  = sh.tmp[1] + sh.tmp[2 * step + 4];
      l2                  = sh.tmp[step + 2] + sh.tmp[2 * step + 5];
    }
    const int metric[4] = {l0 + l1 + l2, -l0 + l1 - l2, l0 - l1 - l2, -l0 - l1 + l2};
    uint32_t  best      = 0;
    int       best_m    = 0; // the reference starts at the smallest positive double: only a metric of 1 or more replaces it
    for (uint32_t c = 0; c != 4; ++c) {
      if (metric[c] > best_m) {
        best_m = metric[c];
        best   = c;
      }
    }
    if (lane == 0) {
      out[0] = (uint8_t)(best & 1U);
      out[1] = (uint8_t)(best >> 1);
    }
    m2        = (int64_t)best_m * best_m;
    norm      = (int64_t)l0 * l0 + (int64_t)l1 * l1 + (int64_t)l2 * l2;
    num       = 2;
    den_scale = 3;
    threshold = 0;
  } else {
    // detect_3_11: codeword idx carries the message 2 idx (bit k of the message is bit k - 1 of idx); its correlation is
    // sum(tmp) - 2 sum(tmp over the codeword's ones).
    int t[32], total = 0;
    for (uint32_t i = 0; i != 32; ++i) {
      t[i] = sh.tmp[i];
      total += t[i];
      norm += (int64_t)t[i] * t[i];
    }
    const uint32_t nof_codewords = 1U << (A - 1);
    uint32_t       best_key      = 0; // |correlation| << 11 | (1023 - idx) << 1 | negative: the largest, then the first
    for (uint32_t idx = lane; idx < nof_codewords; idx += WAVE) {
      uint32_t cw = 0;
      for (uint32_t k = 1; k != A; ++k) {
        cw ^= ((idx >> (k - 1)) & 1U) ? UCI_BASIS_COLUMN[k] : 0U;
      }
      int ones = 0;
      for (uint32_t i = 0; i != 32; ++i) {
        ones += ((cw >> i) & 1U) ? t[i] : 0;
      }
      const int      corr = total - 2 * ones;
      const uint32_t key  = ((uint32_t)abs(corr) << 11) | ((1023U - idx) << 1) | (uint32_t)(corr < 0);
      best_key            = max(best_key, key);
    }
    // A lane without a codeword holds key 0, below the key of index 0 whatever its correlation.
    best_key                = wave_reduce_max(best_key);
    const uint32_t best_idx = 1023U - ((best_key >> 1) & 1023U);
    const int64_t  best_abs = best_key >> 11;
    const uint32_t value    = 2 * best_idx + (best_abs != 0 ? (best_key & 1U) : 0U);
    if (lane < A) {
      out[lane] = (uint8_t)((value >> lane) & 1U);
    }
    m2        = best_abs * best_abs;
    num       = 31;
    den_scale = 32;
    threshold = UCI_SHORT_THRESHOLD[A - 1];
  }
  // num m^2 / (den_scale norm - m^2) > threshold in integers.  The denominator is never negative (Cauchy-Schwarz); where it is 0
  // the double quotient is +infinity for m != 0 (above any threshold) and NaN for m = 0 (above none).
  const int64_t den   = den_scale * norm - m2;
  const bool    valid = den == 0 ? m2 != 0 : num * m2 > threshold * den;
  return valid ? NRPHY_UCI_STATUS_VALID : NRPHY_UCI_STATUS_INVALID;
}

// One block: rate de-matching, the simplified successive cancellation decoder, de-allocation and the CRC.  Returns true when
// the CRC remainder is 0; writes the block's message bits (filler and CRC left out) to `out`.
__device__ bool polar_block(const UciCodeDesc& c, const uint16_t* tab16, const uint32_t* ops, const int8_t* llr, uint32_t filler,
                            uint8_t* out, UciShared& sh, uint32_t lane)
{
  const uint32_t  n = c.n, N = 1U << n, E = c.E, K = c.K;
  const uint16_t* ch = tab16 + c.ch_offset;
  // Channel de-interleaver (through ch), bit de-selection, sub-block de-interleaver: position j of the selection buffer lands on
  // decoder input J(j).
  for (uint32_t j = lane; j < N; j += WAVE) {
    int y;
    if (c.mode == 0) {
      y = llr[ch[j]];
      for (uint32_t k = j + N; k < E; k += N) {
        y = llr_sum<UCI_LLR_INFTY>(y, (int)llr[ch[k]]);
      }
    } else if (c.mode == 1) {
      y = j < N - E ? 0 : (int)llr[ch[j - (N - E)]];
    } else {
      y = j < E ? (int)llr[ch[j]] : UCI_LLR_INFTY;
    }
    const uint32_t J   = UCI_SUBBLOCK_PATTERN[(32 * j) >> n] * (N >> 5) + (j & ((N >> 5) - 1));
    sh.llr[N - 1 + J]  = (int8_t)y;
    sh.est[j]          = 0;
    sh.u[j]            = 0;
  }
  __syncthreads();
  ops += c.ops_offset;
  for (uint32_t io = 0; io != c.nof_ops; ++io) {
    const uint32_t op = ops[io], kind = op & 3U, s = (op >> 2) & 15U, pos = op >> 6;
    if (kind == UCI_OP_F) {
      // Stage s to stage s - 1: soft_xor of the two halves.
      const uint32_t h = 1U << (s - 1);
      for (uint32_t i = lane; i < h; i += WAVE) {
        sh.llr[h - 1 + i] = (int8_t)llr_soft_xor(sh.llr[2 * h - 1 + i], sh.llr[3 * h - 1 + i]);
      }
    } else if (kind == UCI_OP_G) {
      // y + x, or y - x where the partial sum of the left child (at pos) is 1.
      const uint32_t h = 1U << (s - 1);
      for (uint32_t i = lane; i < h; i += WAVE) {
        const int x = sh.llr[2 * h - 1 + i], y = sh.llr[3 * h - 1 + i];
        sh.llr[h - 1 + i] = (int8_t)llr_sum<UCI_LLR_MAX>(y, sh.est[pos + i] ? -x : x);
      }
    } else if (kind == UCI_OP_XOR) {
      const uint32_t h = 1U << (s - 1);
      for (uint32_t i = lane; i < h; i += WAVE) {
        sh.est[pos + i] ^= sh.est[pos + h + i];
      }
    } else {
      // Rate-1 node of 2^s bits: hard decisions (value <= 0 is a 1) are the partial sums; the message is their re-encoding.
      const uint32_t size = 1U << s;
      if (size <= WAVE) {
        uint32_t v = 0;
        if (lane < size) {
          v                  = (uint32_t)(sh.llr[size - 1 + lane] <= 0);
          sh.est[pos + lane] = (uint8_t)v;
        }
        for (uint32_t d = 1; d < size; d <<= 1) {
          const uint32_t partner = __shfl_xor(v, d);
          v ^= (lane & d) ? 0U : partner;
        }
        if (lane < size) {
          sh.u[pos + lane] = (uint8_t)v;
        }
      } else {
        for (uint32_t i = lane; i < size; i += WAVE) {
          const uint8_t v = (uint8_t)(sh.llr[size - 1 + i] <= 0);
          sh.est[pos + i] = v;
          sh.u[pos + i]   = v;
        }
        for (uint32_t d = 1; d < size; d <<= 1) {
          __syncthreads();
          for (uint32_t i = lane; i < size / 2; i += WAVE) {
            const uint32_t lo = ((i & ~(d - 1)) << 1) | (i & (d - 1)); // the i-th index whose bit d is clear
            sh.u[pos + lo] ^= sh.u[pos + lo + d];
          }
        }
      }
    }
    __syncthreads();
  }
  // De-allocation and CRC: block bit k sits at decoder output info[k] and adds x^(K - 1 - k) mod g to the remainder.
  const uint16_t* info = tab16 + c.info_offset;
  const uint16_t* crcw = tab16 + c.crc_offset;
  uint32_t        rem  = 0;
  for (uint32_t k = lane; k < K; k += WAVE) {
    const uint8_t bit = sh.u[info[k]];
    rem ^= bit ? (uint32_t)crcw[k] : 0U;
    if (k >= filler && k < K - c.crc_size) {
      out[k - filler] = bit;
    }
  }
  __syncthreads(); // the next block rewrites the shared arrays
  return wave_reduce_xor(rem) == 0;
}

__global__ __launch_bounds__(WAVE) void uci_decoder_kernel(UciLaunch p)
{
  __shared__ UciShared sh;
  const uint32_t       lane = threadIdx.x;
  const UciMsgDesc&    m    = p.msg[blockIdx.x];
  // A message that names a select word runs only when the word holds its value (workgroup-uniform); otherwise it writes nothing,
  // its status included.
  if (p.select != nullptr && m.select_word != NO_SELECT_WORD && p.select[m.select_word] != m.select_value) {
    return;
  }
  const int8_t*        llr  = p.llr + m.llr_offset;
  uint8_t*             out  = p.message + m.message_offset;
  uint32_t             status;
  if (m.code == UCI_NO_CODE) {
    status = short_block(m, llr, out, sh, lane);
  } else {
    // decode_codeword_polar: the first block carries floor(A / C) bits behind A % C filler bits, the second ceil(A / C); a
    // failed first block ends the message (the second block's bytes are not written), a failed second one overrides.
    const UciCodeDesc& c      = p.code[m.code];
    const uint32_t     C      = m.nof_blocks;
    const uint32_t     first  = m.A / C;
    status                    = polar_block(c, p.tab16, p.ops, llr, m.A % C, out, sh, lane) ? NRPHY_UCI_STATUS_VALID : NRPHY_UCI_STATUS_INVALID;
    if (C == 2 && status == NRPHY_UCI_STATUS_VALID) {
      status = polar_block(c, p.tab16, p.ops, llr + c.E, 0, out + first, sh, lane) ? NRPHY_UCI_STATUS_VALID : NRPHY_UCI_STATUS_INVALID;
    }
  }
  if (lane == 0) {
    p.status[blockIdx.x] = status;
  }
}

} // namespace

hipError_t launch_uci_decoder(const UciLaunch& p, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(uci_decoder_kernel, dim3(p.n), dim3(WAVE), 0, stream, p);
  return hipGetLastError();
}

} // namespace nrphy
