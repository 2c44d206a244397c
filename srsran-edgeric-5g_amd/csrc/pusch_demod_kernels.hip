// Channel equaliser and PUSCH demodulator for gfx950.
//
// Replaces channel_equalizer::equalize (R/lib/phy/upper/equalization/channel_equalizer_generic_impl.cpp:225-277 with the scalar
// loops of equalize_zf_1xn.h:126-170, equalize_mmse_1xn.h and equalize_zf_2xn.h:182-252) and pusch_demodulator::demodulate
// (R/lib/phy/upper/channel_processors/pusch/pusch_demodulator_impl.cpp:135-287): RE selection, equalisation, soft demapping,
// descrambling and the post-equalisation SINR in one kernel.  The equaliser (equalize_device.h) is the one __device__ function both the
// standalone call (nrphy_channel_equalize) and the fused kernel run; the demapper is demod_device.h's, the scrambling sequence
// gold_sequence_blocks_wave's: the fused soft bits are those of equalise -> nrphy_demodulate_soft -> nrphy_llr_descramble.
//
// Work split (plan built on the host, pusch_demod_host.cpp): one workgroup per work item = up to 256 data RE of one OFDM symbol
// of one PUSCH, one RE per lane.  A lane finds its subcarrier from the PUSCH's list of allocated PRBs and, on DM-RS symbols, the
// data positions of a PRB; it loads its receive ports' grid words and the layers x ports estimate words (4 bytes each, lanes
// adjacent along subcarriers), equalises in registers and demaps.  Wave 0 meanwhile generates the item's scrambling bits into
// LDS.  The soft bits are staged in LDS with the destination's 16-byte phase and leave as 16-byte stores (bytes at the ends).
// HBM-bound: per RE 4 (ports + layers x ports) bytes in, layers x qm bytes out.
//
// A transform-precoded PUSCH (opt-in, nrphy_pusch_demod_plan_create_ex) takes pusch_tp_demod_kernel instead, one workgroup per
// OFDM symbol with the deprecoder between equaliser and demapper: see it below.  pi/2-BPSK without transform precoding is one
// more instantiation of the item above.
#include "bits_device.h"
#include "demod_device.h"
#include "dft_mixed_device.h"
#include "equalize_device.h"

#include <hip/hip_runtime.h>

namespace nrphy {
namespace {

__global__ __launch_bounds__(256) void channel_equalize_kernel(EqualizeLaunch p)
{
  const uint32_t re = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (re >= p.nof_re) {
    return;
  }
  const uint32_t P = p.nof_rx_ports, L = p.nof_layers;
  uint32_t       y[NRPHY_MAX_PORTS] = {}, h[2][NRPHY_MAX_PORTS] = {};
  float          nv[NRPHY_MAX_PORTS] = {};
#pragma unroll
  for (uint32_t i = 0; i != NRPHY_MAX_PORTS; ++i) {
    if (i < P) {
      y[i]  = p.rx[((size_t)b * P + i) * p.nof_re + re];
      nv[i] = p.noise[(size_t)b * P + i];
#pragma unroll
      for (uint32_t l = 0; l != 2; ++l) {
        if (l < L) {
          h[l][i] = p.ch[(((size_t)b * L + l) * P + i) * p.nof_re + re];
        }
      }
    }
  }
  float2 x[2];
  float  v[2];
  equalize_re(p.algorithm, L, P, y, h, nv, max_noise(nv, P), p.tx_scaling, x, v);
  const size_t o = ((size_t)b * p.nof_re + re) * L;
#pragma unroll
  for (uint32_t l = 0; l != 2; ++l) {
    if (l < L) {
      reinterpret_cast<float2*>(p.eq)[o + l] = x[l];
      p.eq_nvars[o + l]                      = v[l];
    }
  }
}

constexpr uint32_t SEQ_WORDS   = 160;                          // >= (31 + 256 * 16) / 32 + 2, and >= the 31 head words
constexpr uint32_t STAGE_BYTES = PUSCH_DEMOD_THREADS * 16 + 16; // soft bits of an item at the destination's 16-byte phase

// Soft bits per symbol of a demapper instantiation, and its entry of PuschDemodLaunch::demod (pi/2-BPSK, NRPHY_MOD_PI2_BPSK = 0,
// comes last).
template <uint32_t MOD>
constexpr uint32_t demod_qm()
{
  return MOD == NRPHY_MOD_PI2_BPSK ? 1u : MOD;
}
template <uint32_t MOD>
constexpr uint32_t demod_slot()
{
  return MOD == NRPHY_MOD_PI2_BPSK ? 4u : MOD / 2u - 1u;
}

struct PuschDemodShared {
  Tables   t;
  uint32_t seq[SEQ_WORDS];
  double   red[2][PUSCH_DEMOD_THREADS / WAVE];
  __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
  double   evm_red[PUSCH_DEMOD_THREADS / WAVE]; // behind what the path without EVM uses, which stays where it was
};

// ---- EVM (nrphy_pusch_demod_run_evm) -------------------------------------------------------------------------------------------
// evm_calculator_generic_impl::calculate (R/lib/phy/upper/channel_modulation/evm_calculator_generic_impl.cpp:30-73) is handed,
// per OFDM symbol, the equalised (deprecoded) symbols x_j and the demapper's soft bits before descrambling
// (pusch_demodulator_impl.cpp:244-252): hard decisions (1 where the soft bit is <= 0), those mapped to the constellation point
// m_j (modulation_mapper_lut_impl.cpp:39-65: levels +-1, +-3, ... times one float per modulation; pi/2-BPSK alternates two
// tables by the parity of j), then sqrt(sum |m_j - x_j|^2 / n).  A lane has x_j and the soft bits in registers at one point of
// the item; evm_term is what it adds there: the float term with the reference's roundings (srsvec::subtract, then the
// re * re + im * im of srsvec::dot_prod), summed in double by the reduction the SINR sums take.
template <uint32_t MOD>
__device__ __forceinline__ float evm_term(const LlrBytes& out, uint32_t first, uint32_t j, float re, float im, float scale)
{
  constexpr uint32_t QM = demod_qm<MOD>();
  int                s[QM]; // 1 - 2 b of the symbol's hard bits b
#pragma unroll
  for (uint32_t k = 0; k != QM; ++k) {
    s[k] = (int8_t)out.get(first + k) <= 0 ? -1 : 1;
  }
  int lr, li;
  if constexpr (MOD == NRPHY_MOD_PI2_BPSK) {
    lr = (j & 1u) ? -s[0] : s[0];
    li = s[0];
  } else if constexpr (MOD == NRPHY_MOD_QPSK) {
    lr = s[0];
    li = s[1];
  } else if constexpr (MOD == NRPHY_MOD_QAM16) {
    lr = s[0] * (2 - s[2]);
    li = s[1] * (2 - s[3]);
  } else if constexpr (MOD == NRPHY_MOD_QAM64) {
    lr = s[0] * (4 - s[2] * (2 - s[4]));
    li = s[1] * (4 - s[3] * (2 - s[5]));
  } else {
    lr = s[0] * (8 - s[2] * (4 - s[4] * (2 - s[6])));
    li = s[1] * (8 - s[3] * (4 - s[5] * (2 - s[7])));
  }
  const float dr = __fsub_rn(__fmul_rn((float)lr, scale), re), di = __fsub_rn(__fmul_rn((float)li, scale), im);
  return __fadd_rn(__fmul_rn(dr, dr), __fmul_rn(di, di));
}

// Stage bytes [lo, hi) -> base[lo, hi), base 16-byte aligned and the stage at the same phase: 16-byte stores, bytes at the ends.
__device__ __forceinline__ void store_staged(const uint8_t* stage, int8_t* base, uint32_t lo, uint32_t hi, uint32_t tid)
{
  const uint32_t c_first = (lo + 15u) / 16u, c_last = hi / 16u;
  if (c_first >= c_last) {
    for (uint32_t b = lo + tid; b < hi; b += PUSCH_DEMOD_THREADS) {
      base[b] = (int8_t)stage[b];
    }
    return;
  }
  for (uint32_t c = c_first + tid; c < c_last; c += PUSCH_DEMOD_THREADS) {
    reinterpret_cast<uint4*>(base)[c] = reinterpret_cast<const uint4*>(stage)[c];
  }
  const uint32_t head = 16u * c_first - lo, tail = hi - 16u * c_last;
  if (tid < head) {
    base[lo + tid] = (int8_t)stage[lo + tid];
  } else if (tid >= 16u && tid < 16u + tail) {
    const uint32_t b = 16u * c_last + (tid - 16u);
    base[b]          = (int8_t)stage[b];
  }
}

template <uint32_t MOD, bool EVM>
__device__ __forceinline__ void pusch_demod_item(const PuschDemodLaunch& p, const PuschDemodItem& it, const PuschDemodDesc& d,
                                                 PuschDemodShared& s)
{
  constexpr uint32_t QM   = demod_qm<MOD>();
  const DemodLaunch& dm   = p.demod[demod_slot<MOD>()];
  const uint32_t     tid  = threadIdx.x, lane = tid % WAVE;
  if constexpr (MOD >= NRPHY_MOD_QAM64) {
    for (uint32_t k = tid; k < DEMOD_MAX_PAIRS * 16u; k += PUSCH_DEMOD_THREADS) {
      s.t.line[k / 16u][k % 16u] = make_float2(dm.slope[k / 16u][k % 16u], dm.intercept[k / 16u][k % 16u]);
    }
  }
  const uint32_t L = d.nof_layers, P = d.nof_rx_ports, nb = L * QM;
  const bool     active = tid < it.count;

  // The lane's RE: data RE r of the symbol -> PRB of the allocation and subcarrier within it.
  uint32_t y[NRPHY_MAX_PORTS] = {}, h[2][NRPHY_MAX_PORTS] = {};
  if (active) {
    const uint32_t r     = it.re_first + tid;
    const uint32_t per   = it.dmrs ? d.dmrs_re_per_prb : NRPHY_NRE;
    const uint32_t ord   = r / per, k = r - ord * per;
    const uint32_t subc  = NRPHY_NRE * (uint32_t)p.prbs[d.prb_first + ord] + (it.dmrs ? (uint32_t)d.dmrs_subc[k] : k);
    const size_t   nsubc = p.grid_nof_subc;
#pragma unroll
    for (uint32_t i = 0; i != NRPHY_MAX_PORTS; ++i) {
      if (i < P) {
        y[i] = p.grid[(((size_t)d.grid_index * p.grid_nof_ports + d.rx_ports[i]) * NRPHY_NSYMB + it.symbol) * nsubc + subc];
#pragma unroll
        for (uint32_t l = 0; l != 2; ++l) {
          if (l < L) {
            h[l][i] = p.ch[d.ce_offset + (((size_t)l * P + i) * NRPHY_NSYMB + it.symbol) * nsubc + subc];
          }
        }
      }
    }
  }

  // Wave 0: the item's scrambling bits c(n), n in [32 first_word, 32 (first_word + nwords)), into s.seq.
  const uint32_t first_word = it.bit_offset >> 5;
  const uint32_t nwords     = ((it.bit_offset & 31u) + it.count * nb + 31u) >> 5;
  if (tid < WAVE) {
    gold_sequence_blocks_wave(p.gold, d.c_init, first_word, nwords, s.seq, lane, [&](uint32_t base, uint32_t avail) {
      for (uint32_t k = lane; k < avail; k += WAVE) {
        s.seq[base + k] ^= p.x1_words[first_word + base + k];
      }
      wave_lds_fence();
    });
  }
  __syncthreads();

  LlrBytes out;
  double   vsum = 0.0, vcnt = 0.0, esum = 0.0;
  if (active) {
    float nv[NRPHY_MAX_PORTS];
#pragma unroll
    for (uint32_t i = 0; i != NRPHY_MAX_PORTS; ++i) {
      nv[i] = p.noise[(size_t)it.pusch * NRPHY_MAX_PORTS + i];
    }
    float2 x[2];
    float  v[2];
    equalize_re(d.equalizer, L, P, y, h, nv, max_noise(nv, P), 1.0f, x, v);
#pragma unroll
    for (uint32_t l = 0; l != 2; ++l) {
      if (l < L) {
        const uint32_t j = it.span_pos + tid * L + l; // position in the OFDM symbol's span (the reference's demapper call)
        if (j < it.nof_vector) {
          demodulate_symbol<MOD, true>(dm, s.t, j, x[l].x, x[l].y, v[l], out, l * QM);
        } else {
          demodulate_symbol<MOD, false>(dm, s.t, j, x[l].x, x[l].y, v[l], out, l * QM);
        }
        if (!__builtin_isinf(v[l])) { // pusch_demodulator_impl.cpp:203-215: the infinite variances (DC, dropped RE) are left out
          vsum += (double)v[l];
          vcnt += 1.0;
        }
        if constexpr (EVM) { // the RE with infinite variance count: soft bits 0, hard bits 1
          esum += (double)evm_term<MOD>(out, l * QM, j, x[l].x, x[l].y, p.evm_scale[demod_slot<MOD>()]);
        }
      }
    }
    // Descrambling: this lane's nb <= 16 soft bits start at bit b0 of the sequence words.
    const uint32_t b0   = (it.bit_offset & 31u) + tid * nb;
    const uint64_t pair = ((uint64_t)s.seq[b0 >> 5] << 32) | s.seq[(b0 >> 5) + 1u];
    const uint32_t bits = (uint32_t)(pair >> (48u - (b0 & 31u))) & 0xFFFFu; // first soft bit in bit 15
#pragma unroll
    for (uint32_t w = 0; w != 4; ++w) {
      out.w[w] = negate_bytes(out.w[w], byte_masks_msb_first((bits >> (12u - 4u * w)) & 0xFu));
    }
  }

  // SINR partial sums of the item: wave sums, then the four waves in order.
  vsum = wave_sum(vsum);
  vcnt = wave_sum(vcnt);
  if (lane == 0) {
    s.red[0][tid / WAVE] = vsum;
    s.red[1][tid / WAVE] = vcnt;
  }
  if constexpr (EVM) {
    esum = wave_sum(esum);
    if (lane == 0) {
      s.evm_red[tid / WAVE] = esum;
    }
  }

  // Soft bits staged at the destination's 16-byte phase.
  int8_t*        dst   = p.llr + (size_t)it.pusch * p.llr_stride + it.bit_offset;
  const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
  if (active) {
    uint8_t* st = s.stage + shift + tid * nb;
#pragma unroll
    for (uint32_t k = 0; k != 16; ++k) {
      if (k < nb) {
        st[k] = out.get(k);
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    double* part = p.partial + 2u * (size_t)(blockIdx.x);
    part[0]      = (s.red[0][0] + s.red[0][1]) + (s.red[0][2] + s.red[0][3]);
    part[1]      = (s.red[1][0] + s.red[1][1]) + (s.red[1][2] + s.red[1][3]);
    if constexpr (EVM) {
      p.evm_partial[blockIdx.x] = (s.evm_red[0] + s.evm_red[1]) + (s.evm_red[2] + s.evm_red[3]);
    }
  }
  store_staged(s.stage, dst - shift, shift, shift + it.count * nb, tid);
}

// EVM: whether the launch computes the EVM's partial sums as well; the instantiation without is the kernel as it was.
template <bool EVM>
__global__ __launch_bounds__(PUSCH_DEMOD_THREADS) void pusch_demod_kernel(PuschDemodLaunch p)
{
  __shared__ PuschDemodShared s;
  const PuschDemodItem  it = p.items[blockIdx.x];
  const PuschDemodDesc& d  = p.desc[it.pusch]; // read in place: dmrs_subc is indexed per lane
  switch (d.qm) { // workgroup-uniform
    case 1:
      pusch_demod_item<NRPHY_MOD_PI2_BPSK, EVM>(p, it, d, s);
      break;
    case NRPHY_MOD_QPSK:
      pusch_demod_item<NRPHY_MOD_QPSK, EVM>(p, it, d, s);
      break;
    case NRPHY_MOD_QAM16:
      pusch_demod_item<NRPHY_MOD_QAM16, EVM>(p, it, d, s);
      break;
    case NRPHY_MOD_QAM64:
      pusch_demod_item<NRPHY_MOD_QAM64, EVM>(p, it, d, s);
      break;
    default:
      pusch_demod_item<NRPHY_MOD_QAM256, EVM>(p, it, d, s);
      break;
  }
}

// ---- transform-precoded PUSCH: one workgroup per OFDM symbol -----------------------------------------------------------------
// pusch_demodulator_impl.cpp:186-201 puts precoder->deprecode_ofdm_symbol(eq_re, eq_re) between the equaliser and the demapper,
// and the transform needs the whole symbol, so the 256-RE items above cannot be used: the workgroup equalises the symbol's
// 12 M_rb RE (thread t those with r = t mod 256) into LDS, runs mixed_dft_inverse() -- the stand-alone deprecoder's routine --,
// scales by the float 1 / sqrt(M_sc) and demaps symbol j with the variance of RE j: the reference leaves the variances alone.
// A dropped RE (symbol 0, variance +inf) enters the transform as 0.  The soft bits are staged in the buffer the transform left
// free.  LDS: two buffers of 3248 complex + 3248 variances + 832 sequence words + the demapper's lines = 68.9 KB, two
// workgroups per CU.
constexpr uint32_t TP_BUF_POINTS = MIXED_DFT_MAX_POINTS + 8;                           // soft bits: 8 x 3240 + the 16-byte phase
constexpr uint32_t TP_SEQ_WORDS  = (31u + MIXED_DFT_MAX_POINTS * 8u + 31u) / 32u + 21u; // the symbol's words, and one read past them
static_assert(TP_BUF_POINTS * 8u >= MIXED_DFT_MAX_POINTS * 8u + 32u, "stage");
static_assert(PUSCH_DEMOD_THREADS == MIXED_DFT_THREADS, "one workgroup shape for the item and the transform");

struct PuschTpShared {
  __attribute__((aligned(16))) cf buf[2][TP_BUF_POINTS];
  float    var[TP_BUF_POINTS];
  Tables   t;
  uint32_t seq[TP_SEQ_WORDS];
  double   red[2][PUSCH_DEMOD_THREADS / WAVE];
  double   evm_red[PUSCH_DEMOD_THREADS / WAVE];
};

template <uint32_t MOD, bool EVM>
__device__ __forceinline__ void pusch_tp_item(const PuschDemodLaunch& p, const PuschTpItem& it, const PuschDemodDesc& d,
                                              const MixedDftPlan& plan, PuschTpShared& s)
{
  constexpr uint32_t QM   = demod_qm<MOD>();
  const DemodLaunch& dm   = p.demod[demod_slot<MOD>()];
  const uint32_t     tid  = threadIdx.x, lane = tid % WAVE;
  if constexpr (MOD >= NRPHY_MOD_QAM64) {
    for (uint32_t k = tid; k < DEMOD_MAX_PAIRS * 16u; k += PUSCH_DEMOD_THREADS) {
      s.t.line[k / 16u][k % 16u] = make_float2(dm.slope[k / 16u][k % 16u], dm.intercept[k / 16u][k % 16u]);
    }
  }
  const uint32_t P = d.nof_rx_ports;
  float          nv[NRPHY_MAX_PORTS];
#pragma unroll
  for (uint32_t i = 0; i != NRPHY_MAX_PORTS; ++i) {
    nv[i] = p.noise[(size_t)it.pusch * NRPHY_MAX_PORTS + i];
  }
  const float nv_max = max_noise(nv, P);

  // Gather and equalise: one layer, 12 data RE per PRB on every symbol that carries data.
  double       vsum = 0.0, vcnt = 0.0, esum = 0.0;
  const size_t nsubc = p.grid_nof_subc;
  for (uint32_t r = tid; r < it.count; r += PUSCH_DEMOD_THREADS) {
    const uint32_t ord  = r / NRPHY_NRE;
    const uint32_t subc = NRPHY_NRE * (uint32_t)p.prbs[d.prb_first + ord] + (r - ord * NRPHY_NRE);
    uint32_t       y[NRPHY_MAX_PORTS] = {}, h[2][NRPHY_MAX_PORTS] = {};
#pragma unroll
    for (uint32_t i = 0; i != NRPHY_MAX_PORTS; ++i) {
      if (i < P) {
        y[i]    = p.grid[(((size_t)d.grid_index * p.grid_nof_ports + d.rx_ports[i]) * NRPHY_NSYMB + it.symbol) * nsubc + subc];
        h[0][i] = p.ch[d.ce_offset + ((size_t)i * NRPHY_NSYMB + it.symbol) * nsubc + subc];
      }
    }
    float2 x[2];
    float  v[2];
    equalize_re(d.equalizer, 1u, P, y, h, nv, nv_max, 1.0f, x, v);
    s.buf[0][r] = make_cf(x[0].x, x[0].y);
    s.var[r]    = v[0];
    if (!__builtin_isinf(v[0])) { // pusch_demodulator_impl.cpp:203-215
      vsum += (double)v[0];
      vcnt += 1.0;
    }
  }

  // Wave 0: the symbol's scrambling bits, as in pusch_demod_item.
  const uint32_t first_word = it.bit_offset >> 5;
  const uint32_t nwords     = ((it.bit_offset & 31u) + it.count * QM + 31u) >> 5;
  if (tid < WAVE) {
    gold_sequence_blocks_wave(p.gold, d.c_init, first_word, nwords, s.seq, lane, [&](uint32_t base, uint32_t avail) {
      for (uint32_t k = lane; k < avail; k += WAVE) {
        s.seq[base + k] ^= p.x1_words[first_word + base + k];
      }
      wave_lds_fence();
    });
  }

  const cf* z     = mixed_dft_inverse(plan, s.buf[0], s.buf[1], tid);
  uint8_t*  stage = reinterpret_cast<uint8_t*>(z == s.buf[0] ? s.buf[1] : s.buf[0]);

  int8_t*        dst   = p.llr + (size_t)it.pusch * p.llr_stride + it.bit_offset;
  const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
  for (uint32_t r = tid; r < it.count; r += PUSCH_DEMOD_THREADS) {
    const cf    zr = z[r];
    const float re = __fmul_rn(zr.x, plan.scale), im = __fmul_rn(zr.y, plan.scale); // transform_precoder_dft_impl.cpp:53-56
    LlrBytes    out;
    if (r < it.nof_vector) {
      demodulate_symbol<MOD, true>(dm, s.t, r, re, im, s.var[r], out, 0);
    } else {
      demodulate_symbol<MOD, false>(dm, s.t, r, re, im, s.var[r], out, 0);
    }
    if constexpr (EVM) { // the deprecoded symbol and its soft bits before descrambling
      esum += (double)evm_term<MOD>(out, 0, r, re, im, p.evm_scale[demod_slot<MOD>()]);
    }
    const uint32_t b0   = (it.bit_offset & 31u) + r * QM;
    const uint64_t pair = ((uint64_t)s.seq[b0 >> 5] << 32) | s.seq[(b0 >> 5) + 1u];
    const uint32_t bits = (uint32_t)(pair >> (48u - (b0 & 31u))) & 0xFFFFu; // first soft bit in bit 15
#pragma unroll
    for (uint32_t w = 0; w != (QM + 3u) / 4u; ++w) {
      out.w[w] = negate_bytes(out.w[w], byte_masks_msb_first((bits >> (12u - 4u * w)) & 0xFu));
    }
    uint8_t* st = stage + shift + r * QM;
#pragma unroll
    for (uint32_t k = 0; k != QM; ++k) {
      st[k] = out.get(k);
    }
  }

  // SINR partial sums of the symbol: a thread's RE in ascending order, wave sums, then the four waves in order.
  vsum = wave_sum(vsum);
  vcnt = wave_sum(vcnt);
  if (lane == 0) {
    s.red[0][tid / WAVE] = vsum;
    s.red[1][tid / WAVE] = vcnt;
  }
  if constexpr (EVM) { // a thread's symbols in ascending order, then as the SINR sums
    esum = wave_sum(esum);
    if (lane == 0) {
      s.evm_red[tid / WAVE] = esum;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double* part = p.partial + 2u * (size_t)(p.n_items + blockIdx.x);
    part[0]      = (s.red[0][0] + s.red[0][1]) + (s.red[0][2] + s.red[0][3]);
    part[1]      = (s.red[1][0] + s.red[1][1]) + (s.red[1][2] + s.red[1][3]);
    if constexpr (EVM) {
      p.evm_partial[p.n_items + blockIdx.x] = (s.evm_red[0] + s.evm_red[1]) + (s.evm_red[2] + s.evm_red[3]);
    }
  }
  store_staged(stage, dst - shift, shift, shift + it.count * QM, tid);
}

template <bool EVM>
__global__ __launch_bounds__(PUSCH_DEMOD_THREADS) void pusch_tp_demod_kernel(PuschDemodLaunch p)
{
  __shared__ PuschTpShared s;
  const PuschTpItem     it   = p.tp_items[blockIdx.x];
  const PuschDemodDesc& d    = p.desc[it.pusch];
  const MixedDftPlan&   plan = p.dft[it.dft]; // read in place: a copy indexed by the stage would be put in LDS
  switch (d.qm) { // workgroup-uniform
    case 1:
      pusch_tp_item<NRPHY_MOD_PI2_BPSK, EVM>(p, it, d, plan, s);
      break;
    case NRPHY_MOD_QPSK:
      pusch_tp_item<NRPHY_MOD_QPSK, EVM>(p, it, d, plan, s);
      break;
    case NRPHY_MOD_QAM16:
      pusch_tp_item<NRPHY_MOD_QAM16, EVM>(p, it, d, plan, s);
      break;
    case NRPHY_MOD_QAM64:
      pusch_tp_item<NRPHY_MOD_QAM64, EVM>(p, it, d, plan, s);
      break;
    default:
      pusch_tp_item<NRPHY_MOD_QAM256, EVM>(p, it, d, plan, s);
      break;
  }
}

// One wave per PUSCH: its items' partial sums in a fixed order, then the SINR (pusch_demodulator_impl.cpp:255-262).
__global__ __launch_bounds__(WAVE) void pusch_sinr_kernel(PuschDemodLaunch p)
{
  const uint32_t       lane = threadIdx.x;
  const PuschDemodDesc d    = p.desc[blockIdx.x];
  double               sum = 0.0, cnt = 0.0;
  for (uint32_t k = lane; k < d.nof_items; k += WAVE) {
    sum += p.partial[2u * (size_t)(d.item_first + k)];
    cnt += p.partial[2u * (size_t)(d.item_first + k) + 1u];
  }
  sum = wave_sum(sum);
  cnt = wave_sum(cnt);
  if (lane == 0) {
    p.sinr[blockIdx.x] = (cnt != 0.0 && sum > 0.0) ? (float)(-10.0 * log10(sum / cnt)) : F_INF;
  }
}

// One wave per PUSCH: lane k adds the partial sums of the PUSCH's k-th OFDM symbol with data in item order and takes the symbol's
// EVM, e_s = sqrt(P_s / n_s) (evm_calculator_generic_impl.cpp:72); then every lane runs pusch_demodulator_impl.cpp:249-251 and
// :275 over the symbols in ascending order in float -- acc += n_s * e_s, cnt += n_s, acc / cnt -- and lane 0 stores.
__global__ __launch_bounds__(WAVE) void pusch_evm_kernel(PuschDemodLaunch p)
{
  const uint32_t      lane = threadIdx.x;
  const PuschEvmDesc& d    = p.evm_desc[blockIdx.x];
  float               e    = 0.f;
  uint32_t            n    = 0;
  if (lane < d.nof_symbols) {
    double sum = 0.0;
    for (uint32_t k = d.item_first[lane]; k != d.item_first[lane + 1u]; ++k) {
      sum += p.evm_partial[k];
    }
    n = d.count[lane];
    e = __fsqrt_rn((float)(sum / (double)n));
  }
  float    acc = 0.f;
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t k = 0; k != NRPHY_NSYMB; ++k) {
    const float    ek = __shfl(e, k);
    const uint32_t nk = __shfl(n, k);
    if (k < d.nof_symbols) {
      acc = __fadd_rn(acc, __fmul_rn((float)nk, ek));
      cnt += nk;
    }
  }
  if (lane == 0) {
    p.evm[blockIdx.x] = __fdiv_rn(acc, (float)cnt); // a plan has no PUSCH without data RE
  }
}

} // namespace

hipError_t launch_channel_equalize(const EqualizeLaunch& p, hipStream_t stream)
{
  if (p.n_batch == 0 || p.nof_re == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(channel_equalize_kernel, dim3((p.nof_re + 255u) / 256u, p.n_batch), dim3(256), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_pusch_demod(const PuschDemodLaunch& p, hipStream_t stream)
{
  if (p.n_items == 0 && p.n_tp_items == 0) {
    return hipSuccess;
  }
  const bool evm = p.evm != nullptr; // uniform over the launch: the kernels without EVM are the ones of nrphy_pusch_demod_run
  if (p.n_items != 0) {
    hipLaunchKernelGGL(evm ? pusch_demod_kernel<true> : pusch_demod_kernel<false>, dim3(p.n_items), dim3(PUSCH_DEMOD_THREADS), 0,
                       stream, p);
  }
  if (p.n_tp_items != 0) {
    hipLaunchKernelGGL(evm ? pusch_tp_demod_kernel<true> : pusch_tp_demod_kernel<false>, dim3(p.n_tp_items),
                       dim3(PUSCH_DEMOD_THREADS), 0, stream, p);
  }
  if (p.sinr != nullptr) {
    hipLaunchKernelGGL(pusch_sinr_kernel, dim3(p.n_pusch), dim3(WAVE), 0, stream, p);
  }
  if (evm) {
    hipLaunchKernelGGL(pusch_evm_kernel, dim3(p.n_pusch), dim3(WAVE), 0, stream, p);
  }
  return hipGetLastError();
}

} // namespace nrphy
