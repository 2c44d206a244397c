// First stage of a PDSCH codeblock wave (pdsch_kernels.hip): the LDS of the wave, segmentation of the transport block and
// the TB and CB CRC attachment.  One wavefront builds one codeblock; the LDPC encoder (ldpc_device.h) takes it from there.
#pragma once

#include "bits_device.h"
#include "crc24b_fold.h"
#include "ldpc_device.h"
#include "nrphy_internal.h"

namespace nrphy {

// ================================================================================================================
// Codeblock construction in LDS (TS 38.212 Section 5.2.2; reference: ldpc_segmenter_impl.cpp:148-217).
// ================================================================================================================
// LDS of one codeblock wavefront: `lin` (the codeblock, sized per launch from the largest one the plan contains) and one
// scratch region `u` that the stages of the wave use one after the other:
//   building the codeblock   --                                (the codeblock CRC folds in registers: crc24b_fold.h)
//   LDPC                     u[0, LDPC_DBL_WORDS)              the systematic blocks doubled (ldpc_device.h)
//                            then LdpcScratch (core rows), then row pointers + edges of the lifted graph rows needed
//   output stage             u[0, 512)                         the modulation table (index = Qm bits, value = ci8 symbol as floats)
//                            u[512, ...)                       interleaver output: one byte per modulation symbol
// At the headline configuration that is 1.3 + 3.2 KB of LDS per wave: 8 waves per SIMD fit the CU's 160 KB.  (The codeblock
// CRC once went through three byte tables in u[0, 768); a plan whose graph rows and symbol bytes need less than that -- few
// parity rows, few RE per work item -- now takes the smaller region.)
constexpr uint32_t CB_U_QAM_WORDS     = 512;
constexpr uint32_t CB_U_LDPC_WORDS    = (sizeof(LdpcScratch) / 4u + 3u) & ~3u;
constexpr uint32_t CB_U_GRAPH_OFFSET  = LDPC_DBL_WORDS + CB_U_LDPC_WORDS;
static_assert(CB_U_GRAPH_OFFSET == NRPHY_CB_U_GRAPH_OFFSET, "host and device agree on the layout of the scratch region");

struct CbShared {
  uint32_t* lin;   // codeblock bits, (Kb + rows) * Zc bits (+ read-ahead)
  uint32_t* u;     // the scratch region
  uint32_t* symb;  // u + CB_U_QAM_WORDS
  uint32_t* graph; // u + CB_U_GRAPH_OFFSET
  LdpcScratch* ldpc; // u + LDPC_DBL_WORDS
};

// Segmentation: lin[0, total_words) <- the `used` transport-block bits from bit `tb_pos` on, then zeros (the TB CRC and the
// zero padding of the last codeblock, the CB CRC, the filler bits and the parity region).
// The transport-block words of SEG_UNROLL trips are requested before the first is used: taken trip by trip, every trip
// waited out a trip to memory (stage timing: this loop alone cost 0.045 ms per 1024 slots for a hundred instructions).
constexpr uint32_t SEG_UNROLL = 5; // 320 words: a whole high-rate codeblock with its four core parity blocks
static_assert(WAVE * SEG_UNROLL * 32u >= 22u * 384u, "one trip holds the payload of the largest codeblock");

// The codeblock starts on a word boundary of the transport block: always the first one, and all of them when info_bits is a
// multiple of 32, as at the headline.  The limits are wave-uniform (seg_aligned, crc24b_fold.h): a row of 64 words below the
// first limit is load, byte swap, store behind scalar branches; only the one row that holds the limits tests its lanes and
// masks the codeblock's last word; the rows behind it are zeros.
constexpr uint32_t SEG_WHOLE_ROWS = 22u * 384u / 32u / WAVE; // 4: rows of whole payload words in the largest codeblock
__device__ __forceinline__ void segment_aligned(const uint32_t* src, uint32_t used, uint32_t* lin, uint32_t total_words, uint32_t lane)
{
  const SegAligned seg  = seg_aligned(used);
  const uint32_t   rows = seg.whole / WAVE; // <= SEG_WHOLE_ROWS
  const uint32_t   j    = rows * WAVE + lane; // this lane's word of the row with the limits
  uint32_t         w[SEG_WHOLE_ROWS];
#pragma unroll
  for (uint32_t k = 0; k != SEG_WHOLE_ROWS; ++k) {
    if (k < rows) {
      w[k] = src[WAVE * k + lane];
    }
  }
  uint32_t edge = 0;
  if (j < seg.loads) { // never a word that lies entirely beyond the transport block
    edge = src[j];
  }
#pragma unroll
  for (uint32_t k = 0; k != SEG_WHOLE_ROWS; ++k) {
    if (k < rows) {
      lin[WAVE * k + lane] = __builtin_bswap32(w[k]);
    }
  }
  if (j < total_words) {
    lin[j] = seg_aligned_word(seg, j, __builtin_bswap32(edge)); // (the words behind the last one were not loaded: zero)
  }
  for (uint32_t z = j + WAVE; z < total_words; z += WAVE) {
    lin[z] = 0u;
  }
}

// Any bit offset: two words per codeblock word, a funnel shift, and the bounds per word.
__device__ __forceinline__ void segment_unaligned(const uint32_t* tbw, uint32_t tb_bits, uint32_t tb_pos, uint32_t used, uint32_t* lin,
                                                  uint32_t total_words, uint32_t lane)
{
  for (uint32_t base = lane; base < total_words; base += WAVE * SEG_UNROLL) {
    uint32_t hi[SEG_UNROLL], lo[SEG_UNROLL];
#pragma unroll
    for (uint32_t k = 0; k != SEG_UNROLL; ++k) {
      const uint32_t pos = 32u * (base + WAVE * k);
      hi[k] = 0;
      lo[k] = 0;
      if (pos < used) { // never touch words that lie entirely beyond the transport block
        const uint32_t abs_pos = tb_pos + pos;
        const uint32_t i = abs_pos >> 5, sft = abs_pos & 31u;
        hi[k] = tbw[i];
        if (sft != 0 && 32u * (i + 1) < tb_bits) {
          lo[k] = tbw[i + 1];
        }
      }
    }
#pragma unroll
    for (uint32_t k = 0; k != SEG_UNROLL; ++k) {
      const uint32_t j = base + WAVE * k, pos = 32u * j;
      if (j < total_words) {
        uint32_t v = 0;
        if (pos < used) {
          v = seg_unaligned_word(__builtin_bswap32(hi[k]), __builtin_bswap32(lo[k]), (tb_pos + pos) & 31u, used - pos);
        }
        lin[j] = v;
      }
    }
  }
}

// Fills lin with the K bits of codeblock `cb` (payload, TB CRC + zero padding on the last codeblock, CB CRC, filler
// zeros) and zeroes the parity region up to `total_words`.
__device__ inline void build_codeblock(PduRef pd, uint32_t cb, const uint32_t* tbw, const uint32_t* tb_crc_part,
                                       const GoldTables* tables, CbShared* sh, uint32_t total_words, uint32_t lane,
                                       uint32_t profile_stage)
{
  const bool     last   = (cb == pd.C - 1);
  const uint32_t used   = pd.info_bits - (last ? pd.tb_crc_bits + pd.zero_pad : 0u);
  const uint32_t tb_pos = cb * pd.info_bits;
  if ((tb_pos & 31u) == 0) { // wave-uniform
    segment_aligned(tbw + (tb_pos >> 5), used, sh->lin, total_words, lane);
  } else {
    segment_unaligned(tbw, pd.tb_bytes * 8u, tb_pos, used, sh->lin, total_words, lane);
  }
  wave_sync();
  if (profile_stage == 7) {
    return;
  }
  if (last) { // wave-uniform: the transport-block CRC = XOR of the shares of its regions (prologue)
    const uint32_t tb_crc = wave_xor(lane < pd.crc_count ? tb_crc_part[pd.crc_first + lane] : 0u);
    if (lane == 0) {
      or_bits_lds_exclusive(sh->lin, used, tb_crc << (32u - pd.tb_crc_bits), pd.tb_crc_bits);
    }
  }
  wave_sync();
  if (pd.cb_crc_bits) {
    // CRC24B over the first info_bits bits.  Leading zeros do not change a zero-initialised CRC, so the bit string
    // is right-aligned to a word boundary: word j holds message bits [32j - pad, 32j - pad + 32).
    const uint32_t n   = pd.info_bits;
    const uint32_t pad = (32u - (n & 31u)) & 31u;
    const uint32_t nw  = (n + pad) >> 5;
    const uint32_t per = (nw + WAVE - 1) / WAVE;
    uint32_t       a   = lane * per;
    uint32_t       b   = a + per;
    a                  = a > nw ? nw : a;
    b                  = b > nw ? nw : b;
    // The lane's words are requested together and folded modulo x^23 + x^5 + 1 in registers, no table (crc24b_fold.h).  Every
    // lane takes `per` steps that end at its word b - 1: a lane with fewer words leads with `skip` zero words, which leave
    // the zero residue and the parity alone, so only the reads test the lane.
    constexpr uint32_t CRC_MAX_PER = (22u * 384u / 32u + WAVE - 1u) / WAVE; // words per lane of the largest codeblock
    const uint32_t     first = b - per, skip = a - first;
    uint32_t           word[CRC_MAX_PER];
    if (pad == 0) { // wave-uniform
#pragma unroll
      for (uint32_t i = 0; i != CRC_MAX_PER; ++i) {
        word[i] = 0;
        if (i < per && i >= skip) {
          word[i] = sh->lin[first + i];
        }
      }
    } else {
#pragma unroll
      for (uint32_t i = 0; i != CRC_MAX_PER; ++i) {
        const uint32_t j = first + i;
        word[i]          = 0;
        if (i < per && i >= skip) {
          word[i] = (j == 0) ? sh->lin[0] >> pad : ext32(sh->lin, 32u * j - pad);
        }
      }
    }
    uint32_t res = 0, parity = 0;
#pragma unroll
    for (uint32_t i = 0; i != CRC_MAX_PER; ++i) {
      if (i < per) { // wave-uniform
        res = crc24b_fold_word(res, word[i]);
        parity ^= word[i];
      }
    }
    const uint32_t reg = crc24b_fold_finish(res, parity); // the CRC24B register after the lane's words
    // The lane's partial times x^(32 (nw - b)): six independent table look-ups (one per nibble).
    uint32_t part = 0;
    {
      const uint32_t m = nw - b;
#pragma unroll
      for (uint32_t k = 0; k != 6; ++k) {
        part ^= tables->crc24b_mul[m][k][(reg >> (4u * k)) & 15u];
      }
    }
    uint32_t crc = wave_xor(part);
    if (lane == 0) {
      or_bits_lds_exclusive(sh->lin, n, crc << 8, 24);
    }
    wave_sync();
  }
}

} // namespace nrphy
