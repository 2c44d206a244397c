// Rate matching and bit interleaving of a PDSCH codeblock wave (pdsch_kernels.hip): the circular-buffer index arithmetic,
// the word gather and phase A of the output stage, which turns the wave's slice of the codeword into one byte per modulation symbol.
#pragma once

#include "bits_device.h"
#include "codeblock_build_device.h"
#include "nrphy_internal.h"

namespace nrphy {

// ================================================================================================================
// Rate matching index arithmetic (TS 38.212 Section 5.4.2; reference: ldpc_rate_matcher_impl.cpp:37-144).
// Bit t of the selected sequence e_0, e_1, ... is circular-buffer bit pos(t); the buffer skips the filler interval
// [fs, fs + flen) and wraps at Ncb.  lin holds the codeblock including the 2*Zc punctured bits, hence the + 2*Zc.
// ================================================================================================================
struct RmIndex {
  uint32_t fs;       // first filler position (clamped to Ncb)
  uint32_t flen;     // filler positions inside the circular buffer
  uint32_t n_valid;  // Ncb - flen
  uint32_t rank0;    // rank of k0 among the valid positions
  float    inv_valid;
};

__device__ __forceinline__ RmIndex rm_index_init(PduRef pd)
{
  RmIndex  r;
  uint32_t nsys = (pd.kb - 2u) * pd.zc;
  uint32_t fs   = nsys - pd.filler;
  uint32_t fe   = nsys;
  fs            = fs > pd.n_cb ? pd.n_cb : fs;
  fe            = fe > pd.n_cb ? pd.n_cb : fe;
  r.fs          = fs;
  r.flen        = fe - fs;
  r.n_valid     = pd.n_cb - r.flen;
  r.rank0       = pd.k0 < fs ? pd.k0 : (pd.k0 < fe ? fs : pd.k0 - r.flen);
  r.inv_valid   = 1.0f / (float)r.n_valid;
  return r;
}

// 32 consecutive selected bits e_t .. e_(t+31), first bit in the MSB (bits beyond the codeblock's E are don't-care).
// A run of selected bits is contiguous in lin until it meets the filler gap or the end of the circular buffer; the
// common case is one funnel read, crossings are stitched piece by piece.  WRAP = false: rank0 + E <= n_valid.
template <bool WRAP>
__device__ __forceinline__ uint32_t rm_gather32(const RmIndex& r, const uint32_t* lin, uint32_t zc2, uint32_t t)
{
  uint32_t u = r.rank0 + t;
  if (WRAP && u >= r.n_valid) {
    uint32_t q = (uint32_t)((float)u * r.inv_valid);
    u -= q * r.n_valid;
    if ((int32_t)u < 0) {
      u += r.n_valid;
    } else if (u >= r.n_valid) {
      u -= r.n_valid;
    }
  }
  uint32_t run = (u < r.fs) ? r.fs - u : r.n_valid - u; // selected bits until the next discontinuity
  uint32_t out = ext32(lin, (u < r.fs ? u : u + r.flen) + zc2);
  if (run >= 32u) {
    return out;
  }
  out &= topmask(run);
  uint32_t filled = run;
  while (filled < 32u) {
    u += run;
    if (u >= r.n_valid) {
      if (!WRAP) {
        break; // past the end of the selection: the remaining bits are never used
      }
      u = 0;
    }
    run            = (u < r.fs) ? r.fs - u : r.n_valid - u;
    run            = run > 32u - filled ? 32u - filled : run;
    uint32_t piece = ext32(lin, (u < r.fs ? u : u + r.flen) + zc2);
    out |= (piece & topmask(run)) >> filled;
    filled += run;
  }
  return out;
}

// 8x8 bit-matrix transposition of the 64-bit word (hi:lo), rows = bytes (most significant first), columns = bits
// (most significant first): three rounds of masked swaps (Hacker's Delight 7-3), on 32-bit halves.
// Bits of a where m is set, bits of b elsewhere: ONE v_bitop3_b32 (truth table 0xCA).  Written as (a & m) | (b & ~m) with
// constant masks the compiler re-associated the shifts and masks of transpose8x8 into some sixty and / or / shift
// instructions per transposition; this way it is two shifts and two of these per half and round.
__device__ __forceinline__ uint32_t bit_select(uint32_t m, uint32_t a, uint32_t b)
{
  return __builtin_amdgcn_bitop3_b32(m, a, b, 0xCA);
}

__device__ __forceinline__ void transpose8x8(uint32_t& hi, uint32_t& lo)
{
  // Each round keeps the bits under one mask, takes the left-shifted word under a second one and the right-shifted
  // word elsewhere (the three masks partition the word): two shifts and two bit-selects.
  hi = bit_select(0xAA55AA55u, hi, bit_select(0x55005500u, hi << 7, hi >> 7));
  lo = bit_select(0xAA55AA55u, lo, bit_select(0x55005500u, lo << 7, lo >> 7));
  hi = bit_select(0xCCCC3333u, hi, bit_select(0x33330000u, hi << 14, hi >> 14));
  lo = bit_select(0xCCCC3333u, lo, bit_select(0x33330000u, lo << 14, lo >> 14));
  const uint32_t nhi = bit_select(0xF0F0F0F0u, hi, lo >> 4);
  const uint32_t nlo = bit_select(0x0F0F0F0Fu, lo, hi << 4);
  hi                 = nhi;
  lo                 = nlo;
}

// ================================================================================================================
// Output stage of the codeblock kernel for one (modulation order, layer count).
//
// Phase A -- rate matching + bit interleaving (TS 38.212 Section 5.4.2.2) as a bit-matrix transposition: the
//   interleaver writes E/Qm-bit rows and reads columns, so 32 consecutive modulation symbols are the columns of
//   Qm row words.  A lane gathers the Qm row words of its 32 symbols and transposes them 8x8-block-wise into one
//   byte per symbol (symbol bits in the byte's MSBs) -- 8x less work than extracting bit by bit.
// Phase B -- per RE: scramble, QAM table lookup, layer mapping + precoding, bf16, coalesced stores (re_map_device.h).
//
// The two phases are separate functions and read the PDU descriptor where they use it (scalar loads through the
// constant address space) instead of carrying its fields from the top of the kernel: as one function inlined 32 times
// into one kernel the scalar register file overflowed (106 SGPRs, 393 spilled, 2,387 v_readlane restores -- vector
// instructions in a kernel bound by vector issue).
// ================================================================================================================
template <int QM, int L, bool WRAP>
__device__ __forceinline__ void phase_a(const PdschLaunch& p, PduRef pd, const CbWork& wk, const CbShared& sh,
                                        uint32_t E, uint32_t lane)
{
  const uint32_t esym = E / QM; // rows of the bit interleaver have esym bits
  const uint32_t zc2  = 2u * pd.zc;
  const RmIndex  rm   = rm_index_init(pd);
  const uint32_t s0   = wk.re_begin * L;             // first modulation symbol of the chunk (multiple of 32)
  const uint32_t nblk = (wk.re_count * L + 31u) >> 5;
  // The modulation table's trip to memory starts here and ends behind the two passes below.
  constexpr uint32_t LUT_TRIPS = ((1u << QM) + WAVE - 1u) / WAVE;
  float2             lut[LUT_TRIPS];
#pragma unroll
  for (uint32_t k = 0; k != LUT_TRIPS; ++k) {
    lut[k] = lane + WAVE * k < (1u << QM) ? p.gold->qam_lut[QM / 2 - 1][lane + WAVE * k] : make_float2(0.f, 0.f);
  }
  // Two passes over the wave's 64 lanes instead of one lane per block (a 281-RE codeblock has 36 blocks: 36 busy lanes doing
  // Qm gathers and four transpositions each).  First the Qm * nblk row words, one gather per item, into the block's eight
  // words of `symb` (word 8 blk + j = row j); then the 4 * nblk (block, byte column) items: eight byte reads, one 8x8
  // transposition, two words back into the same eight words (the four items of a block sit in neighbouring lanes of one
  // instruction: all their reads precede their writes).
  for (uint32_t item = lane; item < QM * nblk; item += WAVE) {
    const uint32_t blk = item / QM, j = item - blk * QM;
    sh.symb[8u * blk + j] = rm_gather32<WRAP>(rm, sh.lin, zc2, j * esym + s0 + 32u * blk);
  }
  wave_sync();
  const uint8_t* rows = reinterpret_cast<const uint8_t*>(sh.symb);
  for (uint32_t item = lane; item < 4u * nblk; item += WAVE) {
    const uint32_t blk = item >> 2, m = item & 3u;
    const uint8_t* b   = rows + 32u * blk + (3u - m); // byte 3 - m of a row word holds its columns 8m .. 8m + 7
    uint32_t       r8[8];
#pragma unroll
    for (int j = 0; j != 8; ++j) {
      r8[j] = (j < QM) ? b[4 * j] : 0u;
    }
    uint32_t hi = (r8[0] << 24) | (r8[1] << 16) | (r8[2] << 8) | r8[3];
    uint32_t lo = (r8[4] << 24) | (r8[5] << 16) | (r8[6] << 8) | r8[7];
    transpose8x8(hi, lo);
    sh.symb[8u * blk + 2u * m]      = hi;
    sh.symb[8u * blk + 2u * m + 1u] = lo;
  }
  if (lane < 8) {
    sh.symb[8u * nblk + lane] = 0; // read-ahead padding
  }
  // Modulation table, requested before the gathers (`lut` above), into the scratch region behind the symbol bytes' use of it.
#pragma unroll
  for (uint32_t k = 0; k != LUT_TRIPS; ++k) {
    if (lane + WAVE * k < (1u << QM)) {
      reinterpret_cast<float2*>(sh.u)[lane + WAVE * k] = lut[k];
    }
  }
  wave_sync();
}

} // namespace nrphy
