// CRC24B (TS 38.212 Section 5.1, g = x^24 + x^23 + x^6 + x^5 + x + 1) without tables, and the range arithmetic of the
// word-aligned segmentation: plain C++ that the codeblock kernel (codeblock_build_device.h) and a host test program
// (tests/crc24b_fold_check.cpp) compile from this one text.
//
// The generator factors: g = (x + 1) (x^23 + x^5 + 1).  Modulo the trinomial p = x^23 + x^5 + 1, x^23 = x^5 + 1: a polynomial
// H x^23 + L (L below 2^23) is congruent to H + (H << 5) + L, so two such folds take 55 bits down to 23 with shifts and XORs.
// Modulo x + 1 a polynomial is the parity of its coefficients.  The two residues give the residue modulo g back (Chinese
// remainder theorem): it is r or r + p, r the residue modulo p, and p has odd parity, so the parities decide.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define NRPHY_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define NRPHY_HD inline
#endif

namespace nrphy {

constexpr uint32_t CRC24B_P      = 0x800021u; // x^23 + x^5 + 1
constexpr uint32_t CRC24B_P_MASK = 0x7FFFFFu;

// (hi x^23 + lo) mod p for any 32-bit hi and lo below 2^23: the one function behind the word step and the finish.
NRPHY_HD uint32_t crc24b_fold(uint32_t hi, uint32_t lo)
{
  const uint32_t low = hi ^ (hi << 5) ^ lo; // bits 0..31 of hi (x^5 + 1) + lo; hi >> 27 holds its bits 32..36
  const uint32_t h2  = (low >> 23) | ((hi >> 27) << 9); // (a funnel shift: v_alignbit_b32)
  return (low & CRC24B_P_MASK) ^ h2 ^ (h2 << 5); // h2 below 2^14: nothing reaches bit 23
}

// One Horner step in x^32: (r x^32 + word) mod p, r below 2^23.
NRPHY_HD uint32_t crc24b_fold_word(uint32_t r, uint32_t word)
{
  const uint32_t hi = (r << 9) | (word >> 23);
  return crc24b_fold(hi, word & CRC24B_P_MASK);
}

// The CRC24B register after the words: (W x^24) mod g for W = the words folded into `r` by crc24b_fold_word; `parity_word`
// = the XOR of those words (its parity is W mod (x + 1), and so is that of W x^24).
NRPHY_HD uint32_t crc24b_fold_finish(uint32_t r, uint32_t parity_word)
{
  const uint32_t rp  = crc24b_fold(r << 1, 0u); // (r x^24) mod p
  const uint32_t odd = (uint32_t)__builtin_popcount(rp ^ parity_word) & 1u;
  return rp ^ (odd ? CRC24B_P : 0u);
}

// Codeblock segmentation when the codeblock's first bit lies on a word boundary of the transport block.  The codeblock takes
// `used` bits of it: `whole` words as they are, then, if `tail_mask` is not zero, one word of which the bits in
// `tail_mask` (MSB first) belong to it; every word from `loads` on is zero.
struct SegAligned {
  uint32_t whole;
  uint32_t loads;     // words read from the transport block: whole + (tail_mask != 0)
  uint32_t tail_mask;
};
NRPHY_HD SegAligned seg_aligned(uint32_t used)
{
  const uint32_t whole = used >> 5, rem = used & 31u;
  return {whole, whole + (rem != 0u ? 1u : 0u), rem != 0u ? 0xFFFFFFFFu << (32u - rem) : 0u};
}
// Word j of the codeblock from transport-block word j (`msb_first`: its bytes in stream order, first byte in the MSBs; zero
// for j >= loads, which is not read).
NRPHY_HD uint32_t seg_aligned_word(const SegAligned& seg, uint32_t j, uint32_t msb_first)
{
  return msb_first & (j == seg.whole ? seg.tail_mask : 0xFFFFFFFFu);
}

// The same at any bit offset: the codeblock's 32 bits from bit `shift` of the word pair (hi : lo), both MSB first, of which
// the first `remaining` belong to it.
NRPHY_HD uint32_t seg_unaligned_word(uint32_t hi, uint32_t lo, uint32_t shift, uint32_t remaining)
{
  const uint32_t v = (hi << shift) | ((lo >> 1) >> (31u - shift)); // upper word of (hi : lo) << shift, shift = 0 included
  return remaining < 32u ? v & (0xFFFFFFFFu << (32u - remaining)) : v; // (remaining > 0)
}

} // namespace nrphy
