// Host check of csrc/crc24b_fold.h, the text the codeblock kernel compiles (tests/test_crc24b_fold_host.py builds and runs it):
//   1. the table-free CRC24B -- one pass and split over the 64 lanes exactly as build_codeblock() splits it -- against bitwise
//      long division by 0x1800063;
//   2. the segmentation's range arithmetic, aligned and unaligned, against a bit-by-bit model, with the words it reads.
// Usage: crc24b_fold_check RANDOM_MESSAGES_PER_LENGTH.  Prints a summary line and exits 0, or the first mismatch and exits 1.
#include "crc24b_fold.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace nrphy;

namespace {

constexpr uint32_t WAVE = 64;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

int fail(const char* what, uint32_t a, uint32_t b, uint32_t got, uint32_t want)
{
  std::printf("MISMATCH %s (%u, %u): got %08x want %08x\n", what, a, b, got, want);
  return 1;
}

uint32_t get_bit(const std::vector<uint32_t>& a, uint32_t pos)
{
  return (a[pos >> 5] >> (31u - (pos & 31u))) & 1u;
}

// The reference: the remainder of M(x) x^24 by g(x) = 0x1800063, one message bit at a time.
uint32_t crc24b_division(const std::vector<uint32_t>& msg, uint32_t nbits)
{
  uint32_t reg = 0;
  for (uint32_t i = 0; i < nbits; i += 32) {
    uint32_t       w = msg[i >> 5];
    const uint32_t k = nbits - i < 32u ? nbits - i : 32u;
    for (uint32_t s = 0; s != k; ++s, w <<= 1) {
      const uint32_t top = ((reg >> 23) ^ (w >> 31)) & 1u;
      reg                = (reg << 1) & 0xFFFFFFu;
      reg ^= top ? 0x800063u : 0u;
    }
  }
  return reg;
}

// a x^(32 m) mod g, bit by bit: what GoldTables::crc24b_mul[m] holds per nibble of a.
uint32_t mul_x32m(uint32_t a, uint32_t m)
{
  static std::vector<uint32_t> pow32; // x^(32 m) mod g
  if (pow32.empty()) {
    uint32_t v = 1;
    for (uint32_t i = 0; i != 321; ++i) {
      pow32.push_back(v);
      for (uint32_t s = 0; s != 32; ++s) {
        v <<= 1;
        if (v & 0x1000000u) {
          v ^= 0x1800063u;
        }
      }
    }
  }
  uint32_t r = 0; // a pow32[m] mod g, Horner over the bits of a
  for (int i = 23; i >= 0; --i) {
    r <<= 1;
    if (r & 0x1000000u) {
      r ^= 0x1800063u;
    }
    if ((a >> i) & 1u) {
      r ^= pow32[m];
    }
  }
  return r;
}

// 32 bits from bit `pos` of an MSB-first array (bits_device.h, ext32).
uint32_t ext32(const std::vector<uint32_t>& a, uint32_t pos)
{
  const uint32_t x = a[pos >> 5], y = a[(pos >> 5) + 1], sh = pos & 31u;
  return (x << sh) | ((y >> 1) >> (31u - sh));
}

// build_codeblock()'s CRC stage over lin[0, n bits): word j of the right-aligned message, the lanes' shares, their sum.
uint32_t message_word(const std::vector<uint32_t>& lin, uint32_t j, uint32_t pad)
{
  return pad == 0 ? lin[j] : (j == 0 ? lin[0] >> pad : ext32(lin, 32u * j - pad));
}

uint32_t crc24b_by_lanes(const std::vector<uint32_t>& lin, uint32_t n)
{
  const uint32_t pad = (32u - (n & 31u)) & 31u, nw = (n + pad) >> 5, per = (nw + WAVE - 1) / WAVE;
  uint32_t       crc = 0;
  for (uint32_t lane = 0; lane != WAVE; ++lane) {
    uint32_t a = lane * per, b = a + per;
    a          = a > nw ? nw : a;
    b          = b > nw ? nw : b;
    const uint32_t first = b - per, skip = a - first;
    uint32_t       res = 0, parity = 0;
    for (uint32_t i = 0; i != per; ++i) {
      const uint32_t word = i >= skip ? message_word(lin, first + i, pad) : 0u;
      res                 = crc24b_fold_word(res, word);
      parity ^= word;
    }
    crc ^= mul_x32m(crc24b_fold_finish(res, parity), nw - b);
  }
  return crc;
}

uint32_t crc24b_one_pass(const std::vector<uint32_t>& lin, uint32_t n)
{
  const uint32_t pad = (32u - (n & 31u)) & 31u, nw = (n + pad) >> 5;
  uint32_t       res = 0, parity = 0;
  for (uint32_t j = 0; j != nw; ++j) {
    const uint32_t word = message_word(lin, j, pad);
    res                 = crc24b_fold_word(res, word);
    parity ^= word;
  }
  return crc24b_fold_finish(res, parity);
}

int check_message(std::vector<uint32_t>& lin, uint32_t n, uint32_t tag)
{
  // bits beyond the message are not part of it: the kernel's array holds zeros (CRC position) there
  if (n & 31u) {
    lin[n >> 5] &= 0xFFFFFFFFu << (32u - (n & 31u));
  }
  for (size_t k = (n + 31u) >> 5; k != lin.size(); ++k) {
    lin[k] = 0;
  }
  const uint32_t want = crc24b_division(lin, n);
  uint32_t       got  = crc24b_one_pass(lin, n);
  if (got != want) {
    return fail("one pass", n, tag, got, want);
  }
  got = crc24b_by_lanes(lin, n);
  if (got != want) {
    return fail("lane split", n, tag, got, want);
  }
  return 0;
}

int check_crc(uint32_t nof_random, unsigned long* count)
{
  const uint32_t rems[] = {0, 1, 8, 24, 31};
  for (uint32_t words = 1; words <= 320; ++words) {
    for (uint32_t rem : rems) {
      const uint32_t        n = 32u * (words - 1) + (rem ? rem : 32u); // `words` words when right-aligned, n % 32 = rem
      std::vector<uint32_t> lin(words + 2);
      int                   bad = 0;
      lin.assign(words + 2, 0u);
      bad |= check_message(lin, n, 0);
      lin.assign(words + 2, 0xFFFFFFFFu);
      bad |= check_message(lin, n, 1);
      const uint32_t single[] = {0, n - 1, n / 2, rnd() % n, rnd() % n, rnd() % n};
      for (uint32_t pos : single) {
        lin.assign(words + 2, 0u);
        lin[pos >> 5] = 0x80000000u >> (pos & 31u);
        bad |= check_message(lin, n, 2);
      }
      for (uint32_t r = 0; r != nof_random && !bad; ++r) {
        for (uint32_t& w : lin) {
          w = rnd();
        }
        bad |= check_message(lin, n, 3);
      }
      if (bad) {
        return 1;
      }
      *count += 8 + nof_random;
    }
  }
  return 0;
}

// ---- segmentation ------------------------------------------------------------------------------------------------------
struct Reads {
  uint32_t limit; // words of the transport block that may be read: its bytes rounded up to a multiple of 4
  bool     beyond = false;
  uint32_t word(const std::vector<uint8_t>& tb, uint32_t i) // bytes 4i .. 4i + 3, first byte in the MSBs (a byte swap of the load)
  {
    if (i >= limit) {
      beyond = true;
      return 0;
    }
    return (uint32_t)tb[4 * i] << 24 | (uint32_t)tb[4 * i + 1] << 16 | (uint32_t)tb[4 * i + 2] << 8 | tb[4 * i + 3];
  }
};

// build_codeblock()'s segmentation, word by word with the kernel's own tests for what is read.
void segment(const std::vector<uint8_t>& tb, uint32_t tb_bytes, uint32_t tb_pos, uint32_t used, uint32_t total_words,
             std::vector<uint32_t>& lin, Reads& rd)
{
  if ((tb_pos & 31u) == 0) {
    const SegAligned seg = seg_aligned(used);
    for (uint32_t j = 0; j != total_words; ++j) {
      const uint32_t w = j < seg.loads ? rd.word(tb, (tb_pos >> 5) + j) : 0u;
      lin[j]           = j < seg.whole ? w : seg_aligned_word(seg, j, w);
    }
    return;
  }
  const uint32_t tb_bits = tb_bytes * 8u;
  for (uint32_t j = 0; j != total_words; ++j) {
    const uint32_t pos = 32u * j;
    uint32_t       v   = 0;
    if (pos < used) {
      const uint32_t abs_pos = tb_pos + pos, i = abs_pos >> 5, sft = abs_pos & 31u;
      const uint32_t hi = rd.word(tb, i);
      const uint32_t lo = (sft != 0 && 32u * (i + 1) < tb_bits) ? rd.word(tb, i + 1) : 0u;
      v                 = seg_unaligned_word(hi, lo, sft, used - pos);
    }
    lin[j] = v;
  }
}

int check_one_segment(const std::vector<uint8_t>& tb, uint32_t tb_bytes, uint32_t tb_pos, uint32_t used, uint32_t total_words)
{
  std::vector<uint32_t> lin(total_words, 0xDEADBEEFu);
  Reads                 rd;
  rd.limit = (tb_bytes + 3u) / 4u;
  segment(tb, tb_bytes, tb_pos, used, total_words, lin, rd);
  if (rd.beyond) {
    return fail("read beyond the transport block", tb_pos, used, 0, 0);
  }
  for (uint32_t k = 0; k != 32u * total_words; ++k) {
    uint32_t want = 0;
    if (k < used) {
      const uint32_t p = tb_pos + k;
      want             = (tb[p >> 3] >> (7u - (p & 7u))) & 1u;
    }
    if (get_bit(lin, k) != want) {
      return fail("segmentation bit", tb_pos, used, k, want);
    }
  }
  return 0;
}

int check_segmentation(unsigned long* count)
{
  // Every (tb_pos & 31, used & 31) pair, short and long codeblocks (none, some and four rows of whole words; a last word that
  // closes a row of 64), in the middle of a transport block and with the codeblock's last bit its last bit.
  const uint32_t whole_words[] = {0, 1, 2, 63, 64, 65, 127, 200, 255, 256, 261, 263};
  for (uint32_t start = 0; start != 32; ++start) {
    for (uint32_t rem = 0; rem != 32; ++rem) {
      for (uint32_t whole : whole_words) {
        const uint32_t used = 32u * whole + rem;
        if (used == 0) {
          continue;
        }
        for (uint32_t at_end = 0; at_end != 2; ++at_end) {
          const uint32_t tb_pos = 32u * (rnd() % 5u) + start;
          uint32_t       bits   = tb_pos + used + (at_end ? 0u : 8u * (1u + rnd() % 600u));
          if (bits & 7u) {
            if (at_end) {
              continue; // a transport block is whole bytes
            }
            bits = (bits + 7u) & ~7u;
          }
          const uint32_t       tb_bytes = bits / 8u;
          std::vector<uint8_t> tb(((tb_bytes + 3u) & ~3u) + 8u);
          for (uint8_t& x : tb) {
            x = (uint8_t)rnd();
          }
          const uint32_t total_words = ((used + 31u) >> 5) + 1u + rnd() % 200u;
          if (check_one_segment(tb, tb_bytes, tb_pos, used, total_words)) {
            return 1;
          }
          ++*count;
        }
      }
    }
  }
  // Last codeblocks: C codeblocks of info_bits each hold the transport block, its CRC of 16 or 24 bits and the zero padding.
  for (uint32_t tb_crc : {16u, 24u}) {
    for (uint32_t zero_pad : {0u, 1u, 5u, 31u, 40u}) {
      for (uint32_t C : {1u, 2u, 3u, 7u}) {
        for (uint32_t info_bits = 100; info_bits != 100 + 64; ++info_bits) {
          const uint32_t total = C * info_bits;
          if (total <= tb_crc + zero_pad + 8u || (total - tb_crc - zero_pad) % 8u != 0 || (C - 1) * info_bits >= total - tb_crc - zero_pad) {
            continue;
          }
          const uint32_t       tb_bytes = (total - tb_crc - zero_pad) / 8u;
          std::vector<uint8_t> tb(((tb_bytes + 3u) & ~3u) + 8u);
          for (uint8_t& x : tb) {
            x = (uint8_t)rnd();
          }
          for (uint32_t cb = 0; cb != C; ++cb) {
            const uint32_t used = info_bits - (cb == C - 1 ? tb_crc + zero_pad : 0u);
            if (check_one_segment(tb, tb_bytes, cb * info_bits, used, (info_bits + 24u + 31u) / 32u + 6u)) {
              return 1;
            }
            ++*count;
          }
        }
      }
    }
  }
  return 0;
}

} // namespace

int main(int argc, char** argv)
{
  const uint32_t nof_random = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 200u;
  unsigned long  messages = 0, segments = 0;
  if (check_crc(nof_random, &messages) || check_segmentation(&segments)) {
    return 1;
  }
  std::printf("ok: %lu messages, %lu codeblock segments\n", messages, segments);
  return 0;
}
