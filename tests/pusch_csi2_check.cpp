// Stand-alone check of csrc/pusch_csi2_host.h (no GPU, no HIP): the checks of a CSI part 2 size description, its evaluation on a
// CSI part 1 payload and the enumeration of its sizes, exactly as pusch_csi2_host.cpp uses them.  Built and run by
// tests/test_pusch_csi2_host.py, once plainly and once under the address and undefined-behaviour sanitizers.
#include "pusch_csi2_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                                    \
      std::exit(1);                                                                                                    \
    }                                                                                                                  \
    ++checks;                                                                                                          \
  } while (0)

static unsigned checks = 0;

namespace {

nrphy_pusch_csi2_desc_t blank()
{
  nrphy_pusch_csi2_desc_t d;
  std::memset(&d, 0, sizeof(d));
  return d;
}

// One entry {offset, width} with the map given.
nrphy_pusch_csi2_desc_t one_entry(uint32_t offset, uint32_t width, std::vector<uint32_t> map)
{
  nrphy_pusch_csi2_desc_t d = blank();
  d.nof_entries               = 1;
  d.entries[0].nof_parameters = 1;
  d.entries[0].offset[0]      = offset;
  d.entries[0].width[0]       = width;
  d.entries[0].map_size       = (uint32_t)map.size();
  for (size_t i = 0; i != map.size() && i != 16; ++i) {
    d.entries[0].map[i] = map[i];
  }
  return d;
}

// uci_part2_get_size written the reference's way: the slice read into a 64-bit word with its first bit lowest, the word's bits
// reversed, shifted down by 64 - width.
uint32_t size_by_reversal(const nrphy_pusch_csi2_desc_t& d, const std::vector<uint8_t>& bits)
{
  uint32_t result = 0;
  for (uint32_t e = 0; e != d.nof_entries; ++e) {
    uint32_t index = 0;
    for (uint32_t k = 0; k != d.entries[e].nof_parameters; ++k) {
      const uint32_t width = d.entries[e].width[k];
      uint64_t       slice = 0;
      for (uint32_t j = 0; j != width; ++j) {
        slice |= (uint64_t)bits[d.entries[e].offset[k] + j] << j;
      }
      uint64_t reversed = 0;
      for (uint32_t j = 0; j != 64; ++j) {
        reversed |= ((slice >> j) & 1U) << (63 - j);
      }
      index = (index << width) | (width != 0 ? (uint32_t)(reversed >> (64 - width)) : 0U);
    }
    result += d.entries[e].map[index];
  }
  return result;
}

void structure()
{
  const std::vector<uint32_t> four = {0, 1, 2, 7};
  CHECK(pusch_csi2_desc_ok(one_entry(1, 2, four), 6));
  CHECK(pusch_csi2_desc_ok(one_entry(4, 2, four), 6));           // ends with the payload
  CHECK(!pusch_csi2_desc_ok(one_entry(5, 2, four), 6));          // one bit beyond it
  CHECK(!pusch_csi2_desc_ok(one_entry(7, 0, {3}), 6));           // an offset beyond it, even with no bit read
  CHECK(!pusch_csi2_desc_ok(one_entry(0xFFFFFFFFu, 2, four), 6)); // offset + width wraps
  CHECK(!pusch_csi2_desc_ok(one_entry(1, 2, four), 0));          // no CSI part 1
  CHECK(!pusch_csi2_desc_ok(one_entry(1, 2, {0, 1, 2}), 6));     // map_size != 1 << width
  CHECK(!pusch_csi2_desc_ok(one_entry(0, 5, std::vector<uint32_t>(32, 1)), 6));
  CHECK(pusch_csi2_desc_ok(one_entry(0, 0, {9}), 6));            // the fixed size: one parameter of no bits
  CHECK(!pusch_csi2_desc_ok(blank(), 6));                        // no entry is no description
  nrphy_pusch_csi2_desc_t d = one_entry(1, 2, four);
  d.nof_entries             = 3;
  CHECK(!pusch_csi2_desc_ok(d, 6));
  d                           = one_entry(1, 2, four);
  d.entries[0].nof_parameters = 3;
  CHECK(!pusch_csi2_desc_ok(d, 6));
  d                           = one_entry(0, 3, std::vector<uint32_t>(32, 1));
  d.entries[0].nof_parameters = 2; // 3 + 2 bits
  d.entries[0].offset[1]      = 3;
  d.entries[0].width[1]       = 2;
  CHECK(!pusch_csi2_desc_ok(d, 6));
  d.entries[0].width[1] = 1; // 3 + 1 bits, 16 values
  d.entries[0].map_size = 16;
  CHECK(pusch_csi2_desc_ok(d, 6));
}

void evaluation()
{
  // a missing reversal: width 2 with map[1] != map[2]
  const nrphy_pusch_csi2_desc_t d = one_entry(1, 2, {0, 1, 2, 7});
  const uint8_t                 low[6] = {0, 1, 0, 0, 0, 0}, high[6] = {0, 0, 1, 0, 0, 0}, both[6] = {1, 1, 1, 1, 1, 1};
  CHECK(pusch_csi2_size(d, low) == 2); // the payload bit at `offset` is the value's most significant bit
  CHECK(pusch_csi2_size(d, high) == 1);
  CHECK(pusch_csi2_size(d, both) == 7);
  // a swapped parameter order: {0, 1} then {5, 2}, the first parameter in the index's high bit
  nrphy_pusch_csi2_desc_t two = blank();
  two.nof_entries               = 1;
  two.entries[0].nof_parameters = 2;
  two.entries[0].offset[0]      = 0;
  two.entries[0].width[0]       = 1;
  two.entries[0].offset[1]      = 5;
  two.entries[0].width[1]       = 2;
  two.entries[0].map_size       = 8;
  for (uint32_t i = 0; i != 8; ++i) {
    two.entries[0].map[i] = 10 + i;
  }
  const uint8_t first[8] = {1, 0, 0, 0, 0, 0, 0, 0}, second[8] = {0, 0, 0, 0, 0, 1, 0, 0}, third[8] = {0, 0, 0, 0, 0, 0, 1, 0};
  CHECK(pusch_csi2_size(two, first) == 14);
  CHECK(pusch_csi2_size(two, second) == 12);
  CHECK(pusch_csi2_size(two, third) == 11);
  // only bit 0 of a payload byte counts
  const uint8_t wide[6] = {0, 3, 2, 0, 0, 0};
  CHECK(pusch_csi2_size(d, wide) == 2);
}

void random_descriptions()
{
  std::mt19937 rng(7);
  auto         upto = [&](uint32_t n) { return (uint32_t)(rng() % (n + 1)); };
  for (unsigned round = 0; round != 2000; ++round) {
    const uint32_t          nof_bits = 1 + upto(40);
    nrphy_pusch_csi2_desc_t d        = blank();
    d.nof_entries                    = 1 + upto(1);
    for (uint32_t e = 0; e != d.nof_entries; ++e) {
      nrphy_pusch_csi2_entry_t& entry = d.entries[e];
      entry.nof_parameters            = upto(2);
      uint32_t left = NRPHY_PUSCH_CSI2_MAX_ENTRY_BITS, total = 0;
      for (uint32_t k = 0; k != entry.nof_parameters; ++k) {
        entry.width[k]  = upto(std::min(left, nof_bits));
        entry.offset[k] = upto(nof_bits - entry.width[k]);
        left -= entry.width[k];
        total += entry.width[k];
      }
      entry.map_size = 1U << total;
      for (uint32_t i = 0; i != entry.map_size; ++i) {
        entry.map[i] = upto(3) == 0 ? 0 : 3 * upto(5); // few distinct values, zeros among them
      }
    }
    CHECK(pusch_csi2_desc_ok(d, nof_bits));
    uint32_t   n = 0, sizes[NRPHY_PUSCH_CSI2_MAX_VARIANTS];
    const bool fits = pusch_csi2_enumerate(d, &n, sizes);
    std::set<uint32_t> seen;
    for (unsigned t = 0; t != 64; ++t) {
      std::vector<uint8_t> bits(nof_bits);
      for (uint8_t& b : bits) {
        b = (uint8_t)(rng() & 1U);
      }
      const uint32_t size = pusch_csi2_size(d, bits.data());
      CHECK(size == size_by_reversal(d, bits));
      seen.insert(size);
    }
    if (!fits) {
      continue;
    }
    CHECK(n >= 1 && n <= NRPHY_PUSCH_CSI2_MAX_VARIANTS && sizes[0] == 0);
    for (uint32_t i = 1; i != n; ++i) {
      CHECK(sizes[i] > sizes[i - 1]); // ascending and distinct, none of them 0
    }
    for (uint32_t size : seen) { // the table cannot miss
      CHECK(std::find(sizes, sizes + n, size) != sizes + n);
    }
  }
}

void limits()
{
  uint32_t n = 0, sizes[NRPHY_PUSCH_CSI2_MAX_VARIANTS];
  // 16 distinct sizes fit, with size 0 among the map values or not; 17 do not
  std::vector<uint32_t> map(16);
  for (uint32_t i = 0; i != 16; ++i) {
    map[i] = 5 + i;
  }
  CHECK(pusch_csi2_enumerate(one_entry(0, 4, map), &n, sizes) && n == 17 && sizes[1] == 5 && sizes[16] == 20);
  map[3] = 0;
  CHECK(pusch_csi2_enumerate(one_entry(0, 4, map), &n, sizes) && n == 16);
  nrphy_pusch_csi2_desc_t d = one_entry(0, 4, map);
  d.nof_entries             = 2;
  d.entries[1]              = d.entries[0];
  d.entries[1].map[3]       = 100; // 0..20 plus 5..20 and 100: more than 16 sums
  CHECK(!pusch_csi2_enumerate(d, &n, sizes));
  // two entries whose sums coincide: 4 x 4 index pairs, 7 sums, 6 of them above 0
  nrphy_pusch_csi2_desc_t s = one_entry(0, 2, {0, 10, 20, 30});
  s.nof_entries             = 2;
  s.entries[1]              = s.entries[0];
  CHECK(pusch_csi2_enumerate(s, &n, sizes) && n == 7 && sizes[6] == 60);
  // 1706 bits is the most a UCI part may have
  CHECK(pusch_csi2_enumerate(one_entry(0, 1, {1706, 4}), &n, sizes) && n == 3 && sizes[2] == 1706);
  CHECK(!pusch_csi2_enumerate(one_entry(0, 1, {1707, 4}), &n, sizes));
  s.entries[0].map[3] = 1700;
  CHECK(!pusch_csi2_enumerate(s, &n, sizes)); // 1700 + 30
  s.entries[0].map[3] = 0xFFFFFFF0u;          // a sum that wraps
  CHECK(!pusch_csi2_enumerate(s, &n, sizes));
}

} // namespace

int main()
{
  structure();
  evaluation();
  random_descriptions();
  limits();
  std::printf("ok: %u checks\n", checks);
  return 0;
}
