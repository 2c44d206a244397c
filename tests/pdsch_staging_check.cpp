// Stand-alone host check of the device-free layout part of csrc/pdsch_staging_host.h (tests/test_pdsch_staging_host.py builds
// and runs it): pdsch_staging_layout + pdsch_staging_copy_blocks for 1, 3 and 64 PDUs with every block size of the list, and
// totals that land exactly on and one byte past a 256-byte boundary.
#include "pdsch_staging_host.h"

#include <cstdio>
#include <cstdlib>

static const uint32_t SIZES[] = {1, 3, 4, 5, 255, 256, 257};
static const uint8_t  FILL    = 0xA5; // what the region holds before a call
static long           nof_cases = 0, nof_blocks = 0;

#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                                    \
      std::exit(1);                                                                                                    \
    }                                                                                                                  \
  } while (0)

// One call with blocks of the given sizes; every block sits in a heap allocation of exactly its size, so that a read beyond
// it is an error under the address sanitizer.
static void run_case(const std::vector<uint32_t>& sizes)
{
  const uint32_t                    n = (uint32_t)sizes.size();
  std::vector<nrphy_pdsch_pdu_t>    pdus(n);
  std::vector<std::vector<uint8_t>> blocks(n);
  std::vector<const uint8_t*>       tbs(n);
  std::memset(pdus.data(), 0, n * sizeof(nrphy_pdsch_pdu_t));
  for (uint32_t i = 0; i != n; ++i) {
    pdus[i].tb_size_bytes = sizes[i];
    blocks[i].resize(sizes[i]);
    for (uint32_t b = 0; b != sizes[i]; ++b) {
      blocks[i][b] = (uint8_t)(1 + (i * 131 + b * 7) % 255); // never zero, never confused with the padding
    }
    tbs[i] = blocks[i].data();
  }
  PdschStagingLayout l;
  CHECK(pdsch_staging_layout(n, pdus.data(), tbs.data(), l) == NRPHY_OK);
  CHECK(l.tb_off.size() == n);
  size_t end = 0;
  for (uint32_t i = 0; i != n; ++i) {
    CHECK(l.tb_off[i] % 4 == 0);
    CHECK(l.tb_off[i] == end); // back to back
    end += ((size_t)sizes[i] + 7) & ~(size_t)3;
  }
  CHECK(l.tb_total == end);
  CHECK(l.tables_at % 256 == 0 && l.tables_at >= l.tb_total && l.tables_at - l.tb_total < 256);

  // The region up to tables_at and a guard behind it, which must keep its fill (as must the bytes from tb_total to tables_at).
  const size_t         guard = 64;
  std::vector<uint8_t> region(l.tables_at + guard, FILL);
  pdsch_staging_copy_blocks(l, n, pdus.data(), tbs.data(), region.data());
  for (uint32_t i = 0; i != n; ++i) {
    const size_t next = i + 1 != n ? (size_t)l.tb_off[i + 1] : l.tb_total;
    CHECK(std::memcmp(region.data() + l.tb_off[i], blocks[i].data(), sizes[i]) == 0);
    const size_t pad = next - l.tb_off[i] - sizes[i];
    CHECK(pad >= 4 && pad <= 7);
    for (size_t b = l.tb_off[i] + sizes[i]; b != next; ++b) {
      CHECK(region[b] == 0);
    }
    ++nof_blocks;
  }
  for (size_t b = l.tb_total; b != region.size(); ++b) {
    CHECK(region[b] == FILL); // nothing between the blocks' end and tables_at, nothing beyond tables_at
  }

  // A later call's blocks behind an earlier call's: the region before the offset stays as it was.
  std::vector<uint8_t> two(2 * l.tables_at + guard, FILL);
  pdsch_staging_copy_blocks(l, n, pdus.data(), tbs.data(), two.data() + l.tables_at);
  for (size_t b = 0; b != l.tables_at; ++b) {
    CHECK(two[b] == FILL);
  }
  CHECK(std::memcmp(two.data() + l.tables_at, region.data(), l.tables_at + guard) == 0);
  // ... and the last block alone, placed where it lies in this call, leaves everything before its offset as it was.
  {
    const uint32_t       k = n - 1;
    PdschStagingLayout   single;
    std::vector<uint8_t> one(region.size(), FILL);
    CHECK(pdsch_staging_layout(1, &pdus[k], &tbs[k], single) == NRPHY_OK);
    pdsch_staging_copy_blocks(single, 1, &pdus[k], &tbs[k], one.data() + l.tb_off[k]);
    for (size_t b = 0; b != l.tb_off[k]; ++b) {
      CHECK(one[b] == FILL);
    }
    CHECK(std::memcmp(one.data() + l.tb_off[k], region.data() + l.tb_off[k], region.size() - l.tb_off[k]) == 0);
  }

  // Refusals: a null block or an empty one, at the first, a middle and the last place, before anything is written -- the
  // layout part never sees the region, and the layout it returns is not used.
  const uint32_t places[3] = {0, n / 2, n - 1};
  for (uint32_t at : places) {
    std::vector<const uint8_t*> bad_tbs = tbs;
    bad_tbs[at]                       = nullptr;
    PdschStagingLayout bad;
    CHECK(pdsch_staging_layout(n, pdus.data(), bad_tbs.data(), bad) == NRPHY_ERR_ARGUMENT);
    std::vector<nrphy_pdsch_pdu_t> bad_pdus = pdus;
    bad_pdus[at].tb_size_bytes            = 0;
    CHECK(pdsch_staging_layout(n, bad_pdus.data(), tbs.data(), bad) == NRPHY_ERR_ARGUMENT);
  }
  ++nof_cases;
}

int main()
{
  const size_t nof_sizes = sizeof(SIZES) / sizeof(SIZES[0]);
  // One PDU: every size.
  for (uint32_t a : SIZES) {
    run_case({a});
  }
  // Three PDUs: every ordered triple of sizes.
  for (uint32_t a : SIZES) {
    for (uint32_t b : SIZES) {
      for (uint32_t c : SIZES) {
        run_case({a, b, c});
      }
    }
  }
  // 64 PDUs: one size throughout, and the list in rotation from every start.
  for (size_t first = 0; first != nof_sizes; ++first) {
    std::vector<uint32_t> same(64, SIZES[first]), mixed(64);
    for (size_t i = 0; i != 64; ++i) {
      mixed[i] = SIZES[(first + i) % nof_sizes];
    }
    run_case(same);
    run_case(mixed);
  }
  // Totals exactly on a 256-byte boundary and one byte past the last size that still reaches it: a block of s bytes takes
  // (s + 7) & ~3, so 249..252 give 256 and 253 gives 260; the same behind blocks that fill 256 and 512 bytes before it.
  for (uint32_t last : {249U, 252U, 253U}) {
    run_case({last});
    run_case({252, last});
    run_case({252, 252, last});
    std::vector<uint32_t> many(63, 252);
    many.push_back(last);
    run_case(many);
  }
  {
    const nrphy_pdsch_pdu_t pdu_on = [] { nrphy_pdsch_pdu_t p; std::memset(&p, 0, sizeof(p)); p.tb_size_bytes = 252; return p; }();
    nrphy_pdsch_pdu_t       pdu_past = pdu_on;
    pdu_past.tb_size_bytes           = 253;
    const uint8_t      byte[253] = {};
    const uint8_t*     tb        = byte;
    PdschStagingLayout l;
    CHECK(pdsch_staging_layout(1, &pdu_on, &tb, l) == NRPHY_OK && l.tb_total == 256 && l.tables_at == 256);
    CHECK(pdsch_staging_layout(1, &pdu_past, &tb, l) == NRPHY_OK && l.tb_total == 260 && l.tables_at == 512);
  }
  std::printf("ok: %ld calls, %ld blocks\n", nof_cases, nof_blocks);
  return 0;
}
