// Stand-alone check of csrc/ul_slot_state_host.h (no GPU, no HIP): the order rules of an uplink slot and the layout of its result
// block, exactly as ul_slot_async.cpp uses them.  Built and run by tests/test_ul_slot_state_host.py, once plainly and once under
// the host sanitizers; every span the layout hands out is written in a heap block of exactly the layout's size, so an overlap or
// an overrun is a wrong byte or a sanitizer report.
#include "ul_slot_state_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                                    \
      std::exit(1);                                                                                                    \
    }                                                                                                                  \
  } while (0)

static unsigned checks = 0;

static UlSlotLimits limits(uint32_t nsymb, uint32_t pusch, uint32_t pucch, uint32_t pf2, uint32_t srs, uint32_t tb, uint32_t uci)
{
  UlSlotLimits l;
  l.nsymb        = nsymb;
  l.max_pusch    = pusch;
  l.max_pucch    = pucch;
  l.max_pf2      = pf2;
  l.max_srs      = srs;
  l.max_tb_bytes = tb;
  l.max_uci_bits = uci;
  return l;
}

// ---- order rules -------------------------------------------------------------------------------------------------------------
static void order_rules(uint32_t nsymb)
{
  UlSlotState s;
  ul_slot_state_init(s, limits(nsymb, 2, 2, 2, 2, 100, 100));
  // nothing delivered: no receiver, no run that does not start at 0, no empty run, no run beyond the slot
  for (uint32_t start = 0; start != 16; ++start) {
    for (uint32_t n = 0; n != 16; ++n) {
      CHECK(ul_slot_accept_receiver(s, start, n) == NRPHY_ERR_ARGUMENT);
      CHECK((ul_slot_accept_samples(s, start, n) == NRPHY_OK) == (start == 0 && n >= 1 && n <= nsymb));
      checks += 2;
    }
  }
  CHECK(ul_slot_accept_samples(s, 0, 0xFFFFFFFFu) == NRPHY_ERR_ARGUMENT);
  CHECK(ul_slot_accept_samples(s, 0xFFFFFFFFu, 2) == NRPHY_ERR_ARGUMENT);
  CHECK(ul_slot_accept_open_call(s) == NRPHY_OK);
  // every prefix delivered in every split into runs of 1..3 symbols: a receiver is accepted exactly when its last symbol is in
  for (uint32_t step = 1; step != 4; ++step) {
    ul_slot_state_open(s);
    while (s.symbols != nsymb) {
      const uint32_t n = step < nsymb - s.symbols ? step : nsymb - s.symbols;
      CHECK(ul_slot_accept_samples(s, s.symbols + 1, n) == NRPHY_ERR_ARGUMENT); // skips a symbol
      CHECK(s.symbols == 0 || ul_slot_accept_samples(s, s.symbols - 1, n) == NRPHY_ERR_ARGUMENT); // repeats one
      CHECK(ul_slot_accept_samples(s, s.symbols, nsymb - s.symbols + 1) == NRPHY_ERR_ARGUMENT);
      CHECK(ul_slot_accept_samples(s, s.symbols, n) == NRPHY_OK);
      s.symbols += n;
      for (uint32_t start = 0; start != 15; ++start) {
        for (uint32_t len = 1; len != 15; ++len) {
          CHECK((ul_slot_accept_receiver(s, start, len) == NRPHY_OK) == (start + len <= s.symbols));
          ++checks;
        }
      }
      CHECK(ul_slot_accept_receiver(s, 0, 0) == NRPHY_ERR_ARGUMENT);
      CHECK(ul_slot_accept_receiver(s, 0xFFFFFFFFu, 2) == NRPHY_ERR_ARGUMENT); // start + len does not wrap
      CHECK(ul_slot_accept_receiver(s, 1, 0xFFFFFFFFu) == NRPHY_ERR_ARGUMENT);
    }
    CHECK(ul_slot_accept_samples(s, nsymb, 1) == NRPHY_ERR_ARGUMENT);
  }
  // symbols declared by the caller: the count only grows, up to the symbols a slot has (12 of the 14 rows with extended CP)
  ul_slot_state_open(s);
  CHECK(ul_slot_accept_symbols_written(s, 0) == NRPHY_OK);
  CHECK(ul_slot_accept_symbols_written(s, 5) == NRPHY_OK);
  s.symbols = 5;
  CHECK(ul_slot_accept_symbols_written(s, 4) == NRPHY_ERR_ARGUMENT);
  CHECK(ul_slot_accept_symbols_written(s, 5) == NRPHY_OK);
  for (uint32_t upto = 6; upto != 17; ++upto) {
    CHECK((ul_slot_accept_symbols_written(s, upto) == NRPHY_OK) == (upto <= nsymb));
  }
  CHECK(ul_slot_accept_symbols_written(s, 0xFFFFFFFFu) == NRPHY_ERR_ARGUMENT);
  CHECK(ul_slot_accept_receiver(s, 3, 2) == NRPHY_OK && ul_slot_accept_receiver(s, 3, 3) == NRPHY_ERR_ARGUMENT);
  // a grid filled some other way (load_grid, symbols_written up to the slot's last symbol): no sample run fits behind it ...
  s.symbols = nsymb;
  for (uint32_t first = 0; first != 17; ++first) {
    for (uint32_t n = 0; n != 5; ++n) {
      CHECK(ul_slot_accept_samples(s, first, n) == NRPHY_ERR_ARGUMENT);
      ++checks;
    }
  }
  // ... and whatever `symbols` holds, a run that starts at or behind the slot's last symbol is refused: nsymb - first does not wrap
  for (uint32_t have = nsymb; have != 16; ++have) {
    s.symbols = have;
    for (uint32_t n = 0; n != 5; ++n) {
      CHECK(ul_slot_accept_samples(s, have, n) == NRPHY_ERR_ARGUMENT);
      CHECK(ul_slot_accept_samples(s, have, 0xFFFFFFFFu - n) == NRPHY_ERR_ARGUMENT);
      checks += 2;
    }
    CHECK(ul_slot_accept_symbols_written(s, have) == (have <= nsymb ? NRPHY_OK : NRPHY_ERR_ARGUMENT));
  }
  // after finish: nothing but what only reads
  s.symbols  = nsymb;
  s.finished = true;
  CHECK(ul_slot_accept_open_call(s) == NRPHY_ERR_ARGUMENT); // finish twice, load_grid
  CHECK(ul_slot_accept_receiver(s, 0, 1) == NRPHY_ERR_ARGUMENT);
  CHECK(ul_slot_accept_samples(s, nsymb, 1) == NRPHY_ERR_ARGUMENT);
  CHECK(ul_slot_accept_symbols_written(s, 14) == NRPHY_ERR_ARGUMENT);
  // ... and a new open starts over
  ul_slot_state_open(s);
  CHECK(!s.finished && s.symbols == 0 && s.used.n_pusch == 0 && s.used.tb_at == 0 && s.used.uci_at == 0);
  CHECK(ul_slot_accept_samples(s, 0, 1) == NRPHY_OK && ul_slot_accept_open_call(s) == NRPHY_OK);
  checks += 30;
}

// ---- layout ------------------------------------------------------------------------------------------------------------------
struct Claim {
  size_t at, size;
};

// Every claimed range gets a tag of its own; afterwards every range still holds its tag and the rest of the block is untouched.
static void fill_and_verify(const UlSlotLayout& l, const std::vector<Claim>& claims)
{
  std::vector<uint8_t>* block = new std::vector<uint8_t>(l.total, 0xEE);
  for (size_t k = 0; k != claims.size(); ++k) {
    CHECK(claims[k].at + claims[k].size <= l.total);
    if (claims[k].size != 0) {
      std::memset(block->data() + claims[k].at, (int)(k % 200) + 1, claims[k].size);
    }
  }
  size_t claimed = 0;
  for (size_t k = 0; k != claims.size(); ++k) {
    for (size_t i = 0; i != claims[k].size; ++i) {
      CHECK((*block)[claims[k].at + i] == (uint8_t)((k % 200) + 1)); // nobody wrote over it: no overlap
    }
    claimed += claims[k].size;
  }
  size_t untouched = 0;
  for (uint8_t b : *block) {
    untouched += b == 0xEE;
  }
  CHECK(untouched + claimed == l.total);
  delete block;
  ++checks;
}

static void layout_of(const UlSlotLimits& lim, const std::vector<uint32_t>& call_sizes)
{
  const UlSlotLayout l = ul_slot_layout(lim);
  const size_t       at[] = {l.pusch, l.pucch, l.pf2_status, l.pf2_csi, l.srs, l.tb, l.uci, l.host_bytes, l.pf2_llr};
  for (size_t k = 0; k != sizeof(at) / sizeof(at[0]); ++k) {
    CHECK(at[k] % 64 == 0);
    CHECK(k == 0 || at[k] >= at[k - 1]);
  }
  CHECK(l.pusch == 0 && l.total % 64 == 0 && l.total >= 64 && l.host_bytes <= l.pf2_llr && l.pf2_llr <= l.total);
  CHECK(l.pucch - l.pusch >= (size_t)lim.max_pusch * sizeof(nrphy_pusch_result_t));
  CHECK(l.pf2_status - l.pucch >= (size_t)lim.max_pucch * sizeof(nrphy_pucch_result_t));
  CHECK(l.pf2_csi - l.pf2_status >= (size_t)lim.max_pf2 * sizeof(uint32_t));
  CHECK(l.srs - l.pf2_csi >= (size_t)lim.max_pf2 * sizeof(nrphy_pf2_csi_t));
  CHECK(l.tb - l.srs >= (size_t)lim.max_srs * sizeof(nrphy_srs_result_t));
  CHECK(l.uci - l.tb >= ul_slot_tb_region_bytes(lim));
  CHECK(l.host_bytes - l.uci >= lim.max_uci_bits);
  CHECK(l.total - l.pf2_llr >= (size_t)lim.max_pf2 * UL_SLOT_PF2_LLR_BYTES || lim.max_pf2 == 0);

  // Calls of call_sizes[k] PDUs each, kind after kind, until the limits say stop; sizes rotate over awkward values.
  static const uint32_t tb_sizes[] = {1, 3, 4, 5, 255, 256, 257, 0};
  static const uint32_t uci_sizes[] = {0, 1, 11, 12, 0, 3};
  UlSlotState           s;
  ul_slot_state_init(s, lim);
  std::vector<Claim> claims;
  uint32_t           turn = 0;
  for (uint32_t n : call_sizes) {
    // PUSCH: a call is taken whole or not at all
    UlSlotUsed              used = s.used;
    std::vector<UlSlotSpan> tb(n), uci(n);
    int                     rc = NRPHY_OK;
    uint32_t                want_tb = 0, want_uci = 0;
    for (uint32_t i = 0; i != n && rc == NRPHY_OK; ++i, ++turn) {
      const uint32_t tb_bytes = tb_sizes[turn % 8], uci_bits = uci_sizes[turn % 6];
      want_tb += tb_bytes;
      want_uci += uci_bits;
      rc = ul_slot_take_pusch(lim, used, tb_bytes, uci_bits, tb[i], uci[i]);
    }
    const bool fits = s.used.n_pusch + n <= lim.max_pusch && s.used.tb_bytes + want_tb <= lim.max_tb_bytes &&
                      s.used.uci_at + want_uci <= lim.max_uci_bits;
    CHECK(n == 0 || rc == NRPHY_OK || rc == NRPHY_ERR_CAPACITY);
    if (rc == NRPHY_OK && n != 0) {
      CHECK(fits);
      for (uint32_t i = 0; i != n; ++i) {
        CHECK(tb[i].at % 4 == 0);
        CHECK(tb[i].at + tb[i].size <= ul_slot_tb_region_bytes(lim) && uci[i].at + uci[i].size <= lim.max_uci_bits);
        claims.push_back({l.pusch + (size_t)(s.used.n_pusch + i) * sizeof(nrphy_pusch_result_t), sizeof(nrphy_pusch_result_t)});
        claims.push_back({l.tb + tb[i].at, tb[i].size});
        claims.push_back({l.uci + uci[i].at, uci[i].size});
        CHECK((l.pusch + (size_t)(s.used.n_pusch + i) * sizeof(nrphy_pusch_result_t)) % 8 == 0);
      }
      s.used = used;
    } else if (n != 0) {
      CHECK(!fits); // (the sums stop at the PDU that was refused: they are already over a limit there)
    }
    // format 2: messages share the UCI region with the PUSCH payloads
    used = s.used;
    std::vector<UlSlotSpan> msg(n);
    rc       = NRPHY_OK;
    want_uci = 0;
    for (uint32_t i = 0; i != n && rc == NRPHY_OK; ++i) {
      const uint32_t bits = 3 + 7 * i;
      want_uci += bits;
      rc = ul_slot_take_pf2(lim, used, bits, msg[i]);
    }
    const bool pf2_fits = s.used.n_pf2 + n <= lim.max_pf2 && s.used.uci_at + want_uci <= lim.max_uci_bits;
    CHECK((rc == NRPHY_OK) == pf2_fits || n == 0);
    if (rc == NRPHY_OK && n != 0) {
      for (uint32_t i = 0; i != n; ++i) {
        const uint32_t k = s.used.n_pf2 + i;
        claims.push_back({l.uci + msg[i].at, msg[i].size});
        claims.push_back({l.pf2_status + (size_t)k * 4, 4});
        claims.push_back({l.pf2_csi + (size_t)k * sizeof(nrphy_pf2_csi_t), sizeof(nrphy_pf2_csi_t)});
        claims.push_back({l.pf2_llr + (size_t)k * UL_SLOT_PF2_LLR_BYTES, UL_SLOT_PF2_LLR_BYTES});
        CHECK(l.uci + msg[i].at + msg[i].size <= l.host_bytes);
      }
      s.used = used;
    }
    // PUCCH formats 0 / 1 and SRS: counts
    used = s.used;
    if (ul_slot_take_count(lim.max_pucch, used.n_pucch, n) == NRPHY_OK) {
      CHECK(s.used.n_pucch + n <= lim.max_pucch);
      for (uint32_t i = 0; i != n; ++i) {
        claims.push_back({l.pucch + (size_t)(s.used.n_pucch + i) * sizeof(nrphy_pucch_result_t), sizeof(nrphy_pucch_result_t)});
      }
      s.used = used;
    } else {
      CHECK(s.used.n_pucch + n > lim.max_pucch && used.n_pucch == s.used.n_pucch);
    }
    used = s.used;
    if (ul_slot_take_count(lim.max_srs, used.n_srs, n) == NRPHY_OK) {
      CHECK(s.used.n_srs + n <= lim.max_srs);
      for (uint32_t i = 0; i != n; ++i) {
        const size_t here = l.srs + (size_t)(s.used.n_srs + i) * sizeof(nrphy_srs_result_t);
        CHECK(here % 8 == 0);
        claims.push_back({here, sizeof(nrphy_srs_result_t)});
      }
      s.used = used;
    } else {
      CHECK(s.used.n_srs + n > lim.max_srs && used.n_srs == s.used.n_srs);
    }
  }
  fill_and_verify(l, claims);
}

// One byte, one bit or one PDU under, on and over each limit.
static void capacity_edges()
{
  const UlSlotLimits lim = limits(14, 3, 2, 2, 1, 1000, 50);
  UlSlotSpan         tb, uci, msg;
  for (int delta = -1; delta <= 1; ++delta) {
    UlSlotUsed u;
    CHECK(ul_slot_take_pusch(lim, u, 400, 20, tb, uci) == NRPHY_OK);
    CHECK(ul_slot_take_pusch(lim, u, 401, 10, tb, uci) == NRPHY_OK && tb.at == 400 && uci.at == 20);
    const UlSlotUsed before = u;
    // the third block starts at 804 (401 rounded up) and may still take what max_tb_bytes leaves: 199 bytes
    const int rc = ul_slot_take_pusch(lim, u, (uint32_t)(199 + delta), 0, tb, uci);
    CHECK(rc == (delta <= 0 ? NRPHY_OK : NRPHY_ERR_CAPACITY));
    if (rc == NRPHY_OK) {
      CHECK(tb.at == 804 && tb.at + tb.size <= ul_slot_tb_region_bytes(lim) && u.n_pusch == 3 && u.tb_bytes == 1000u + delta);
      CHECK(ul_slot_take_pusch(lim, u, 0, 0, tb, uci) == NRPHY_ERR_CAPACITY); // a fourth PDU, however small
    } else {
      CHECK(std::memcmp(&before, &u, sizeof(u)) == 0);
    }
    UlSlotUsed v = before;
    CHECK(ul_slot_take_pusch(lim, v, 0, (uint32_t)(20 + delta), tb, uci) == (delta <= 0 ? NRPHY_OK : NRPHY_ERR_CAPACITY));
    v = before;
    CHECK(ul_slot_take_pf2(lim, v, (uint32_t)(20 + delta), msg) == (delta <= 0 ? NRPHY_OK : NRPHY_ERR_CAPACITY));
    CHECK(delta > 0 || (msg.at == 30 && v.uci_at == 50u + delta && v.n_pf2 == 1));
    v = before;
    CHECK(ul_slot_take_pf2(lim, v, 3, msg) == NRPHY_OK && ul_slot_take_pf2(lim, v, 3, msg) == NRPHY_OK);
    CHECK(ul_slot_take_pf2(lim, v, 3, msg) == NRPHY_ERR_CAPACITY && v.n_pf2 == 2);
    uint32_t n = 0;
    CHECK(ul_slot_take_count(2, n, (uint32_t)(2 + delta)) == (delta <= 0 ? NRPHY_OK : NRPHY_ERR_CAPACITY));
    CHECK(n == (delta <= 0 ? 2u + delta : 0u));
    CHECK(ul_slot_take_count(2, n, 0xFFFFFFFFu) == NRPHY_ERR_CAPACITY);
    checks += 12;
  }
  // sizes near 2^32 do not wrap
  UlSlotUsed u;
  CHECK(ul_slot_take_pusch(lim, u, 10, 10, tb, uci) == NRPHY_OK);
  CHECK(ul_slot_take_pusch(lim, u, 0xFFFFFFFFu, 0, tb, uci) == NRPHY_ERR_CAPACITY);
  CHECK(ul_slot_take_pusch(lim, u, 0, 0xFFFFFFFFu, tb, uci) == NRPHY_ERR_CAPACITY);
  CHECK(ul_slot_take_pf2(lim, u, 0xFFFFFFF7u, msg) == NRPHY_ERR_CAPACITY);
  // nothing allowed at all
  const UlSlotLimits none = limits(14, 0, 0, 0, 0, 0, 0);
  UlSlotUsed         z;
  CHECK(ul_slot_take_pusch(none, z, 0, 0, tb, uci) == NRPHY_ERR_CAPACITY && ul_slot_take_pf2(none, z, 0, msg) == NRPHY_ERR_CAPACITY);
  CHECK(ul_slot_layout(none).total == 64 && ul_slot_layout(none).host_bytes == 0);
  checks += 6;
}

int main()
{
  order_rules(14);
  order_rules(12);
  const UlSlotLimits shapes[] = {limits(14, 1, 1, 1, 1, 257, 12),   limits(14, 3, 3, 3, 3, 600, 40),  limits(14, 8, 16, 4, 2, 1100, 64),
                                 limits(12, 64, 64, 64, 8, 8192, 900), limits(14, 5, 0, 0, 0, 4, 0),   limits(14, 0, 7, 0, 3, 0, 0),
                                 limits(14, 2, 2, 2, 2, 1u << 20, 1706 * 2)};
  for (const UlSlotLimits& lim : shapes) {
    const uint32_t max = lim.max_pusch > lim.max_pf2 ? lim.max_pusch : lim.max_pf2;
    layout_of(lim, {1});
    layout_of(lim, {3});
    layout_of(lim, {max});
    layout_of(lim, {max + 1});
    layout_of(lim, {1, 3, max, 1, 3});
    layout_of(lim, {3, 1, 1, 1, 3, max});
    layout_of(lim, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1});
  }
  capacity_edges();
  std::printf("ok: %u checks\n", checks);
  return 0;
}
