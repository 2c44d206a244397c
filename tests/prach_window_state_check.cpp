// Stand-alone check of csrc/prach_window_state_host.h (no GPU, no HIP): the order rules of a PRACH window, the agreement of the
// two configurations of an open, the pool's limits, the plan key, and the layout of a window's buffer and result block, exactly as
// prach_window_async.cpp uses them.  Built and run by tests/test_prach_window_state_host.py, once plainly and once under the host
// sanitizers; every record and every buffer element a layout hands out is written in a heap block of exactly the layout's size, so
// an overlap or an overrun is a wrong byte or a sanitizer report.
#include "prach_window_state_host.h"

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
    ++checks;                                                                                                          \
  } while (0)

static unsigned checks = 0;

// ---- order rules -------------------------------------------------------------------------------------------------------------
// A window of `length` delivered in runs of `run` samples (cycling through three lengths): every call takes
// min(length - collected, offered), the call that reaches `length` completes it and no call before, and afterwards nothing is accepted.
static void sample_runs(uint32_t length, const uint32_t (&run)[3])
{
  PrachWindowState s;
  prach_window_state_open(s, length);
  CHECK(prach_window_accept_buffer_written(s) == NRPHY_OK); // nothing has happened yet: either way of filling is open
  uint32_t collected = 0, taken = 77, calls = 0;
  while (true) {
    const uint32_t offered = run[calls++ % 3];
    CHECK(prach_window_accept_samples(s, offered, taken) == NRPHY_OK);
    CHECK(taken == (offered < length - collected ? offered : length - collected));
    CHECK(s.collected == collected && !s.completed); // accepting changes nothing
    const bool done = prach_window_commit_samples(s, taken);
    collected += taken;
    CHECK(s.collected == collected && done == (collected == length) && s.completed == done && s.samples_seen);
    CHECK(prach_window_accept_buffer_written(s) == NRPHY_ERR_ARGUMENT); // not after a sample run, complete or not
    if (done) {
      break;
    }
    CHECK(calls < 4 * (uint64_t)length + 8);
  }
  for (uint32_t offered : {0u, 1u, length, 0xFFFFFFFFu}) {
    taken = 77;
    CHECK(prach_window_accept_samples(s, offered, taken) == NRPHY_ERR_ARGUMENT && taken == 0);
  }
  CHECK(prach_window_accept_buffer_written(s) == NRPHY_ERR_ARGUMENT);
  prach_window_state_open(s, length / 2 + 1); // a fresh open forgets all of it
  CHECK(s.collected == 0 && !s.completed && !s.samples_seen && !s.written && s.window_length == length / 2 + 1);
  CHECK(prach_window_accept_samples(s, 1, taken) == NRPHY_OK && taken == 1);
}

static void order_rules()
{
  const uint32_t lengths[] = {1, 2, 1098, 2744, 13872, 92160, 0xFFFFFFFFu};
  const uint32_t runs[][3] = {{1, 1, 1}, {1, 7, 1009}, {0, 3, 0}, {548, 548, 549}, {0xFFFFFFFFu, 1, 1}, {30720, 30720, 30720}, {5000, 0, 100}};
  for (uint32_t length : lengths) {
    for (const auto& run : runs) {
      if ((uint64_t)length / (run[0] / 3 + run[1] / 3 + run[2] / 3 + 1) < 200000) { // keep the walk short
        sample_runs(length, run);
      }
    }
  }
  // a run that overshoots by 100: the remainder is taken
  PrachWindowState s;
  uint32_t         taken = 0;
  prach_window_state_open(s, 2744);
  CHECK(prach_window_accept_samples(s, 2694, taken) == NRPHY_OK && taken == 2694 && !prach_window_commit_samples(s, taken));
  CHECK(prach_window_accept_samples(s, 150, taken) == NRPHY_OK && taken == 50 && prach_window_commit_samples(s, taken));
  // a run of nothing still counts as a sample run
  prach_window_state_open(s, 10);
  CHECK(prach_window_accept_samples(s, 0, taken) == NRPHY_OK && taken == 0 && !prach_window_commit_samples(s, taken));
  CHECK(prach_window_accept_buffer_written(s) == NRPHY_ERR_ARGUMENT);
  // split 7.2: once per open, and no sample run behind it
  prach_window_state_open(s, 10);
  CHECK(prach_window_accept_buffer_written(s) == NRPHY_OK);
  prach_window_commit_buffer_written(s);
  CHECK(s.completed && s.written && s.collected == 0);
  CHECK(prach_window_accept_buffer_written(s) == NRPHY_ERR_ARGUMENT);
  CHECK(prach_window_accept_samples(s, 5, taken) == NRPHY_ERR_ARGUMENT && taken == 0);
  CHECK(prach_window_accept_samples(s, 0, taken) == NRPHY_ERR_ARGUMENT);
}

// ---- the two configurations of an open -----------------------------------------------------------------------------------------
static nrphy_prach_demod_cfg_t demod_cfg(uint32_t srate, uint32_t format, uint32_t mu, uint32_t ports)
{
  nrphy_prach_demod_cfg_t c;
  std::memset(&c, 0, sizeof(c));
  c.srate_hz         = srate;
  c.format           = format;
  c.nof_td_occasions = 1;
  c.nof_fd_occasions = 1;
  c.nof_prb_ul_grid  = 52;
  c.pusch_numerology = mu;
  c.nof_rx_ports     = ports;
  return c;
}

static nrphy_prach_cfg_t detect_cfg(uint32_t format, uint32_t ra_scs, uint32_t ports)
{
  nrphy_prach_cfg_t c;
  std::memset(&c, 0, sizeof(c));
  c.format               = format;
  c.ra_scs               = ra_scs;
  c.nof_preamble_indices = 64;
  c.nof_rx_ports         = ports;
  return c;
}

static void pair_rules()
{
  const uint32_t map[4] = {2, 0, 1, 2};
  // the spacing the demodulator derives: 1.25 kHz for formats 0..2, 5 kHz for format 3, the PUSCH spacing for every short format
  for (uint32_t format = 0; format != NRPHY_PRACH_FORMAT_COUNT; ++format) {
    for (uint32_t mu = 0; mu != 4; ++mu) {
      const uint32_t want = format <= NRPHY_PRACH_FORMAT_2 ? (uint32_t)NRPHY_PRACH_SCS_1_25
                            : format == NRPHY_PRACH_FORMAT_3 ? (uint32_t)NRPHY_PRACH_SCS_5
                                                             : mu;
      CHECK(prach_window_ra_scs(format, mu) == want);
      for (uint32_t scs = 0; scs != NRPHY_PRACH_SCS_COUNT; ++scs) {
        for (uint32_t other = 0; other != NRPHY_PRACH_FORMAT_COUNT; ++other) {
          const int rc = prach_window_pair_agrees(demod_cfg(30720000, format, mu, 2), detect_cfg(other, scs, 2), map, 30720000, 3);
          CHECK((rc == NRPHY_OK) == (other == format && scs == want));
          CHECK(rc == NRPHY_OK || rc == NRPHY_ERR_ARGUMENT);
        }
      }
    }
  }
  const nrphy_prach_demod_cfg_t demod  = demod_cfg(30720000, NRPHY_PRACH_FORMAT_B4, 1, 2);
  const nrphy_prach_cfg_t       detect = detect_cfg(NRPHY_PRACH_FORMAT_B4, NRPHY_PRACH_SCS_30, 2);
  CHECK(prach_window_pair_agrees(demod, detect, map, 30720000, 3) == NRPHY_OK);
  CHECK(prach_window_pair_agrees(demod, detect, map, 30720001, 3) == NRPHY_ERR_ARGUMENT);  // not the pool's rate
  CHECK(prach_window_pair_agrees(demod, detect, map, 61440000, 3) == NRPHY_ERR_ARGUMENT);
  CHECK(prach_window_pair_agrees(demod, detect, nullptr, 30720000, 3) == NRPHY_ERR_ARGUMENT);
  CHECK(prach_window_pair_agrees(demod, detect, map, 30720000, 2) == NRPHY_ERR_ARGUMENT);  // PRACH port 0 wants radio port 2
  CHECK(prach_window_pair_agrees(demod, detect, map, 30720000, 0) == NRPHY_ERR_ARGUMENT);
  for (uint32_t ports = 1; ports != 5; ++ports) {                                           // the port counts must be one
    for (uint32_t other = 1; other != 5; ++other) {
      const int rc = prach_window_pair_agrees(demod_cfg(30720000, NRPHY_PRACH_FORMAT_B4, 1, ports),
                                              detect_cfg(NRPHY_PRACH_FORMAT_B4, NRPHY_PRACH_SCS_30, other), map, 30720000, 3);
      CHECK((rc == NRPHY_OK) == (ports == other));
    }
  }
  // only the mapped entries are looked at: with one port, the out-of-range entries behind it do not matter
  const uint32_t one[4] = {0, 99, 99, 99};
  CHECK(prach_window_pair_agrees(demod_cfg(30720000, NRPHY_PRACH_FORMAT_0, 0, 1), detect_cfg(NRPHY_PRACH_FORMAT_0, NRPHY_PRACH_SCS_1_25, 1),
                                 one, 30720000, 1) == NRPHY_OK);
  CHECK(prach_window_pair_agrees(demod_cfg(30720000, NRPHY_PRACH_FORMAT_0, 0, 2), detect_cfg(NRPHY_PRACH_FORMAT_0, NRPHY_PRACH_SCS_1_25, 2),
                                 one, 30720000, 1) == NRPHY_ERR_ARGUMENT);

  // the plan key: the same bytes reuse, any field or mapped port that differs does not
  PrachWindowKey key;
  CHECK(!prach_window_key_equal(key, demod, detect, map)); // nothing made yet
  prach_window_key_set(key, demod, detect, map);
  CHECK(prach_window_key_equal(key, demod, detect, map));
  const uint32_t same_mapped[4] = {2, 0, 3, 3}; // ports beyond nof_rx_ports are not part of the map
  CHECK(prach_window_key_equal(key, demod, detect, same_mapped));
  const uint32_t swapped[4] = {0, 2, 1, 2};
  CHECK(!prach_window_key_equal(key, demod, detect, swapped));
  for (size_t word = 0; word != sizeof(demod) / 4; ++word) {
    nrphy_prach_demod_cfg_t d = demod;
    reinterpret_cast<uint32_t*>(&d)[word] ^= 1U;
    CHECK(!prach_window_key_equal(key, d, detect, map));
  }
  for (size_t word = 0; word != sizeof(detect) / 4; ++word) {
    nrphy_prach_cfg_t d = detect;
    reinterpret_cast<uint32_t*>(&d)[word] ^= 1U;
    CHECK(!prach_window_key_equal(key, demod, d, map));
  }
  key.valid = false;
  CHECK(!prach_window_key_equal(key, demod, detect, map));
}

// ---- limits and layouts ------------------------------------------------------------------------------------------------------
static PrachWindowDims dims(uint32_t ports, uint32_t td, uint32_t fd, uint32_t symbols, uint32_t L, uint32_t window)
{
  PrachWindowDims d;
  d.nof_ports       = ports;
  d.nof_td          = td;
  d.nof_fd          = fd;
  d.nof_symbols     = symbols;
  d.sequence_length = L;
  d.window_samples  = window;
  return d;
}

static void limits_and_layouts()
{
  // every (symbols, L_RA) a format has, per occasion: symbols of get_prach_preamble_long_info / _short_info
  const uint32_t shapes[][2] = {{1, 839}, {2, 839}, {4, 839}, {2, 139}, {4, 139}, {6, 139}, {12, 139}, {1, 139}};
  for (uint32_t max_ports = 1; max_ports != 5; ++max_ports) {
    for (uint32_t max_td : {1u, 4u, 7u}) {
      for (uint32_t max_fd : {1u, 8u}) {
        PrachWindowLimits lim;
        lim.max_window_samples = 92160;
        lim.max_ports          = max_ports;
        lim.max_td_occasions   = max_td;
        lim.max_fd_occasions   = max_fd;
        const size_t          elems = prach_window_buffer_elems(lim);
        std::vector<uint32_t> owner(elems); // allocated at exactly the pool's size
        for (const auto& shape : shapes) {
          for (uint32_t ports = 1; ports <= max_ports + 1; ++ports) {
            for (uint32_t td : {1u, max_td, max_td + 1}) {
              for (uint32_t fd : {1u, max_fd, max_fd + 1}) {
                const PrachWindowDims d    = dims(ports, td, fd, shape[0], shape[1], 92160);
                const bool            fits = ports <= max_ports && td <= max_td && fd <= max_fd;
                CHECK((prach_window_fits(lim, d) == NRPHY_OK) == fits);
                CHECK(fits || prach_window_fits(lim, d) == NRPHY_ERR_CAPACITY);
                if (!fits) {
                  continue;
                }
                // every element of every (port, td, fd, symbol) lies inside the pool's buffer and belongs to nobody else
                const PrachWindowStrides st = prach_window_strides(d);
                CHECK(st.elems <= elems && st.elems == (uint64_t)ports * td * fd * shape[0] * shape[1]);
                std::fill(owner.begin(), owner.end(), 0u);
                uint32_t id = 0;
                for (uint32_t p = 0; p != ports; ++p) {
                  for (uint32_t t = 0; t != td; ++t) {
                    for (uint32_t f = 0; f != fd; ++f) {
                      for (uint32_t s = 0; s != shape[0]; ++s) {
                        ++id;
                        const uint64_t at = p * st.port + t * st.td + f * st.fd + s * st.symbol;
                        for (uint32_t k = 0; k != shape[1]; ++k) {
                          if (owner.at(at + k) != 0) {
                            CHECK(false);
                          }
                          owner[at + k] = id;
                        }
                      }
                    }
                  }
                }
                for (uint64_t e = 0; e != elems; ++e) {
                  if ((owner[e] != 0) != (e < st.elems)) { // C-contiguous: the used elements are the first st.elems
                    CHECK(false);
                  }
                }
                ++checks;
              }
            }
          }
        }
        CHECK(prach_window_fits(lim, dims(1, 1, 1, 1, 839, 92161)) == NRPHY_ERR_CAPACITY); // one sample too long
        CHECK(prach_window_fits(lim, dims(1, 1, 1, 1, 839, 92160)) == NRPHY_OK);
        CHECK(prach_window_fits(lim, dims(1, 1, 1, 1, 839, 0xFFFFFFFFu)) == NRPHY_ERR_CAPACITY);

        // the result block: the headers and the 64 records of every occasion written in a heap block of exactly the pool's size
        const size_t bytes = prach_window_result_bytes(lim);
        CHECK(bytes % 64 == 0);
        for (uint32_t n = 1; n <= max_td * max_fd; ++n) {
          const PrachWindowLayout l = prach_window_layout(n);
          CHECK(l.results == 0 && l.preambles % 64 == 0 && l.preambles >= n * sizeof(nrphy_prach_result_t) && l.host_bytes <= bytes);
          CHECK(l.host_bytes == l.preambles + (size_t)n * NRPHY_PRACH_MAX_PREAMBLES * sizeof(nrphy_prach_preamble_t));
          uint8_t* block = static_cast<uint8_t*>(std::malloc(bytes));
          CHECK(block != nullptr);
          std::memset(block, 0xEE, bytes);
          auto* results   = reinterpret_cast<nrphy_prach_result_t*>(block + l.results);
          auto* preambles = reinterpret_cast<nrphy_prach_preamble_t*>(block + l.preambles);
          for (uint32_t i = 0; i != n; ++i) {
            std::memset(&results[i], (int)i + 1, sizeof(nrphy_prach_result_t));
            for (uint32_t k = 0; k != NRPHY_PRACH_MAX_PREAMBLES; ++k) {
              std::memset(&preambles[(size_t)i * NRPHY_PRACH_MAX_PREAMBLES + k], (int)(i + 1) | 0x80, sizeof(nrphy_prach_preamble_t));
            }
          }
          for (uint32_t i = 0; i != n; ++i) { // the records did not run into the headers
            const uint8_t* r = reinterpret_cast<const uint8_t*>(&results[i]);
            CHECK(r[0] == i + 1 && r[sizeof(nrphy_prach_result_t) - 1] == i + 1);
          }
          for (size_t b = l.host_bytes; b != bytes; ++b) {
            if (block[b] != 0xEE) {
              CHECK(false);
            }
          }
          std::free(block);
        }
      }
    }
  }
  CHECK(sizeof(nrphy_prach_result_t) % 8 == 0 && sizeof(nrphy_prach_preamble_t) % 4 == 0);
  CHECK(PRACH_WINDOW_MAX_OCCASION_ELEMS >= 12 * 139 && PRACH_WINDOW_MAX_OCCASION_ELEMS >= 4 * 839);
}

int main()
{
  order_rules();
  pair_rules();
  limits_and_layouts();
  std::printf("ok: %u checks\n", checks);
  return 0;
}
