// What the golden recorders share over the reference's interfaces: cbf16 words, the grid they hand to the reference, and the
// symbol start epochs of their channels.  Compiled against a checkout of srsRAN-5G-ER, as the recorders are.
#pragma once

#include "recorder_io.h"
#include "srsran/adt/complex.h"
#include "srsran/phy/support/resource_grid_reader.h"

#include <numeric>

// A cbf16 value as the fixtures store it: one uint32 word, re in the low half.
inline uint32_t word_of(srsran::cbf16_t v)
{
  const srsran::cf_t c = srsran::to_cf(v);
  return bf16_bits(c.real()) | (bf16_bits(c.imag()) << 16);
}
inline srsran::cbf16_t cbf16_of(uint32_t w)
{
  return srsran::cbf16_t(bf16_value(w & 0xFFFFU), bf16_value(w >> 16)); // exact: the halves are bf16 values
}

// The start of the useful part of each of the 14 symbols of a slot, in useful-symbol lengths (normal cyclic prefix).
inline std::vector<double> epochs(int numerology)
{
  std::vector<double> out;
  double              e = 0.0;
  for (int l = 0; l != 14; ++l) {
    const int cp = (144 >> numerology) + ((l == 0 || l == 7 * (1 << numerology)) ? 16 : 0);
    e += cp * (1 << numerology) / 2048.0 + (l == 0 ? 0.0 : 1.0);
    out.push_back(e);
  }
  return out;
}

// A grid [ports][14][subc] of cbf16, zero at first, behind the reference's reader interface.  word() and set() name a grid
// port; the reader's port i, and at(), is grid port map[i] -- 0, 1, ..., ports - 1 until a recorder says otherwise.
class word_grid : public srsran::resource_grid_reader
{
  using cf_t    = srsran::cf_t;
  using cbf16_t = srsran::cbf16_t;
  using re_mask = srsran::bounded_bitset<srsran::MAX_RB * srsran::NRE>;
  template <typename T>
  using span = srsran::span<T>;

  size_t row(unsigned grid_port, unsigned l) const { return ((size_t)grid_port * 14 + l) * subc; }

public:
  unsigned              ports, subc;
  std::vector<cbf16_t>  re;
  std::vector<unsigned> map;

  word_grid(unsigned ports_, unsigned subc_) : ports(ports_), subc(subc_), re((size_t)ports_ * 14 * subc_), map(ports_)
  {
    std::iota(map.begin(), map.end(), 0U);
  }
  uint32_t word(unsigned grid_port, unsigned l, unsigned k) const { return word_of(re[row(grid_port, l) + k]); }
  void     set(unsigned grid_port, unsigned l, unsigned k, uint32_t word) { re[row(grid_port, l) + k] = cbf16_of(word); }
  void     set(unsigned grid_port, unsigned l, unsigned k, float real, float imag) // rounded to bf16: nearest, ties to even
  {
    set(grid_port, l, k, bf16_bits(real) | (bf16_bits(imag) << 16));
  }
  cf_t at(unsigned port, unsigned l, unsigned k) const { return srsran::to_cf(re[row(map[port], l) + k]); }

  unsigned   get_nof_ports() const override { return ports; }
  unsigned   get_nof_subc() const override { return subc; }
  unsigned   get_nof_symbols() const override { return 14; }
  bool       is_empty(unsigned) const override { return false; }
  bool       is_empty() const override { return false; }
  span<cf_t> get(span<cf_t> symbols, unsigned port, unsigned l, unsigned k_init, const re_mask& mask) const override
  {
    unsigned n = 0;
    mask.for_each(0, mask.size(), [&](unsigned k) { symbols[n++] = at(port, l, k_init + k); });
    return symbols.last(symbols.size() - n);
  }
  span<cbf16_t> get(span<cbf16_t> symbols, unsigned port, unsigned l, unsigned k_init, const re_mask& mask) const override
  {
    unsigned n = 0;
    mask.for_each(0, mask.size(), [&](unsigned k) { symbols[n++] = re[row(map[port], l) + k_init + k]; });
    return symbols.last(symbols.size() - n);
  }
  void get(span<cf_t> symbols, unsigned port, unsigned l, unsigned k_init, unsigned stride) const override
  {
    for (unsigned i = 0; i != symbols.size(); ++i) {
      symbols[i] = at(port, l, k_init + stride * i);
    }
  }
  void get(span<cbf16_t> symbols, unsigned port, unsigned l, unsigned k_init) const override
  {
    for (unsigned i = 0; i != symbols.size(); ++i) {
      symbols[i] = re[row(map[port], l) + k_init + i];
    }
  }
  span<const cbf16_t> get_view(unsigned port, unsigned l) const override
  {
    return span<const cbf16_t>(re).subspan(row(map[port], l), subc);
  }
};
