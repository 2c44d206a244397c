// The two LDPC base graphs as edge lists (TS 38.212 Tables 5.3.2-2/-3, nr_ldpc_bg.inc) for the host code that lifts them:
// the encoder's graphs (nrphy_host.cpp) and the decoder's (ldpc_decoder_host.cpp).  Each of the two keeps its own copy of
// the tables (18 bytes per edge, 513 edges).
#pragma once

#include <cstdint>

#pragma GCC visibility push(hidden)

struct nr_ldpc_edge_t {
  uint8_t  row;
  uint8_t  col;
  uint16_t shift[8];
};
#include "nr_ldpc_bg.inc"

// Lifting-set index i_LS: Zc = a * 2^j, a in {2, 3, 5, 7, 9, 11, 13, 15} (TS 38.212 Table 5.3.2-1).
inline int lifting_set_index(unsigned zc)
{
  static const unsigned base[8] = {2, 3, 5, 7, 9, 11, 13, 15};
  for (int i = 0; i != 8; ++i) {
    for (unsigned v = base[i]; v <= 384; v *= 2) {
      if (v == zc) {
        return i;
      }
    }
  }
  return -1;
}

#pragma GCC visibility pop
