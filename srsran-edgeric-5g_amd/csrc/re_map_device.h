// RE mapping of a PDSCH codeblock wave (pdsch_kernels.hip): phase B of the output stage -- scrambling, QAM mapping through
// the LDS table, layer mapping, precoding and the stores into the grid -- and map_chunk, which runs both phases for one
// (modulation order, layer count).  The precoding products and the cbf16 packing here also serve the DM-RS waves.
#pragma once

#include "bits_device.h"
#include "codeblock_build_device.h"
#include "nrphy_internal.h"
#include "rate_match_device.h"

namespace nrphy {

// x * w evaluated like the reference's SIMD precoder (channel_precoder_avx2.cpp:51-56):
// fmaddsub(x, w.re, swap(x) * w.im) -- one rounding on the imaginary-weight product, one fused on the rest.
__device__ __forceinline__ void cmul_ref(float xr, float xi, float wr, float wi, float& outr, float& outi)
{
  float t0 = __fmul_rn(xi, wi);
  float t1 = __fmul_rn(xr, wi);
  outr     = __fmaf_rn(xr, wr, -t0);
  outi     = __fmaf_rn(xi, wr, t1);
}

// The same on packed FP32: a complex number is one 64-bit register pair (re, im), the product two v_pk_*_f32
// instructions instead of four scalar ones -- t = (x.im w.im, x.re w.im) rounded, then (fma(x.re, w.re, -t.lo),
// fma(x.im, w.re, t.hi)): operation for operation what cmul_ref does.  The codeblock launch is VALU-bound (PMC: the
// vector units are busy 87 % of its cycles) and the 4 x 4 precoding products are its largest block of arithmetic.
typedef float cf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ cf2 cmul_ref_packed(cf2 x, cf2 w)
{
  cf2 t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1]" : "=v"(t) : "v"(x), "v"(w));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] neg_lo:[0,0,1]" : "=v"(r) : "v"(x), "v"(w), "v"(t));
  return r;
}
// Wave-uniform weight held in an SGPR pair (wideband precoding).
__device__ __forceinline__ cf2 cmul_ref_packed_uniform(cf2 x, cf2 w)
{
  cf2 t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1]" : "=v"(t) : "v"(x), "s"(w));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] neg_lo:[0,0,1]" : "=v"(r) : "v"(x), "s"(w), "v"(t));
  return r;
}

// (re, im) -> cbf16 word, round to nearest even like to_bf16 (R/include/srsran/adt/bf16.h:39-56); v_cvt_pk_bf16_f32.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float  f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_cbf16(float re, float im)
{
  f32x2_t  v = {re, im};
  bf16x2_t b = __builtin_convertvector(v, bf16x2_t);
  return *reinterpret_cast<uint32_t*>(&b);
}

// Data RE go to the grid with non-temporal stores: 0.75 GB per 1024 slots that this kernel never reads back would
// otherwise displace the transport blocks, sequences and tables it does read.  Measured (A/B on one box): codeblock
// launch 0.486 -> 0.427 ms, whole step +7 %.  The same policy on the DM-RS / zero-fill stores, on the loads of the
// transport block or of the scrambling words, or on the prologue's sequence stores did not pay (0 ... -4 %).
__device__ __forceinline__ void grid_store(uint32_t* p, uint32_t v)
{
  __builtin_nontemporal_store(v, p);
}

constexpr int GRID_STORE_AUX = 2; // buffer-store cache policy of the data RE: 2 = non-temporal (0 = default)

struct ChunkGeom {
  uint32_t E;      // rate-matched length of the codeblock
  uint32_t cw_cb;  // first codeword bit of the codeblock
  uint32_t bit0;   // first codeword bit of the chunk
};

// A wave-uniform complex weight as an opaque value in one aligned scalar register pair: the compiler can neither
// re-load it inside the RE loop (it used to: one s_load_dwordx8 + s_waitcnt per port and 64 RE) nor split the pair.
__device__ __forceinline__ void pin_scalar(cf2& w)
{
  asm volatile("" : "+s"(w));
}

// What phase B knows about the chunk before it looks at a resource element.
struct ChunkMap {
  uint32_t re0;      // first RE of the chunk within the PDU
  uint32_t word0;    // first scrambling word of the chunk (valid when the chunk starts on a word and L * Qm = 32)
  bool     aligned;  // L * Qm = 32 and the chunk starts on a word boundary: one scrambling word per RE
  const uint32_t* gwords; // the scrambling words in global memory: the PDU's sequence (words form) or the x1 table (seeds form)
};

// The L * Qm scrambling bits of RE r of the chunk (MSB first), or their x1 part, from global memory (L2), requested a trip
// ahead; zero beyond the chunk.  Words form: cm.gwords is the PDU's whole sequence c = x1 ^ x2, which the prologue wrote once
// for all the PDUs that share it, and these are the bits.  Seeds form: cm.gwords is the x1 table every sequence shares, and
// the x2 part is XORed in from LDS (x2_bits).  L * Qm = 32 with a word-aligned chunk (the headline shape) makes the bits one
// word.  The last read stays inside the sequence: a misaligned read of the chunk's last bits runs one word past the word of
// the codeword's last bit at most, and PduDev::scr_words counts that word and 31 more.
template <int QM, int L>
__device__ __forceinline__ uint32_t global_bits(const ChunkGeom& g, const ChunkMap& cm, uint32_t re_count, uint32_t r)
{
  uint32_t bits = 0;
  if (r < re_count) {
    if (QM * L == 32 && cm.aligned) { // wave-uniform: scalar base, small per-lane index
      bits = (cm.gwords + cm.word0)[r];
    } else {
      bits = ext32(cm.gwords, g.bit0 + r * (uint32_t)(QM * L));
    }
  }
  return bits;
}
// Seeds form: x2 depends on the PDU: the wave has expanded its seed into LDS, x2[0] = the word the chunk's first bit lies in (r < re_count).
template <int QM, int L>
__device__ __forceinline__ uint32_t x2_bits(const uint32_t* x2, const ChunkGeom& g, const ChunkMap& cm, uint32_t r)
{
  if (QM * L == 32 && cm.aligned) { // wave-uniform
    return x2[r];
  }
  return ext32(x2, (g.bit0 & 31u) + r * (uint32_t)(QM * L));
}

// The RE's L symbol bytes (first in the MSB) and its L*Qm scrambling bits.  Four layers make the first a whole word.
template <int QM, int L, bool WORDS>
__device__ __forceinline__ void re_bits(const CbShared& sh, const ChunkGeom& g, const ChunkMap& cm,
                                        uint32_t re_count, uint32_t r, uint32_t& bytes, uint32_t& gbits)
{
  if constexpr (L == 4) {
    bytes = sh.symb[r];
  } else {
    bytes = ext32(sh.symb, 8u * r * L);
  }
  gbits = global_bits<QM, L>(g, cm, re_count, r);
  if constexpr (!WORDS) {
    gbits ^= x2_bits<QM, L>(sh.lin, g, cm, r);
  }
}

// The grid loop of phase B for P ports with wideband precoding (every weight in a scalar register pair for the whole
// loop, no guards, no loads), or -- P = 0 -- for any port count with weights per PRG read from memory per RE.
template <int QM, int L, int P, bool WORDS>
__device__ __forceinline__ void phase_b_grid(const PdschLaunch& p, PduRef pd, const PduDev* __restrict__ pd_global,
                                             const CbWork& wk, const CbShared& sh, const ChunkGeom& g, const ChunkMap& cm,
                                             uint32_t first_gbits, uint32_t lane, uint32_t* __restrict__ d_grid)
{
  const size_t   grid_base   = (size_t)pd.grid_index * p.grid_nof_ports * NRPHY_NSYMB * p.grid_nof_subc;
  const uint32_t plane_words = NRPHY_NSYMB * p.grid_nof_subc;
  // The PDU's grid through a buffer descriptor (scalar base, 32-bit per-lane offsets, the port plane in the scalar offset):
  // no 64-bit address arithmetic in the vector unit.  (Profiling aid, NRPHY_PROFILE_STAGE=11: a zero-sized descriptor
  // drops the data stores, everything else runs.)
  const __amdgpu_buffer_rsrc_t grid_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      d_grid + grid_base, 0, (int)(NRPHY_STAGE(p) == 11 ? 0u : p.grid_nof_ports * plane_words * 4u), 0x00020000);
  cf2 wu[P > 0 ? P : 1][L];
  if constexpr (P > 0) {
    const float NRPHY_CONSTANT* wuni = to_constant(p.weights + pd.weights_offset);
#pragma unroll
    for (int port = 0; port != P; ++port) {
#pragma unroll
      for (int l = 0; l != L; ++l) {
        wu[port][l] = cf2{wuni[2 * (port * L + l)], wuni[2 * (port * L + l) + 1]};
      }
    }
#pragma unroll
    for (int port = 0; port != P; ++port) {
#pragma unroll
      for (int l = 0; l != L; ++l) {
        pin_scalar(wu[port][l]);
      }
    }
  }
  // The OFDM symbol of the chunk's first RE, found once; the loop below only checks (on the scalar unit) whether the
  // next 64 RE stay inside the current symbol and walks on when they do not.  What the loop needs of the current symbol
  // travels in scalar registers (loaded when the symbol changes, not per 64 RE).
  uint32_t l_cur = 0;
#pragma unroll 1
  while (l_cur + 1u < NRPHY_NSYMB && cm.re0 >= pd.sym_re_start[l_cur + 1u]) {
    ++l_cur;
  }
  uint32_t cur_start = pd.sym_re_start[l_cur], cur_end = pd.sym_re_start[l_cur + 1u];
  uint32_t cur_arg = pd.sym_arg[l_cur], cur_row = l_cur * p.grid_nof_subc;
  bool     cur_table = pd.sym_kind[l_cur] == SYM_TABLE;
  // The scrambling bits (seeds form: their x1 part) come from global memory (L2): the words of the NEXT 64 RE are requested
  // before a trip's arithmetic starts, those of the first 64 RE were requested before rate matching (map_chunk).  Seeds form:
  // the x2 part is in LDS (sh.lin, expanded from the work item's seed).
  uint32_t gbits_next = first_gbits;

  for (uint32_t r0 = 0; r0 < wk.re_count; r0 += WAVE) { // r0 is wave-uniform
    const uint32_t r        = r0 + lane;
    const uint32_t gcur     = gbits_next;
    gbits_next              = global_bits<QM, L>(g, cm, wk.re_count, r + WAVE);
    const uint32_t re_first = cm.re0 + r0;
    const uint32_t re_last  = re_first + ((wk.re_count - r0 < WAVE ? wk.re_count - r0 : WAVE) - 1u);
    if (re_first >= cur_end && l_cur + 1u < NRPHY_NSYMB) { // wave-uniform
#pragma unroll 1
      do { // skips symbols without data RE
        ++l_cur;
        cur_start = cur_end;
        cur_end   = pd.sym_re_start[l_cur + 1u];
      } while (re_first >= cur_end && l_cur + 1u < NRPHY_NSYMB);
      cur_arg   = pd.sym_arg[l_cur];
      cur_row   = l_cur * p.grid_nof_subc;
      cur_table = pd.sym_kind[l_cur] == SYM_TABLE;
    }
    if (r >= wk.re_count) {
      continue;
    }
    __builtin_assume(r < (uint32_t)RE_CHUNK + WAVE);
    uint32_t gbits = gcur;
    if constexpr (!WORDS) {
      gbits ^= x2_bits<QM, L>(sh.lin, g, cm, r);
    }
    // The RE's L symbol bytes (first in the MSB): four layers make them a whole word.
    uint32_t bytes;
    if constexpr (L == 4) {
      bytes = sh.symb[r];
    } else {
      bytes = ext32(sh.symb, 8u * r * L);
    }
    // RE position: OFDM symbol from the per-symbol prefix counts, subcarrier from the symbol's pattern.
    const uint32_t re_pdu = re_first + lane;
    uint32_t       subc, word_offset;
    if (re_last < cur_end) { // wave-uniform: the whole group lies in the current symbol
      subc = cur_arg + (re_pdu - cur_start);
      if (cur_table) {
        subc = (uint32_t)p.re_table[subc];
      }
      word_offset = cur_row + subc;
    } else {
      // The group runs into the next symbol(s): rare (once per symbol and codeblock at most), so each lane walks on by
      // itself -- the scalar formulation of this search kept 27 prefix counts and pattern arguments in scalar registers
      // through the whole loop.
      uint32_t l_sym = l_cur, start = cur_start, end = cur_end;
#pragma unroll 1
      while (re_pdu >= end && l_sym + 1u < NRPHY_NSYMB) {
        ++l_sym;
        start = end;
        end   = pd_global->sym_re_start[l_sym + 1u];
      }
      subc = pd_global->sym_arg[l_sym] + (re_pdu - start);
      if (pd_global->sym_kind[l_sym] == SYM_TABLE) {
        subc = (uint32_t)p.re_table[subc];
      }
      word_offset = l_sym * p.grid_nof_subc + subc;
    }
    // Scrambling (TS 38.211 Section 7.3.1.1), modulation (table lookup), layer mapping + precoding
    // (resource_grid_mapper_impl.cpp:279-437, channel_precoder_avx2.cpp:214-342).
    cf2 x[L];
#pragma unroll
    for (int l = 0; l != L; ++l) {
      const uint32_t raw   = ((bytes >> (24 - 8 * l)) & 0xFFu) >> (8 - QM);
      const uint32_t idx   = raw ^ ((gbits >> (32 - (l + 1) * QM)) & ((1u << QM) - 1u));
      const float2   point = reinterpret_cast<const float2*>(sh.u)[idx];
      x[l]                 = cf2{point.x, point.y};
    }
    if constexpr (P > 0) {
#pragma unroll
      for (int port = 0; port != P; ++port) {
        cf2 acc = cmul_ref_packed_uniform(x[0], wu[port][0]);
#pragma unroll
        for (int l = 1; l != L; ++l) {
          acc += cmul_ref_packed_uniform(x[l], wu[port][l]);
        }
        __builtin_amdgcn_raw_buffer_store_b32(pack_cbf16(acc.x, acc.y), grid_rsrc, (int)(word_offset * 4u),
                                              (int)(port * plane_words * 4u), GRID_STORE_AUX);
      }
    } else {
      const uint32_t nof_ports = pd.nof_ports;
      uint32_t       prg       = subc / pd.prg_size_subc;
      prg                      = prg >= pd.nof_prg ? pd.nof_prg - 1 : prg;
      const float* w = p.weights + pd.weights_offset + 2u * prg * nof_ports * L;
#pragma unroll 1
      for (uint32_t port = 0; port != nof_ports; ++port) {
        cf2 acc = cmul_ref_packed(x[0], cf2{w[2 * port * L], w[2 * port * L + 1]});
#pragma unroll
        for (int l = 1; l != L; ++l) {
          acc += cmul_ref_packed(x[l], cf2{w[2 * (port * L + l)], w[2 * (port * L + l) + 1]});
        }
        __builtin_amdgcn_raw_buffer_store_b32(pack_cbf16(acc.x, acc.y), grid_rsrc, (int)(word_offset * 4u),
                                              (int)(port * plane_words * 4u), GRID_STORE_AUX);
      }
    }
  }
}

template <int QM, int L, bool WORDS>
__device__ __forceinline__ void phase_b(const PdschLaunch& p, PduRef pd, const PduDev* __restrict__ pd_global,
                                        const CbWork& wk, const CbShared& sh, const ChunkGeom& g, const ChunkMap& cm,
                                        uint32_t first_gbits, uint32_t lane, uint32_t* __restrict__ d_grid,
                                        uint32_t* __restrict__ d_cw_rm, uint32_t* __restrict__ d_cw_scr)
{
  constexpr uint32_t LQ = QM * L;
  // Codeword taps (parity tests, seam B): a loop of their own, so that the grid loop carries none of this.
  if (d_cw_rm != nullptr || d_cw_scr != nullptr) { // wave-uniform
    const uint64_t cw_bit0 = pd.cw_bit_offset + g.cw_cb + (uint64_t)wk.re_begin * LQ;
    for (uint32_t r = lane; r < wk.re_count; r += WAVE) {
      uint32_t bytes, gbits;
      re_bits<QM, L, WORDS>(sh, g, cm, wk.re_count, r, bytes, gbits);
      uint32_t v_rm = 0;
#pragma unroll
      for (int l = 0; l != L; ++l) {
        const uint32_t raw = ((bytes >> (24 - 8 * l)) & 0xFFu) >> (8 - QM);
        v_rm |= raw << (32 - (l + 1) * QM);
      }
      if (d_cw_rm) {
        or_bits_global(d_cw_rm, cw_bit0 + (uint64_t)r * LQ, v_rm, LQ);
      }
      if (d_cw_scr) {
        or_bits_global(d_cw_scr, cw_bit0 + (uint64_t)r * LQ, v_rm ^ (gbits & topmask(LQ)), LQ);
      }
    }
  }
  if (d_grid == nullptr) {
    return;
  }
  // One copy of the grid loop per port count (wave-uniform): straight-line port code with its weights in registers.
  const uint32_t nof_ports = pd.nof_prg == 1 ? pd.nof_ports : 0u;
  if (nof_ports == 4u) {
    phase_b_grid<QM, L, 4, WORDS>(p, pd, pd_global, wk, sh, g, cm, first_gbits, lane, d_grid);
  } else if (L <= 3 && nof_ports == 3u) {
    phase_b_grid<QM, (L <= 3 ? L : 1), 3, WORDS>(p, pd, pd_global, wk, sh, g, cm, first_gbits, lane, d_grid);
  } else if (L <= 2 && nof_ports == 2u) {
    phase_b_grid<QM, (L <= 2 ? L : 1), 2, WORDS>(p, pd, pd_global, wk, sh, g, cm, first_gbits, lane, d_grid);
  } else if (L == 1 && nof_ports == 1u) {
    phase_b_grid<QM, 1, 1, WORDS>(p, pd, pd_global, wk, sh, g, cm, first_gbits, lane, d_grid);
  } else {
    phase_b_grid<QM, L, 0, WORDS>(p, pd, pd_global, wk, sh, g, cm, first_gbits, lane, d_grid); // weights per PRG (or fewer ports than layers)
  }
}

// Stages 3 and 4 of a codeblock wave for one (Qm, layers): this wave's slice of the codeword, rate matching ... RE mapping.
template <int QM, int L, bool WORDS>
__device__ __forceinline__ void map_chunk(const PdschLaunch& p, PduRef pd, const PduDev* pd_global, const CbWork& wk,
                                          uint32_t item, const CbShared& sh, uint32_t lane, uint32_t* d_grid,
                                          uint32_t* d_cw_rm, uint32_t* d_cw_scr)
{
  const bool is_long = wk.cb >= pd.n_short;
  ChunkGeom  g;
  g.E     = is_long ? pd.e_long : pd.e_short;
  g.cw_cb = is_long ? pd.n_short * pd.e_short + (wk.cb - pd.n_short) * pd.e_long : wk.cb * pd.e_short;
  g.bit0  = g.cw_cb + wk.re_begin * (uint32_t)(QM * L);
  if (NRPHY_STAGE(p) == 3) {
    return;
  }
  ChunkMap cm;
  cm.re0     = g.cw_cb / (uint32_t)(QM * L) + wk.re_begin;
  cm.word0   = g.bit0 >> 5;
  cm.aligned = (g.bit0 & 31u) == 0;
  cm.gwords  = WORDS ? p.scr_seq + pd.scr_word_offset : p.x1_words;
  // The global words of the chunk's first 64 RE and, in the seeds form, the work item's seed (the 31 x2 words from the one its
  // first bit lies in; prologue) are requested here: their trip to memory rides under rate matching.
  uint32_t seed_word = 0u;
  if constexpr (!WORDS) {
    const uint32_t seed_slot = pd.seed_first + (item - pd.item_first); // the PDU's own items, or those of the PDU it shares with
    seed_word                = lane < 31u ? p.scr_seq[(size_t)seed_slot * 32u + lane] : 0u;
  }
  const uint32_t first_gbits = global_bits<QM, L>(g, cm, wk.re_count, lane);
  {
    const RmIndex rm = rm_index_init(pd);
    if (rm.rank0 + g.E > rm.n_valid) { // wave-uniform: the selection wraps around Ncb
      phase_a<QM, L, true>(p, pd, wk, sh, g.E, lane);
    } else {
      phase_a<QM, L, false>(p, pd, wk, sh, g.E, lane);
    }
  }
  if (NRPHY_STAGE(p) == 4) {
    return;
  }
  NRPHY_WG_TRACE_MARK(3); // rate matched and interleaved
  if constexpr (!WORDS) {
    // The codeblock's LDS is free now: the chunk's x2 words go there, from the word its first bit lies in up to the word a
    // misaligned read of its last bits runs into (the plan sized the region for it).
    static_assert((31u + (uint32_t)RE_CHUNK * 32u + 31u) / 32u + 1u <= GOLD_EXPAND_MAX_WORDS, "a work item's scrambling words");
    gold_expand_seed_wave(sh.lin, seed_word, ((g.bit0 & 31u) + wk.re_count * (uint32_t)(QM * L) + 31u) / 32u + 1u, lane);
  }
  phase_b<QM, L, WORDS>(p, pd, pd_global, wk, sh, g, cm, first_gbits, lane, d_grid, d_cw_rm, d_cw_scr);
}

template <int QM, bool WORDS>
__device__ __forceinline__ void map_chunk_layers(const PdschLaunch& p, PduRef pd, const PduDev* pd_global,
                                                 const CbWork& wk, uint32_t item, const CbShared& sh, uint32_t lane,
                                                 uint32_t* d_grid, uint32_t* d_cw_rm, uint32_t* d_cw_scr)
{
  switch (pd.nof_layers) { // wave-uniform
    case 1:
      map_chunk<QM, 1, WORDS>(p, pd, pd_global, wk, item, sh, lane, d_grid, d_cw_rm, d_cw_scr);
      break;
    case 2:
      map_chunk<QM, 2, WORDS>(p, pd, pd_global, wk, item, sh, lane, d_grid, d_cw_rm, d_cw_scr);
      break;
    case 3:
      map_chunk<QM, 3, WORDS>(p, pd, pd_global, wk, item, sh, lane, d_grid, d_cw_rm, d_cw_scr);
      break;
    default:
      map_chunk<QM, 4, WORDS>(p, pd, pd_global, wk, item, sh, lane, d_grid, d_cw_rm, d_cw_scr);
      break;
  }
}

} // namespace nrphy
