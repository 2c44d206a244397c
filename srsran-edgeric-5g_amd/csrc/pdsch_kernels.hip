// PDSCH processor kernels for gfx950 (MI355X).
//
//   prologue_kernel    per-PDU work the codeblock waves consume: the transport-block CRC (a workgroup per run of 16 KiB
//                      regions, Horner's rule through byte tables in LDS, one share per workgroup), every distinct scrambling
//                      sequence (its words, or a 31-word seed per codeblock work item where the words of all sequences
//                      would not stay in an L2: PdschLaunch::scr_as_words), and the DM-RS sequences
//   codeblock_kernel   one wavefront per codeblock (or per 512-RE chunk of it): segmentation, CB-CRC, LDPC
//                      base-graph expansion in LDS, rate matching + bit interleaving as a word-level bit-matrix
//                      transposition, Gold scrambling, QAM mapping through an LDS table, layer mapping, precoding
//                      and RE mapping straight into the grid
//   dmrs_kernel        PDSCH DM-RS generation, CDM, precoding and mapping, one wavefront per 32 PRBs of a symbol
//   ldpc_encode_kernel the LDPC encoder alone (seam B / unit parity)
//
// Together they replace pdsch_processor_impl::process (R/lib/phy/upper/channel_processors/pdsch_processor_impl.cpp:30-184)
// in its per-codeblock form (pdsch_processor_concurrent_impl.cpp:55-338, pdsch_codeblock_processor.cpp:27-141).
//
// This file holds the kernels, their launch functions and the wave-level glue of the codeblock kernels (which wave takes
// which work item, and the order of its stages).  What a wave does in a stage is in the device headers:
//   codeblock_build_device.h  the LDS of a codeblock wave (CbShared), segmentation, TB-CRC and CB-CRC attachment
//   ldpc_device.h             LDPC base-graph expansion
//   rate_match_device.h       rate matching + bit interleaving (phase A of the output stage)
//   re_map_device.h           scrambling, QAM, layer mapping, precoding, RE mapping (phase B), map_chunk
//   pdsch_dmrs_device.h       the DM-RS waves and the zero-fill waves
//   bits_device.h             packed-bit helpers, the TB-CRC regions, the Gold sequence generators, NRPHY_STAGE
#include "bits_device.h"
#include "codeblock_build_device.h"
#include "ldpc_device.h"
#include "nrphy_internal.h"
#include "pdsch_dmrs_device.h"
#include "re_map_device.h"

namespace nrphy {

// ================================================================================================================
// Prologue: per-PDU work the codeblock waves consume.
//
// Transport block CRC (TS 38.212 Section 5.1; reference: ldpc_segmenter_impl.cpp:126, crc_calculator_lut_impl.cpp).
// A CRC is the remainder of a polynomial, so it splits: the transport block is cut into 16 KiB regions, a workgroup
// takes a run of them (CrcWork: one region each in a small batch, up to eight in a big one, the next region's words in
// flight while the current one is reduced) and the codeblock wave that attaches the CRC adds the workgroups' shares up.
// Inside a region thread t owns four groups of four consecutive words (16-byte loads, coalesced, straight from HBM):
// Horner's rule in x^32 inside a group, in y1k = x^(32 * 1024) across the groups -- four independent table look-ups per
// word; the 256 partials are folded by one wavefront the same way with y8k = x^(128 * 64); from region to region those
// 64 lanes step with yz = x^(8 * 16384), and only once per workgroup do they pay for a multiplication by a per-lane
// constant.
//
// Scrambling sequences (words, or seeds per work item) and DM-RS sequences: see gold_sequence_blocks_wave() and gold_sequence_wave().
// ================================================================================================================
// Blocks [0, n_scr_work): the scrambling sequence of one PDU, as words or as seeds (a part of it where the plan has few sequences) and
// its DM-RS sequences (TS 38.211 Sections 7.3.1.1, 7.4.1.1.1; reference: pdsch_modulator_impl.cpp:43-60,
// dmrs_pdsch_processor_impl.cpp:84-106) -- once per distinct sequence of the plan: the PDUs that ask for the same one read the
// same words (PduDev::scr_word_offset) or seeds (seed_first) and DM-RS words (dmrs_seq_offset).  The blocks after them: transport-block CRC.
__global__ __launch_bounds__(TB_CRC_THREADS) void prologue_kernel(PdschLaunch p, const uint8_t* __restrict__ d_tb)
{
  constexpr uint32_t LDS_WORDS = TB_CRC_LDS_WORDS; // CRC role: four tables and two buffers of partials (18 KB: 8 workgroups per CU)
  __shared__ __attribute__((aligned(16))) uint32_t lds[LDS_WORDS]; // sequence role: seed rows + DM-RS scratch
  static_assert(LDS_WORDS >= GOLD_RING_WORDS, "LDS of the sequence role");
  const uint32_t tid = threadIdx.x;

  // Order of the two roles in the grid: the sequence workgroups first, then the CRC workgroups.  A sequence workgroup is one
  // long wave (plus three short DM-RS waves) and holds its slot on the CU for the whole time.  History: a run-time knob once
  // spread the sequence workgroups evenly among the CRC workgroups instead, every XCD taking a contiguous run of that list (block
  // b runs on XCD b % 8); measured within 1 % of this order (profiles/r03_prologue_trace.txt), so it went.
  // (With the workgroup-wide generator of rounds 1-3 -- a ring in LDS walked by all four waves -- interleaving cost +95 %:
  // ring and byte tables slowed each other down; and CRC first +11 %.  profiles/r02_codeblock_experiments.txt.)
  const uint32_t scr_index = blockIdx.x, crc_index = blockIdx.x - p.n_scr_work;
  const bool     scr_role  = blockIdx.x < p.n_scr_work;
  NRPHY_WG_TRACE_MARK(0);
  NRPHY_WG_TRACE_WHERE(scr_role ? 1 : 2);
  if (scr_role) { // workgroup-uniform
    if (NRPHY_STAGE(p) == 8) {
      return;
    }
    const auto*    swc   = to_constant(&p.scr_work[scr_index]);
    const uint32_t first = swc->first, count = swc->count;
    const bool     with_dmrs = swc->with_dmrs != 0;
    PduRef         pd    = *to_constant(&p.pdus[swc->pdu]);
    const uint32_t wave = tid / WAVE, lane = tid % WAVE;
    // The four waves of the workgroup work on their own, each on LDS of its own, without a barrier.  Wave 0 walks the part's
    // scrambling sequence (its x2 part: the codeblock waves add the x1 words, which every sequence shares) with the
    // recurrence in registers (gold_sequence_blocks_wave) and stores, for every work item of the PDU, the 31 words that
    // start at the word the item's first codeword bit lies in: the codeblock wave expands them to the few hundred words it
    // needs (gold_expand_seed_wave).  13 MB of seeds per 1024 config-3 slots instead of 121 MB of sequences out and back -- and
    // 13 KB where the slots are one UE's and share the sequence.
    constexpr uint32_t DMRS_WAVES = TB_CRC_THREADS / WAVE - 1, DMRS_SCRATCH = (GOLD_RING_WORDS - 2048u) / DMRS_WAVES;
    static_assert(GOLD_SEED_WORDS <= 2048u && GOLD_RING_WORDS > 2048u, "LDS of the sequence role");
    static_assert((12u * NRPHY_MAX_RB + 31u) / 32u + 1u <= DMRS_SCRATCH, "DM-RS scratch per wave");
    if (wave == 0) {
      if (count == 0) { // a PDU that shares its scrambling sequence and has DM-RS sequences of its own
        return;
      }
      if (p.scr_as_words != 0) { // launch-uniform
        // Words form: the part's words [first, first + count) of the whole sequence c = x1 ^ x2, 64 consecutive words per
        // store, where every codeblock wave of every PDU that shares the sequence reads them (served from L2 like the x1
        // table: the plan takes this form only while all its sequences fit one).  The parts of a sequence are disjoint and
        // cover [0, scr_words), and the blocks of a part are: every word is written once.
        constexpr uint32_t SCR_STORE_ROWS = 8;
        uint32_t*       out = p.scr_seq + pd.scr_word_offset + first;
        const uint32_t* x1  = p.x1_words + first;
        // The x1 words of SCR_STORE_ROWS rows are requested together: one trip to memory per batch instead of one per row
        // (a row at a time, the walk of the headline's sequence took longer than the whole TB-CRC role beside it).
        gold_sequence_blocks_wave(p.gold, pd.c_init, first, count, lds, lane, [&](uint32_t base, uint32_t avail) {
          for (uint32_t k0 = lane; k0 < avail; k0 += SCR_STORE_ROWS * WAVE) { // (k0 - lane is wave-uniform)
            uint32_t x[SCR_STORE_ROWS];
#pragma unroll
            for (uint32_t i = 0; i != SCR_STORE_ROWS; ++i) {
              const uint32_t k = k0 + i * WAVE;
              x[i]             = k < avail ? x1[base + k] : 0u;
            }
#pragma unroll
            for (uint32_t i = 0; i != SCR_STORE_ROWS; ++i) {
              const uint32_t k = k0 + i * WAVE;
              if (k < avail) {
                out[base + k] = lds[k] ^ x[i];
              }
            }
          }
        });
        NRPHY_WG_TRACE_MARK(6);
        return;
      }
      // The PDU's work items in the order the plan lists them (pdsch_plan_build.cpp: codeblock by codeblock, RE_CHUNK resource
      // elements per item), walked with scalar arithmetic alongside the blocks: w0 = the word of the item's first bit.
      const uint32_t lq = pd.qm * pd.nof_layers, n_short = pd.n_short, e_short = pd.e_short, e_long = pd.e_long, C = pd.C;
      const uint32_t nre_short = e_short / lq, nre_long = e_long / lq; // (the only divisions: the walk itself has none)
      struct Cursor {
        uint32_t cb, re_begin, item, bit_cb, nre; // item: its seed slot
      };
      Cursor resume = {0u, 0u, pd.seed_first, 0u, n_short != 0 ? nre_short : nre_long}; // the first item whose seed is not complete yet
      auto   advance = [&](Cursor& c) {
        c.re_begin += RE_CHUNK;
        if (c.re_begin >= c.nre) {
          c.bit_cb += c.cb < n_short ? e_short : e_long;
          ++c.cb;
          c.re_begin = 0;
          c.nre      = c.cb < n_short ? nre_short : nre_long;
        }
        ++c.item;
      };
      gold_sequence_blocks_wave(p.gold, pd.c_init, first, count, lds, lane, [&](uint32_t base, uint32_t avail) {
        const uint32_t lo = first + base, hi = lo + avail; // the block holds words [lo, hi) of the PDU's sequence
        // Every item whose 31 words meet the block gets what the block holds of them.  Seeds of neighbouring items overlap
        // when an item is short (the tail of a codeblock cut into RE_CHUNK pieces): an item that runs beyond the block does not
        // end the walk, it only marks where the next block (or the next part's first) takes it up again.
        Cursor c        = resume;
        bool   resuming = false;
        while (c.cb < C) { // wave-uniform
          const uint32_t w0 = (c.bit_cb + c.re_begin * lq) >> 5;
          if (w0 >= hi) {
            break;
          }
          if (w0 + 31u > lo) {
            const uint32_t k = w0 + lane;
            if (lane < 31u && k >= lo && k < hi) {
              p.scr_seq[(size_t)c.item * 32u + lane] = lds[k - lo];
            }
          }
          if (w0 + 31u > hi && !resuming) {
            resume   = c;
            resuming = true;
          }
          advance(c);
        }
        if (!resuming) {
          resume = c;
        }
      });
      NRPHY_WG_TRACE_MARK(6);
    } else if (with_dmrs && pd.dmrs_seq_words <= DMRS_SCRATCH) {
      // Waves 1-3 of the PDU's first workgroup: the DM-RS sequences, from bit 0 to the last allocated PRB -- short, so one
      // wave generates one; the waves take the DM-RS symbols in turn.
      uint32_t ordinal = 0;
      for (uint32_t mask = pd.dmrs_symbol_mask; mask != 0; mask &= mask - 1u, ++ordinal) { // uniform
        if (ordinal % DMRS_WAVES == wave - 1u) {
          const uint32_t l = (uint32_t)__ffs(mask) - 1u;
          gold_sequence_wave(p.gold, p.x1_words, pd.dmrs_c_init[l], pd.dmrs_seq_words,
                             p.scr + pd.dmrs_seq_offset + ordinal * pd.dmrs_seq_words,
                             lds + 2048u + (wave - 1u) * DMRS_SCRATCH, lane);
        }
      }
    }
    return;
  }

  if (NRPHY_STAGE(p) == 9) {
    return;
  }
  const auto*     wkc = to_constant(&p.crc_work[crc_index]);
  const uint32_t  wk_pdu = wkc->pdu, wk_region = wkc->region, wk_factor = wkc->factor, wk_count = wkc->count;
  PduRef          pd  = *to_constant(&p.pdus[wk_pdu]);
  const uint32_t  sel = (pd.tb_crc_bits == 16) ? 1u : 0u;
  const CrcPoly   c   = sel ? crc16() : crc24a();
  const uint32_t  n   = pd.tb_bytes;
  const uint32_t* tbw = reinterpret_cast<const uint32_t*>(d_tb + pd.tb_offset);
#ifdef NRPHY_WG_TRACE
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // (trace builds: the descriptors have arrived)
  NRPHY_WG_TRACE_MARK(3);
#endif
  const uint32_t share = tbcrc_regions_workgroup(p.tbcrc, sel, c, tbw, n, wk_region, wk_count, wk_factor, lds, tid);
  if (tid == 0) {
    // The workgroup's share of the PDU's CRC in a slot of its own: the codeblock wave that attaches the CRC adds the
    // shares up, so a run neither relies on nor leaves behind any accumulator state.
    p.tb_crc_part[crc_index] = share;
  }
  NRPHY_WG_TRACE_MARK(6);
}

#ifdef NRPHY_WG_TRACE
extern "C" int nrphy_debug_wg_trace(uint64_t* out, uint32_t nof_blocks)
{
  const size_t n = 8 * (size_t)(nof_blocks < WG_TRACE_MAX ? nof_blocks : WG_TRACE_MAX) * sizeof(uint64_t);
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg_trace), n, 0, hipMemcpyDeviceToHost);
}
#endif

hipError_t launch_prologue(const PdschLaunch& p, const uint8_t* d_tb, hipStream_t stream)
{
  if (p.n_crc_work + p.n_scr_work == 0) {
    return hipSuccess;
  }
  // (The zero-fill waves were tried as a third role of this launch, which leaves most of the memory bandwidth unused: the
  // prologue 0.084 -> 0.095 ms, the codeblock launch 0.303 -> 0.352 ms, the OFDM launch 0.50 -> 0.475 ms, the whole step
  // -4 %: profiles/r03_codeblock_experiments.txt.  They stay at the tail of the codeblock launch.)
  hipLaunchKernelGGL(prologue_kernel, dim3(p.n_crc_work + p.n_scr_work), dim3(TB_CRC_THREADS), 0, stream, p, d_tb);
  return hipGetLastError();
}

// ================================================================================================================
// The codeblock kernels.  Blocks [0, n_work) build codeblocks; the launch may carry two more kinds of wave behind
// them so that their short, latency-bound work overlaps the codeblock waves instead of paying for own launches:
// DM-RS waves and zero-fill waves for the grid words nobody maps.
//
// The plan sorts its work items by (modulation order, layers) -- a "bucket".  A plan with one bucket (every batch of
// like PDUs: the headline workload) or with big buckets runs codeblock_kernel_t<QM, L>, one launch per bucket, whose
// output stage exists once and whose scalar registers hold only what that stage needs; a small mixed plan (one slot
// with PDUs of several modulations) runs the one-launch codeblock_kernel, which selects the output stage per wave.
// ================================================================================================================

// A workgroup is CB_WAVES independent waves, each with its own work unit and its own slice of the dynamic LDS (no
// barrier between them): the dispatcher hands out a quarter of the workgroups for the same waves (an empty launch of the
// headline's 138 k one-wave workgroups alone took 0.035 ms).
constexpr uint32_t CB_WAVES = 4;

struct CbWave {
  uint32_t  lane;
  uint32_t  wave;  // wave-uniform (scalar register)
  uint32_t* lds;   // this wave's slice of the dynamic LDS
};
__device__ __forceinline__ CbWave cb_wave(const PdschLaunch& p, uint32_t* dyn_lds)
{
  CbWave w;
  w.lane = threadIdx.x % WAVE;
  w.wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  w.lds  = dyn_lds + w.wave * (p.lds_lin_words + p.lds_u_words);
  return w;
}
__host__ __device__ __forceinline__ uint32_t cb_blocks(uint32_t n_units)
{
  return (n_units + CB_WAVES - 1u) / CB_WAVES;
}

// The launch's extra waves (DM-RS, zero fill) sit in the workgroups behind the codeblock ones; true when this wave
// belongs to one of those (whether or not a unit was left for it).
__device__ __forceinline__ bool extra_wave(const PdschLaunch& p, const CbWave& w, uint32_t* __restrict__ d_grid)
{
  const uint32_t nb = cb_blocks(p.n_work);
  if (blockIdx.x < nb) { // workgroup-uniform
    return false;
  }
  const uint32_t extra = (blockIdx.x - nb) * CB_WAVES + w.wave;
  if (extra < p.n_dmrs_in_launch) {
    dmrs_wave(p, extra, d_grid, w.lane, w.lds);
  } else if (extra - p.n_dmrs_in_launch < p.n_zero_work) {
    zero_wave(p, extra - p.n_dmrs_in_launch, d_grid, w.lane);
  }
  return true;
}

// Workgroups go to the eight XCDs round-robin (block b runs on XCD b % 8).  Give each XCD a contiguous run of work
// items, so that codeblocks which share cache lines -- neighbours in the transport block and in the grid rows --
// meet in one L2 instead of leaving partial lines in two.  Returns the wave's work item, or n_work when none is left.
__device__ __forceinline__ uint32_t xcd_work_item(uint32_t n_work, const CbWave& w)
{
  const uint32_t nb  = cb_blocks(n_work);
  const uint32_t xcd = blockIdx.x & 7u, turn = blockIdx.x >> 3;
  const uint32_t q = nb >> 3, r = nb & 7u;
  const uint32_t item = (xcd * q + (xcd < r ? xcd : r) + turn) * CB_WAVES + w.wave;
  return item < n_work ? item : n_work;
}

// Stages 1 and 2 of a codeblock wave: segmentation + CRC attachment (the graph rows ride along: their loads overlap the
// transport block's), LDPC encoding (only the parity rows that rate matching can reach).  False: a profiling stage stopped the wave.
__device__ __forceinline__ bool codeblock_front(const PdschLaunch& p, PduRef pd, const CbWork& wk, CbShared& sh,
                                                const uint8_t* __restrict__ d_tb, uint32_t lane)
{
  const uint32_t zc = pd.zc, kb = pd.kb;
  if (NRPHY_STAGE(p) == 5 || NRPHY_STAGE(p) == 6) {
    return false;
  }
  const uint32_t total_words = (((kb + pd.nof_rows) * zc + 31u) >> 5) + 2u;
  // The graph rows are requested now and stored in the scratch region once the codeblock is built: their trip to memory
  // rides under the segmentation and the CRC instead of standing between the CRC and the encoder.
  GraphRows rows;
  rows.fetch(&p.graphs[pd.graph], pd.nof_rows, lane);
  build_codeblock(pd, wk.cb, reinterpret_cast<const uint32_t*>(d_tb + pd.tb_offset), p.tb_crc_part, p.gold, &sh,
                  total_words, lane, NRPHY_STAGE(p));
  if (NRPHY_STAGE(p) == 1 || NRPHY_STAGE(p) == 7) {
    return false;
  }
  NRPHY_WG_TRACE_MARK(1); // codeblock built (segmentation, CRCs)
  rows.store(pd.nof_rows, sh.graph, lane); // (build_codeblock ends with a wave barrier; ldpc_encode_wave synchronises before it reads)
  ldpc_encode_wave(&p.graphs[pd.graph], sh.graph, kb, zc, pd.nof_rows, sh.lin, sh.u, sh.ldpc, lane);
  NRPHY_WG_TRACE_MARK(2); // encoded
  return NRPHY_STAGE(p) != 2;
}

// One codeblock wave of a bucket launch.  WORDS: the form of the launch's scrambling sequences (PdschLaunch::scr_as_words) as a
// compile-time constant -- the words form has no seed load, no expansion in LDS and no x2 read per 64 RE at all.
template <int QM, int L, bool WORDS>
__device__ __forceinline__ void codeblock_wave_t(const PdschLaunch& p, const uint8_t* __restrict__ d_tb,
                                                 uint32_t* __restrict__ d_grid, uint32_t* __restrict__ d_cw_rm,
                                                 uint32_t* __restrict__ d_cw_scr, uint32_t* dyn_lds)
{
  const CbWave   w    = cb_wave(p, dyn_lds);
  const uint32_t lane = w.lane;
  CbShared       sh;
  sh.lin   = w.lds;
  sh.u     = w.lds + p.lds_lin_words;
  sh.symb  = sh.u + CB_U_QAM_WORDS;
  sh.graph = sh.u + CB_U_GRAPH_OFFSET;
  sh.ldpc  = reinterpret_cast<LdpcScratch*>(sh.u + LDPC_DBL_WORDS);
  if (NRPHY_STAGE(p) == 10 || extra_wave(p, w, d_grid)) {
    return;
  }
  const uint32_t item = xcd_work_item(p.n_work, w);
  if (item == p.n_work) { // wave-uniform: the last workgroup's spare waves
    return;
  }
  NRPHY_WG_TRACE_MARK(0);
  NRPHY_WG_TRACE_WHERE(3);
  const auto*  wkc = to_constant(&p.work[item]);
  const CbWork wk  = {wkc->pdu, wkc->cb, wkc->re_begin, wkc->re_count};
  PduRef       pd  = *to_constant(&p.pdus[wk.pdu]);
  if (!codeblock_front(p, pd, wk, sh, d_tb, lane)) {
    return;
  }
  map_chunk<QM, L, WORDS>(p, pd, &p.pdus[wk.pdu], wk, p.work_base + item, sh, lane, d_grid, d_cw_rm, d_cw_scr);
  NRPHY_WG_TRACE_MARK(6);
}

// Seeds form ...
template <int QM, int L>
__global__ __launch_bounds__(WAVE * CB_WAVES) void codeblock_kernel_t(PdschLaunch p, const uint8_t* __restrict__ d_tb,
                                                              uint32_t* __restrict__ d_grid, uint32_t* __restrict__ d_cw_rm,
                                                              uint32_t* __restrict__ d_cw_scr)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn_lds[];
  codeblock_wave_t<QM, L, false>(p, d_tb, d_grid, d_cw_rm, d_cw_scr, dyn_lds);
}
// ... and words form of the plan's scrambling sequences.
template <int QM, int L>
__global__ __launch_bounds__(WAVE * CB_WAVES) void codeblock_words_kernel_t(PdschLaunch p, const uint8_t* __restrict__ d_tb,
                                                                    uint32_t* __restrict__ d_grid, uint32_t* __restrict__ d_cw_rm,
                                                                    uint32_t* __restrict__ d_cw_scr)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn_lds[];
  codeblock_wave_t<QM, L, true>(p, d_tb, d_grid, d_cw_rm, d_cw_scr, dyn_lds);
}

// One codeblock wave of the one-launch mixed kernel: the output stage is selected per wave.
template <bool WORDS>
__device__ __forceinline__ void codeblock_wave_mixed(const PdschLaunch& p, const uint8_t* __restrict__ d_tb,
                                                     uint32_t* __restrict__ d_grid, uint32_t* __restrict__ d_cw_rm,
                                                     uint32_t* __restrict__ d_cw_scr, uint32_t* dyn_lds)
{
  const CbWave   w    = cb_wave(p, dyn_lds);
  const uint32_t lane = w.lane;
  CbShared       sh;
  sh.lin   = w.lds;
  sh.u     = w.lds + p.lds_lin_words;
  sh.symb  = sh.u + CB_U_QAM_WORDS;
  sh.graph = sh.u + CB_U_GRAPH_OFFSET;
  sh.ldpc  = reinterpret_cast<LdpcScratch*>(sh.u + LDPC_DBL_WORDS);
  if (NRPHY_STAGE(p) == 10 || extra_wave(p, w, d_grid)) {
    return;
  }
  const uint32_t item = xcd_work_item(p.n_work, w);
  if (item == p.n_work) { // wave-uniform: the last workgroup's spare waves
    return;
  }
  const auto*  wkc = to_constant(&p.work[item]);
  const CbWork wk  = {wkc->pdu, wkc->cb, wkc->re_begin, wkc->re_count};
  PduRef       pd  = *to_constant(&p.pdus[wk.pdu]);
  if (!codeblock_front(p, pd, wk, sh, d_tb, lane)) {
    return;
  }
  switch (pd.qm) { // wave-uniform
    case 2:
      map_chunk_layers<2, WORDS>(p, pd, &p.pdus[wk.pdu], wk, p.work_base + item, sh, lane, d_grid, d_cw_rm, d_cw_scr);
      break;
    case 4:
      map_chunk_layers<4, WORDS>(p, pd, &p.pdus[wk.pdu], wk, p.work_base + item, sh, lane, d_grid, d_cw_rm, d_cw_scr);
      break;
    case 6:
      map_chunk_layers<6, WORDS>(p, pd, &p.pdus[wk.pdu], wk, p.work_base + item, sh, lane, d_grid, d_cw_rm, d_cw_scr);
      break;
    default:
      map_chunk_layers<8, WORDS>(p, pd, &p.pdus[wk.pdu], wk, p.work_base + item, sh, lane, d_grid, d_cw_rm, d_cw_scr);
      break;
  }
}

__global__ __launch_bounds__(WAVE * CB_WAVES) void codeblock_kernel(PdschLaunch p, const uint8_t* __restrict__ d_tb,
                                                         uint32_t* __restrict__ d_grid, uint32_t* __restrict__ d_cw_rm,
                                                         uint32_t* __restrict__ d_cw_scr)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn_lds[];
  codeblock_wave_mixed<false>(p, d_tb, d_grid, d_cw_rm, d_cw_scr, dyn_lds);
}
__global__ __launch_bounds__(WAVE * CB_WAVES) void codeblock_words_kernel(PdschLaunch p, const uint8_t* __restrict__ d_tb,
                                                               uint32_t* __restrict__ d_grid, uint32_t* __restrict__ d_cw_rm,
                                                               uint32_t* __restrict__ d_cw_scr)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn_lds[];
  codeblock_wave_mixed<true>(p, d_tb, d_grid, d_cw_rm, d_cw_scr, dyn_lds);
}

typedef void (*CodeblockKernel)(PdschLaunch, const uint8_t*, uint32_t*, uint32_t*, uint32_t*);

static CodeblockKernel bucket_kernel(uint32_t bucket, bool words)
{
  static const CodeblockKernel seeds_table[CB_BUCKETS] = {
      codeblock_kernel_t<2, 1>, codeblock_kernel_t<2, 2>, codeblock_kernel_t<2, 3>, codeblock_kernel_t<2, 4>,
      codeblock_kernel_t<4, 1>, codeblock_kernel_t<4, 2>, codeblock_kernel_t<4, 3>, codeblock_kernel_t<4, 4>,
      codeblock_kernel_t<6, 1>, codeblock_kernel_t<6, 2>, codeblock_kernel_t<6, 3>, codeblock_kernel_t<6, 4>,
      codeblock_kernel_t<8, 1>, codeblock_kernel_t<8, 2>, codeblock_kernel_t<8, 3>, codeblock_kernel_t<8, 4>};
  static const CodeblockKernel words_table[CB_BUCKETS] = {
      codeblock_words_kernel_t<2, 1>, codeblock_words_kernel_t<2, 2>, codeblock_words_kernel_t<2, 3>, codeblock_words_kernel_t<2, 4>,
      codeblock_words_kernel_t<4, 1>, codeblock_words_kernel_t<4, 2>, codeblock_words_kernel_t<4, 3>, codeblock_words_kernel_t<4, 4>,
      codeblock_words_kernel_t<6, 1>, codeblock_words_kernel_t<6, 2>, codeblock_words_kernel_t<6, 3>, codeblock_words_kernel_t<6, 4>,
      codeblock_words_kernel_t<8, 1>, codeblock_words_kernel_t<8, 2>, codeblock_words_kernel_t<8, 3>, codeblock_words_kernel_t<8, 4>};
  return words ? words_table[bucket] : seeds_table[bucket];
}

// bucket_begin[b] .. bucket_begin[b + 1]: the work items of bucket b = cb_bucket(Qm, layers) (the plan sorts them).
// dispatch: 0 = by plan shape, 1 = always the one-launch mixed kernel, 2 = always one launch per bucket.
bool codeblocks_take_bucket_launches(const PdschLaunch& p, const uint32_t* bucket_begin, int dispatch, uint32_t* nof_buckets)
{
  uint32_t n = 0;
  for (uint32_t b = 0; b != CB_BUCKETS; ++b) {
    n += bucket_begin[b + 1] != bucket_begin[b] ? 1u : 0u;
  }
  *nof_buckets = n;
  return !(dispatch == 1 || (dispatch == 0 && n > 1 && p.n_work < CB_MIXED_MAX_WORK));
}

// streams[0] is the caller's stream; with more than one bucket and n_streams > 1 the bucket launches are dealt to the
// streams in turn, biggest bucket first (the caller has made streams[1 ...] wait for what precedes on streams[0] and
// joins them afterwards): the buckets of a mixed batch then share the device like the waves of one launch instead of
// running one after the other, each with a tail of its own.
hipError_t launch_codeblocks(const PdschLaunch& p, const uint32_t* bucket_begin, int dispatch, const uint8_t* d_tb,
                             uint32_t* d_grid, uint32_t* d_cw_rm, uint32_t* d_cw_scr, const hipStream_t* streams, uint32_t n_streams)
{
  if (p.n_work == 0) {
    return hipSuccess;
  }
  const size_t   lds_bytes = 4u * (size_t)(p.lds_lin_words + p.lds_u_words) * CB_WAVES;
  const uint32_t extras    = d_grid ? p.n_dmrs_in_launch + p.n_zero_work : 0u;
  uint32_t       nof_buckets = 0;
  if (!codeblocks_take_bucket_launches(p, bucket_begin, dispatch, &nof_buckets)) {
    hipLaunchKernelGGL(p.scr_as_words != 0 ? codeblock_words_kernel : codeblock_kernel, dim3(cb_blocks(p.n_work) + cb_blocks(extras)),
                       dim3(WAVE * CB_WAVES), lds_bytes, streams[0], p, d_tb, d_grid, d_cw_rm, d_cw_scr);
    return hipGetLastError();
  }
  uint32_t order[CB_BUCKETS], n_order = 0; // non-empty buckets, biggest first
  for (uint32_t b = 0; b != CB_BUCKETS; ++b) {
    if (bucket_begin[b + 1] != bucket_begin[b]) {
      uint32_t k = n_order++;
      for (; k != 0 && bucket_begin[order[k - 1] + 1] - bucket_begin[order[k - 1]] < bucket_begin[b + 1] - bucket_begin[b]; --k) {
        order[k] = order[k - 1];
      }
      order[k] = b;
    }
  }
  for (uint32_t i = 0; i != n_order; ++i) {
    const uint32_t b = order[i], n = bucket_begin[b + 1] - bucket_begin[b];
    PdschLaunch    q = p;
    q.work           = p.work + bucket_begin[b];
    q.work_base      = bucket_begin[b];
    q.n_work         = n;
    if (i != 0) { // the DM-RS and zero-fill waves ride at the end of the biggest bucket's launch
      q.n_dmrs_in_launch = 0;
      q.n_zero_work      = 0;
    }
    const uint32_t blocks = cb_blocks(n) + (i == 0 ? cb_blocks(extras) : 0u);
    hipLaunchKernelGGL(bucket_kernel(b, p.scr_as_words != 0), dim3(blocks), dim3(WAVE * CB_WAVES), lds_bytes, streams[n_streams > 1 ? i % n_streams : 0], q,
                       d_tb, d_grid, d_cw_rm, d_cw_scr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      return e;
    }
  }
  return hipSuccess;
}

__global__ __launch_bounds__(WAVE) void dmrs_kernel(PdschLaunch p, uint32_t* __restrict__ d_grid)
{
  __shared__ uint32_t tab[8 * NRPHY_MAX_PORTS * 2];
  dmrs_wave(p, blockIdx.x, d_grid, threadIdx.x, tab);
}

hipError_t launch_dmrs(const PdschLaunch& p, uint32_t* d_grid, hipStream_t stream)
{
  if (p.n_dmrs_work == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(dmrs_kernel, dim3(p.n_dmrs_work), dim3(WAVE), 0, stream, p, d_grid);
  return hipGetLastError();
}

// ================================================================================================================
// Stand-alone LDPC encoder: ldpc_encoder::encode for n_cb codeblocks of one (base graph, lifting size).
// ================================================================================================================
__global__ __launch_bounds__(WAVE) void ldpc_encode_kernel(const LiftedGraph* graphs, uint32_t graph, uint32_t kb,
                                                           uint32_t zc, const uint8_t* __restrict__ d_msg,
                                                           uint32_t msg_stride, uint32_t out_bits,
                                                           uint8_t* __restrict__ d_out, uint32_t out_stride)
{
  __shared__ uint32_t    lin[LDPC_LIN_WORDS];
  __shared__ uint32_t    gbuf[LDPC_GRAPH_ROWPTR + MAX_BG_EDGES];
  __shared__ uint32_t    dbl[LDPC_DBL_WORDS];
  __shared__ LdpcScratch scratch;
  const uint32_t         lane = threadIdx.x;
  const uint8_t*         msg  = d_msg + (size_t)blockIdx.x * msg_stride;
  uint8_t*               out  = d_out + (size_t)blockIdx.x * out_stride;

  // Codeblock length the encoder has to produce (ldpc_encoder_impl.cpp:63-72).
  const uint32_t K   = kb * zc;
  uint32_t       len = out_bits + 2u * zc;
  len                = len < (kb + 4u) * zc ? (kb + 4u) * zc : len;
  const uint32_t nof_rows    = (len + zc - 1u) / zc - kb;
  const uint32_t total_words = (((kb + nof_rows) * zc + 31u) >> 5) + 2u;
  const uint32_t msg_bytes   = (K + 7u) >> 3;
  for (uint32_t j = lane; j < total_words; j += WAVE) {
    uint32_t v = 0;
    for (uint32_t k = 0; k != 4; ++k) {
      uint32_t byte = 4u * j + k;
      v             = (v << 8) | (byte < msg_bytes ? (uint32_t)msg[byte] : 0u);
    }
    uint32_t pos = 32u * j;
    v            = pos >= K ? 0u : (K - pos < 32u ? v & topmask(K - pos) : v);
    lin[j]       = v;
  }
  stage_graph(&graphs[graph], nof_rows, gbuf, lane);
  wave_sync();
  ldpc_encode_wave(&graphs[graph], gbuf, kb, zc, nof_rows, lin, dbl, &scratch, lane);
  const uint32_t out_bytes = (out_bits + 7u) >> 3;
  for (uint32_t j = lane; 4u * j < out_bytes; j += WAVE) {
    uint32_t v   = ext32(lin, 2u * zc + 32u * j);
    uint32_t pos = 32u * j;
    if (out_bits - pos < 32u) {
      v &= topmask(out_bits - pos);
    }
    for (uint32_t k = 0; k != 4 && 4u * j + k < out_bytes; ++k) {
      out[4u * j + k] = (uint8_t)(v >> (24 - 8 * k));
    }
  }
}

hipError_t launch_ldpc_encode(const LiftedGraph* graphs, uint32_t graph, uint32_t kb, uint32_t zc, uint32_t n_cb,
                              const uint8_t* d_msg, uint32_t msg_stride, uint32_t out_bits, uint8_t* d_out,
                              uint32_t out_stride, hipStream_t stream)
{
  if (n_cb == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(ldpc_encode_kernel, dim3(n_cb), dim3(WAVE), 0, stream, graphs, graph, kb, zc, d_msg, msg_stride,
                     out_bits, d_out, out_stride);
  return hipGetLastError();
}

} // namespace nrphy
