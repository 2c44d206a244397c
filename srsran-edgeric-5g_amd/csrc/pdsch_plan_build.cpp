// What a PDSCH plan is: per-PDU scalar derivation (what pdsch_processor_impl / ldpc_segmenter_impl / ldpc_rate_matcher_impl
// compute on the CPU before their loops) and the builder of a plan's host fields and tables.  Pure host arithmetic: no HIP
// runtime call and no context here, so that all of it runs -- and can be checked -- without a device (pdsch_host.cpp has the rest).
#include "pdsch_plan.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <new>
#include <unordered_map>
#include <vector>

namespace {

// What decides the sequences a PDU asks the prologue for (SequenceSharing).  scr: c_init, C, n_short, e_short, e_long, bits per
// resource element -- the sequence and where the work items' seeds lie in it (with RE_CHUNK).  dmrs: symbol mask, words per
// symbol, c_init of the DM-RS symbols.
struct SeqKey {
  std::array<uint32_t, 6>               scr;
  std::array<uint32_t, 2 + NRPHY_NSYMB> dmrs;
  bool operator==(const SeqKey& o) const { return scr == o.scr && dmrs == o.dmrs; }
};
struct SeqKeyHash {
  size_t operator()(const SeqKey& k) const
  {
    uint64_t h = 0xCBF29CE484222325ULL; // FNV-1a over the words
    for (uint32_t w : k.scr) {
      h = (h ^ w) * 0x100000001B3ULL;
    }
    for (uint32_t w : k.dmrs) {
      h = (h ^ w) * 0x100000001B3ULL;
    }
    return (size_t)(h ^ (h >> 32));
  }
};
struct SeqShare {
  uint32_t seed_first;      // PduDev::seed_first of the PDUs that share the scrambling sequence (seeds form)
  uint32_t scr_word_offset; // PduDev::scr_word_offset of the same PDUs (words form)
  uint32_t dmrs_seq_offset; // PduDev::dmrs_seq_offset of those that share the DM-RS sequences
};
constexpr uint8_t SEQ_NEW_SCR = 1, SEQ_NEW_DMRS = 2;
// A plan stores its distinct scrambling sequences as words while they take no more than this: one XCD's L2, so that the words,
// written once by the prologue, are served from every L2 like the x1 table.  Beyond it a plan stores seeds (a batch of 1024
// PDUs that share nothing would write and read back 121 MB of sequences).
constexpr uint64_t SCR_WORDS_BUDGET_BYTES = 4ULL << 20;

} // namespace

// pdsch_processor_validator_impl::is_valid (R/lib/phy/upper/channel_processors/pdsch_processor_validator_impl.cpp:99-181),
// plus the checks the reference leaves to assertions deeper in the chain (modulation, rv, base graph, sizes).
extern "C" int nrphy_pdsch_validate(const nrphy_pdsch_pdu_t* pdu)
{
  if (pdu == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  const unsigned nsymb = pdu->cp ? 12 : 14;
  const int      lo = mask_lowest(pdu->prb_mask), hi = mask_highest(pdu->prb_mask);
  if (lo < 0 || (unsigned)lo < pdu->bwp_start_rb || (unsigned)hi >= pdu->bwp_start_rb + pdu->bwp_size_rb ||
      pdu->bwp_start_rb + pdu->bwp_size_rb > NRPHY_MAX_RB) {
    return NRPHY_ERR_INVALID_PDU; // freq_alloc.is_bwp_valid
  }
  if (pdu->dmrs_symbol_mask == 0 || (pdu->dmrs_symbol_mask >> nsymb) != 0) {
    return NRPHY_ERR_INVALID_PDU;
  }
  const unsigned first_dmrs = (unsigned)__builtin_ctz(pdu->dmrs_symbol_mask);
  const unsigned last_dmrs  = 31U - (unsigned)__builtin_clz(pdu->dmrs_symbol_mask);
  if (first_dmrs < pdu->start_symbol_index || last_dmrs >= pdu->start_symbol_index + pdu->nof_symbols ||
      nsymb < pdu->start_symbol_index + pdu->nof_symbols) {
    return NRPHY_ERR_INVALID_PDU;
  }
  if (pdu->dmrs_type != 1 || pdu->nof_cdm_groups_without_data > 2 || !pdu->vrb_contiguous) {
    return NRPHY_ERR_INVALID_PDU;
  }
  for (int prb = lo; prb <= hi; ++prb) { // "only contiguous allocation": the flag and the mask must tell the same story
    if (!mask_test(pdu->prb_mask, (unsigned)prb)) {
      return NRPHY_ERR_INVALID_PDU;
    }
  }
  if (pdu->nof_ports == 0 || pdu->nof_ports > NRPHY_MAX_PORTS || pdu->nof_layers == 0 ||
      pdu->nof_layers > pdu->nof_ports) {
    return NRPHY_ERR_INVALID_PDU;
  }
  if (pdu->nof_codewords != 1 || pdu->tbs_lbrm_bytes == 0 || pdu->nof_reserved > NRPHY_MAX_RESERVED) {
    return NRPHY_ERR_INVALID_PDU;
  }
  for (unsigned r = 0; r != pdu->nof_reserved; ++r) {
    if (pdu->reserved[r].symbol_mask & pdu->dmrs_symbol_mask) {
      return NRPHY_ERR_INVALID_PDU; // check_dmrs_and_reserved_collision
    }
  }
  if ((pdu->qm != 2 && pdu->qm != 4 && pdu->qm != 6 && pdu->qm != 8) || pdu->rv > 3 ||
      (pdu->ldpc_base_graph != 1 && pdu->ldpc_base_graph != 2) || pdu->tb_size_bytes == 0 ||
      pdu->tb_size_bytes > NRPHY_MAX_TB_BYTES || pdu->nof_prg == 0 || pdu->nof_prg > NRPHY_MAX_PRG || pdu->prg_size_rb == 0 || pdu->prg_size_rb > NRPHY_MAX_RB || pdu->precoding == nullptr || pdu->cp > 1) {
    // (nof_prg sizes the read of the caller's weight array: at most one PRG per resource block)
    return NRPHY_ERR_INVALID_PDU;
  }
  return NRPHY_OK;
}

namespace {

// Data-RE mask of OFDM symbol l: allocation minus reserved minus DM-RS pattern
// (pdsch_modulator_impl.cpp:52-106, re_pattern.cpp:27-60, dmrs_mapping.h:69-123).
// (the mask as a plain array of nof_subc bytes: through a vector that lives in an object, every byte stored would make
// the loops read the vector's pointers again)
void data_re_mask(const nrphy_pdsch_pdu_t& pdu, unsigned l, uint8_t* mask, unsigned nof_subc)
{
  std::fill(mask, mask + nof_subc, 0);
  if (l < pdu.start_symbol_index || l >= pdu.start_symbol_index + pdu.nof_symbols) {
    return;
  }
  const unsigned nof_prb = nof_subc / 12;
  for (unsigned p = 0; p != nof_prb; ++p) {
    if (mask_test(pdu.prb_mask, p)) {
      std::fill(mask + 12 * p, mask + 12 * p + 12, 1);
    }
  }
  for (unsigned r = 0; r != pdu.nof_reserved; ++r) {
    const nrphy_re_pattern_t& pat = pdu.reserved[r];
    if (!((pat.symbol_mask >> l) & 1U)) {
      continue;
    }
    for (unsigned p = 0; p != nof_prb; ++p) {
      if (!mask_test(pat.prb_mask, p)) {
        continue;
      }
      for (unsigned k = 0; k != 12; ++k) {
        if ((pat.re_mask >> k) & 1U) {
          mask[12 * p + k] = 0;
        }
      }
    }
  }
  if ((pdu.dmrs_symbol_mask >> l) & 1U) {
    for (unsigned p = pdu.bwp_start_rb; p < pdu.bwp_start_rb + pdu.bwp_size_rb && p < nof_prb; ++p) {
      for (unsigned k = 0; k != 12; ++k) {
        if ((k % 2) < pdu.nof_cdm_groups_without_data) {
          mask[12 * p + k] = 0;
        }
      }
    }
  }
}

} // namespace

void derive(const nrphy_pdsch_pdu_t& pdu, unsigned nof_re, nrphy_pdsch_derived_t& d, const uint32_t* nref_override)
{
  const unsigned bg      = pdu.ldpc_base_graph;
  const unsigned tb_bits = 8 * pdu.tb_size_bytes;
  const unsigned tb_crc  = (tb_bits <= 3824) ? 16 : 24;
  const unsigned b       = tb_bits + tb_crc;
  const unsigned kcb     = (bg == 1) ? 8448 : 3840;
  const unsigned C       = (b <= kcb) ? 1 : divide_ceil(b, kcb - 24);
  const unsigned b_out   = b + ((C > 1) ? 24 * C : 0);
  unsigned       ref_len = 22;
  if (bg == 2) {
    ref_len = (b > 640) ? 10 : (b > 560) ? 9 : (b > 192) ? 8 : 6;
  }
  unsigned zc = 0;
  for (unsigned i = 0; i != NOF_LIFTING_SIZES; ++i) {
    if (LIFTING_SIZES[i] * C * ref_len >= b_out) {
      zc = LIFTING_SIZES[i];
      break;
    }
  }
  const unsigned K      = ((bg == 1) ? 22 : 10) * zc;
  const unsigned cb_crc = (C > 1) ? 24 : 0;
  const unsigned info   = divide_ceil(b_out, C) - cb_crc;
  const unsigned N      = ((bg == 1) ? 66 : 50) * zc;
  uint64_t       nref   = ((uint64_t)pdu.tbs_lbrm_bytes * 8 * 3) / (2 * C); // ldpc::compute_N_ref
  if (nref_override != nullptr) {
    nref = *nref_override;
  }
  nref                  = std::min<uint64_t>(nref, 66 * 384);
  d.nof_re              = nof_re;
  d.nof_codeblocks      = C;
  d.lifting_size        = zc;
  d.segment_length      = K;
  d.cb_info_bits        = info;
  d.nof_filler_bits     = K - info - cb_crc;
  d.nof_tb_crc_bits     = tb_crc;
  d.nof_cb_crc_bits     = cb_crc;
  d.zero_pad            = (info + cb_crc) * C - b_out;
  d.full_length         = N;
  d.n_ref               = (uint32_t)nref;
  d.n_cb                = (nref > 0 && nref < N) ? (uint32_t)nref : N;
  static const double shift_bg1[4] = {0, 17, 33, 56};
  static const double shift_bg2[4] = {0, 13, 25, 43};
  const double tmp      = (((bg == 1) ? shift_bg1 : shift_bg2)[pdu.rv] * d.n_cb) / N; // ldpc_rate_matcher_impl.cpp:89-90
  d.k0                  = (uint32_t)((uint16_t)std::floor(tmp)) * zc;
  d.nof_short_segments  = C - (nof_re % C);
  d.rm_length_short     = (nof_re / C) * pdu.nof_layers * pdu.qm;
  d.rm_length_long      = divide_ceil(nof_re, C) * pdu.nof_layers * pdu.qm;
  d.codeword_bits       = nof_re * pdu.nof_layers * pdu.qm;
}

namespace {

unsigned count_data_re(const nrphy_pdsch_pdu_t& pdu)
{
  std::vector<uint8_t> mask(NRPHY_MAX_RB * 12);
  unsigned             count = 0;
  for (unsigned l = 0; l != NRPHY_NSYMB; ++l) {
    data_re_mask(pdu, l, mask.data(), (unsigned)mask.size());
    for (uint8_t m : mask) {
      count += m;
    }
  }
  return count;
}

} // namespace

extern "C" int nrphy_pdsch_derive(const nrphy_pdsch_pdu_t* pdu, nrphy_pdsch_derived_t* out)
{
  if (pdu == nullptr || out == nullptr || pdu->tb_size_bytes == 0 || pdu->nof_layers == 0 || pdu->qm == 0 ||
      (pdu->ldpc_base_graph != 1 && pdu->ldpc_base_graph != 2) || pdu->rv > 3) {
    return NRPHY_ERR_ARGUMENT;
  }
  derive(*pdu, count_data_re(*pdu), *out);
  return NRPHY_OK;
}

// TS 38.214 Section 5.1.3.2 (tbs_calculator_calculate, R/lib/ran/sch/tbs_calculator.cpp:31-144).
extern "C" uint32_t nrphy_tbs_calculate(uint32_t nof_symb_sh, uint32_t nof_dmrs_prb, uint32_t nof_oh_prb, uint32_t qm,
                                        float target_code_rate, uint32_t nof_layers, uint32_t n_prb)
{
  static const uint16_t table[93] = {
      24,   32,   40,   48,   56,   64,   72,   80,   88,   96,   104,  112,  120,  128,  136,  144,  152,  160,  168,
      176,  184,  192,  208,  224,  240,  256,  272,  288,  304,  320,  336,  352,  368,  384,  408,  432,  456,  480,
      504,  528,  552,  576,  608,  640,  672,  704,  736,  768,  808,  848,  888,  928,  984,  1032, 1064, 1128, 1160,
      1192, 1224, 1256, 1288, 1320, 1352, 1416, 1480, 1544, 1608, 1672, 1736, 1800, 1864, 1928, 2024, 2088, 2152, 2216,
      2280, 2408, 2472, 2536, 2600, 2664, 2728, 2792, 2856, 2976, 3104, 3240, 3368, 3496, 3624, 3752, 3824};
  const unsigned nof_re_prime = 12 * nof_symb_sh - nof_dmrs_prb - nof_oh_prb;
  const unsigned nof_re       = std::min(nof_re_prime, 156U) * n_prb;
  const float    tcr          = target_code_rate * (1.F / 1024);
  const float    nof_info     = 1.0F * (float)nof_re * tcr * (float)qm * (float)nof_layers;
  if (nof_info <= 3824) {
    unsigned n = 3;
    if (nof_info > 512) {
      n = (unsigned)std::floor(std::log2(nof_info)) - 6U;
    }
    const unsigned p2    = 1U << n;
    const unsigned prime = std::max(24U, p2 * (unsigned)std::floor(nof_info / (float)p2));
    for (uint16_t v : table) {
      if (v >= prime) {
        return v;
      }
    }
    return 3824;
  }
  const unsigned n     = (unsigned)(std::floor(std::log2(nof_info - 24)) - 5.0F);
  const unsigned p2    = 1U << n;
  const unsigned prime = std::max(3840U, p2 * (unsigned)std::round((nof_info - 24) / (float)p2));
  unsigned       C     = 1;
  if (tcr <= 0.25F) {
    C = divide_ceil(prime + 24, 3816);
  } else if (prime > 8424) {
    C = divide_ceil(prime + 24, 8424);
  }
  return 8 * C * divide_ceil(prime + 24, 8 * C) - 24;
}

// ================================================================================================================
// PDSCH plan
// ================================================================================================================
namespace {

// Everything the RE mapping of a PDU depends on (data_re_mask + the DM-RS comb): PDUs of a batch that repeat an
// allocation share its tables instead of rebuilding them.
void append_allocation_signature(const nrphy_pdsch_pdu_t& pdu, std::vector<uint64_t>& sig)
{
  sig.insert(sig.end(), std::begin(pdu.prb_mask), std::end(pdu.prb_mask));
  sig.push_back(((uint64_t)pdu.start_symbol_index << 48) | ((uint64_t)pdu.nof_symbols << 40) |
                ((uint64_t)pdu.nof_cdm_groups_without_data << 36) | ((uint64_t)pdu.nof_layers << 32) |
                pdu.dmrs_symbol_mask);
  sig.push_back(((uint64_t)pdu.bwp_start_rb << 32) | ((uint64_t)pdu.bwp_size_rb << 8) | pdu.nof_reserved);
  for (unsigned r = 0; r != pdu.nof_reserved; ++r) {
    sig.insert(sig.end(), std::begin(pdu.reserved[r].prb_mask), std::end(pdu.reserved[r].prb_mask));
    sig.push_back(((uint64_t)pdu.reserved[r].re_mask << 32) | pdu.reserved[r].symbol_mask);
  }
}

} // namespace

PlanShapeCache* plan_shape_cache_create()
{
  return new (std::nothrow) PlanShapeCache;
}
void plan_shape_cache_destroy(PlanShapeCache* c)
{
  delete c;
}

namespace {

// sym_re_start, sym_kind and sym_arg travel together between a ReMapping and a PduDev.
template <typename To, typename From>
void copy_mapping(To& to, const From& from)
{
  static_assert(sizeof(to.sym_re_start) == sizeof(from.sym_re_start) && sizeof(to.sym_kind) == sizeof(from.sym_kind) &&
                    sizeof(to.sym_arg) == sizeof(from.sym_arg),
                "the RE mapping of a PDU has one layout");
  std::memcpy(to.sym_re_start, from.sym_re_start, sizeof(to.sym_re_start));
  std::memcpy(to.sym_kind, from.sym_kind, sizeof(to.sym_kind));
  std::memcpy(to.sym_arg, from.sym_arg, sizeof(to.sym_arg));
}

// Which sequences the PDUs of a plan share.  Owns the look-up and the running totals of both forms of the scrambling
// sequences; reads the PDU descriptors it is shown and writes nothing else.
class SequenceSharing
{
public:
  struct Shared {
    SeqShare at;    // PduDev::seed_first, scr_word_offset and dmrs_seq_offset of the PDU
    uint8_t  fresh; // SEQ_NEW_SCR / SEQ_NEW_DMRS: the PDU is the first that asks for the sequence, and generates it
  };
  std::vector<uint8_t> fresh;          // per PDU: Shared::fresh
  uint32_t             seed_slots = 0; // seed slots handed out: one per work item of every distinct scrambling sequence
  uint64_t             words = 0;      // the same sequences as words: where the next one would start, and their plain sum (the rule)
  uint64_t             words_sum = 0;
  bool                 words_fit = true; // every sequence within the x1 table and the 32-bit offsets
  uint64_t             dmrs_words = 0;   // words of the distinct DM-RS sequences: they lead the plan's scratch
  uint32_t             n_scr_seq = 0, n_dmrs_seq = 0;

  // The next PDU of the plan, described in `pd` (sizes, c_init values, scr_words, dmrs_seq_words) with `nof_items` work items;
  // alone: the plan has no other PDU to share with.
  Shared add_pdu(const PduDev& pd, uint32_t nof_items, bool alone)
  {
    // Sequences are generated once per run and distinct sequence, not once per PDU: a batch of slots of one UE asks for the
    // same scrambling seeds in every slot and for the same DM-RS sequences in every frame.  The seeds depend on c_init and on
    // where the work items start in the codeword; the DM-RS sequences on the DM-RS symbols' c_init and on their length.  One
    // look-up per PDU (both keys at once); what a new pair shares with earlier PDUs is found by a look-up per half.  Nothing
    // here outlives the plan's creation, and every run still computes every distinct sequence from scratch.
    const uint32_t nof_dmrs_words = (uint32_t)(((uint64_t)pd.dmrs_seq_words * (unsigned)__builtin_popcount(pd.dmrs_symbol_mask) + 3U) & ~3ULL);
    Shared         s = {{seed_slots, (uint32_t)words, (uint32_t)dmrs_words}, (uint8_t)(SEQ_NEW_SCR | (nof_dmrs_words != 0 ? SEQ_NEW_DMRS : 0))};
    if (!alone) {
      SeqKey key;
      key.scr  = {pd.c_init, pd.C, pd.n_short, pd.e_short, pd.e_long, pd.nof_layers * pd.qm};
      key.dmrs = {};
      key.dmrs[0] = pd.dmrs_symbol_mask;
      key.dmrs[1] = pd.dmrs_seq_words;
      for (unsigned l = 0; l != NRPHY_NSYMB; ++l) {
        key.dmrs[2 + l] = ((pd.dmrs_symbol_mask >> l) & 1U) ? pd.dmrs_c_init[l] : 0U;
      }
      auto both = shares.find(key);
      if (both != shares.end()) {
        s = {both->second, 0};
      } else {
        SeqKey half = key;
        half.dmrs   = {};
        half.dmrs[1] = ~0U; // (no DM-RS sequence has this length)
        auto scr_known = shares.insert({half, s.at});
        if (!scr_known.second) {
          s.at.seed_first      = scr_known.first->second.seed_first;
          s.at.scr_word_offset = scr_known.first->second.scr_word_offset;
          s.fresh &= (uint8_t)~SEQ_NEW_SCR;
        }
        if (nof_dmrs_words != 0) {
          half     = key;
          half.scr = {}; // (no codeword has zero bits per resource element)
          auto dmrs_known = shares.insert({half, s.at});
          if (!dmrs_known.second) {
            s.at.dmrs_seq_offset = dmrs_known.first->second.dmrs_seq_offset;
            s.fresh &= (uint8_t)~SEQ_NEW_DMRS;
          }
        }
        shares.insert({key, s.at});
      }
    }
    if (s.fresh & SEQ_NEW_SCR) {
      seed_slots += nof_items;
      words_sum += pd.scr_words;
      words += (pd.scr_words + 15U) & ~15ULL; // every sequence starts a 64-byte line
      words_fit = words_fit && pd.scr_words <= (uint32_t)GOLD_X1_WORDS && words <= 0xFFFFFFFFULL;
      ++n_scr_seq;
    }
    if (s.fresh & SEQ_NEW_DMRS) {
      dmrs_words += nof_dmrs_words;
      ++n_dmrs_seq;
    }
    fresh.push_back(s.fresh);
    return s;
  }

private:
  std::unordered_map<SeqKey, SeqShare, SeqKeyHash> shares; // the sequences earlier PDUs of the plan ask for
};

// One build of a plan: the arguments of pdsch_plan_build, the scratch containers that serve every PDU in turn (none is
// allocated per PDU: this runs on the submit path of the asynchronous queue), and the steps in the order build() takes them.
class PlanBuilder
{
public:
  PlanBuilder(const LiftedGraph* graphs_, const Tunables& tune_, uint32_t n_pdu_, const nrphy_pdsch_pdu_t* pdus_,
              const uint64_t* tb_offset_, const uint32_t* grid_index_, uint32_t nof_grids_, uint32_t grid_nof_ports_,
              uint32_t grid_nof_subc_, const EncodeOnly* enc_, PlanShapeCache* shapes_, nrphy_pdsch_plan& plan_, PlanTables& tables)
    : graphs(graphs_), tune(tune_), n_pdu(n_pdu_), pdus(pdus_), tb_offset(tb_offset_), grid_index(grid_index_), nof_grids(nof_grids_),
      grid_nof_ports(grid_nof_ports_), grid_nof_subc(grid_nof_subc_), enc(enc_), shapes(shapes_), plan(plan_), t(tables),
      pdus_of_grid(nof_grids_), mask(grid_nof_subc_)
  {
  }
  int build(size_t scratch_capacity_words);

private:
  using Runs = std::array<uint32_t, 3>; // a zero-fill run list in PlanTables::zero_segs: (begin, count, long runs)

  int      check_pdu(uint32_t i) const;
  unsigned map_resource_elements(uint32_t i, PduDev& pd);
  void     build_remap(const nrphy_pdsch_pdu_t& pdu, PlanShapeCache::Remap& built);
  void     describe_pdu(uint32_t i, const nrphy_pdsch_derived_t& d, PduDev& pd);
  uint32_t add_codeblock_work(uint32_t i, const nrphy_pdsch_derived_t& d, const PduDev& pd);
  void     add_sequence_work();
  int      add_tb_crc_work();
  void     build_zero_fill();
  Runs     zero_runs(uint32_t g, uint32_t port);
  void     cover(uint32_t g, uint32_t port);
  void     sort_into_buckets();
  void     choose_scrambling_form(size_t scratch_capacity_words);

  const LiftedGraph*       graphs;
  const Tunables&          tune;
  const uint32_t           n_pdu;
  const nrphy_pdsch_pdu_t* pdus;
  const uint64_t*          tb_offset;
  const uint32_t*          grid_index;
  const uint32_t           nof_grids, grid_nof_ports, grid_nof_subc;
  const EncodeOnly*        enc;
  PlanShapeCache*          shapes;
  nrphy_pdsch_plan&        plan;
  PlanTables&              t;

  uint64_t                                   cw_bits = 0;
  SequenceSharing                            seqs;
  std::vector<std::vector<uint32_t>>         pdus_of_grid;
  std::map<std::vector<uint64_t>, ReMapping> remap_cache; // allocation -> its mapping in this plan
  std::map<std::vector<uint64_t>, Runs>      seen;         // zero fill: segment list -> its runs
  std::map<std::vector<uint64_t>, Runs>      by_signature; // zero fill: allocations on a (grid, port) -> their runs
  // scratch
  std::vector<uint8_t>  mask; // one symbol of the grid
  std::vector<uint16_t> list;
  std::vector<uint64_t> remap_sig;
  std::vector<uint8_t>  cov; // every symbol of one (grid, port)
  std::vector<uint64_t> key, sig, shape_key;
};

// Reads PDU i and the grid shape; appends to nothing.  The status plan creation refuses the PDU with, or NRPHY_OK.
int PlanBuilder::check_pdu(uint32_t i) const
{
  const nrphy_pdsch_pdu_t& pdu = pdus[i];
  if (enc == nullptr ? nrphy_pdsch_validate(&pdu) != NRPHY_OK
                     : (pdu.qm < 2 || pdu.qm > 8 || (pdu.qm & 1U) || pdu.rv > 3 || pdu.nof_layers == 0 ||
                        pdu.nof_layers > NRPHY_MAX_LAYERS || pdu.tb_size_bytes == 0 ||
                        pdu.tb_size_bytes > NRPHY_MAX_TB_BYTES || (pdu.ldpc_base_graph != 1 && pdu.ldpc_base_graph != 2))) {
    return NRPHY_ERR_INVALID_PDU;
  }
  const uint32_t g = grid_index ? grid_index[i] : 0;
  if (g >= nof_grids || pdu.nof_ports > grid_nof_ports || (tb_offset[i] & 3U) != 0 ||
      (enc == nullptr && 12U * (unsigned)(mask_highest(pdu.prb_mask) + 1) > grid_nof_subc)) {
    return NRPHY_ERR_ARGUMENT;
  }
  return NRPHY_OK;
}

// The RE mapping of one allocation with its table entries numbered from zero.  Reads the PDU's allocation; writes `built`
// alone (mask and list are scratch).
void PlanBuilder::build_remap(const nrphy_pdsch_pdu_t& pdu, PlanShapeCache::Remap& built)
{
  const unsigned nof_subc = grid_nof_subc; // (a local: the loops below store, and a member would be read again after every store)
  unsigned       nof_re   = 0;
  for (unsigned l = 0; l != NRPHY_NSYMB; ++l) {
    built.m.sym_re_start[l] = nof_re;
    built.m.sym_arg[l]      = 0;
    uint8_t* m = mask.data();
    data_re_mask(pdu, l, m, nof_subc);
    // The subcarriers of the symbol's data RE, written through a plain pointer (a push_back per RE on a member costs more
    // than everything else here).
    list.resize(nof_subc);
    uint16_t* out   = list.data();
    unsigned  count = 0;
    for (unsigned k = 0; k != nof_subc; ++k) {
      out[count] = (uint16_t)k;
      count += m[k];
    }
    list.resize(count);
    if (list.empty()) {
      built.m.sym_kind[l] = SYM_NONE;
    } else if ((unsigned)(list.back() - list.front()) + 1 == list.size()) {
      built.m.sym_kind[l] = SYM_CONTIGUOUS;
      built.m.sym_arg[l]  = list.front();
    } else {
      built.m.sym_kind[l] = SYM_TABLE;
      built.m.sym_arg[l]  = (uint32_t)built.table.size();
      // Reuse an earlier symbol's list when identical (the common case).
      for (unsigned lp = 0; lp != l; ++lp) {
        if (built.m.sym_kind[lp] == SYM_TABLE && built.m.sym_re_start[lp + 1] - built.m.sym_re_start[lp] == list.size() &&
            std::equal(list.begin(), list.end(), built.table.begin() + built.m.sym_arg[lp])) {
          built.m.sym_arg[l] = built.m.sym_arg[lp];
          break;
        }
      }
      if (built.m.sym_arg[l] == built.table.size()) {
        built.table.insert(built.table.end(), list.begin(), list.end());
      }
    }
    nof_re += (unsigned)list.size();
    built.m.sym_re_start[l + 1] = nof_re;
  }
}

// RE mapping tables of PDU i into pd.sym_*; returns its count of data RE.  Three sources: a PDU of this plan with the same
// allocation (remap_cache), the caller's shape cache, or a fresh build.  Appends to re_table, remap_cache and the shape cache.
unsigned PlanBuilder::map_resource_elements(uint32_t i, PduDev& pd)
{
  if (enc != nullptr) {
    const unsigned nof_re = enc[i].nof_re; // no RE mapping: every symbol empty, the count given
    for (unsigned l = 0; l <= NRPHY_NSYMB; ++l) {
      pd.sym_re_start[l] = (l == NRPHY_NSYMB) ? nof_re : 0;
    }
    return nof_re;
  }
  remap_sig.clear();
  append_allocation_signature(pdus[i], remap_sig);
  auto cached = remap_cache.find(remap_sig);
  if (cached != remap_cache.end()) {
    copy_mapping(pd, cached->second);
    return pd.sym_re_start[NRPHY_NSYMB];
  }
  // The mapping with its table entries numbered from zero (`rel`): from the caller's shape cache, or built here.
  PlanShapeCache::Remap        built;
  const PlanShapeCache::Remap* rel = nullptr;
  if (shapes != nullptr) {
    auto known = shapes->remap.find(remap_sig);
    if (known != shapes->remap.end()) {
      rel = &known->second;
    }
  }
  if (rel == nullptr) {
    build_remap(pdus[i], built);
    rel = &built;
    if (shapes != nullptr) {
      rel = &shapes->remap.insert({remap_sig, built}).first->second;
    }
  }
  // Into this plan: the table entries behind what the plan holds already.
  const uint32_t base = (uint32_t)t.re_table.size();
  t.re_table.insert(t.re_table.end(), rel->table.begin(), rel->table.end());
  ReMapping m;
  copy_mapping(m, rel->m);
  for (unsigned l = 0; l != NRPHY_NSYMB; ++l) {
    m.sym_arg[l] += (m.sym_kind[l] == SYM_TABLE ? base : 0U);
  }
  copy_mapping(pd, m);
  remap_cache.insert({remap_sig, m});
  return pd.sym_re_start[NRPHY_NSYMB];
}

// The descriptor of PDU i from the PDU and its derived sizes `d`: sizes, reachable parity rows, precoding weights, DM-RS
// constants, PRB mask, lengths of its sequences.  Appends to weights, dmrs and pdus_of_grid; reads cw_bits.
void PlanBuilder::describe_pdu(uint32_t i, const nrphy_pdsch_derived_t& d, PduDev& pd)
{
  const nrphy_pdsch_pdu_t& pdu = pdus[i];
  const unsigned           kb  = (pdu.ldpc_base_graph == 1) ? 22 : 10;
  pd.tb_offset      = tb_offset[i];
  pd.cw_bit_offset  = cw_bits;
  pd.tb_bytes       = pdu.tb_size_bytes;
  pd.grid_index     = grid_index ? grid_index[i] : 0;
  pd.graph          = (pdu.ldpc_base_graph - 1) * NOF_LIFTING_SIZES + (uint32_t)lifting_position(d.lifting_size);
  pd.zc             = d.lifting_size;
  pd.kb             = kb;
  pd.K              = d.segment_length;
  pd.info_bits      = d.cb_info_bits;
  pd.filler         = d.nof_filler_bits;
  pd.tb_crc_bits    = d.nof_tb_crc_bits;
  pd.cb_crc_bits    = d.nof_cb_crc_bits;
  pd.zero_pad       = d.zero_pad;
  pd.C              = d.nof_codeblocks;
  pd.n_short        = d.nof_short_segments;
  pd.e_short        = d.rm_length_short;
  pd.e_long         = d.rm_length_long;
  pd.n_cb           = d.n_cb;
  pd.k0             = d.k0;
  pd.qm             = pdu.qm;
  pd.nof_layers     = pdu.nof_layers;
  pd.nof_ports      = pdu.nof_ports;
  pd.c_init         = (pdu.rnti << 15) + pdu.n_id; // q = 0 (pdsch_modulator_impl.cpp:35)
  pd.nof_re         = d.nof_re;
  // Parity rows rate matching can reach (the reference always computes all of them, pdsch_encoder_impl.cpp:52).
  {
    const unsigned nsys = (kb - 2) * d.lifting_size;
    unsigned       fs = std::min(nsys - d.nof_filler_bits, d.n_cb), fe = std::min(nsys, d.n_cb);
    const unsigned flen = fe - fs, n_valid = d.n_cb - flen;
    const unsigned rank0 = d.k0 < fs ? d.k0 : (d.k0 < fe ? fs : d.k0 - flen);
    unsigned       last; // highest circular-buffer position read
    if (rank0 + d.rm_length_long > n_valid) {
      last = d.n_cb - 1;
    } else {
      unsigned u = rank0 + d.rm_length_long - 1;
      last       = u < fs ? u : u + flen;
    }
    const unsigned nodes = divide_ceil(last + 1 + 2 * d.lifting_size, d.lifting_size);
    pd.nof_rows          = std::max(4U, nodes > kb ? nodes - kb : 0U);
  }
  // Precoding weights: data weights carry the modulation and power scaling (pdsch_modulator_impl.cpp:98-102).
  {
    const float avg     = (pdu.qm == 2) ? 2.0F : (pdu.qm == 4) ? 10.0F : (pdu.qm == 6) ? 42.0F : 170.0F;
    float       scaling = std::sqrt(1 / avg);
    const float cfg     = std::pow(10.0F, -pdu.ratio_pdsch_data_to_sss_dB / 20.0F);
    if (std::isnormal(cfg)) {
      scaling *= cfg;
    }
    const unsigned nw      = 2 * pdu.nof_prg * pdu.nof_ports * pdu.nof_layers;
    pd.weights_offset      = (uint32_t)t.weights.size();
    for (unsigned k = 0; k != nw; ++k) {
      t.weights.push_back(pdu.precoding ? pdu.precoding[k] * scaling : 0.0F); // no weights in an encode-only plan
    }
    pd.dmrs_weights_offset = (uint32_t)t.weights.size();
    for (unsigned k = 0; k != nw; ++k) {
      t.weights.push_back(pdu.precoding ? pdu.precoding[k] : 0.0F);
    }
    pd.nof_prg       = pdu.nof_prg;
    pd.prg_size_subc = pdu.prg_size_rb * 12;
  }
  // DM-RS (dmrs_pdsch_processor_impl.cpp:84-106).
  pd.dmrs_symbol_mask = pdu.dmrs_symbol_mask;
  pd.dmrs_zero_other_group = (pdu.nof_cdm_groups_without_data == 2 && (pdu.nof_layers + 1) / 2 == 1) ? 1U : 0U;
  pd.dmrs_ref_rb      = (pdu.ref_point == 1) ? pdu.bwp_start_rb : 0;
  {
    const float amp   = std::pow(10.0F, -pdu.ratio_pdsch_dmrs_to_sss_dB / 20.0F);
    pd.dmrs_amplitude = (float)(M_SQRT1_2 * (double)amp);
  }
  for (unsigned l = 0; l != NRPHY_NSYMB; ++l) {
    // 14 symbols per slot also with extended cyclic prefix: the reference takes get_nsymb_per_slot(NORMAL) here
    // (dmrs_pdsch_processor_impl.cpp:95), and a drop-in has to produce the same pilots.
    const uint64_t a  = (uint64_t)(14 * pdu.slot_index + l + 1) * (2 * pdu.scrambling_id + 1);
    pd.dmrs_c_init[l] = (uint32_t)(((a << 17) + (2 * pdu.scrambling_id + (pdu.n_scid ? 1 : 0))) & 0x7FFFFFFFULL);
    if ((pdu.dmrs_symbol_mask >> l) & 1U) {
      const uint32_t first = (uint32_t)mask_lowest(pdu.prb_mask), end = (uint32_t)mask_highest(pdu.prb_mask) + 1;
      for (uint32_t b = first; b < end; b += DMRS_PRB_CHUNK) {
        t.dmrs.push_back({i, l, b, std::min<uint32_t>(end, b + DMRS_PRB_CHUNK)});
      }
    }
  }
  for (unsigned w = 0; w != NRPHY_PRB_WORDS; ++w) {
    pd.prb_mask[2 * w]     = (uint32_t)pdu.prb_mask[w];
    pd.prb_mask[2 * w + 1] = (uint32_t)(pdu.prb_mask[w] >> 32);
  }
  pd.first_prb = (uint32_t)mask_lowest(pdu.prb_mask);
  pd.end_prb   = (uint32_t)mask_highest(pdu.prb_mask) + 1;
  if (pdu.nof_cdm_groups_without_data < (pdu.nof_layers + 1) / 2) {
    plan.dmrs_separate = true; // data is mapped on RE that also carry DM-RS: the reference lets DM-RS win
  }
  pdus_of_grid[pd.grid_index].push_back(i);
  // Scrambling sequence of the PDU: one word per 32 codeword bits plus the word a misaligned read runs into, plus the
  // length of a seed (the last work item's 31 words may reach beyond the codeword; the sequence simply goes on).  Stored
  // are these words or only the work items' seeds, one form per plan (behind the DM-RS sequences, choose_scrambling_form).
  pd.scr_words = (d.codeword_bits + 31U) / 32U + 1U + 31U;
  // One DM-RS sequence per DM-RS symbol.
  pd.dmrs_seq_words = (12U * (pd.end_prb - pd.dmrs_ref_rb) + 31U) / 32U + 1U;
}

// Work items of PDU i: every codeblock owns a whole number of RE (rm_length is a multiple of nof_layers * Qm).  Appends to
// work and raises the plan's LDS sizes; reads the derived sizes, the descriptor and the PDU's lifted graph.  Returns the
// number of items.
uint32_t PlanBuilder::add_codeblock_work(uint32_t i, const nrphy_pdsch_derived_t& d, const PduDev& pd)
{
  const unsigned lq = pd.nof_layers * pd.qm;
  const size_t   work_before = t.work.size();
  for (unsigned cb = 0; cb != d.nof_codeblocks; ++cb) {
    const unsigned nre = ((cb < d.nof_short_segments) ? d.rm_length_short : d.rm_length_long) / lq;
    for (unsigned begin = 0; begin < nre; begin += RE_CHUNK) {
      const unsigned count = std::min<unsigned>(RE_CHUNK, nre - begin);
      t.work.push_back({i, cb, begin, count});
      {
        // The wave expands its scrambling words from a 31-word seed into the LDS that held the codeblock: room for them
        // (the chunk's words from the one its first bit lies in, plus the word a misaligned read runs into).
        const uint64_t bit0 = (uint64_t)(cb < d.nof_short_segments ? cb * d.rm_length_short
                                                                   : d.nof_short_segments * d.rm_length_short +
                                                                         (cb - d.nof_short_segments) * d.rm_length_long) +
                              (uint64_t)begin * lq;
        const uint32_t need = std::max<uint32_t>(31U, (uint32_t)(((bit0 & 31U) + (uint64_t)count * lq + 31U) / 32U) + 1U);
        plan.lds_lin_words = std::max<uint32_t>(plan.lds_lin_words, (need + 3U) & ~3U);
      }
      // LDS the wave needs for the symbol bytes (32 per block + 8 words).
      plan.lds_symb_words = std::max<uint32_t>(plan.lds_symb_words, (((count * pd.nof_layers + 31) / 32) * 8 + 8 + 3) & ~3U);
    }
  }
  plan.lds_lin_words = std::max<uint32_t>(plan.lds_lin_words, ((((pd.kb + pd.nof_rows) * d.lifting_size + 31) / 32) + 2 + 3) & ~3U);
  plan.lds_graph_words = std::max<uint32_t>(
      plan.lds_graph_words, (48U + graphs[pd.graph].row_ptr[std::min<uint32_t>(pd.nof_rows, MAX_BG_ROWS)] + 3U) & ~3U);
  return (uint32_t)(t.work.size() - work_before);
}

// Sequence work: a workgroup per distinct scrambling sequence -- the first PDU that asks for it walks it -- with that
// PDU's DM-RS sequences on its spare waves if they are new too; a PDU that shares its scrambling sequence and has DM-RS
// sequences of its own (another slot of the same UE) gets a workgroup that generates those alone.  Appends to scr_work;
// reads the descriptors and what SequenceSharing found fresh.
void PlanBuilder::add_sequence_work()
{
  // A plan with many sequences fills the device with one workgroup each (seeding a generator is the costly part:
  // measured 0.111 / 0.098 / 0.096 ms per 1024 distinct config-3 sequences with 4 / 2 / 1 parts); one with few is split
  // for latency.
  // (A/B and test knob: parts of a sequence in a plan of many)
  const uint32_t parts_big = tune.scr_parts_big > 0 ? (uint32_t)std::min((int)SCR_PARTS, tune.scr_parts_big) : 1U;
  const uint32_t parts_max = seqs.n_scr_seq >= 128 ? parts_big : SCR_PARTS;
  for (uint32_t i = 0; i != n_pdu; ++i) {
    const PduDev&  pd       = plan.pdus[i];
    const uint32_t own_dmrs = (seqs.fresh[i] & SEQ_NEW_DMRS) ? 1U : 0U;
    if (seqs.fresh[i] & SEQ_NEW_SCR) {
      const uint32_t parts = std::min<uint32_t>(parts_max, std::max<uint32_t>(1, pd.scr_words >> 11));
      const uint32_t chunk = divide_ceil(pd.scr_words, parts);
      for (uint32_t first = 0, k = 0; first < pd.scr_words; first += chunk, ++k) {
        t.scr_work.push_back({i, first, std::min(chunk, pd.scr_words - first), k == 0 ? own_dmrs : 0U});
      }
    } else if (own_dmrs) {
      t.scr_work.push_back({i, 0U, 0U, 1U});
    }
  }
}

// TB-CRC work: the transport block in 16 KiB regions, a workgroup per run of regions.  A small batch gets a workgroup
// per region (latency); a big one has workgroups enough and lets each walk several regions, the next one's words in
// flight while it reduces the current one (a workgroup per region spent two thirds of its time waiting for its loads:
// profiles/r03_prologue_trace.txt).  Appends to crc_work and writes crc_first / crc_count of every descriptor;
// NRPHY_ERR_INVALID_PDU for a transport block of more shares than a wave has lanes.
int PlanBuilder::add_tb_crc_work()
{
  for (uint32_t i = 0; i != n_pdu; ++i) {
    PduDev&         pd = plan.pdus[i];
    const CrcField& f  = (pd.tb_crc_bits == 16) ? CRC16_FIELD : CRC24A_FIELD;
    const uint32_t  n  = pd.tb_bytes;
    const uint32_t  regions = divide_ceil(n, TB_CRC_REGION_BYTES);
    const uint32_t  want  = std::max<uint32_t>(1, std::min<uint32_t>(regions, TB_CRC_TARGET_WORK / std::max<uint32_t>(1, n_pdu)));
    uint32_t        per   = std::min<uint32_t>(TB_CRC_MAX_REGIONS_PER_WORK, divide_ceil(regions, want));
    if (tune.crc_regions > 0) { // (A/B and test knob: regions per workgroup)
      per = std::max(1, std::min((int)TB_CRC_MAX_REGIONS_PER_WORK, tune.crc_regions));
    }
    pd.crc_first      = (uint32_t)t.crc_work.size();
    pd.crc_count      = divide_ceil(regions, per);
    if (pd.crc_count > 64) { // one lane of the attaching wave per share
      return NRPHY_ERR_INVALID_PDU;
    }
    for (uint32_t region = 0; region < regions; region += per) {
      const uint32_t count      = std::min(per, regions - region);
      const int64_t  region_end = (int64_t)(region + count) * TB_CRC_REGION_BYTES;
      t.crc_work.push_back({i, region, f.xpow((int64_t)f.order + 8 * ((int64_t)n - region_end)), count});
    }
  }
  return NRPHY_OK;
}

// Coverage of one (grid, port): the runs of subcarriers that no PDU on it maps (data or DM-RS), symbol by symbol, into `key`
// as (symbol << 32 | first << 16 | length).  Reads the PDUs of the grid; mask and cov are scratch.
void PlanBuilder::cover(uint32_t g, uint32_t port)
{
  const unsigned nof_subc = grid_nof_subc; // (a local: the loops below store bytes, and a member would be read again after every store)
  cov.assign((size_t)NRPHY_NSYMB * nof_subc, 0);
  for (uint32_t i : pdus_of_grid[g]) {
    const nrphy_pdsch_pdu_t& pdu = pdus[i];
    if (port >= pdu.nof_ports) {
      continue;
    }
    for (unsigned l = 0; l != NRPHY_NSYMB; ++l) {
      uint8_t* row = &cov[(size_t)l * nof_subc];
      uint8_t* m = mask.data();
      data_re_mask(pdu, l, m, nof_subc);
      for (unsigned k = 0; k != nof_subc; ++k) {
        row[k] |= m[k];
      }
      if ((pdu.dmrs_symbol_mask >> l) & 1U) {
        // RE of a CDM group that is reserved (no data) but carries no pilots of this PDU are zeroed by the
        // DM-RS waves themselves (dmrs_zero_other_group): as zero-fill work they would be 1-RE segments.
        const unsigned groups = (pdu.nof_cdm_groups_without_data == 2) ? 2 : (pdu.nof_layers + 1) / 2;
        for (unsigned prb = 0; 12 * prb < nof_subc; ++prb) {
          if (mask_test(pdu.prb_mask, prb)) {
            for (unsigned k = 0; k != 12; ++k) {
              row[12 * prb + k] |= (k % 2) < groups;
            }
          }
        }
      }
    }
  }
  key.clear();
  for (unsigned l = 0; l != NRPHY_NSYMB; ++l) {
    const uint8_t* row = &cov[(size_t)l * nof_subc];
    unsigned       k   = 0;
    while (k < nof_subc) {
      if (row[k]) {
        ++k;
        continue;
      }
      unsigned k0 = k;
      while (k < nof_subc && !row[k]) {
        ++k;
      }
      key.push_back(((uint64_t)l << 32) | ((uint64_t)k0 << 16) | (k - k0));
    }
  }
}

// The run list of a (grid, port) whose allocations (`sig`) this plan meets for the first time: from an earlier plan of the
// caller (the shape cache), a copy of an identical list of this plan (seen), or new.  Appends to zero_segs, seen and the
// shape cache.
PlanBuilder::Runs PlanBuilder::zero_runs(uint32_t g, uint32_t port)
{
  if (shapes != nullptr) {
    // The key of this coverage in the caller's cache (the grid size is part of it).
    shape_key = sig;
    shape_key.push_back(((uint64_t)grid_nof_subc << 32) | port);
    auto kept = shapes->zero.find(shape_key);
    if (kept != shapes->zero.end()) {
      const Runs where = {(uint32_t)t.zero_segs.size(), (uint32_t)kept->second.segs.size(), kept->second.nof_long};
      t.zero_segs.insert(t.zero_segs.end(), kept->second.segs.begin(), kept->second.segs.end());
      return where;
    }
  }
  cover(g, port);
  Runs runs = {0, 0, 0};
  if (!key.empty()) {
    auto it = seen.find(key);
    if (it == seen.end()) {
      // Long runs first (the wave clears each one together), then the short ones (one lane per run).
      const uint32_t begin = (uint32_t)t.zero_segs.size();
      uint32_t       nof_long = 0;
      for (int pass = 0; pass != 2; ++pass) {
        for (uint64_t v : key) {
          const bool is_long = (v & 0xFFFF) >= ZERO_LONG_RUN;
          if (is_long == (pass == 0)) {
            t.zero_segs.push_back({(uint16_t)(v >> 32), (uint16_t)((v >> 16) & 0xFFFF), (uint16_t)(v & 0xFFFF), 0});
            nof_long += is_long ? 1U : 0U;
          }
        }
      }
      it = seen.insert({key, {begin, (uint32_t)key.size(), nof_long}}).first;
    }
    runs = it->second;
  }
  if (shapes != nullptr) {
    PlanShapeCache::Zero z;
    z.segs.assign(t.zero_segs.begin() + runs[0], t.zero_segs.begin() + runs[0] + runs[1]);
    z.nof_long = runs[2];
    shapes->zero.insert({shape_key, std::move(z)});
  }
  return runs;
}

// Zero-fill work: per (grid, port) the runs of subcarriers no PDU maps (data or DM-RS).  Appends to zero_work (and, through
// zero_runs, to zero_segs); reads the PDUs of every grid.
void PlanBuilder::build_zero_fill()
{
  for (uint32_t g = 0; g != (enc ? 0U : nof_grids); ++g) { // an encode-only plan writes no grid
    for (uint32_t port = 0; port != grid_nof_ports; ++port) {
      // Everything the coverage of this (grid, port) depends on: grids that repeat an allocation (the normal case
      // in a batch of slots) reuse its segment list without rebuilding the RE masks.
      sig.clear();
      for (uint32_t i : pdus_of_grid[g]) {
        if (port < pdus[i].nof_ports) {
          append_allocation_signature(pdus[i], sig);
        }
      }
      auto known = by_signature.find(sig);
      if (known == by_signature.end()) {
        known = by_signature.insert({sig, zero_runs(g, port)}).first;
      }
      const Runs& runs = known->second;
      if (runs[1] != 0) {
        t.zero_work.push_back({g, port, runs[0], runs[1], runs[2]});
      }
    }
  }
}

// One bucket per (modulation order, layers), PDU and codeblock order kept inside (launch_codeblocks).  Sorts work; writes
// bucket_begin and item_first of every descriptor.
void PlanBuilder::sort_into_buckets()
{
  const auto bucket_of = [&](const CbWork& w) { return cb_bucket(plan.pdus[w.pdu].qm, plan.pdus[w.pdu].nof_layers); };
  std::stable_sort(t.work.begin(), t.work.end(), [&](const CbWork& a, const CbWork& b) { return bucket_of(a) < bucket_of(b); });
  for (const CbWork& w : t.work) {
    ++plan.bucket_begin[bucket_of(w) + 1];
  }
  for (uint32_t b = 0; b != CB_BUCKETS; ++b) {
    plan.bucket_begin[b + 1] += plan.bucket_begin[b];
  }
  // A PDU's work items stay together and in order (one bucket per PDU, stable sort): where they start.
  for (size_t k = t.work.size(); k-- != 0;) {
    plan.pdus[t.work[k].pdu].item_first = (uint32_t)k;
  }
}

// The distinct scrambling sequences behind the DM-RS sequences: their words while those stay within the budget, else their
// seeds, 32 words per work item.  One form per plan, so that a launch has one.  The sharing key is the same in both forms
// (the words alone would need only c_init).  (A/B and test knob: NRPHY_SCR_WORDS = 0 always seeds, 1 always words.)
// Writes scr_as_words, seed_offset and scr_words of the plan; reads SequenceSharing's totals and the size of crc_work.
void PlanBuilder::choose_scrambling_form(size_t scratch_capacity_words)
{
  const uint64_t words_offset = (seqs.dmrs_words + 15U) & ~15ULL; // the words start a 64-byte line
  plan.scr_as_words = seqs.words_fit && (tune.scr_words < 0 ? seqs.words_sum * 4U <= SCR_WORDS_BUDGET_BYTES : tune.scr_words != 0);
  if (plan.scr_as_words && scratch_capacity_words != 0 &&
      words_offset + seqs.words + std::max<size_t>(4, t.crc_work.size()) > scratch_capacity_words) {
    plan.scr_as_words = false; // caller-owned scratch sized for seeds
  }
  plan.seed_offset = plan.scr_as_words ? words_offset : (seqs.dmrs_words + 3U) & ~3ULL;
  plan.scr_words   = plan.seed_offset + (plan.scr_as_words ? seqs.words : 32ULL * seqs.seed_slots);
}

int PlanBuilder::build(size_t scratch_capacity_words)
{
  if (shapes != nullptr && shapes->remap.size() + shapes->zero.size() > PlanShapeCache::MAX_ENTRIES) {
    shapes->remap.clear();
    shapes->zero.clear();
  }
  plan.nof_grids      = nof_grids;
  plan.grid_nof_ports = grid_nof_ports;
  plan.grid_nof_subc  = grid_nof_subc;
  plan.encode_only    = enc != nullptr;
  for (uint32_t i = 0; i != n_pdu; ++i) {
    const int status = check_pdu(i);
    if (status != NRPHY_OK) {
      return status;
    }
    PduDev pd;
    std::memset(&pd, 0, sizeof(pd));
    // RE mapping tables (shared by the PDUs of the batch that repeat this allocation).
    const unsigned nof_re = map_resource_elements(i, pd);
    if (nof_re == 0) {
      return NRPHY_ERR_INVALID_PDU;
    }
    nrphy_pdsch_derived_t d;
    derive(pdus[i], nof_re, d, enc ? &enc[i].nref : nullptr);
    if (d.lifting_size == 0 || d.nof_codeblocks > NRPHY_MAX_CODEBLOCKS || d.nof_codeblocks > nof_re || d.rm_length_short == 0) {
      return NRPHY_ERR_INVALID_PDU;
    }
    describe_pdu(i, d, pd);
    const uint32_t                nof_items = add_codeblock_work(i, d, pd);
    const SequenceSharing::Shared shared    = seqs.add_pdu(pd, nof_items, n_pdu == 1);
    pd.seed_first      = shared.at.seed_first;
    pd.scr_word_offset = shared.at.scr_word_offset;
    pd.dmrs_seq_offset = shared.at.dmrs_seq_offset;
    plan.n_cb += d.nof_codeblocks;
    plan.cw_offset.push_back(cw_bits);
    cw_bits += (d.codeword_bits + 31U) & ~31ULL;
    plan.pdus.push_back(pd);
  }
  add_sequence_work();
  const int status = add_tb_crc_work();
  if (status != NRPHY_OK) {
    return status;
  }
  build_zero_fill();
  sort_into_buckets();
  choose_scrambling_form(scratch_capacity_words);
  // The codeblock waves load 2 * NRPHY_MAX_PORTS * layers weights whatever the port count (re_map_device.h, phase_b).
  t.weights.insert(t.weights.end(), 2 * NRPHY_MAX_PORTS * NRPHY_MAX_PORTS, 0.0F);
  plan.cw_bits     = cw_bits;
  plan.n_work      = (uint32_t)t.work.size();
  plan.n_dmrs      = (uint32_t)t.dmrs.size();
  plan.n_crc_work  = (uint32_t)t.crc_work.size();
  plan.n_scr_work  = (uint32_t)t.scr_work.size();
  plan.n_zero_work = (uint32_t)t.zero_work.size();
  plan.n_scr_seq   = seqs.n_scr_seq;
  plan.n_dmrs_seq  = seqs.n_dmrs_seq;
  // The dynamic LDS of the codeblock launch also serves the DM-RS waves it may carry.
  plan.lds_lin_words = std::max<uint32_t>(plan.lds_lin_words, 64);
  // The scratch region the stages of a codeblock wave share (codeblock_build_device.h, CbShared): doubled systematic blocks + graph
  // rows, then modulation table + symbol bytes.
  plan.lds_u_words = std::max<uint32_t>(NRPHY_CB_U_GRAPH_OFFSET + plan.lds_graph_words, 512U + plan.lds_symb_words);
  return NRPHY_OK;
}

} // namespace

int pdsch_plan_build(const LiftedGraph* graphs, const Tunables& tune, uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus,
                     const uint64_t* tb_offset, const uint32_t* grid_index, uint32_t nof_grids, uint32_t grid_nof_ports,
                     uint32_t grid_nof_subc, const EncodeOnly* enc, PlanShapeCache* shapes, size_t scratch_capacity_words,
                     nrphy_pdsch_plan& plan, PlanTables& tables)
{
  if ((n_pdu != 0 && (pdus == nullptr || tb_offset == nullptr)) || grid_nof_ports == 0 || grid_nof_ports > NRPHY_MAX_PORTS ||
      grid_nof_subc == 0 || grid_nof_subc % 12 != 0 || grid_nof_subc > NRPHY_MAX_RB * 12) {
    return NRPHY_ERR_ARGUMENT;
  }
  return PlanBuilder(graphs, tune, n_pdu, pdus, tb_offset, grid_index, nof_grids, grid_nof_ports, grid_nof_subc, enc, shapes, plan, tables)
      .build(scratch_capacity_words);
}
