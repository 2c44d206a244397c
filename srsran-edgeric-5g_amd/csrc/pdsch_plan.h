// The PDSCH plan between its two translation units: pdsch_plan_build.cpp says what a plan is (pure host arithmetic, no device),
// pdsch_host.cpp where its tables live and how it is launched.  Not part of the ABI.
#pragma once

#include "nrphy_host_internal.h"
#include "pdsch_staging_host.h"

#include <map>
#include <vector>

struct nrphy_pdsch_plan {
  nrphy_ctx*            ctx = nullptr;
  std::vector<PduDev>   pdus;
  std::vector<uint64_t> cw_offset;
  uint64_t              cw_bits = 0;
  uint32_t              nof_grids = 0, grid_nof_ports = 0, grid_nof_subc = 0;
  void*                 d_arena = nullptr; // the one device allocation every d_* pointer below points into
  bool                  arena_external = false; // the tables live in memory the caller owns (nrphy_pdsch_plan_create_placed)
  PduDev*               d_pdus = nullptr;
  CbWork*               d_work = nullptr;
  DmrsWork*             d_dmrs = nullptr;
  float*                d_weights = nullptr;
  uint16_t*             d_re_table = nullptr;
  uint32_t*             d_tb_crc = nullptr;
  CrcWork*              d_crc_work = nullptr;
  ScrWork*              d_scr_work = nullptr;
  uint32_t              n_scr_work = 0;
  uint32_t              n_scr_seq = 0, n_dmrs_seq = 0; // distinct scrambling sequences / DM-RS sequence sets a run generates
  ZeroWork*             d_zero_work = nullptr;
  ZeroSeg*              d_zero_segs = nullptr;
  uint32_t*             d_scr = nullptr;    // scrambling sequences, rewritten by every run's prologue
  uint64_t              scr_words = 0;   // words of the run's scratch: the distinct DM-RS sequences, then the distinct scrambling sequences (seeds or words)
  uint64_t              seed_offset = 0; // where the scrambling sequences start
  bool                  scr_as_words = false; // the form of the scrambling sequences: words (true) or seeds (PdschLaunch::scr_as_words)
  uint32_t              n_zero_work = 0;
  bool                  encode_only = false;   // seam B plan: no RE mapping, nrphy_pdsch_run only with d_grid = NULL
  bool                  dmrs_separate = false; // DM-RS must overwrite data RE: keep it in its own, later launch
  uint32_t              n_work = 0, n_dmrs = 0, n_cb = 0, n_crc_work = 0;
  uint32_t              lds_lin_words = 0, lds_symb_words = 0, lds_graph_words = 0, lds_u_words = 0;
  uint32_t              bucket_begin[CB_BUCKETS + 1] = {}; // work items sorted by (modulation order, layers)
  // A batch with several big buckets runs their launches side by side on streams of the plan's own (created at the first
  // such run), forked from and joined to the caller's stream with events.
  static constexpr uint32_t MAX_AUX = 3;
  hipStream_t           aux_stream[MAX_AUX] = {};
  hipEvent_t            fork_event = nullptr, join_event[MAX_AUX] = {};
  uint32_t              n_aux = 0;
  std::vector<hipEvent_t> events; // 4 per recorded run: start, after tb_crc, after codeblocks, after dmrs (only when a DM-RS launch follows)
  std::vector<uint8_t>  timed_dmrs; // per recorded run: its fourth event was recorded
  uint32_t              timed_runs = 0, max_timed_runs = 0;
  uint32_t              timing_stride = 1, timing_counter = 0; // every timing_stride-th run is recorded
};

struct ReMapping {
  uint32_t sym_re_start[NRPHY_NSYMB + 1];
  uint32_t sym_kind[NRPHY_NSYMB];
  uint32_t sym_arg[NRPHY_NSYMB];
};

// What a plan derives from the SHAPE of its PDUs alone -- allocation, symbols, DM-RS and reserved patterns, ports and
// layers -- kept across plans by a caller that builds one plan per PDU (the asynchronous queue): RE mapping tables and
// zero-fill run lists.  Everything else in a plan (slot index, RNTI, scrambling identities, transport-block size and
// the sizes derived from it, weights) is per PDU and rebuilt every time; it costs a few microseconds.
struct PlanShapeCache {
  struct Remap {
    ReMapping             m;     // sym_arg of SYM_TABLE symbols relative to `table`
    std::vector<uint16_t> table;
  };
  struct Zero {
    std::vector<ZeroSeg> segs; // long runs first
    uint32_t             nof_long = 0;
  };
  std::map<std::vector<uint64_t>, Remap> remap;
  std::map<std::vector<uint64_t>, Zero>  zero; // key: grid size + port + the allocation signatures of the PDUs on the port
  static constexpr size_t MAX_ENTRIES = 256;   // shapes in use at a time are few; a full cache starts over
};

// Seam B (encode + rate match + interleave only): the codeword size and N_ref are given, there is no allocation.
struct EncodeOnly {
  uint32_t nof_re; // channel symbols per layer
  uint32_t nref;
};

// The host vectors behind a plan's device tables (with nrphy_pdsch_plan::pdus): what pdsch_host.cpp uploads or places.
struct PlanTables {
  std::vector<CbWork>   work;
  std::vector<DmrsWork> dmrs;
  std::vector<CrcWork>  crc_work;
  std::vector<ScrWork>  scr_work;
  std::vector<float>    weights;
  std::vector<uint16_t> re_table;
  std::vector<ZeroWork> zero_work;
  std::vector<ZeroSeg>  zero_segs;
};

// Sizes derived from a PDU and its count of data RE (nrphy_pdsch_derive without the RE count).  nref_override: the
// limited-buffer size given directly (seam B hands N_ref, not TBS_LBRM); nullptr = from the PDU.
void derive(const nrphy_pdsch_pdu_t& pdu, unsigned nof_re, nrphy_pdsch_derived_t& d, const uint32_t* nref_override = nullptr);

// The builder: the host fields of `plan` (everything but ctx and the device pointers, streams and events) and `tables` from a
// batch of PDUs.  Pure host arithmetic, no device: `graphs` is the context's host copy of the lifted graphs (NOF_GRAPHS of
// them).  enc: null, or one entry per PDU for an encode-only plan.  shapes: the caller's shape cache, may be null.
// scratch_capacity_words: of a placed plan, the caller's scratch -- only the choice of the scrambling form reads it; 0 = unlimited.
// Returns NRPHY_OK, NRPHY_ERR_ARGUMENT or NRPHY_ERR_INVALID_PDU; the plan stays the caller's either way.
int pdsch_plan_build(const LiftedGraph* graphs, const Tunables& tune, uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus,
                     const uint64_t* tb_offset, const uint32_t* grid_index, uint32_t nof_grids, uint32_t grid_nof_ports,
                     uint32_t grid_nof_subc, const EncodeOnly* enc, PlanShapeCache* shapes, size_t scratch_capacity_words,
                     nrphy_pdsch_plan& plan, PlanTables& tables);
