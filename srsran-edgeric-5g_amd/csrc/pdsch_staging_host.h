// PDSCH plans in memory the caller owns, and the one way the asynchronous seams (pdsch_async.cpp, dl_slot_async.cpp) stage a
// call there: transport blocks back to back in a pinned region, the plan's tables behind them, one copy for both.  Needs the
// public header alone (the layout part is host arithmetic that tests/pdsch_staging_check.cpp compiles by itself).  Not part of
// the ABI.
#pragma once

#include "mi355_nrphy.h"

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// ---- PDSCH plans in caller-owned memory (the asynchronous queue) ----------------------------------------------------------
// nrphy_pdsch_plan_create allocates device memory and copies the plan's tables there with a blocking copy: right for a
// plan that is built once and run many times, wrong on a path that sees a new PDU per call.  The placed form writes the
// tables into host memory of the caller (pinned staging it copies in stream order, together with the transport block)
// and points the plan at the device addresses they will have; it makes no HIP call.  NRPHY_ERR_CAPACITY when the plan
// does not fit.  The plan must be destroyed before the memory is reused.
struct PlanShapeCache;
PlanShapeCache* plan_shape_cache_create();
void            plan_shape_cache_destroy(PlanShapeCache* cache);
struct PlanPlacement {
  uint8_t*        h_tables = nullptr; // host memory the tables are written to
  uint8_t*        d_tables = nullptr; // device address they will be copied to (256-byte aligned)
  size_t          table_capacity = 0;
  size_t          table_bytes    = 0; // out: bytes to copy
  uint32_t*       d_scratch = nullptr; // device memory for what every run rewrites (sequences, TB-CRC shares)
  size_t          scratch_capacity_words = 0;
  PlanShapeCache* cache = nullptr;    // may be null; one cache per thread of use
};
int nrphy_pdsch_plan_create_placed(nrphy_ctx_t* ctx, uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus, const uint64_t* tb_offset,
                                   const uint32_t* grid_index, uint32_t nof_grids, uint32_t grid_nof_ports,
                                   uint32_t grid_nof_subc, PlanPlacement* place, nrphy_pdsch_plan_t** out);

#pragma GCC visibility push(hidden)

// ---- Sizes of a seam's buffers --------------------------------------------------------------------------------------------
// Room for the tables of one operation (PDU descriptors, work lists, weights, RE tables, zero-fill lists: a few KB for a
// wideband PDU; non-contiguous allocations add two bytes per RE) ...
inline size_t pdsch_staging_table_capacity(uint32_t grid_nof_subc)
{
  return ((size_t)64 * 1024 + (size_t)NRPHY_NSYMB * grid_nof_subc * 6 + 255) & ~(size_t)255;
}
// ... and for what the runs on one grid rewrite (one sequence word per 32 codeword bits -- at most 32 bits per RE -- plus
// DM-RS sequences).
inline size_t pdsch_staging_scratch_words(uint32_t grid_nof_subc)
{
  return (size_t)NRPHY_NSYMB * grid_nof_subc * 2 + 16384;
}

// ---- Layout part: no HIP call, no plan ------------------------------------------------------------------------------------
// The transport blocks of a call back to back from the start of its region, each readable to the next multiple of 4; the
// plan's tables follow them on a 256-byte boundary.
struct PdschStagingLayout {
  std::vector<uint64_t> tb_off;       // per PDU, relative to the region (what the plan records)
  size_t                tb_total  = 0; // end of the last block's readable extent
  size_t                tables_at = 0; // first multiple of 256 at or after tb_total
};

// NRPHY_ERR_ARGUMENT for a missing or empty block, before anything is written anywhere.
inline int pdsch_staging_layout(uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus, const uint8_t* const* tbs, PdschStagingLayout& l)
{
  l.tb_off.resize(n_pdu);
  l.tb_total = 0;
  for (uint32_t i = 0; i != n_pdu; ++i) {
    if (tbs[i] == nullptr || pdus[i].tb_size_bytes == 0) {
      return NRPHY_ERR_ARGUMENT;
    }
    l.tb_off[i] = l.tb_total;
    l.tb_total += ((size_t)pdus[i].tb_size_bytes + 7) & ~(size_t)3;
  }
  l.tables_at = (l.tb_total + 255) & ~(size_t)255;
  return NRPHY_OK;
}

// The blocks into the region at `h_base`, each zero-padded to the start of the next (the last one to tb_total).
inline void pdsch_staging_copy_blocks(const PdschStagingLayout& l, uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus,
                                      const uint8_t* const* tbs, uint8_t* h_base)
{
  for (uint32_t i = 0; i != n_pdu; ++i) {
    const size_t span = (i + 1 != n_pdu ? l.tb_off[i + 1] : l.tb_total) - l.tb_off[i];
    std::memcpy(h_base + l.tb_off[i], tbs[i], pdus[i].tb_size_bytes);
    std::memset(h_base + l.tb_off[i] + pdus[i].tb_size_bytes, 0, span - pdus[i].tb_size_bytes); // readable to the next multiple of 4
  }
}

// ---- The plan of a laid-out call ------------------------------------------------------------------------------------------
struct PdschStagedPlan {
  nrphy_pdsch_plan_t* plan        = nullptr;
  size_t              table_bytes = 0;     // of a placed plan: what lies at tables_at
  bool                own_memory  = false; // the tables did not fit: the plan has device memory of its own
  // What one H2D copy from the region's start has to carry: blocks and tables, or the blocks alone.
  size_t copy_bytes(const PdschStagingLayout& l) const { return own_memory ? l.tb_total : l.tables_at + table_bytes; }
};

// Builds the plan of the call (all PDUs into one grid) with its tables behind the blocks of the region [h_base, h_base +
// capacity), whose device twin is at d_base, then copies the blocks in.  Tables too big for what the region has left: a plan
// with device memory of its own (an allocation and a blocking copy; rare: hundreds of PDUs, or RE tables for most of a
// fragmented grid).  The offsets the plan records are relative to the pointer nrphy_pdsch_run gets: d_base or h_base.
// Nothing is written when the plan cannot be built.  The caller has checked that the blocks fit (capacity >= tables_at).
inline int pdsch_staging_create_plan(nrphy_ctx_t* ctx, uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus, const uint8_t* const* tbs,
                                     uint32_t grid_nof_ports, uint32_t grid_nof_subc, const PdschStagingLayout& l, uint8_t* h_base,
                                     uint8_t* d_base, size_t capacity, uint32_t* d_scratch, size_t scratch_words,
                                     PlanShapeCache* cache, PdschStagedPlan& out)
{
  std::vector<uint32_t> grid_of(n_pdu, 0);
  PlanPlacement         place;
  place.h_tables               = h_base + l.tables_at;
  place.d_tables               = d_base + l.tables_at;
  place.table_capacity         = (capacity - l.tables_at) & ~(size_t)255;
  place.d_scratch              = d_scratch;
  place.scratch_capacity_words = scratch_words;
  place.cache                  = cache;
  out = PdschStagedPlan();
  int rc = nrphy_pdsch_plan_create_placed(ctx, n_pdu, pdus, l.tb_off.data(), grid_of.data(), 1, grid_nof_ports, grid_nof_subc, &place,
                                          &out.plan);
  if (rc == NRPHY_ERR_CAPACITY) {
    rc             = nrphy_pdsch_plan_create(ctx, n_pdu, pdus, l.tb_off.data(), grid_of.data(), 1, grid_nof_ports, grid_nof_subc, &out.plan);
    out.own_memory = true;
  }
  if (rc != NRPHY_OK) {
    return rc;
  }
  out.table_bytes = place.table_bytes;
  pdsch_staging_copy_blocks(l, n_pdu, pdus, tbs, h_base);
  return NRPHY_OK;
}

#pragma GCC visibility pop
