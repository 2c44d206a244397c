/*
 * mi355_nrphy.h -- C ABI of the MI355X-native 5G NR downlink PHY hot path.
 *
 * This is the drop-in boundary for the PDSCH processor + OFDM modulator of the reference
 * (ushasigh/srsran-edgeric-5g, srsRAN-5G-ER/lib/phy).  Every entry point names the reference
 * interface it replaces (R/ = srsRAN-5G-ER/).  Plain C: POD structs, raw pointers and sizes, int
 * status codes, no exceptions, no C++ or torch types.
 *
 * Conventions
 *  - Bit buffers are MSB-first packed bytes (bit i lives in byte i/8, mask 0x80 >> (i%8)), the layout
 *    of the reference's bit_buffer (R/include/srsran/adt/bit_buffer.h:98-190).
 *  - A resource grid is an array [port][symbol(14)][subcarrier] of cbf16 (two bf16, real then
 *    imaginary, 4 bytes), subcarrier fastest -- the layout of resource_grid_impl
 *    (R/lib/phy/support/resource_grid_impl.cpp:29-57).  Batches add a leading [grid] dimension.
 *  - IQ output is complex float32 (real, imag), [grid][port][sample] with the slot's symbols back
 *    to back (cyclic prefix first), as ofdm_slot_modulator produces it
 *    (R/lib/phy/lower/modulation/ofdm_modulator_impl.cpp:115-139).
 *  - Pointers named d_* are device (HBM) pointers valid on the context's device; `stream` is a
 *    hipStream_t passed as void* (NULL = the context's own stream).  Calls that take a stream are
 *    asynchronous with respect to the host.  The plan-based calls (nrphy_pdsch_run, nrphy_ofdm_run,
 *    nrphy_ofdm_demod_run, nrphy_demodulate_soft, nrphy_llr_descramble, and nrphy_dft_run for the sizes up to 6144) neither
 *    allocate nor touch host memory and can be captured in a hipGraph, any number of them in any order -- a size's twiddle
 *    table is uploaded by the first call that uses it (plan creation, or one call outside the capture); nrphy_dft_run at
 *    the sizes above 6144 allocates its scratch in stream order (hipMallocAsync), which a capture records as memory nodes
 *    of the graph; the others say what they do at the call.  The grid writers
 *    that take host descriptors (nrphy_csi_rs_map, nrphy_pdcch_process, nrphy_ssb_process, nrphy_grid_put) copy them from
 *    host memory when called, like a plan creation: asynchronous, but not for capture (a replay would read host memory the
 *    caller has long released).
 *  - A PDSCH plan owns device scratch that every run rewrites before reading it (sequences, CRC shares): runs of
 *    ONE plan must be ordered (one stream, or events between streams); different plans may run concurrently.
 *    Every run is self-contained -- no state is carried from one run of a plan to the next.
 *  - Host-span entry points (*_host) are blocking and serialised per context (one lock for the whole call);
 *    they may be called from several threads.
 */
#ifndef MI355_NRPHY_H
#define MI355_NRPHY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRPHY_MAX_RB 275
#define NRPHY_NRE 12
#define NRPHY_NSYMB 14
#define NRPHY_MAX_PORTS 4
#define NRPHY_MAX_LAYERS 4
#define NRPHY_PRB_WORDS 5      /* 5 x 64 bits >= 275 PRB */
#define NRPHY_MAX_RESERVED 4   /* re_pattern_list::MAX_RE_PATTERN, R/include/srsran/phy/support/re_pattern.h:142 */
#define NRPHY_MAX_CODEBLOCKS 162 /* MAX_NOF_SEGMENTS, R/include/srsran/ran/sch/sch_constants.h:38 */
#define NRPHY_MAX_PRG ((NRPHY_MAX_RB + 3) / 4) /* precoding_constants::MAX_NOF_PRG: what the reference's precoding_configuration holds */
#define NRPHY_MAX_TB_BYTES (NRPHY_MAX_CODEBLOCKS * 8448 / 8) /* a transport block never has more bits than its codeblocks hold */

/* Status codes.  The reference aborts (srsran_assert) on argument errors; this ABI returns a code. */
enum {
  NRPHY_OK               = 0,
  NRPHY_ERR_INVALID_PDU  = 1, /* pdsch_pdu_validator::is_valid() == false */
  NRPHY_ERR_ARGUMENT     = 2, /* size mismatch, null pointer, unsupported size */
  NRPHY_ERR_DEVICE       = 3, /* HIP runtime error (no GPU, launch failure) */
  NRPHY_ERR_CAPACITY     = 4, /* batch exceeds the plan/context limits */
  NRPHY_ERR_NOT_READY    = 5  /* nrphy_dl_slot_poll: the slot's IQ has not reached the host yet */
};

/* RE pattern: {prb_mask, re_mask, symbols} of R/include/srsran/phy/support/re_pattern.h:40-77.
 * prb_mask bit p = PRB p of the grid (CRB index), re_mask bit k = subcarrier k of the PRB,
 * symbol_mask bit l = OFDM symbol l of the slot. */
typedef struct nrphy_re_pattern {
  uint64_t prb_mask[NRPHY_PRB_WORDS];
  uint16_t re_mask;
  uint16_t symbol_mask;
  uint32_t reserved_;
} nrphy_re_pattern_t;

/* POD mirror of pdsch_processor::pdu_t (R/include/srsran/phy/upper/channel_processors/pdsch_processor.h:58-155). */
typedef struct nrphy_pdsch_pdu {
  uint32_t slot_index;       /* slot_point::slot_index(): slot within the radio frame (DM-RS c_init) */
  uint32_t rnti;
  uint32_t bwp_start_rb;
  uint32_t bwp_size_rb;
  uint32_t cp;               /* 0 = normal (14 symbols per slot), 1 = extended (12; grid rows 12 and 13 stay zero) */
  uint32_t qm;               /* bits per symbol of codeword 0: 2 QPSK, 4 16QAM, 6 64QAM, 8 256QAM */
  uint32_t rv;               /* redundancy version 0..3 */
  uint32_t nof_codewords;    /* must be 1 (validator) */
  uint32_t n_id;
  uint32_t ref_point;        /* 0 = CRB0, 1 = PRB0 */
  uint32_t dmrs_symbol_mask; /* bit l = symbol l carries DM-RS */
  uint32_t dmrs_type;        /* 1 or 2; only 1 is valid */
  uint32_t scrambling_id;
  uint32_t n_scid;
  uint32_t nof_cdm_groups_without_data;
  uint32_t start_symbol_index;
  uint32_t nof_symbols;
  uint32_t ldpc_base_graph;  /* 1 or 2 */
  uint32_t tbs_lbrm_bytes;
  uint32_t vrb_contiguous;   /* rb_allocation::is_contiguous() of the VRB mask (validator rule) */
  uint64_t prb_mask[NRPHY_PRB_WORDS]; /* freq_alloc.get_prb_mask(bwp_start_rb, bwp_size_rb): allocated PRBs, grid-indexed */
  uint32_t nof_reserved;
  uint32_t tb_size_bytes;    /* data[0].size() */
  nrphy_re_pattern_t reserved[NRPHY_MAX_RESERVED];
  float    ratio_pdsch_dmrs_to_sss_dB;
  float    ratio_pdsch_data_to_sss_dB;
  /* precoding_configuration (R/include/srsran/phy/support/precoding_configuration.h) */
  uint32_t nof_layers;
  uint32_t nof_ports;
  uint32_t prg_size_rb;
  uint32_t nof_prg;          /* 1 .. NRPHY_MAX_PRG (prg_size_rb: 1 .. NRPHY_MAX_RB, NRPHY_MAX_RB = wideband) */
  const float* precoding;    /* host pointer: [nof_prg][nof_ports][nof_layers] complex (re, im).  PRGs count from PRB 0 of the
                              * grid: PRB b, data and DM-RS alike, takes the weights of PRG min(b / prg_size_rb, nof_prg - 1) */
} nrphy_pdsch_pdu_t;

/* Scalars the reference derives per PDU (pdsch_processor_impl.cpp:75-136, ldpc_segmenter_impl.cpp:90-160,
 * ldpc.h:128-228).  Filled by nrphy_pdsch_derive(); useful to size buffers. */
typedef struct nrphy_pdsch_derived {
  uint32_t nof_re;            /* data RE per layer */
  uint32_t nof_codeblocks;    /* C */
  uint32_t lifting_size;      /* Zc */
  uint32_t segment_length;    /* K = Kb*Zc */
  uint32_t cb_info_bits;      /* K' - L_cb */
  uint32_t nof_filler_bits;   /* F */
  uint32_t nof_tb_crc_bits;   /* 16 or 24 */
  uint32_t nof_cb_crc_bits;   /* 0 or 24 */
  uint32_t zero_pad;          /* zero bits appended to the last CB */
  uint32_t full_length;       /* N = 66*Zc or 50*Zc */
  uint32_t n_ref;             /* Nref */
  uint32_t n_cb;              /* Ncb = min(N, Nref) */
  uint32_t k0;                /* rate-matching start */
  uint32_t nof_short_segments;
  uint32_t rm_length_short;   /* E of the short segments */
  uint32_t rm_length_long;    /* E of the others */
  uint32_t codeword_bits;     /* G */
} nrphy_pdsch_derived_t;

/* ofdm_modulator_configuration, R/include/srsran/phy/lower/modulation/ofdm_modulator.h:34-47. */
typedef struct nrphy_ofdm_config {
  uint32_t numerology;
  uint32_t bw_rb;
  uint32_t dft_size;
  uint32_t cp;        /* 0 normal, 1 extended (12 symbols per slot, each with a cyclic prefix of dft_size / 4) */
  float    scale;
  double   center_freq_hz;
} nrphy_ofdm_config_t;

typedef struct nrphy_ctx nrphy_ctx_t;
typedef struct nrphy_pdsch_plan nrphy_pdsch_plan_t;
typedef struct nrphy_ofdm_plan nrphy_ofdm_plan_t;

/* ---- library ------------------------------------------------------------------------------- */
const char* nrphy_version(void);
const char* nrphy_strerror(int status);
/* Trace ranges: the entry points bracket their work in rocTX ranges named like the reference's trace points -- "process_pdsch"
 * (R/lib/phy/upper/downlink_processor_single_executor_impl.cpp:116-125), "CB batch", "process_dmrs"
 * (R/lib/phy/upper/channel_processors/pdsch_processor_concurrent_impl.cpp:265,317,342,367), "process_pdcch", "process_ssb",
 * "process_nzp_csi_rs", "process_pusch", "cb_decode", "downlink_baseband" -- when the process has the rocTX library loaded
 * (a profiler: rocprofv3 --marker-trace) or NRPHY_TRACE=1 is set; NRPHY_TRACE=0 switches them off.  1 = ranges are live. */
int nrphy_trace_enabled(void);

/* Creates the device context (streams, constant tables).  Replaces the factory chain
 * create_downlink_processor_factory_sw / _hw (R/lib/phy/upper/upper_phy_factories.cpp:659-919).
 * Fails with NRPHY_ERR_DEVICE when no HIP device is present: there is no CPU fallback. */
int nrphy_create(nrphy_ctx_t** ctx, int device_id);
int nrphy_destroy(nrphy_ctx_t* ctx);
int nrphy_synchronize(nrphy_ctx_t* ctx, void* stream);

/* ---- host-only helpers (no device work) ------------------------------------------------------ */
/* pdsch_pdu_validator::is_valid (R/lib/phy/upper/channel_processors/pdsch_processor_validator_impl.cpp:99-181).
 * Returns NRPHY_OK or NRPHY_ERR_INVALID_PDU. */
int nrphy_pdsch_validate(const nrphy_pdsch_pdu_t* pdu);
/* Per-PDU derived scalars (see nrphy_pdsch_derived_t). */
int nrphy_pdsch_derive(const nrphy_pdsch_pdu_t* pdu, nrphy_pdsch_derived_t* out);
/* tbs_calculator_calculate (R/lib/ran/sch/tbs_calculator.cpp:124-144); returns TBS in bits. */
uint32_t nrphy_tbs_calculate(uint32_t nof_symb_sh, uint32_t nof_dmrs_prb, uint32_t nof_oh_prb, uint32_t qm,
                             float target_code_rate, uint32_t nof_layers, uint32_t n_prb);
/* ofdm_symbol_modulator::get_symbol_size (R/lib/phy/lower/modulation/ofdm_modulator_impl.h:68-71),
 * symbol_index counted within the subframe; and ofdm_slot_modulator::get_slot_size. */
uint32_t nrphy_ofdm_symbol_size(const nrphy_ofdm_config_t* cfg, uint32_t symbol_index);
uint32_t nrphy_ofdm_slot_size(const nrphy_ofdm_config_t* cfg, uint32_t slot_index);

/* ---- seam A: pdsch_processor::process, batched ------------------------------------------------
 * Replaces pdsch_processor::process (pdsch_processor.h:167-170; impl pdsch_processor_impl.cpp:30-73,
 * per-codeblock form pdsch_processor_concurrent_impl.cpp:55-338).
 *
 * A plan holds n_pdu PDUs.  PDU i reads its transport block at d_tb + tb_offset[i] and writes grid
 * number grid_index[i] of a batch of grids with nof_ports x 14 x nof_subc cbf16 each.  Creating a plan
 * validates every PDU (NRPHY_ERR_INVALID_PDU names none; use nrphy_pdsch_validate to find it), derives
 * the per-PDU and per-codeblock descriptors and uploads them; it may be run any number of times (runs of one plan
 * ordered with respect to each other, see the conventions above). */
int nrphy_pdsch_plan_create(nrphy_ctx_t* ctx, uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus,
                            const uint64_t* tb_offset, const uint32_t* grid_index, uint32_t nof_grids,
                            uint32_t grid_nof_ports, uint32_t grid_nof_subc, nrphy_pdsch_plan_t** plan);
int nrphy_pdsch_plan_destroy(nrphy_pdsch_plan_t* plan);
/* Total number of codeblocks / rate-matched codeword bits of the plan, and PDU i's offset (in bits,
 * a multiple of 32) into the codeword tap buffers. */
uint32_t nrphy_pdsch_plan_nof_codeblocks(const nrphy_pdsch_plan_t* plan);
uint64_t nrphy_pdsch_plan_codeword_bits(const nrphy_pdsch_plan_t* plan);
uint64_t nrphy_pdsch_plan_codeword_offset(const nrphy_pdsch_plan_t* plan, uint32_t pdu);
/* The numbers of distinct scrambling sequences and of distinct sets of DM-RS sequences a run of the plan
 * generates: PDUs with the same scrambling initialisation and codeword layout (codeblock count and lengths,
 * bits per resource element) share one sequence, PDUs with the same DM-RS symbols, initialisations and
 * length one set -- the slots of one UE in a batch, for instance.  Either pointer may be NULL. */
int nrphy_pdsch_plan_nof_sequences(const nrphy_pdsch_plan_t* plan, uint32_t* scrambling, uint32_t* dmrs);

/* The form in which a run of the plan hands its distinct scrambling sequences from the prologue to the codeblock
 * waves: 1 = whole words (the sequences of the plan fit a level-2 cache), 0 = one 31-word seed per work item,
 * which the waves expand.  The outputs do not depend on it.  -1: plan is NULL. */
int nrphy_pdsch_plan_scrambling_form(const nrphy_pdsch_plan_t* plan);

/* How a run of the plan launches its codeblock waves: 1 = one launch of the mixed kernel, which selects (Qm, layers)
 * per wave, 2 = one launch per (Qm, layers) bucket of the plan.  The choice follows the plan's shape unless the
 * context was created under NRPHY_CB_DISPATCH=1 or =2.  The outputs do not depend on it.  -1: plan is NULL. */
int nrphy_pdsch_plan_codeblock_dispatch(const nrphy_pdsch_plan_t* plan);

/* Runs the whole PDSCH path of every PDU of the plan: TB CRC, segmentation, CB CRC, LDPC encoding,
 * rate matching, bit interleaving, scrambling, modulation, layer mapping, precoding, RE mapping and
 * DM-RS generation.  d_grid may be NULL (encode only, seam B semantics).  Optional taps, either may be
 * NULL: d_cw_rm receives the rate-matched + interleaved codeword of pdsch_encoder::encode
 * (pdsch_encoder_impl.cpp:28-72) packed MSB-first, d_cw_scrambled the same after scrambling
 * (pdsch_modulator_impl.cpp:30-44).  The caller zeroes the grids (resource_grid::set_all_zero) or
 * passes zero_grids != 0 to have the run clear them first. */
int nrphy_pdsch_run(nrphy_pdsch_plan_t* plan, const uint8_t* d_tb, void* d_grid, uint8_t* d_cw_rm,
                    uint8_t* d_cw_scrambled, int zero_grids, void* stream);

/* Per-kernel device timing for the benchmark (the counterpart of logging_pdsch_processor_decorator,
 * R/lib/phy/upper/channel_processors/channel_processor_factories.cpp:1164-1240, which times process()).
 * After enabling with room for max_runs runs, every nrphy_pdsch_run records HIP events around its kernels on the
 * stream it launches on.  nrphy_pdsch_plan_kernel_times synchronises those events and returns the average
 * duration in milliseconds of {tb_crc, codeblock, dmrs, whole run} over the recorded runs (count in *nof_runs),
 * then resets the recording. */
int nrphy_pdsch_plan_enable_timing(nrphy_pdsch_plan_t* plan, uint32_t max_runs);
int nrphy_pdsch_plan_kernel_times(nrphy_pdsch_plan_t* plan, float avg_ms[4], uint32_t* nof_runs);
/* Only every stride-th run records its events (default 1: every run): an event between two launches costs the stream a few
 * microseconds -- 0.02 ms of a 0.88 ms step of the benchmark with six of them per step. */
int nrphy_pdsch_plan_timing_stride(nrphy_pdsch_plan_t* plan, uint32_t stride);

/* Host-span convenience with the reference's single-PDU semantics: copies the TB in, runs, copies
 * the grid out (blocking).  grid points to nof_ports x 14 x nof_subc cbf16 in host memory and is
 * overwritten only on the REs the PDU maps (like resource_grid_mapper), unless it is NULL.
 * cw_rm / cw_scrambled: optional host taps of codeword_bits bits (packed). */
int nrphy_pdsch_process_host(nrphy_ctx_t* ctx, const nrphy_pdsch_pdu_t* pdu, const uint8_t* tb, void* grid,
                             uint32_t grid_nof_ports, uint32_t grid_nof_subc, uint8_t* cw_rm,
                             uint8_t* cw_scrambled);
/* All PDSCH PDUs of one slot from host spans, blocking: one plan and one launch for the n_pdu transport blocks (tbs[i]:
 * pdus[i].tb_size_bytes bytes), all mapped into the one host grid, which is read first (what other channels wrote stays)
 * and written back.  What a FAPI DL_TTI.request carries for a slot (R/lib/fapi_adaptor/phy/fapi_to_phy_translator.cpp:
 * every dl_pdsch_pdu goes to its own pdsch_processor::process there) in one call; the PDUs' allocations are disjoint, as
 * the scheduler guarantees.  Statuses as nrphy_pdsch_plan_create. */
int nrphy_pdsch_process_slot_host(nrphy_ctx_t* ctx, uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus, const uint8_t* const* tbs,
                                  void* grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc);

/* Asynchronous host-span form: pdsch_processor::process "may return before completion, the notifier fires from any
 * thread exactly once" (pdsch_processor.h:157-170; the reference's own asynchronous pool:
 * R/lib/phy/upper/channel_processors/pdsch_processor_asynchronous_pool.h:39-143).  A queue keeps up to `depth` PDUs in
 * flight, each on a stream of its own with pinned staging.  Every submit derives the PDU's state anew, like the reference
 * (pdsch_processor_concurrent_impl.cpp:55-207) -- live traffic brings a new pdu_t per slot -- straight into the operation's
 * staging: no device allocation, no blocking copy, one host-to-device copy for the tables and the transport block; only what
 * depends on the SHAPE of the PDU (RE mapping tables, zero-fill lists) is kept from earlier submits.  Submit copies the
 * transport block (the caller's span is free on return) and returns at once;
 * `done(user, status, grid)` runs on a thread of the HIP runtime when the PDU's grid has reached the host: `grid`
 * points at [grid_nof_ports][14][grid_nof_subc] cbf16 (zeros + the PDU's resource elements, DM-RS included), valid until
 * `done` returns -- the handler merges the PDU's RE into the caller's grid and signals its notifier; `status` is
 * NRPHY_ERR_DEVICE when the operation's stream reported an error.  NRPHY_ERR_CAPACITY: `depth` PDUs in flight
 * (nrphy_pdsch_async_wait_slot, or retry).  The handler must not call HIP or this library.
 * Tunable, read when the queue is created: environment variable NRPHY_ASYNC_ZERO_COPY = 1 lets the kernels read the
 * transport block from the operation's pinned staging instead of copying it to the device first, = 3 also lets them write
 * the grid into the pinned buffer `done` receives (pays with many operations in flight). */
typedef struct nrphy_pdsch_async nrphy_pdsch_async_t;
typedef void (*nrphy_pdsch_done_fn)(void* user, int status, const void* grid);
int nrphy_pdsch_async_create(nrphy_ctx_t* ctx, uint32_t depth, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                             uint32_t max_tb_bytes, nrphy_pdsch_async_t** queue);
int nrphy_pdsch_async_submit(nrphy_pdsch_async_t* queue, const nrphy_pdsch_pdu_t* pdu, const uint8_t* tb,
                             nrphy_pdsch_done_fn done, void* user);
/* All PDSCH PDUs of one slot as ONE operation (one plan, one launch, one grid, one completion): what a FAPI DL_TTI.request
 * carries for a slot.  The transport blocks together (each rounded up to a multiple of 4, plus 4) must fit max_tb_bytes of
 * nrphy_pdsch_async_create; the PDUs' allocations are disjoint.  Statuses as nrphy_pdsch_async_submit. */
int nrphy_pdsch_async_submit_slot(nrphy_pdsch_async_t* queue, uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus,
                                  const uint8_t* const* tbs, nrphy_pdsch_done_fn done, void* user);
int nrphy_pdsch_async_wait(nrphy_pdsch_async_t* queue);    /* until nothing is in flight */
int nrphy_pdsch_async_wait_slot(nrphy_pdsch_async_t* queue); /* until fewer than `depth` operations are in flight */
int nrphy_pdsch_async_destroy(nrphy_pdsch_async_t* queue); /* waits, then frees */
/* A completion handler that counts: `user` points at a uint64_t incremented atomically per successful PDU. */
void nrphy_pdsch_async_count_done(void* user, int status, const void* grid);

/* ---- seam B: pdsch_encoder::encode / hal::hw_accelerator_pdsch_enc in transport-block mode --------
 * Replaces pdsch_encoder::encode (R/include/srsran/phy/upper/channel_processors/pdsch_encoder.h;
 * impl R/lib/phy/upper/channel_processors/pdsch_encoder_impl.cpp:28-77) and what
 * pdsch_encoder_hw_impl::encode (pdsch_encoder_hw_impl.cpp:34-180) asks of a hardware accelerator:
 * TB CRC + segmentation + CB CRC + LDPC encoding + rate matching + bit interleaving of one transport
 * block, no scrambling.  The fields are pdsch_encoder::configuration (base_graph 1|2, rv, qm = bits per
 * symbol of `mod`, Nref with 0 = unlimited, nof_layers, nof_ch_symbols = RE x layers) + the TB size.
 * codeword_bits (nof_ch_symbols * qm bytes, one bit per byte: the reference's codeword span) and
 * codeword_packed (the same bits MSB-first) may each be NULL.  Host spans, blocking. */
typedef struct nrphy_pdsch_encoder_cfg {
  uint32_t base_graph;
  uint32_t rv;
  uint32_t qm;
  uint32_t nref;
  uint32_t nof_layers;
  uint32_t nof_ch_symbols;
  uint32_t tb_size_bytes;
} nrphy_pdsch_encoder_cfg_t;
int nrphy_pdsch_encode_host(nrphy_ctx_t* ctx, const nrphy_pdsch_encoder_cfg_t* cfg, const uint8_t* tb,
                            uint8_t* codeword_bits, uint8_t* codeword_packed);

/* ---- seam B pieces: ldpc_encoder::encode, batched ----------------------------------------------
 * Replaces ldpc_encoder::encode (R/lib/phy/upper/channel_coding/ldpc/ldpc_encoder_impl.cpp:44-81) for
 * n_cb codeblocks that share (base graph, lifting size).  d_msg: n_cb messages of Kb*Zc bits, each
 * starting on a multiple of msg_stride_bytes; filler bits are zeros.  d_out: n_cb outputs of
 * out_bits bits (the codeblock without its first 2*Zc bits, out_bits <= (N_full-2)*Zc), each starting
 * on a multiple of out_stride_bytes. */
int nrphy_ldpc_encode(nrphy_ctx_t* ctx, uint32_t base_graph, uint32_t lifting_size, uint32_t n_cb,
                      const uint8_t* d_msg, uint32_t msg_stride_bytes, uint32_t out_bits, uint8_t* d_out,
                      uint32_t out_stride_bytes, void* stream);

/* ---- seam C: ofdm_slot_modulator / ofdm_symbol_modulator, batched -------------------------------
 * Replaces ofdm_symbol_modulator::modulate and ofdm_slot_modulator::modulate
 * (R/include/srsran/phy/lower/modulation/ofdm_modulator.h:54-101; impl ofdm_modulator_impl.cpp:56-139).
 * Grid layout as above with nof_subc = 12*bw_rb.  Grid g is modulated as slot slot_index[g] of the
 * subframe (NULL: all slot 0) into d_iq + g * nof_ports * slot_size_max, port after port, where
 * slot_size_max = nrphy_ofdm_plan_slot_stride() (the size of slot 0, the largest). */
int nrphy_ofdm_plan_create(nrphy_ctx_t* ctx, const nrphy_ofdm_config_t* cfg, uint32_t nof_ports,
                           nrphy_ofdm_plan_t** plan);
int nrphy_ofdm_plan_destroy(nrphy_ofdm_plan_t* plan);
uint32_t nrphy_ofdm_plan_slot_stride(const nrphy_ofdm_plan_t* plan);
int nrphy_ofdm_run(nrphy_ofdm_plan_t* plan, uint32_t nof_grids, const void* d_grid, const uint32_t* slot_index,
                   float* d_iq, void* stream);
/* Same for the OFDM kernel: average milliseconds per nrphy_ofdm_run launch. */
int nrphy_ofdm_plan_enable_timing(nrphy_ofdm_plan_t* plan, uint32_t max_runs);
int nrphy_ofdm_plan_kernel_time(nrphy_ofdm_plan_t* plan, float* avg_ms, uint32_t* nof_runs);
int nrphy_ofdm_plan_timing_stride(nrphy_ofdm_plan_t* plan, uint32_t stride); /* as nrphy_pdsch_plan_timing_stride */
/* Host-span single-symbol form of ofdm_symbol_modulator::modulate: grid is one grid in host memory. */
int nrphy_ofdm_modulate_symbol_host(nrphy_ofdm_plan_t* plan, const void* grid, uint32_t port_index,
                                    uint32_t symbol_index, float* output, uint32_t output_size);

/* Host-span whole-slot form of ofdm_slot_modulator::modulate for every port of one grid: iq receives
 * nof_ports x nrphy_ofdm_slot_size(cfg, slot_index) complex samples, port after port (blocking). */
int nrphy_ofdm_modulate_slot_host(nrphy_ofdm_plan_t* plan, const void* grid, uint32_t slot_index, float* iq);

/* ---- device-resident resource grid: sparse writes from the host --------------------------------------
 * The channels this library does not generate (PRS, PT-RS, ...) stay on the CPU; their resource elements
 * -- a few hundred per slot -- are merged into the grid in HBM with one call per slot instead of moving the
 * grid.  Counterpart of resource_grid_writer::put(port, l, k_init, mask, symbols)
 * (R/include/srsran/phy/support/resource_grid_writer.h) for a grid that lives on the device: later entries
 * win over earlier ones, everything else in the grid is left alone. */
typedef struct nrphy_grid_re {
  uint16_t port;
  uint16_t symbol;
  uint32_t subc;
  uint32_t value;  /* cbf16: bf16 real part in the low half, imaginary part in the high half */
} nrphy_grid_re_t;
/* d_grid: ONE grid [nof_ports][14][nof_subc] in device memory; entries: host array, copied at the call into a
 * staging buffer of the call's own (stream-ordered allocation: hipMallocAsync / hipFreeAsync on `stream`).
 * Asynchronous on `stream` afterwards. */
int nrphy_grid_put(nrphy_ctx_t* ctx, void* d_grid, uint32_t nof_ports, uint32_t nof_subc, uint32_t n,
                   const nrphy_grid_re_t* entries, void* stream);

/* ---- soft-bit descrambling ("next" row, SURVEY.md section 8f-1: the step between the demodulation mapper and the
 * UL-SCH decoder) -------------------------------------------------------------------------------------------
 * Replaces pseudo_random_generator::apply_xor(span<log_likelihood_ratio>, span<const log_likelihood_ratio>)
 * (R/include/srsran/phy/upper/sequence_generators/pseudo_random_generator.h; implementation
 * R/lib/phy/upper/sequence_generators/pseudo_random_generator_impl.cpp:423-523) after init(c_init), and the same
 * operation written out in pusch_demodulator_impl (revert_scrambling on the generated sequence,
 * R/lib/phy/upper/channel_processors/pusch/pusch_demodulator_impl.cpp:38-100, 254-259, one OFDM symbol at a time):
 * out[i] = c(i) ? -in[i] : in[i] in 8-bit two's complement (-128 stays -128), c = the Gold sequence of TS 38.211
 * Section 5.2.1 from its first bit.  The UCI placeholder handling of that demodulator is not part of this call.
 * n_cw codewords of `length` soft bits each, row r at d_in + r * in_stride / d_out + r * out_stride (bytes; in place
 * is allowed: d_out == d_in), d_c_init: n_cw values IN DEVICE MEMORY (for PUSCH (rnti << 15) + n_id, TS 38.211
 * Section 6.3.1.1).  length <= 2^21; n_cw <= 65535.  16-byte aligned rows take the wide path.  Asynchronous on
 * `stream` (NULL: the context's stream); no host memory is touched, so the call can be captured in a hipGraph. */
int nrphy_llr_descramble(nrphy_ctx_t* ctx, uint32_t n_cw, const uint32_t* d_c_init, uint32_t length, const int8_t* d_in,
                         size_t in_stride, int8_t* d_out, size_t out_stride, void* stream);
/* One codeword from and to host memory (blocking; for tests and small cases). */
int nrphy_llr_descramble_host(nrphy_ctx_t* ctx, uint32_t c_init, uint32_t length, const int8_t* in, int8_t* out);

/* ---- receive side ("next" row): soft demodulator ("demodulation mapper") -------------------
 * Replaces demodulation_mapper::demodulate_soft (R/include/srsran/phy/upper/channel_modulation/demodulation_mapper.h:
 * 38-62; R/lib/phy/upper/channel_modulation/demodulation_mapper_impl.cpp:33-106 and demodulation_mapper_{qpsk,qam16,
 * qam64,qam256}.cpp): equalised symbols and their noise variances -> 8-bit log-likelihood ratios in [-120, 120],
 * bits-per-symbol values per symbol in the bit order of TS 38.211 Section 5.1.
 * The reference's value depends on the symbol's position in the span it is handed: with AVX2 (the build this library is
 * pinned to) the first floor(n / B) * B symbols (B = 16 QPSK, 8 16-QAM, 16 64-QAM, 4 256-QAM; none for the BPSKs) use
 * 1 / noise_var (0 when the variance is not > 0), floor(v * (1 / width)) for the interval, round-to-nearest-even and
 * blank a COMPONENT with |v| <= 1e-9; the remaining symbols divide by the variance (QPSK, 16-QAM), use floor(v / width),
 * round half away from zero and blank a SYMBOL with |z|^2 < 1e-9.  This call reproduces both, per position, bit for bit;
 * so one call must cover exactly one reference call: nof_spans spans of span_len symbols each, span r at
 * d_symbols + 2 * r * span_len floats (real, imaginary), d_noise_vars + r * span_len, d_llr + r * span_len * Qm
 * (nof_spans <= 65535).
 * A variance that is zero, negative or NaN gives zeros (as in the reference).  Asynchronous on `stream`; no host memory is
 * touched, so the call can be captured in a hipGraph. */
#define NRPHY_MOD_PI2_BPSK 0u
#define NRPHY_MOD_BPSK 1u
#define NRPHY_MOD_QPSK 2u
#define NRPHY_MOD_QAM16 4u
#define NRPHY_MOD_QAM64 6u
#define NRPHY_MOD_QAM256 8u
int nrphy_demodulate_soft(nrphy_ctx_t* ctx, uint32_t modulation, uint32_t nof_spans, uint32_t span_len, const float* d_symbols,
                          const float* d_noise_vars, int8_t* d_llr, void* stream);
/* One span from and to host memory (blocking; for the adaptor, tests and small cases). */
int nrphy_demodulate_soft_host(nrphy_ctx_t* ctx, uint32_t modulation, uint32_t nof_symbols, const float* symbols,
                               const float* noise_vars, int8_t* llr);

/* ---- receive side: channel equaliser -----------------------------------------------------------------------------------
 * Replaces channel_equalizer::equalize (R/include/srsran/phy/upper/equalization/channel_equalizer.h:86; impl
 * R/lib/phy/upper/equalization/channel_equalizer_generic_impl.cpp:225-277 with equalize_{zf_1xn,mmse_1xn,zf_2xn}.h), the
 * reference's scalar arithmetic with exact division:
 *   ZF, one layer:   ports whose noise variance is not in (0, inf) are left out; the others, per RE, when |h|^2 and the
 *                    variance are normal numbers; x = sum(y conj(h)) / (s sum|h|^2), var = sum(|h|^2 nv) / (s sum|h|^2)^2.
 *   MMSE, one layer: h is scaled by s first; per RE and port as above; x = sum(y conj(h)) sum|h|^2 / ((sum|h|^2)^2 + sum(|h|^2 nv)),
 *                    var = sum(|h|^2 nv) / ((sum|h|^2)^2 + sum(|h|^2 nv)) (the reference's denominator, as written).
 *   ZF, two layers on 2 or 4 ports: the 2x2 pseudo-inverse, one noise variance for all ports (their maximum).
 * Where the reference gives up (abnormal denominators), the symbol is 0 and its variance +inf.
 * n_batch independent problems of nof_re RE: d_rx [batch][port][re] cbf16, d_ch [batch][layer][port][re] cbf16,
 * d_noise_vars [batch][nof_rx_ports] f32 -> d_eq [batch][re][layer] complex f32, d_eq_nvars [batch][re][layer] f32.
 * algorithm: NRPHY_EQ_ZF or NRPHY_EQ_MMSE; tx_scaling > 0.  Asynchronous on `stream`, capturable. */
#define NRPHY_EQ_ZF 0u
#define NRPHY_EQ_MMSE 1u
int nrphy_channel_equalize(nrphy_ctx_t* ctx, uint32_t algorithm, uint32_t n_batch, uint32_t nof_re, uint32_t nof_layers,
                           uint32_t nof_rx_ports, const void* d_rx, const void* d_ch, const float* d_noise_vars, float tx_scaling,
                           float* d_eq, float* d_eq_nvars, void* stream);
/* One problem from and to host memory (blocking). */
int nrphy_channel_equalize_host(nrphy_ctx_t* ctx, uint32_t algorithm, uint32_t nof_re, uint32_t nof_layers, uint32_t nof_rx_ports,
                                const void* rx, const void* ch, const float* noise_vars, float tx_scaling, float* eq,
                                float* eq_nvars);

/* ---- receive side: PUSCH demodulator ------------------------------------------------------------------------------------
 * Replaces pusch_demodulator::demodulate (R/include/srsran/phy/upper/channel_processors/pusch/pusch_demodulator.h; impl
 * R/lib/phy/upper/channel_processors/pusch/pusch_demodulator_impl.cpp:135-287): data RE of the allocation taken from the
 * received grid and the channel estimate, equalised (nrphy_channel_equalize, tx_scaling 1), soft-demapped
 * (nrphy_demodulate_soft, one span per OFDM symbol as the reference hands them over) and descrambled (nrphy_llr_descramble,
 * c_init = rnti * 2^15 + n_id), in one kernel, bit for bit what the three calls give.  Codeword order: OFDM symbol, then
 * ascending subcarrier, then layer, then bits.  DM-RS symbols lose the RE of their CDM groups without data (type 1: even
 * or all subcarriers; type 2: pairs {0,1,6,7}, {2,3,8,9}, {4,5,10,11} per group); symbols without data RE are skipped.
 * Receive port i reads grid port rx_ports[i].  Post-equalisation SINR (pusch_demodulator_impl.cpp:203-215, 255-262):
 * -10 log10 of the mean of the equalised noise variances that are not infinite, +inf when there are none or their sum is
 * not positive; reduced in a fixed order (two runs give the same bits).  Transform precoding and pi/2-BPSK are opt-in: see
 * the _ex forms below. */
typedef struct nrphy_pusch_demod_cfg {
  uint32_t rnti, n_id;                    /* c_init = rnti * 2^15 + n_id */
  uint32_t qm;                            /* 2, 4, 6, 8; 1 (pi/2-BPSK) with NRPHY_PUSCH_DEMOD_PI2_BPSK */
  uint32_t start_symbol_index, nof_symbols;
  uint32_t dmrs_symbol_mask;              /* bit l = symbol l carries DM-RS */
  uint32_t dmrs_type;                     /* 1 or 2 */
  uint32_t nof_cdm_groups_without_data;   /* type 1: 1..2, type 2: 1..3 */
  uint32_t nof_tx_layers;                 /* 1 or 2 */
  uint32_t nof_rx_ports;                  /* 1..4 */
  uint32_t rx_ports[NRPHY_MAX_PORTS];     /* grid port of receive port i */
  uint32_t equalizer;                     /* NRPHY_EQ_ZF, NRPHY_EQ_MMSE (one layer only, as the reference) */
  uint32_t transform_precoding;           /* 0; 1 with NRPHY_PUSCH_DEMOD_TRANSFORM_PRECODING */
  uint32_t reserved_;
  uint64_t prb_mask[NRPHY_PRB_WORDS];     /* allocated PRBs, grid-indexed */
} nrphy_pusch_demod_cfg_t;
typedef struct nrphy_pusch_demod_plan nrphy_pusch_demod_plan_t;
/* NRPHY_OK, or NRPHY_ERR_ARGUMENT for: transform precoding; a modulation other than QPSK..256-QAM; more than 2 layers, MMSE
 * with 2 layers, 2 layers on other than 2 or 4 ports; a DM-RS type or CDM-group count the type does not allow; an rx port
 * outside the grid or repeated; PRBs beyond the grid; symbols beyond the slot; an allocation without data RE.  No device work. */
int nrphy_pusch_demod_validate(const nrphy_pusch_demod_cfg_t* cfg, uint32_t grid_nof_ports, uint32_t grid_nof_subc);
/* G = data RE x layers x qm (0 for a configuration the structure cannot describe).  No device work. */
uint64_t nrphy_pusch_demod_codeword_bits(const nrphy_pusch_demod_cfg_t* cfg);
/* n PUSCHs; PUSCH i reads grid grid_index[i] of [nof_grids][grid_nof_ports][14][grid_nof_subc] cbf16 and its channel estimate
 * at element ce_offset[i] of d_ch_est: [layer][rx port i][14][grid_nof_subc] cbf16 (the reference's channel_estimate,
 * subcarrier fastest).  Validates every configuration, builds the work list (PUSCH, OFDM symbol, chunk of data RE) and
 * uploads it (blocking, like nrphy_pdsch_plan_create). */
int nrphy_pusch_demod_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_demod_cfg_t* cfgs, const uint32_t* grid_index,
                                  uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc, const uint64_t* ce_offset,
                                  nrphy_pusch_demod_plan_t** plan);
int nrphy_pusch_demod_plan_destroy(nrphy_pusch_demod_plan_t* plan);
uint64_t nrphy_pusch_demod_plan_codeword_bits(const nrphy_pusch_demod_plan_t* plan, uint32_t i);
/* d_noise_vars: [n][NRPHY_MAX_PORTS] f32 in device memory, entry i of a row = receive port i.  PUSCH i writes its G_i
 * descrambled soft bits at d_llr + i * llr_stride (the input of nrphy_pusch_decode_batch) and, when d_sinr_db is not NULL,
 * its SINR in dB to d_sinr_db[i].  Asynchronous on `stream`; allocates nothing and touches no host memory (capturable).
 * Runs of one plan must be ordered (the plan owns the SINR partial sums). */
int nrphy_pusch_demod_run(nrphy_pusch_demod_plan_t* plan, const void* d_grid, const void* d_ch_est, const float* d_noise_vars,
                          int8_t* d_llr, uint64_t llr_stride, float* d_sinr_db, void* stream);
/* One PUSCH from and to host memory (blocking): grid [grid_nof_ports][14][grid_nof_subc] cbf16, ch_est
 * [layers][nof_rx_ports][14][grid_nof_subc] cbf16, noise_vars[nof_rx_ports] -> llr[G]; sinr_db may be NULL. */
int nrphy_pusch_demodulate_host(nrphy_ctx_t* ctx, const nrphy_pusch_demod_cfg_t* cfg, const void* grid, uint32_t grid_nof_ports,
                                uint32_t grid_nof_subc, const void* ch_est, const float* noise_vars, int8_t* llr, float* sinr_db);
/* The forms with a feature mask.  The three functions above are these with features = 0 (one implementation): a caller written
 * against them keeps getting the refusal of transform precoding and of qm = 1.  The plan type, nrphy_pusch_demod_run,
 * nrphy_pusch_demod_plan_codeword_bits and the output layout are the same; a plan may mix plain and transform-precoded PUSCHs.
 *   NRPHY_PUSCH_DEMOD_TRANSFORM_PRECODING  transform_precoding = 1 is accepted when there is one layer, the DM-RS is type 1 with
 *     2 CDM groups without data (TS 38.214 Section 6.2.2: every symbol that carries data then carries 12 RE per PRB; the reference
 *     would silently run a half-size transform on a DM-RS symbol otherwise) and the number of allocated PRBs M_rb is a size of
 *     nrphy_transform_precoding_nof_prb_valid.  As in the reference the PRBs need not be contiguous: the transform runs over the
 *     12 M_rb allocated subcarriers in ascending order.  Per OFDM symbol with data: equalise, nrphy_transform_deprecode over the
 *     whole symbol, then demap symbol j with the equalised noise variance of RE j -- the deprecoder leaves the variances alone
 *     (pusch_demodulator_impl.cpp:186-215) --, descramble; an RE the equaliser gave up on enters the transform as 0.  One
 *     workgroup per symbol; bit for bit nrphy_channel_equalize -> nrphy_transform_deprecode -> nrphy_demodulate_soft ->
 *     nrphy_llr_descramble.  The channel estimate of such a PUSCH comes from nrphy_pusch_chest_plan_create_ex with the
 *     low-PAPR DM-RS enabled (the reference's dmrs_pusch_estimator of this release has Gold DM-RS only).
 *   NRPHY_PUSCH_DEMOD_PI2_BPSK  qm = 1 is accepted, with or without transform precoding: the pi/2-BPSK demapper of
 *     nrphy_demodulate_soft (NRPHY_MOD_PI2_BPSK), indexed by the symbol's position in its OFDM symbol's span.
 * Everything else of nrphy_pusch_demod_validate applies; a bit outside the two is NRPHY_ERR_ARGUMENT. */
#define NRPHY_PUSCH_DEMOD_TRANSFORM_PRECODING 1u
#define NRPHY_PUSCH_DEMOD_PI2_BPSK 2u
int nrphy_pusch_demod_validate_ex(const nrphy_pusch_demod_cfg_t* cfg, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                                  uint32_t features);
int nrphy_pusch_demod_plan_create_ex(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_demod_cfg_t* cfgs, const uint32_t* grid_index,
                                     uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc, const uint64_t* ce_offset,
                                     uint32_t features, nrphy_pusch_demod_plan_t** plan);
int nrphy_pusch_demodulate_host_ex(nrphy_ctx_t* ctx, const nrphy_pusch_demod_cfg_t* cfg, const void* grid, uint32_t grid_nof_ports,
                                   uint32_t grid_nof_subc, const void* ch_est, const float* noise_vars, uint32_t features,
                                   int8_t* llr, float* sinr_db);
/* The forms with the EVM: what pusch_demodulator_impl reports when it is constructed with an evm_calculator
 * (R/lib/phy/upper/channel_modulation/evm_calculator_generic_impl.cpp, pusch_demodulator_impl.cpp:157-162, 244-252, 266-278).
 * Per OFDM symbol s with data, over its n_s = data RE x layers equalised symbols x_j -- after the deprecoder for a
 * transform-precoded PUSCH -- and the demapper's soft bits before descrambling: hard bit 1 where the soft bit is <= 0 (an RE the
 * equaliser gave up on decides all ones and counts like any other), the hard bits mapped to the constellation point m_j of
 * modulation_mapper_lut_impl, P_s = sum |m_j - x_j|^2, e_s = sqrtf(P_s / n_s); over the symbols in ascending order in float
 * acc += n_s * e_s, cnt += n_s; EVM = acc / cnt.  Every term of P_s is formed in float with the reference's roundings and the
 * terms are added in double in a fixed order (lanes, waves, work items), so the value differs from the reference's float chain
 * by rounding only, and two runs give the same bytes.  d_evm[i] is the EVM of PUSCH i; either of d_sinr_db and d_evm may be
 * NULL, and with d_evm == NULL the call is exactly nrphy_pusch_demod_run (the same kernels).  Works on the plans of both
 * creation calls.  The host form takes the feature mask of nrphy_pusch_demodulate_host_ex; sinr_db and evm may be NULL. */
int nrphy_pusch_demod_run_evm(nrphy_pusch_demod_plan_t* plan, const void* d_grid, const void* d_ch_est, const float* d_noise_vars,
                              int8_t* d_llr, uint64_t llr_stride, float* d_sinr_db, float* d_evm, void* stream);
int nrphy_pusch_demodulate_host_evm(nrphy_ctx_t* ctx, const nrphy_pusch_demod_cfg_t* cfg, const void* grid, uint32_t grid_nof_ports,
                                    uint32_t grid_nof_subc, const void* ch_est, const float* noise_vars, uint32_t features,
                                    int8_t* llr, float* sinr_db, float* evm);

/* ---- receive side: transform deprecoder (DFT-s-OFDM) ----------------------------------------------------------------------
 * Replaces transform_precoder::deprecode_ofdm_symbol (R/include/srsran/phy/generic_functions/transform_precoding/
 * transform_precoder.h; impl R/lib/phy/generic_functions/transform_precoding/transform_precoder_dft_impl.cpp:31-57): the
 * unnormalised inverse DFT of 12 * nof_prb points, then a multiplication by the float 1 / sqrt(12 * nof_prb).  Valid sizes
 * (transform_precoding_helpers.h): nof_prb = 2^a 3^b 5^c up to 275 -- 53 values, the largest 270.  One workgroup per symbol, a
 * run-time radix-{2,3,4,5} transform in LDS; the twiddles exp(+2 pi i k / N) are evaluated in double and rounded once. */
/* 1 for a valid size, else 0.  Host only. */
int nrphy_transform_precoding_nof_prb_valid(uint32_t nof_prb);
/* `batch` symbols of 12 * nof_prb complex f32 back to back, d_in -> d_out (8-byte aligned); d_out == d_in is allowed, the
 * reference calls it in place.  NRPHY_ERR_ARGUMENT for an invalid nof_prb; batch = 0 does nothing.  Asynchronous on `stream`;
 * capturable once the size's twiddle table exists: it is uploaded by a plan creation that needs it or by the first call of that
 * size (the rule of nrphy_dft_run). */
int nrphy_transform_deprecode(nrphy_ctx_t* ctx, uint32_t nof_prb, uint32_t batch, const float* d_in, float* d_out, void* stream);
/* One symbol from and to host memory (blocking). */
int nrphy_transform_deprecode_host(nrphy_ctx_t* ctx, uint32_t nof_prb, const float* in, float* out);

/* ---- receive side: PUSCH DM-RS channel estimator ------------------------------------------------------------------------
 * Replaces dmrs_pusch_estimator::estimate (R/lib/phy/upper/signal_processors/dmrs_pusch_estimator_impl.cpp:71-212, with
 * port_channel_estimator_average_impl::compute, filter smoothing and CFO compensation on: the PUSCH processor's setting) and the
 * PUSCH processor's DC step (pusch_processor_impl.cpp:182-199).  Per (receive port, layer): LS estimates of the DM-RS of every
 * DM-RS symbol, the CFO from the first two, derotation and averaging, scaling by 1 / (nof DM-RS symbols x scaling), virtual
 * pilots and the raised-cosine FIR, RSRP, EPRE, noise variance and SNR, the time alignment from a 4096-point inverse DFT (bins
 * [0, 144) against [3952, 4096), delay on ties), linear interpolation to every subcarrier, cbf16 rounding, the per-symbol CFO
 * rotation (rounded again, as the reference does) and the DC subcarrier zeroed.  DM-RS type 1 only (ports 1000 and 1001: layer 1
 * takes w_f = -1 on every odd pilot), normal cyclic prefix, no frequency hopping.  Receive port i reads grid port rx_ports[i]. */
#define NRPHY_PUSCH_CHEST_NO_DC 0xFFFFFFFFu
#define NRPHY_PUSCH_CHEST_MAX_LAYERS 2
typedef struct nrphy_pusch_chest_cfg {
  uint32_t numerology;                /* 0..4 */
  uint32_t slot_index;                /* slot within the frame: < 10 * 2^numerology */
  uint32_t scrambling_id;             /* N_ID, 0..65535 */
  uint32_t n_scid;                    /* 0 or 1 */
  float    scaling;                   /* beta: DM-RS-to-data amplitude, > 0 and finite */
  uint32_t dmrs_type;                 /* must be 1 */
  uint32_t dmrs_symbol_mask;          /* bit l = symbol l carries DM-RS; every bit inside [start, start + nof) */
  uint32_t start_symbol_index, nof_symbols;
  uint32_t nof_tx_layers;             /* 1 or 2 */
  uint32_t nof_rx_ports;              /* 1..4 */
  uint32_t rx_ports[NRPHY_MAX_PORTS]; /* grid port of receive port i */
  uint32_t dc_position;               /* grid subcarrier of DC, or NRPHY_PUSCH_CHEST_NO_DC */
  uint64_t prb_mask[NRPHY_PRB_WORDS]; /* allocated PRBs, grid-indexed */
} nrphy_pusch_chest_cfg_t;
/* What channel_estimate holds per (PUSCH, receive port, layer). */
typedef struct nrphy_pusch_chest_meas {
  float    noise_var; /* sum |rx - beta h pilot e^{j 2 pi epoch cfo}|^2 / (pilots - 1), at least rsrp / 1e10 */
  float    rsrp;      /* mean |beta h|^2 over the pilots */
  float    epre;      /* mean |rx|^2 over the pilots */
  float    snr;       /* linear: (rsrp / beta^2) / noise_var */
  float    ta_s;      /* time alignment, seconds: ta_bins / (4096 SCS) */
  int32_t  ta_bins;   /* signed inverse-DFT bin of the peak */
  float    cfo_hz;    /* NaN with a single DM-RS symbol */
  uint32_t reserved_;
} nrphy_pusch_chest_meas_t;
typedef struct nrphy_pusch_chest_plan nrphy_pusch_chest_plan_t;
/* NRPHY_OK, or NRPHY_ERR_ARGUMENT for: DM-RS type other than 1; layers other than 1 or 2; no rx port, more than 4, one outside
 * the grid or repeated; PRBs beyond the grid or none; symbols beyond the slot; no DM-RS symbol in [start, start + nof) or a
 * DM-RS bit outside it; numerology above 4 or slot_index >= 10 * 2^numerology; scrambling_id above 65535, n_scid above 1;
 * scaling not positive and finite; dc_position neither NRPHY_PUSCH_CHEST_NO_DC nor inside the grid.  No device work. */
int nrphy_pusch_chest_validate(const nrphy_pusch_chest_cfg_t* cfg, uint32_t grid_nof_ports, uint32_t grid_nof_subc);
/* n PUSCHs; PUSCH i reads grid grid_index[i] of [nof_grids][grid_nof_ports][14][grid_nof_subc] cbf16 and writes its estimate at
 * element ce_offset[i] of d_ch_est: [layer][rx port i][14][grid_nof_subc] cbf16, the convention of nrphy_pusch_demod_plan_create
 * (one buffer feeds both).  Validates every configuration, precomputes the filter taps, c_init per DM-RS symbol and the symbol
 * epochs, and allocates the plan's scratch (blocking). */
int nrphy_pusch_chest_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_chest_cfg_t* cfgs, const uint32_t* grid_index,
                                  uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc, const uint64_t* ce_offset,
                                  nrphy_pusch_chest_plan_t** plan);
int nrphy_pusch_chest_plan_destroy(nrphy_pusch_chest_plan_t* plan);
/* Writes, for every PUSCH, layer and receive port, the allocated PRBs' subcarriers of symbols [start, start + nof) of the
 * estimate and nothing else; d_noise_vars: [n][NRPHY_MAX_PORTS] f32, entry i of row p = layer 0's noise variance of receive port
 * i (what nrphy_pusch_demod_run reads; the other entries are left alone); d_meas (may be NULL):
 * [n][NRPHY_MAX_PORTS][NRPHY_PUSCH_CHEST_MAX_LAYERS].  Asynchronous on `stream`; allocates nothing and touches no host memory
 * (capturable).  Runs of one plan must be ordered: the plan owns its scratch. */
int nrphy_pusch_chest_run(nrphy_pusch_chest_plan_t* plan, const void* d_grid, void* d_ch_est, float* d_noise_vars,
                          nrphy_pusch_chest_meas_t* d_meas, void* stream);
/* One PUSCH from and to host memory (blocking, on the GPU): grid [grid_nof_ports][14][grid_nof_subc] cbf16 -> ch_est
 * [layers][nof_rx_ports][14][grid_nof_subc] cbf16 (only the allocated region is written), noise_vars[nof_rx_ports], meas
 * [nof_rx_ports][NRPHY_PUSCH_CHEST_MAX_LAYERS] (may be NULL). */
int nrphy_pusch_chest_host(nrphy_ctx_t* ctx, const nrphy_pusch_chest_cfg_t* cfg, const void* grid, uint32_t grid_nof_ports,
                           uint32_t grid_nof_subc, void* ch_est, float* noise_vars, nrphy_pusch_chest_meas_t* meas);
/* The forms with the low-PAPR DM-RS of a transform-precoded PUSCH (TS 38.211 Section 6.4.1.1.1.2).  The three functions above
 * are these without a description (lp / lps == NULL; one implementation, the same bytes); the plan type and
 * nrphy_pusch_chest_run are the same, and a plan may mix Gold and low-PAPR PUSCHs (lps[i].enabled per PUSCH).  The reference's
 * dmrs_pusch_estimator generates Gold pilots only; its releases after 24.04 feed
 * low_papr_sequence_generator::generate(seq, n_rs_id % 30, 0, 0, 1) into the unchanged port_channel_estimator, and that is what
 * enabled = 1 does.  Group and sequence hopping are off: u = n_rs_id mod 30, v = 0, alpha = 0, delta = 1.  Pilot q,
 * q = 0 .. 6 M_rb - 1, is r_{u,0}(q) of length M_zc = 6 M_rb, over the allocated PRBs in ascending order (they need not be
 * contiguous, as in the demodulator), on the grid subcarrier the Gold pilot has (12 n + 2 k), the same on every DM-RS symbol,
 * with amplitude 1.  Every element is the entry low_papr_sequence_generator_impl takes of its exponential table
 * (R/lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.cpp:158-244): M_zc = 6, 12, 18, 24 from the phi tables
 * of TS 38.211 Section 5.2.2.2, M_zc >= 36 the Zadoff-Chu sequence of the largest prime below M_zc, q from the reference's float
 * evaluation.  The table's entries are std::polar(1.0F, float(2 pi) index / size) with the bits the reference's build gives them:
 * its cosf and sinf are the C library's (glibc 2.28 and later), which are not correctly rounded -- one float32 step from the
 * exact value's rounding in about 1 % of the entries -- and the kernel restates that routine, so the sequence equals the
 * reference's bit for bit.  M_zc = 30 (5 PRB) is ours and not the reference's,
 * whose generator terminates on that length: TS 38.211 Section 5.2.2.1, exp(-j pi (u + 1)(n + 1)(n + 2) / 31), as entry
 * (62 - ((u + 1)(n + 1)(n + 2) mod 62)) mod 62 of the reference's 62-point exponential table.  Everything behind the pilot is
 * nrphy_pusch_chest_run's.  With enabled = 1, NRPHY_ERR_ARGUMENT also for: more than one layer; n_scid other than 0; n_rs_id
 * above 1007; a number of allocated PRBs that nrphy_transform_precoding_nof_prb_valid rejects; scrambling_id is ignored (its range
 * is still checked).  enabled above 1 is NRPHY_ERR_ARGUMENT. */
typedef struct nrphy_pusch_chest_lowpapr {
  uint32_t enabled; /* 0: Gold DM-RS, 1: low-PAPR DM-RS */
  uint32_t n_rs_id; /* 0..1007 */
} nrphy_pusch_chest_lowpapr_t;
int nrphy_pusch_chest_validate_ex(const nrphy_pusch_chest_cfg_t* cfg, const nrphy_pusch_chest_lowpapr_t* lp, uint32_t grid_nof_ports,
                                  uint32_t grid_nof_subc);
int nrphy_pusch_chest_plan_create_ex(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_chest_cfg_t* cfgs,
                                     const nrphy_pusch_chest_lowpapr_t* lps, const uint32_t* grid_index, uint32_t nof_grids,
                                     uint32_t grid_nof_ports, uint32_t grid_nof_subc, const uint64_t* ce_offset,
                                     nrphy_pusch_chest_plan_t** plan);
int nrphy_pusch_chest_host_ex(nrphy_ctx_t* ctx, const nrphy_pusch_chest_cfg_t* cfg, const nrphy_pusch_chest_lowpapr_t* lp,
                              const void* grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc, void* ch_est, float* noise_vars,
                              nrphy_pusch_chest_meas_t* meas);
/* The low-PAPR DM-RS itself, from the kernel's generator: out[2 n], out[2 n + 1] = re, im of r_{u,0}(n), u = n_rs_id mod 30,
 * n < 6 nof_prb (blocking, as nrphy_srs_sequence_host).  NRPHY_ERR_ARGUMENT for n_rs_id above 1007 or an invalid nof_prb. */
int nrphy_pusch_lowpapr_sequence_host(nrphy_ctx_t* ctx, uint32_t n_rs_id, uint32_t nof_prb, float* out);

/* ---- receive side: PRACH detector -----------------------------------------------------------------------------------------
 * Replaces prach_detector_generic_impl::detect (R/lib/phy/upper/channel_processors/prach_detector_generic_impl.cpp:89-359, with
 * symbol combining on: the factory's setting) and prach_generator_impl::generate (prach_generator_impl.cpp:97-287).  Per
 * occasion: the RSSI; per monitored root sequence and receive port, the sum of the occasion's symbols times the conjugate of the
 * root's frequency-domain sequence, a 1024-point (long preambles) or 256-point (short) inverse DFT, |.|^2 / (N L^2); per cyclic
 * shift window, the reference energy over the window and its margins, numerator and noise estimate accumulated over the ports in
 * port order; per preamble, the metric num / |den|, its maximum (lowest index on a tie) and the three detection conditions.
 * Unrestricted sets only; the thresholds are the reference's table (prach_detector_generic_thresholds.h) or the caller's. */
enum {
  NRPHY_PRACH_FORMAT_0 = 0, NRPHY_PRACH_FORMAT_1, NRPHY_PRACH_FORMAT_2, NRPHY_PRACH_FORMAT_3, NRPHY_PRACH_FORMAT_A1,
  NRPHY_PRACH_FORMAT_A2, NRPHY_PRACH_FORMAT_A3, NRPHY_PRACH_FORMAT_B1, NRPHY_PRACH_FORMAT_B4, NRPHY_PRACH_FORMAT_C0,
  NRPHY_PRACH_FORMAT_C2, NRPHY_PRACH_FORMAT_A1_B1, NRPHY_PRACH_FORMAT_A2_B2, NRPHY_PRACH_FORMAT_A3_B3, NRPHY_PRACH_FORMAT_COUNT
};
enum {
  NRPHY_PRACH_SCS_15 = 0, NRPHY_PRACH_SCS_30, NRPHY_PRACH_SCS_60, NRPHY_PRACH_SCS_120, NRPHY_PRACH_SCS_1_25, NRPHY_PRACH_SCS_5,
  NRPHY_PRACH_SCS_COUNT
};
#define NRPHY_PRACH_MAX_PREAMBLES 64
typedef struct nrphy_prach_cfg {
  uint32_t format;                /* NRPHY_PRACH_FORMAT_* */
  uint32_t ra_scs;                /* NRPHY_PRACH_SCS_*: 1.25 kHz for formats 0..2, 5 kHz for format 3, 15..120 kHz for the short ones */
  uint32_t restricted_set;        /* must be 0 (unrestricted) */
  uint32_t root_sequence_index;   /* logical index: 0..837 (long), 0..137 (short) */
  uint32_t zero_correlation_zone; /* 0..15 */
  uint32_t start_preamble_index, nof_preamble_indices; /* the monitored preambles: start + nof <= 64, nof >= 1 */
  uint32_t nof_rx_ports;          /* 1..4 */
  float    threshold;             /* both 0: the library's table; both non-zero: the caller's threshold and margin */
  uint32_t win_margin;
} nrphy_prach_cfg_t;
typedef struct nrphy_prach_result { /* one per occasion */
  float    rssi_dB;
  float    time_resolution_s;     /* one correlation sample, rounded to T_c as phy_time_unit does */
  float    time_advance_max_s;    /* 0.8 x the largest delay of a window */
  uint32_t nof_detected;
  uint64_t detected_mask;         /* bit i: preamble i was detected */
} nrphy_prach_result_t;
typedef struct nrphy_prach_preamble { /* one per (occasion, preamble index) */
  uint32_t detected;
  uint32_t delay_samples;         /* index of the metric's maximum within the window */
  float    time_advance_s;        /* delay_samples / sampling rate, rounded to T_c */
  float    peak;                  /* the metric's maximum */
  float    detection_metric;      /* peak / threshold */
} nrphy_prach_preamble_t;
typedef struct nrphy_prach_plan nrphy_prach_plan_t;
/* The library's restatement of the reference's table: NRPHY_OK and the row's threshold, window margin and flag (0 red: not
 * suitable for detection, 1 orange, 2 green) where the table has a row for exactly (nof_rx_ports, ra_scs, format,
 * zero_correlation_zone); NRPHY_ERR_ARGUMENT where it has none (no neighbouring row is substituted).  Outputs may be NULL. */
int nrphy_prach_threshold(const nrphy_prach_cfg_t* cfg, float* threshold, uint32_t* win_margin, uint32_t* flag);
/* NRPHY_OK, or NRPHY_ERR_ARGUMENT for: a restricted set; an unknown format or spacing, or a spacing that is not the format's;
 * a zero-correlation zone above 15 (reserved N_CS); start + nof above 64 or nof = 0; no rx port or more than 4; a root sequence
 * index outside 0..837 (long) / 0..137 (short); exactly one of threshold and win_margin set, or a threshold that is not
 * positive and finite, or a margin that makes a reference window longer than the transform; without a caller's threshold, no
 * exact row in the table or a red one (what prach_detector_validator_impl::is_valid refuses).  No device work. */
int nrphy_prach_validate(const nrphy_prach_cfg_t* cfg);
/* n occasions; occasion i reads complex f32 samples at element sym_offset[i] + port * port_stride + symbol * symbol_stride + k,
 * k < L_RA, of d_symbols: a prach_buffer tensor (re, symbol, td occasion, fd occasion, port; re fastest) is read in place, one
 * (td, fd) occasion per item; nrphy_prach_demod_run (below) produces that tensor from baseband samples on the same stream.
 * Validates every configuration and precomputes, in the reference's order of operations, N_CS, the
 * number of shifts and sequences, window width, largest delay, threshold and margin and the monitored sequence numbers. */
int nrphy_prach_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_prach_cfg_t* cfgs, const uint64_t* sym_offset,
                            uint64_t port_stride, uint64_t symbol_stride, nrphy_prach_plan_t** plan);
int nrphy_prach_plan_destroy(nrphy_prach_plan_t* plan);
/* Floats per preamble of d_metric: the widest window of the plan's occasions. */
uint32_t nrphy_prach_plan_metric_stride(const nrphy_prach_plan_t* plan);
/* d_result: [n]; d_preambles: [n][64], written for every monitored index whether detected or not and zeroed for the others;
 * d_metric (may be NULL): [n][64][metric_stride] f32, the whole metric window of every monitored preamble, zeros elsewhere.  A
 * non-normal RSSI (an all-zero occasion) gives the result header and no detections.  Asynchronous on `stream`; allocates
 * nothing, touches no host memory, uses no atomics (capturable; two runs give identical bytes).  Runs of one plan must be
 * ordered: the plan owns one word of scratch per occasion. */
int nrphy_prach_run(nrphy_prach_plan_t* plan, const void* d_symbols, nrphy_prach_result_t* d_result,
                    nrphy_prach_preamble_t* d_preambles, float* d_metric, void* stream);
/* Floats per preamble of the metric of a plan of this one configuration (its window width in correlation samples); 0 where
 * nrphy_prach_validate refuses it.  No device work. */
uint32_t nrphy_prach_window_width(const nrphy_prach_cfg_t* cfg);
/* One occasion from and to host memory (blocking, on the GPU): symbols hold port p, symbol s at element p * port_stride +
 * s * symbol_stride; preambles[64]; metric (may be NULL): [64][nrphy_prach_window_width(cfg)]. */
int nrphy_prach_detect_host(nrphy_ctx_t* ctx, const nrphy_prach_cfg_t* cfg, const void* symbols, uint64_t port_stride,
                            uint64_t symbol_stride, nrphy_prach_result_t* result, nrphy_prach_preamble_t* preambles, float* metric);
/* The frequency-domain sequence of one preamble from the device's generator (what prach_generator::generate returns): y holds
 * L_RA complex f32.  The detection fields of cfg (ports, monitored range, threshold) are not looked at. */
int nrphy_prach_generate_host(nrphy_ctx_t* ctx, const nrphy_prach_cfg_t* cfg, uint32_t preamble_index, float* y);

/* ---- receive side: OFDM PRACH demodulator ---------------------------------------------------------------------------------
 * Replaces ofdm_prach_demodulator_impl::demodulate (R/lib/phy/lower/modulation/ofdm_prach_demodulator_impl.cpp:31-203): baseband
 * samples of a PRACH window to the frequency-domain symbols of a prach_buffer, for every time- and frequency-domain occasion and
 * receive port of a configuration.  Time-domain occasion i_td starts start_symbol + duration * i_td PUSCH symbols of
 * (144 + 2048) >> mu kappa into the window, 16 kappa later when that is after 0 and 16 more when it is after 0.5 ms; its preamble
 * is get_prach_preamble_long_info / _short_info (RA spacing = PUSCH spacing; the mixed formats change in the last occasion), with a
 * short format's cyclic prefix 16 kappa longer for an occasion across time 0 and across 0.5 ms.  Symbol s is the dft_size =
 * srate / ra_scs samples behind the prefix at dft_size * s; its transform is direct and unnormalised, with no phase or frequency
 * correction.  With K = pusch_scs / ra_scs, grid = nof_prb_ul_grid * K * 12 and k_start = K * 12 * (rb_offset + N_RB^RA * i_fd) +
 * k_bar (TS 38.211 Table 6.3.3.2-1), element i < L_RA of frequency-domain occasion i_fd is transform bin
 * (k_start + i - grid / 2) mod dft_size.  Unrestricted by set; complex float samples here, complex int16 ones through
 * nrphy_prach_window_demod_run (below, with the pool of PRACH windows that collects them). */
typedef struct nrphy_prach_demod_cfg {
  uint32_t srate_hz;              /* sampling rate; srate_hz / ra_scs must be a size nrphy_dft_run has */
  uint32_t format;                /* NRPHY_PRACH_FORMAT_* */
  uint32_t nof_td_occasions;      /* 1 for the long formats; start_symbol + duration * nof_td_occasions <= 14 for the short ones */
  uint32_t nof_fd_occasions;      /* 1..8 */
  uint32_t start_symbol;          /* 0..13, of the first time-domain occasion, in PUSCH symbols */
  uint32_t rb_offset;             /* PRACH frequency location, in PUSCH resource blocks */
  uint32_t nof_prb_ul_grid;       /* 1..275 */
  uint32_t pusch_numerology;      /* mu: 15 kHz << mu, 0..3 */
  uint32_t nof_rx_ports;          /* 1..4 */
} nrphy_prach_demod_cfg_t;
typedef struct nrphy_prach_demod_sizes {
  uint32_t dft_size;              /* samples per PRACH symbol */
  uint32_t sequence_length;       /* L_RA: 839 or 139 */
  uint32_t nof_symbols;           /* per occasion */
  uint32_t window_samples;        /* the smallest input length per port: the end of the last occasion, and for the short formats
                                     not less than get_prach_window_duration */
} nrphy_prach_demod_sizes_t;
typedef struct nrphy_prach_demod_plan nrphy_prach_demod_plan_t;
/* NRPHY_OK, or NRPHY_ERR_ARGUMENT for what the reference asserts on: an unknown format or numerology; no time-domain occasion, more
 * than one on a long format, more short ones than fit the slot from start_symbol (a start symbol above 13); no frequency-domain
 * occasion or more than 8; a reserved (RA spacing, PUSCH spacing) row of the mapping table; a sampling rate that is no multiple of
 * the RA spacing or whose srate / ra_scs is not a size nrphy_dft_run supports; a dft_size not above the grid; a last
 * frequency-domain occasion with k_start + L_RA >= grid; a start, prefix, length or window that is not a whole number of samples at
 * the rate (phy_time_unit::is_sample_accurate); ports outside 1..4 or PRB outside 1..275.  No device work. */
int nrphy_prach_demod_validate(const nrphy_prach_demod_cfg_t* cfg);
/* NRPHY_ERR_ARGUMENT (sizes untouched) where nrphy_prach_demod_validate refuses the configuration.  No device work. */
int nrphy_prach_demod_sizes(const nrphy_prach_demod_cfg_t* cfg, nrphy_prach_demod_sizes_t* sizes);
/* n configurations; item i reads port p's complex f32 samples at element in_offset[i] + p * in_port_stride (window_samples of
 * them) of d_samples and writes element k < L_RA of (port p, frequency-domain occasion fd, time-domain occasion td, symbol s) to
 * element out_offset[i] + p * port_stride + fd * fd_stride + td * td_stride + s * symbol_stride + k of d_symbols: a prach_buffer
 * tensor (re, symbol, fd occasion, td occasion, port; re fastest) that nrphy_prach_plan_create reads in place, one (td, fd) occasion
 * per detector item.  Validates every configuration; all window and bin arithmetic happens here.  On an error *plan is NULL. */
int nrphy_prach_demod_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_prach_demod_cfg_t* cfgs, const uint64_t* in_offset,
                                  uint64_t in_port_stride, const uint64_t* out_offset, uint64_t port_stride, uint64_t fd_stride,
                                  uint64_t td_stride, uint64_t symbol_stride, nrphy_prach_demod_plan_t** plan);
int nrphy_prach_demod_plan_destroy(nrphy_prach_demod_plan_t* plan);
/* One workgroup per (item, port, time-domain occasion, symbol), one launch per transform size in the plan.  Writes the k < L_RA
 * elements of its items' (port, td, fd, symbol) and nothing else.  Asynchronous on `stream`; allocates nothing, touches no host
 * memory, uses no atomics (capturable; two runs give identical bytes).  The plan owns no scratch, so runs of one plan need no
 * ordering among themselves unless they write the same d_symbols: a split transform (dft_size above 6144) accumulates its partial
 * sums in the output elements themselves. */
int nrphy_prach_demod_run(nrphy_prach_demod_plan_t* plan, const void* d_samples, void* d_symbols, void* stream);
/* One configuration from and to host memory (blocking, on the GPU): samples hold port p at element p * in_port_stride
 * (window_samples each); symbols is addressed like d_symbols with out_offset 0, and the elements the run does not write keep what
 * the caller had there. */
int nrphy_prach_demodulate_host(nrphy_ctx_t* ctx, const nrphy_prach_demod_cfg_t* cfg, const void* samples, uint64_t in_port_stride,
                                void* symbols, uint64_t port_stride, uint64_t fd_stride, uint64_t td_stride, uint64_t symbol_stride);

/* ---- receive side: PUCCH formats 0 and 1 ----------------------------------------------------------------------------------
 * Replaces pucch_processor_impl::process for format0_configuration and format1_configuration
 * (R/lib/phy/upper/channel_processors/pucch_processor_impl.cpp:29-129): grid to HARQ-ACK, SR and channel state information.
 *
 * Format 0 (pucch_detector_format0::detect, pucch_detector_format0.cpp:66-202): one or two symbols of one PRB each (the second
 * symbol on second_hop_prb when there is one), the EPRE over every (symbol, port), and per candidate cyclic shift m_cs of the
 * reference's five tables (SR only; 1 or 2 ACK bits, each with and without an SR opportunity) the correlation with the
 * conjugate low-PAPR sequence: per (symbol, port) avg_pwr, corr = |sum / 12|^2 and noise_var = max(0, avg_pwr - corr), sum_corr
 * and sum_noise_var += noise_var corr accumulated symbol outer, port inner; metric = sum_corr^2 / sum_noise_var where that is a
 * normal number, else 0.  The best candidate wins by strict >, and is valid above 4.0.  SINR = 10 log10(best metric), RSRP from
 * the best candidate's sum_corr.
 *
 * Format 1: the estimator (dmrs_pucch_processor_format1_impl::estimate, dmrs_pucch_processor_format1_impl.cpp:158-222, on
 * port_channel_estimator_average_impl::compute with smoothing strategy `mean` and CFO compensation off, the setting of
 * signal_processor_factories.cpp:124-126) and the detector (pucch_detector_format1::detect, pucch_detector_format1.cpp:92-293).
 * Per receive port and hop: the LS products of the DM-RS symbols (even symbols of the allocation, z = w_i(m) r_uv^alpha), EPRE,
 * the CFO from the first two DM-RS symbols of the hop, the sum scaled by 1 / nof DM-RS symbols, its mean over the 12 pilots
 * (the estimate: one value per port and hop, rounded to cbf16), RSRP and the noise energy (noise_no_cfo); hops merged as compute
 * does (CFO averaged over the hops that have one, noise floor rsrp / 1e10).  The data symbols (odd symbols) are equalised by ZF
 * with beta 1 over the ports' estimates and noise variances -- the arithmetic of nrphy_channel_equalize --, multiplied by the
 * conjugate OCC (one per hop, of the hop's length) and low-PAPR sequence and averaged; detect_bits, threshold 4.0 and the status
 * of pucch_detector_format1.cpp:162-183 (`unknown` only with SR only and bit 1).  The channel state information is
 * channel_estimate::get_channel_state_information's: EPRE and RSRP averaged over the ports, CFO of the best-SNR port, the
 * layer-average SINR.
 *
 * Time alignment: the reference runs time_alignment_estimator_dft_impl on the smoothed pilots, which under the `mean` strategy
 * are 12 equal values c on consecutive subcarriers.  Their 4096-point inverse DFT has magnitude |c| |sin(12 pi n / 4096) /
 * sin(pi n / 4096)|, whose maximum over the searched bins [0, 144) and [3952, 4096) is at n = 0, 2.8e-5 (relative, in power)
 * above bins 1 and 4095 -- some hundreds of float32 ulps (6e-8) --, ties go to the delay side and an all-zero input returns
 * index 0.  Measured, not only argued: in the recording of the reference (tests/golden/record_pucch_reference.cpp: 146 format 1
 * cases of 4 to 14 symbols, 1 to 4 ports, PRBs 1 to 51, with and without hopping, on noisy two-tap channels, noise alone and a
 * zero grid) the reference's float32 transform put the peak in bin 0 in every one of the 1,240 per-port, per-hop calls and
 * per-port results, through the real path: the format 1 estimator, both hops and their halved sum.  So the time alignment is 0
 * whatever the grid holds, and no transform is computed.
 *
 * Group and sequence: u = n_id % 30, v = 0 (group hopping `neither`, as both reference detectors assert).  Cyclic shift
 * alpha_idx = (initial_cyclic_shift + m_cs + n_cs) % 12, n_cs from the Gold sequence with c_init = n_id
 * (R/include/srsran/phy/upper/pucch_helper.h:79-108), computed per symbol at plan creation.  Normal cyclic prefix only.  Receive
 * port i reads grid port rx_ports[i].  Format 2 is nrphy_pf2_* below; formats 3 and 4 and the srsRAN-side adaptor stay with the
 * caller. */
#define NRPHY_PUCCH_FORMAT_0 0u
#define NRPHY_PUCCH_FORMAT_1 1u
#define NRPHY_PUCCH_NO_HOP 0xFFFFFFFFu
#define NRPHY_PUCCH_STATUS_UNKNOWN 0u /* uci_status */
#define NRPHY_PUCCH_STATUS_VALID 1u
#define NRPHY_PUCCH_STATUS_INVALID 2u
typedef struct nrphy_pucch_cfg {
  uint32_t format;                    /* NRPHY_PUCCH_FORMAT_0 or _1 */
  uint32_t numerology;                /* 0..4 */
  uint32_t slot_index;                /* slot within the frame: < 10 * 2^numerology */
  uint32_t bwp_size_rb, bwp_start_rb; /* the PRBs below are relative to bwp_start_rb */
  uint32_t starting_prb;
  uint32_t second_hop_prb;            /* NRPHY_PUCCH_NO_HOP: no frequency hopping */
  uint32_t start_symbol_index, nof_symbols; /* format 0: 1..2 symbols; format 1: 4..14, start <= 10 */
  uint32_t initial_cyclic_shift;      /* m_0: 0..11 */
  uint32_t time_domain_occ;           /* format 1: 0..6 and below the number of data symbols of a hop; format 0: must be 0 */
  uint32_t n_id;                      /* 0..1023 */
  uint32_t nof_harq_ack;              /* 0..2 */
  uint32_t sr_opportunity;            /* format 0: 0 or 1 (with nof_harq_ack = 0 it must be 1); format 1: must be 0 */
  uint32_t nof_rx_ports;              /* 1..4 */
  uint32_t rx_ports[NRPHY_MAX_PORTS]; /* grid port of receive port i */
  uint32_t reserved_;
} nrphy_pucch_cfg_t;
typedef struct nrphy_pucch_result { /* one per PUCCH */
  uint32_t status;                    /* NRPHY_PUCCH_STATUS_* */
  uint32_t harq_ack[2];               /* the first nof_harq_ack entries; the others 0 */
  uint32_t sr;                        /* format 0 with an SR opportunity: the SR bit; else 0 */
  float    detection_metric;          /* format 1: metric / 4; format 0: the best metric */
  float    sinr_dB, rsrp_dB, epre_dB;
  float    time_alignment_s;          /* 0 (see above) */
  float    cfo_hz;                    /* NaN where the reference has none: format 0, and hops of a single DM-RS symbol */
} nrphy_pucch_result_t;
typedef struct nrphy_pucch_plan nrphy_pucch_plan_t;
/* NRPHY_OK, or NRPHY_ERR_ARGUMENT for what pucch_pdu_validator_impl::is_valid and the two detectors' assertions refuse: an
 * unknown format; bwp_start_rb + bwp_size_rb beyond the grid; starting_prb or second_hop_prb outside the BWP; symbols beyond
 * the slot; format 0 with other than 1 or 2 symbols; format 1 with start_symbol_index above 10 or other than 4 to 14 symbols;
 * an initial cyclic shift above 11; n_id above 1023; more than 2 ACK bits; format 0 without payload (no ACK bit and no SR
 * opportunity) or an sr_opportunity other than 0 or 1; time_domain_occ above 6 or not below the number of data symbols of the
 * (first) hop, or non-zero for format 0; sr_opportunity set for format 1; no rx port, more than 4, one outside the grid or
 * repeated; numerology above 4 or slot_index >= 10 * 2^numerology.  No device work. */
int nrphy_pucch_validate(const nrphy_pucch_cfg_t* cfg, uint32_t grid_nof_ports, uint32_t grid_nof_subc);
/* n PUCCHs of either format; PUCCH i reads grid grid_index[i] of [nof_grids][grid_nof_ports][14][grid_nof_subc] cbf16: the
 * convention of nrphy_pusch_chest_plan_create, one uplink grid buffer feeds PUSCH and PUCCH.  ce_offset may be NULL; where it
 * is not, a format 1 PUCCH writes its estimate at element ce_offset[i] of d_ch_est: [rx port i][14][grid_nof_subc] cbf16.
 * Validates every configuration, computes n_cs per symbol and uploads the descriptors and the sequence tables (blocking). */
int nrphy_pucch_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pucch_cfg_t* cfgs, const uint32_t* grid_index,
                            uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc, const uint64_t* ce_offset,
                            nrphy_pucch_plan_t** plan);
int nrphy_pucch_plan_destroy(nrphy_pucch_plan_t* plan);
/* d_result: [n].  d_meas (may be NULL): [n][NRPHY_MAX_PORTS], format 1's per-port measurements in the layout of
 * nrphy_pusch_chest_meas_t, with ta_s and ta_bins 0; zeros for format 0 and for ports the PUCCH does not have.  d_ch_est (may be
 * NULL; needs a plan created with ce_offset): format 1 writes the 12 subcarriers of the hop's PRB on symbols [start, start +
 * nof) of every receive port and nothing else.  One wavefront per PUCCH.  Asynchronous on `stream`; allocates nothing,
 * touches no host memory, uses no atomics and no scratch (capturable; two runs give identical bytes). */
int nrphy_pucch_run(nrphy_pucch_plan_t* plan, const void* d_grid, nrphy_pucch_result_t* d_result,
                    nrphy_pusch_chest_meas_t* d_meas, void* d_ch_est, void* stream);
/* One PUCCH from and to host memory (blocking, on the GPU): grid [grid_nof_ports][14][grid_nof_subc] cbf16 -> result; meas
 * [nof_rx_ports] (may be NULL); ch_est [nof_rx_ports][14][grid_nof_subc] cbf16 (may be NULL; format 1 writes its region). */
int nrphy_pucch_host(nrphy_ctx_t* ctx, const nrphy_pucch_cfg_t* cfg, const void* grid, uint32_t grid_nof_ports,
                     uint32_t grid_nof_subc, nrphy_pucch_result_t* result, nrphy_pusch_chest_meas_t* meas, void* ch_est);

/* ---- receive side: UCI decoder (short blocks and polar) -----------------------------------------------------------------------
 * Replaces uci_decoder_impl::decode (R/lib/phy/upper/channel_processors/uci/uci_decoder_impl.cpp): the soft bits of one UCI
 * message (HARQ-ACK, CSI part 1 or part 2 taken out of a PUSCH codeword, or a PUCCH format 2 payload: nrphy_pf2_run) to its bits and a
 * status.  Everything is integer arithmetic on int8 soft bits in the reference's domain -- finite values -120..120 and +-127 for
 * infinity --, so the result equals the reference's bit for bit.
 *
 * 1 to 11 bits: short_block_detector_impl::detect (R/lib/phy/upper/channel_coding/short/short_block_detector_impl.cpp).  The rate
 * de-matcher adds the repetitions of each position in ascending order with the saturating sum; an all-zero input gives an all-ones
 * message and INVALID; 1 bit is the sign of the first soft bit (always VALID), 2 bits the best of the four 3-bit codewords over the
 * soft bits the modulation's placement leaves, 3 to 11 bits the first of the 2^(A-1) even-valued codewords of the (32, A) code of
 * TS 38.212 Table 5.3.3.3-1 with the largest |correlation|, whose sign is bit 0.  VALID when the reference's detection metric
 * exceeds its threshold, decided in integers.
 *
 * 12 to 1706 bits: per block (two when A >= 1013, or A >= 360 with E >= 1088; an odd A then gives the first block one filler bit)
 * the channel de-interleaver, bit de-selection (repetitions added with the promoting sum, punctured positions 0, shortened ones
 * +127), the sub-block de-interleaver, the simplified successive cancellation decoder of polar_decoder_impl on the code of
 * polar_code_impl::set(K, E, 10) -- parity-check positions for K = 18..25, which the decoder treats as information and the
 * de-allocator skips --, and the 6- or 11-bit CRC over filler, message and CRC.  VALID when the remainder is 0.  The message is
 * written whether or not the CRC holds.  A failed first block ends the message: status INVALID and the second block's
 * ceil(A / 2) bytes are NOT written, they keep what the buffer held; a failed second block gives INVALID too. */
#define NRPHY_UCI_STATUS_UNKNOWN 0u /* uci_status */
#define NRPHY_UCI_STATUS_VALID 1u
#define NRPHY_UCI_STATUS_INVALID 2u
typedef struct nrphy_uci_decoder_cfg {
  uint32_t message_length; /* A, 1..1706 payload bits */
  uint32_t llr_length;     /* E, soft bits of this message */
  uint32_t modulation;     /* NRPHY_MOD_*; only read for A <= 2 */
  uint32_t reserved_;
} nrphy_uci_decoder_cfg_t;
typedef struct nrphy_uci_decoder_plan nrphy_uci_decoder_plan_t;
/* NRPHY_OK, or NRPHY_ERR_ARGUMENT for what the reference asserts on: A outside 1..1706; for A <= 2 an unknown modulation or E
 * below its bits per symbol; for A in 3..11 E <= A; for A >= 12, per block of K = ceil(A / C) + CRC bits and E / C soft bits, what
 * polar_code_impl::set refuses: K outside 18..25 and 31..1023, more than 8192 soft bits, K + 3 >= E (K <= 25) or K >= E, K not
 * below the code length.  No device work. */
int nrphy_uci_decoder_validate(const nrphy_uci_decoder_cfg_t* cfg);
/* n messages of any mix of sizes; message i reads llr_length soft bits at d_llr + llr_offset[i] and writes message_length bytes
 * (one bit each) at d_message + message_offset[i].  Validates every configuration, builds each distinct polar code (K, E) once and
 * uploads the tables (blocking). */
int nrphy_uci_decoder_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_uci_decoder_cfg_t* cfgs, const uint64_t* llr_offset,
                                  const uint64_t* message_offset, nrphy_uci_decoder_plan_t** plan);
int nrphy_uci_decoder_plan_destroy(nrphy_uci_decoder_plan_t* plan);
/* d_status: [n] NRPHY_UCI_STATUS_*.  One launch, one wavefront per message.  Asynchronous on `stream`; allocates nothing, touches no
 * host memory, uses no atomics and no scratch (capturable; two runs give identical bytes). */
int nrphy_uci_decoder_run(nrphy_uci_decoder_plan_t* plan, const int8_t* d_llr, uint8_t* d_message, uint32_t* d_status, void* stream);
/* One message from and to host memory (blocking, on the GPU).  `message` is read as well: bytes the decoder does not write (the
 * second block behind a failed first one) come back as they went in.  Makes and releases a one-message plan inside the call (code
 * construction, an allocation and a blocking upload each time): for more than a few messages make one plan over all of them. */
int nrphy_uci_decode_host(nrphy_ctx_t* ctx, const nrphy_uci_decoder_cfg_t* cfg, const int8_t* llr, uint8_t* message,
                          uint32_t* status);

/* ---- receive side: PUCCH format 2 -----------------------------------------------------------------------------------------------
 * Replaces pucch_processor_impl::process for format2_configuration
 * (R/lib/phy/upper/channel_processors/pucch_processor_impl.cpp:131-215): grid to UCI payload, status and channel state
 * information.  (The names say pf2: the nrphy_pucch_* calls above stay the format 0 and 1 receivers.)
 *
 * DM-RS (dmrs_pucch_processor_format2_impl.cpp): pilots on subcarriers 1, 4, 7 and 10 of every PRB of every symbol of the
 * allocation; per symbol l the Gold sequence with c_init = ((14 n_slot + l + 1)(2 n_id_0 + 1) 2^17 + 2 n_id_0) mod 2^31, advanced by
 * 8 (bwp_start_rb + starting_prb) bits, as QPSK of amplitude 1 / sqrt(2), real part from the even bits.
 *
 * Estimator: port_channel_estimator_average_impl::compute per receive port with the `filter` smoothing strategy and CFO
 * compensation on (the factory's defaults), one layer, one hop, beta 1 -- the steps of nrphy_pusch_chest_run with pilots every
 * third subcarrier: LS products and EPRE; with two symbols the CFO from their dot product, derotation and sum; scale 1 /
 * nof_symbols; filter_type(min(nof_prb, 3), 3) = 3, 7 or 11 taps; 4, 3 or 5 virtual pilots per side for 1, 2 or more PRBs;
 * convolution_same; RSRP; noise energy (with the CFO phasor when there is one), noise variance floored at rsrp / 1e10, SNR; time
 * alignment from the 4096-point inverse DFT of the pilots at their grid subcarriers, bins [0, 144) against [3952, 4096), delay on
 * ties; linear interpolation with offset 1 and stride 3 (interpolator_linear_impl.cpp:58-78: the first two outputs hold pilot 0,
 * then a running sum of (next - this) / 3 that carries on from the accumulated value, the last output holds the last pilot);
 * cbf16 rounding; per symbol the product with the CFO phasor, rounded again.
 *
 * Demodulator (pucch_demodulator_impl.cpp:31-87): the data REs are the subcarriers k with k mod 3 != 1, symbol by symbol and
 * ascending; ZF over the ports with tx_scaling 1 and the ports' noise variances (the arithmetic of nrphy_channel_equalize), the
 * QPSK demapper of nrphy_demodulate_soft over one span of all data REs, descrambling with c_init = rnti 2^15 + n_id: E = 16
 * nof_prb nof_symbols soft bits, those of equalise -> nrphy_demodulate_soft -> nrphy_llr_descramble on the estimate and noise
 * variances the same run writes out.  Decoder: nrphy_uci_decoder_run with QPSK over A = nof_harq_ack + nof_sr + nof_csi_part1
 * bits, in that order.  Channel state information: channel_estimate::get_channel_state_information's, as for format 1, with the
 * best-SNR port's time alignment.  Normal cyclic prefix only.  Receive port i reads grid port rx_ports[i]. */
typedef struct nrphy_pf2_cfg {
  uint32_t numerology;                /* 0..4 */
  uint32_t slot_index;                /* slot within the frame: < 10 * 2^numerology */
  uint32_t bwp_size_rb, bwp_start_rb; /* starting_prb is relative to bwp_start_rb */
  uint32_t starting_prb, nof_prb;     /* nof_prb: 1..16 */
  uint32_t start_symbol_index, nof_symbols; /* 1..2 symbols */
  uint32_t rnti;                      /* 0..65535 */
  uint32_t n_id;                      /* data scrambling identity, 0..1023 */
  uint32_t n_id_0;                    /* DM-RS scrambling identity, 0..65535 */
  uint32_t nof_harq_ack, nof_sr, nof_csi_part1;
  uint32_t nof_csi_part2;             /* must be 0 */
  uint32_t nof_rx_ports;              /* 1..4 */
  uint32_t rx_ports[NRPHY_MAX_PORTS]; /* grid port of receive port i */
} nrphy_pf2_cfg_t;
typedef struct nrphy_pf2_csi { /* one per PUCCH: channel_state_information */
  float    sinr_dB, rsrp_dB, epre_dB;
  float    time_alignment_s;          /* of the receive port with the best SNR */
  float    cfo_hz;                    /* of the same port; NaN with one symbol */
  uint32_t reserved_[3];
} nrphy_pf2_csi_t;
typedef struct nrphy_pf2_plan nrphy_pf2_plan_t;
/* NRPHY_OK, or NRPHY_ERR_ARGUMENT for what pucch_pdu_validator_impl::is_valid(format2_configuration), assert_format2_config and
 * the demodulator's assertions refuse: bwp_start_rb + bwp_size_rb beyond the grid; starting_prb + nof_prb beyond the BWP; nof_prb
 * outside 1..16; other than 1 or 2 symbols, or symbols beyond the slot; nof_csi_part2 other than 0; A = nof_harq_ack + nof_sr +
 * nof_csi_part1 outside 3..1706; an effective code rate float(A + CRC bits) / float(E) above 0.8f; and whatever
 * nrphy_uci_decoder_validate refuses for (A, E, QPSK).  Also: no rx port, more than 4, one outside the grid or repeated;
 * numerology above 4 or slot_index >= 10 * 2^numerology; rnti or n_id_0 above 65535, n_id above 1023.  No device work. */
int nrphy_pf2_validate(const nrphy_pf2_cfg_t* cfg, uint32_t grid_nof_ports, uint32_t grid_nof_subc);
/* E = 16 nof_prb nof_symbols soft bits and A payload bits of a configuration nrphy_pf2_validate accepts (any grid). */
int nrphy_pf2_sizes(const nrphy_pf2_cfg_t* cfg, uint32_t* nof_llr, uint32_t* nof_payload_bits);
/* n PUCCHs; PUCCH i reads grid grid_index[i] of [nof_grids][grid_nof_ports][14][grid_nof_subc] cbf16 (the convention of
 * nrphy_pucch_plan_create: one uplink grid buffer feeds PUSCH and every PUCCH format; grid_nof_subc a multiple of 4), writes its
 * E soft bits at d_llr + llr_offset[i] and its A payload bits, one per byte, at d_message + message_offset[i].  ce_offset may be
 * NULL; where it is not, PUCCH i writes its estimate at element ce_offset[i] of d_ch_est: [rx port i][14][grid_nof_subc] cbf16.
 * Validates every configuration, computes the DM-RS and scrambling seeds, the taps and the epochs, and makes one UCI decoder plan
 * over the n messages (nrphy_uci_decoder_plan_create) (blocking). */
int nrphy_pf2_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pf2_cfg_t* cfgs, const uint32_t* grid_index, uint32_t nof_grids,
                          uint32_t grid_nof_ports, uint32_t grid_nof_subc, const uint64_t* llr_offset,
                          const uint64_t* message_offset, const uint64_t* ce_offset, nrphy_pf2_plan_t** plan);
int nrphy_pf2_plan_destroy(nrphy_pf2_plan_t* plan);
/* Two launches on `stream`: the receiver (one workgroup per PUCCH), then the UCI decoder reading d_llr in place.  d_grid: 16-byte
 * aligned.  d_status: [n] NRPHY_UCI_STATUS_*; d_message and d_status may both be NULL: the receiver launch alone, for a caller
 * that decodes d_llr with a UCI decoder plan of its own.  d_csi: [n]; d_meas (may be NULL): [n][NRPHY_MAX_PORTS], the per-port measurements
 * (zeros for ports the PUCCH does not have); d_ch_est (may be NULL; needs a plan created with ce_offset): the 12 nof_prb
 * subcarriers of the allocation on its symbols for every receive port, and nothing else -- exactly the words the soft bits were
 * equalised with, as d_meas holds exactly the noise variances.  Asynchronous; allocates nothing, touches no host memory, uses no
 * atomics and no scratch (capturable; two runs give identical bytes). */
int nrphy_pf2_run(nrphy_pf2_plan_t* plan, const void* d_grid, int8_t* d_llr, uint8_t* d_message, uint32_t* d_status,
                  nrphy_pf2_csi_t* d_csi, nrphy_pusch_chest_meas_t* d_meas, void* d_ch_est, void* stream);
/* One PUCCH from and to host memory (blocking, on the GPU): grid [grid_nof_ports][14][grid_nof_subc] cbf16 -> message [A] (read
 * as well: see nrphy_uci_decode_host), status, csi; meas [nof_rx_ports] (may be NULL); ch_est [nof_rx_ports][14][grid_nof_subc]
 * cbf16 (may be NULL; only the allocation is written); llr [E] (may be NULL). */
int nrphy_pf2_host(nrphy_ctx_t* ctx, const nrphy_pf2_cfg_t* cfg, const void* grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                   uint8_t* message, uint32_t* status, nrphy_pf2_csi_t* csi, nrphy_pusch_chest_meas_t* meas, void* ch_est,
                   int8_t* llr);

/* ---- receive side: SRS channel estimator ----------------------------------------------------------------------------------------
 * Replaces srs_estimator_generic_impl::estimate (R/lib/phy/upper/signal_processors/srs/srs_estimator_generic_impl.cpp:62-193):
 * grid to the wideband channel matrix and the time alignment of one sounding reference signal.
 *
 * Mapping (get_srs_information, R/lib/ran/srs/srs_information.cpp:39-105): m_SRS and N from TS 38.211 Table 6.4.1.4.3-1; sequence
 * length M = 12 m_SRS / comb; group u = sequence_id mod 30, number 0; n_cs_max = 8 (comb 2) or 12 (comb 4); antenna port p has
 * cyclic shift (cyclic_shift + n_cs_max p / nof_antenna_ports) mod n_cs_max and sits on subcarriers k0 + comb n, n < M, with
 * k0 = 12 freq_shift + k_TC + sum_b comb M_b ((4 freq_position / m_SRS,b) mod N_b); ports 1 and 3 of a four-port SRS whose
 * cyclic shift is at least n_cs_max / 2 take k_TC = (comb_offset + comb / 2) mod comb.
 *
 * Sequence (low_papr_sequence_generator_impl): r(n) = table[arg(n)] with the table polar(1, float(2 pi) n / size) -- size 8 and
 * arg = phi(n) of TS 38.211 Table 5.2.2.2-2 / -4 for M = 12 / 24; size 2 N_zc and arg = -(q m (m + 1) mod 2 N_zc), m = n mod N_zc,
 * N_zc the largest prime below M, for M >= 36 --, times entry (n n_cs 24 / n_cs_max) mod 24 of the 24-point unit circle where
 * the port's cyclic shift is not 0.
 *
 * Estimate: per receive port and antenna port the LS products y conj(r) of every symbol, added in symbol order and scaled by
 * float(1.0 / nof_symbols) when there is more than one symbol; the time alignment of each path from the 4096-point inverse DFT of
 * the products at inputs comb n: the largest |X|^2 of bins [0, W) against bins [4096 - W, 4096), W = floor(4096 / (n_cs_max
 * comb)) = 256 or 85, the lower bin among equals, the delay on ties; their average in double, antenna port outer and receive port
 * inner; then the products times entry round(1024 (n ps + offset) / 2 pi) mod 1024 of the 1024-point unit circle with ps =
 * float(2 pi ta scs comb) and offset = ps (k0 mod comb) / comb, the index evaluated in single precision operation by operation;
 * their mean is the coefficient.  The reference never writes noise_variance: it is not part of the result.  Normal cyclic
 * prefix.  Receive port i reads grid port rx_ports[i]. */
typedef struct nrphy_srs_cfg {
  uint32_t numerology;                /* 0..4 */
  uint32_t nof_antenna_ports;         /* 1, 2, 4 */
  uint32_t nof_symbols;               /* 1, 2, 4 */
  uint32_t start_symbol;              /* start_symbol + nof_symbols <= 14 */
  uint32_t configuration_index;       /* C_SRS, 0..63 */
  uint32_t sequence_id;               /* 0..1023 */
  uint32_t bandwidth_index;           /* B_SRS, 0..3 */
  uint32_t comb_size;                 /* 2, 4 */
  uint32_t comb_offset;               /* < comb_size */
  uint32_t cyclic_shift;              /* 0..7 with comb 2, 0..11 with comb 4 */
  uint32_t freq_position;             /* n_RRC, 0..67 */
  uint32_t freq_shift;                /* n_shift, 0..268 */
  uint32_t freq_hopping;              /* b_hop, 0..3; must not be below bandwidth_index (no frequency hopping) */
  uint32_t hopping;                   /* group or sequence hopping: must be 0 */
  uint32_t nof_rx_ports;              /* 1..4 */
  uint32_t rx_ports[NRPHY_MAX_PORTS]; /* grid port of receive port i */
} nrphy_srs_cfg_t;
typedef struct nrphy_srs_result { /* one per SRS */
  float   h_re[4][4], h_im[4][4];     /* [rx][tx]; zeros beyond the configured ports */
  int32_t ta_bins[4][4];              /* [rx][tx]: the path's time alignment in bins of the 4096-point inverse DFT (1 / (4096 scs)
                                         seconds each), negative for an advance; zeros beyond the configured ports */
  double  time_alignment_s;           /* the average over the paths */
  uint32_t reserved_[2];
} nrphy_srs_result_t;
typedef struct nrphy_srs_plan nrphy_srs_plan_t;
/* NRPHY_OK, or NRPHY_ERR_ARGUMENT for what srs_validator_generic_impl::is_valid refuses -- a comb offset not below the comb size,
 * a cyclic shift above 7 with comb 2, freq_hopping < bandwidth_index, hopping != 0, no receive port -- and for what the
 * estimator's assertions refuse: symbols beyond the slot; a field outside its range; port or symbol counts other than 1, 2 or 4;
 * a comb other than 2 or 4; more than 4 receive ports, a repeated one or one outside the grid; a last subcarrier k0 + comb (M - 1)
 * beyond the grid for any antenna port.  No device work. */
int nrphy_srs_validate(const nrphy_srs_cfg_t* cfg, uint32_t grid_nof_ports, uint32_t grid_nof_subc);
/* The values of get_srs_information for one antenna port of a configuration whose fields are in range (the grid is not looked at):
 * sequence length M, first subcarrier k0, the port's cyclic shift and its maximum, the sequence group.  No device work. */
int nrphy_srs_info(const nrphy_srs_cfg_t* cfg, uint32_t antenna_port, uint32_t* sequence_length, uint32_t* initial_subcarrier,
                   uint32_t* n_cs, uint32_t* n_cs_max, uint32_t* u);
/* n SRS; SRS i reads grid grid_index[i] of [nof_grids][grid_nof_ports][14][grid_nof_subc] cbf16, the buffer nrphy_pusch_chest_run,
 * nrphy_pucch_run and nrphy_pf2_run read.  Validates every configuration and computes everything that does not depend on the
 * grid: per antenna port M, k0 and the cyclic-shift step, N_zc and the Zadoff-Chu root (in single precision, as zc_sequence_q
 * does), the search window, the unit circles (blocking). */
int nrphy_srs_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_srs_cfg_t* cfgs, const uint32_t* grid_index, uint32_t nof_grids,
                          uint32_t grid_nof_ports, uint32_t grid_nof_subc, nrphy_srs_plan_t** plan);
int nrphy_srs_plan_destroy(nrphy_srs_plan_t* plan);
/* Two launches on `stream`, each of one workgroup per (SRS, receive port, antenna port): the per-path time alignment, then the
 * common time alignment, its compensation and the coefficients.  d_result: [n], 8-byte aligned; every byte of it is written.
 * Asynchronous; allocates nothing, touches no host memory, uses no atomics and no scratch (capturable; two runs give identical
 * bytes). */
int nrphy_srs_run(nrphy_srs_plan_t* plan, const void* d_grid, nrphy_srs_result_t* d_result, void* stream);
/* One SRS from and to host memory (blocking, on the GPU): grid [grid_nof_ports][14][grid_nof_subc] cbf16 -> result. */
int nrphy_srs_host(nrphy_ctx_t* ctx, const nrphy_srs_cfg_t* cfg, const void* grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                   nrphy_srs_result_t* result);
/* The low-PAPR sequence of one antenna port, cyclic shift included, from the device generator the estimator's kernels use
 * (blocking): out [M] complex float (re, im). */
int nrphy_srs_sequence_host(nrphy_ctx_t* ctx, const nrphy_srs_cfg_t* cfg, uint32_t antenna_port, float* out);

/* ---- receive side: UL-SCH demultiplexer (UCI on PUSCH, TS 38.212 Section 6.2.7) -----------------------------------------------
 * Replaces ulsch_demultiplex::demultiplex + set_csi_part2 and the pusch_codeword_buffer it returns
 * (R/lib/phy/upper/channel_processors/pusch/ulsch_demultiplex_impl.cpp): the descrambled soft bits of a codeword, as
 * nrphy_pusch_demod_run writes them (symbol by symbol, subcarrier ascending, nof_layers * Qm per resource element), to the four
 * streams the reference hands to its decoder buffers, in its order.  The UL-SCH stream goes to nrphy_pusch_decode_batch, the other
 * three to nrphy_uci_decoder_run, on the same stream with no host step.  HARQ-ACK of 1 or 2 bits punctures: its REs stay in the
 * UL-SCH stream (or in CSI part 2, where that took a reserved RE) as zeros.  Streams whose payload is 1 or 2 bits get the
 * placeholder corrections of on_uci_placeholder_1bit / _2bit, which re-apply or swap scrambling signs; they need rnti and n_id.
 * The fields are ulsch_demultiplex::configuration plus set_csi_part2's sizes, which have to be known when the plan is made: this
 * equals the reference when set_csi_part2 precedes the first block.  Deriving them from a decoded CSI part 1 is the caller's
 * business (a second plan).  Soft bits are expected in the reference's domain, -127..127. */
typedef struct nrphy_ulsch_demux_cfg {
  uint32_t modulation, nof_layers, nof_prb, start_symbol_index, nof_symbols; /* NRPHY_MOD_*; 1..4; 1..275; symbols of the slot */
  uint32_t dmrs_type, dmrs_symbol_mask, nof_cdm_groups_without_data; /* 0 = type 1, 1 = type 2; bit l = symbol l carries DM-RS */
  uint32_t nof_harq_ack_rvd;                                         /* G^ACK_rvd, soft bits reserved for HARQ-ACK of <= 2 bits */
  uint32_t nof_harq_ack_bits, nof_enc_harq_ack_bits;                 /* O^ACK, G^ACK */
  uint32_t nof_csi_part1_bits, nof_enc_csi_part1_bits;
  uint32_t nof_csi_part2_bits, nof_enc_csi_part2_bits; /* known when the plan is made; 0 = none */
  uint32_t rnti, n_id;                                 /* the codeword's scrambling, as the demodulator's */
} nrphy_ulsch_demux_cfg_t;
typedef struct nrphy_ulsch_demux_sizes {
  uint32_t nof_sch_bits, nof_codeword_bits; /* soft bits of the UL-SCH stream (zeroed ones included) and of the input */
} nrphy_ulsch_demux_sizes_t;
typedef struct nrphy_ulsch_demux_plan nrphy_ulsch_demux_plan_t;
/* NRPHY_OK, or NRPHY_ERR_ARGUMENT for what the reference asserts on or cannot finish: an unknown modulation; layers outside 1..4;
 * PRBs outside 1..275; symbols beyond the slot; a DM-RS type above 1 or CDM groups without data outside 1..2 (type 1) or 1..3
 * (type 2); a DM-RS mask without a DM-RS symbol, without a later symbol free of DM-RS, or with bits above symbol 13; a UCI part
 * with payload bits but no soft bits or the reverse; soft bits of a part that the placement cannot take exactly (not a multiple
 * of nof_layers * Qm, or more than the symbols hold: on_end_codeword's assertions).  Also refused, because the reference's
 * unsigned arithmetic goes wrong there: a reserved set next to HARQ-ACK of more than 2 bits.  No device work. */
int nrphy_ulsch_demux_validate(const nrphy_ulsch_demux_cfg_t* cfg);
int nrphy_ulsch_demux_sizes(const nrphy_ulsch_demux_cfg_t* cfg, nrphy_ulsch_demux_sizes_t* sizes);
/* n codewords of any mix of configurations; codeword i reads nof_codeword_bits soft bits at d_codeword_llr + in_offset[i] and
 * writes its streams at d_sch + sch_offset[i], d_harq_ack + harq_offset[i], d_csi1 + csi1_offset[i], d_csi2 + csi2_offset[i]
 * (nof_sch_bits and the nof_enc_* bits of the configuration).  An offset array may be NULL when no codeword has that part.
 * rnti up to 65535, n_id up to 1023.  The placement is computed here and uploaded as an index table, 4 bytes per resource
 * element (blocking).  Offsets that are multiples of 16 let the kernel move 16 bytes per thread. */
int nrphy_ulsch_demux_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_ulsch_demux_cfg_t* cfgs, const uint64_t* in_offset,
                                  const uint64_t* sch_offset, const uint64_t* harq_offset, const uint64_t* csi1_offset,
                                  const uint64_t* csi2_offset, nrphy_ulsch_demux_plan_t** plan);
int nrphy_ulsch_demux_plan_destroy(nrphy_ulsch_demux_plan_t* plan);
/* One launch.  A stream pointer may be NULL when no codeword of the plan has that part.  Every byte of every stream is written.
 * Asynchronous on `stream`; allocates nothing, touches no host memory, uses no atomics and no scratch (capturable; two runs give
 * identical bytes). */
int nrphy_ulsch_demux_run(nrphy_ulsch_demux_plan_t* plan, const int8_t* d_codeword_llr, int8_t* d_sch, int8_t* d_harq_ack,
                          int8_t* d_csi1, int8_t* d_csi2, void* stream);
/* One codeword from and to host memory (blocking, on the GPU).  Makes and releases a plan inside the call. */
int nrphy_ulsch_demultiplex_host(nrphy_ctx_t* ctx, const nrphy_ulsch_demux_cfg_t* cfg, const int8_t* codeword_llr, int8_t* sch,
                                 int8_t* harq_ack, int8_t* csi1, int8_t* csi2);

/* ---- other downlink grid writers ("next" row): NZP-CSI-RS generator -----------
 * Replaces nzp_csi_rs_generator::map (R/include/srsran/phy/upper/signal_processors/nzp_csi_rs_generator.h:
 * 39-90; impl R/lib/phy/upper/signal_processors/nzp_csi_rs_generator_impl.cpp:96-352 with the RE patterns of
 * R/lib/ran/csi_rs/csi_rs_pattern.cpp and resource_grid_mapper_impl::map, resource_grid_mapper_impl.cpp:
 * 150-277).  The fields are nzp_csi_rs_generator::config_t.  Rows 1 to 5 of TS 38.211 Table 7.4.1.5.3-1 (1, 1,
 * 2, 4, 4 ports: what a grid of NRPHY_MAX_PORTS ports can carry); density and CDM type must be the ones the
 * row allows.  Every CDM group writes its resource elements on ALL ports of the precoding (zeros where the
 * weights are zero), as the reference does. */
typedef struct nrphy_csi_rs_cfg {
  uint32_t slot_index;       /* slot within the frame */
  uint32_t cp;               /* 0 normal, 1 extended */
  uint32_t start_rb;
  uint32_t nof_rb;
  uint32_t row;              /* csi_rs_mapping_table_row, 1..5 */
  uint32_t nof_k_ref;
  uint32_t k_ref[6];         /* freq_allocation_ref_idx */
  uint32_t symbol_l0;
  uint32_t symbol_l1;        /* unused by rows 1..5 */
  uint32_t cdm;              /* csi_rs_cdm_type: 0 no_CDM, 1 fd_CDM2 */
  uint32_t density;          /* csi_rs_freq_density_type: 0 dot5_even_RB, 1 dot5_odd_RB, 2 one, 3 three */
  uint32_t scrambling_id;
  float    amplitude;
  uint32_t nof_ports;        /* ports of the row = ports and layers of the precoding */
  uint32_t prg_size_rb;
  uint32_t nof_prg;          /* must be 1: the reference's generator only handles wideband precoding */
  const float* precoding;    /* [nof_ports][nof_ports] complex: coefficient(layer, port) at [port][layer] */
} nrphy_csi_rs_cfg_t;
/* NRPHY_OK when the configuration is one this library maps (the reference's validator accepts everything). */
int nrphy_csi_rs_validate(const nrphy_csi_rs_cfg_t* cfg);
/* n signals into device grids ([grid][port][14][subc] cbf16): signal i into grid grid_index[i].  The
 * configurations are copied at the call (host pointers, like PDUs at plan creation) into a staging buffer of
 * the call's own (stream-ordered allocation on `stream`); the kernel itself is asynchronous. */
int nrphy_csi_rs_map(nrphy_ctx_t* ctx, uint32_t n, const nrphy_csi_rs_cfg_t* cfgs, const uint32_t* grid_index,
                     void* d_grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc, void* stream);
/* One signal into a host grid [nof_ports][14][nof_subc] cbf16 (read and written; blocking). */
int nrphy_csi_rs_map_host(nrphy_ctx_t* ctx, const nrphy_csi_rs_cfg_t* cfg, void* grid, uint32_t nof_ports,
                          uint32_t nof_subc);

/* ---- other downlink grid writers: PDCCH processor ------------------------------------
 * Replaces pdcch_processor::process (R/include/srsran/phy/upper/channel_processors/pdcch_processor.h:47-151;
 * impl R/lib/phy/upper/channel_processors/pdcch_processor_impl.cpp:66-118) with everything behind it: the
 * CCE-to-REG mapping (R/lib/ran/pdcch/cce_to_prb_mapping.cpp), pdcch_encoder_impl (CRC24C with the RNTI mask, polar
 * interleaver / allocator / encoder / rate matcher: pdcch_encoder_impl.cpp:33-98, channel_coding/polar/), pdcch_modulator_impl
 * (scrambling, QPSK, precoding, mapping: pdcch_modulator_impl.cpp:30-90) and dmrs_pdcch_processor_impl
 * (R/lib/phy/upper/signal_processors/dmrs_pdcch_processor_impl.cpp:32-102).  The fields are pdcch_processor::pdu_t:
 * coreset_description + dci_description.  Precoding has one layer: [nof_prg][nof_ports] complex weights. */
#define NRPHY_PDCCH_MAX_PAYLOAD 128 /* pdcch_constants::MAX_DCI_PAYLOAD_SIZE */
typedef struct nrphy_pdcch_pdu {
  uint32_t slot_index;         /* slot within the radio frame (DM-RS c_init) */
  uint32_t cp;                 /* 0 normal, 1 extended */
  /* coreset_description */
  uint32_t bwp_size_rb;
  uint32_t bwp_start_rb;
  uint32_t start_symbol_index;
  uint32_t duration;           /* 1..3 */
  uint64_t frequency_resources; /* bit i = PRBs [6i, 6i + 6) of the BWP belong to the CORESET (45 bits) */
  uint32_t cce_to_reg_mapping; /* 0 CORESET0, 1 non-interleaved, 2 interleaved */
  uint32_t reg_bundle_size;    /* L, interleaved only */
  uint32_t interleaver_size;   /* R, interleaved only */
  uint32_t shift_index;        /* n_shift (interleaved), physical cell id (CORESET0) */
  /* dci_description */
  uint32_t rnti;
  uint32_t n_id_pdcch_dmrs;
  uint32_t n_id_pdcch_data;
  uint32_t n_rnti;
  uint32_t cce_index;
  uint32_t aggregation_level;  /* 1, 2, 4, 8, 16 */
  float    dmrs_power_offset_dB;
  float    data_power_offset_dB;
  uint32_t payload_size;       /* DCI bits: 12 .. 128 (polar K = payload + 24 in 36 .. 164) */
  uint8_t  payload[NRPHY_PDCCH_MAX_PAYLOAD]; /* one bit per byte, as the reference passes it */
  /* precoding_configuration, one layer */
  uint32_t nof_ports;
  uint32_t prg_size_rb;
  uint32_t nof_prg;
  const float* precoding;      /* host pointer: [nof_prg][nof_ports] complex (re, im) */
} nrphy_pdcch_pdu_t;
/* NRPHY_OK when the PDU is one the reference processes without running into its assertions (its validator accepts
 * everything): duration, aggregation level, payload size, a CCE range inside the CORESET, REG bundles that tile it,
 * PRGs that cover the allocation exactly. */
int nrphy_pdcch_validate(const nrphy_pdcch_pdu_t* pdu);
/* n PDUs into device grids ([grid][port][14][subc] cbf16): PDU i into grid grid_index[i] (NULL: all into grid 0).
 * Descriptors are copied at the call into a staging buffer of the call's own (stream-ordered allocation); the kernel
 * is asynchronous on `stream`.  Only the resource elements of the PDCCH and its DM-RS are written. */
int nrphy_pdcch_process(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pdcch_pdu_t* pdus, const uint32_t* grid_index,
                        void* d_grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc, void* stream);
/* One PDU into a host grid [nof_ports][14][nof_subc] cbf16 (read and written; blocking). */
int nrphy_pdcch_process_host(nrphy_ctx_t* ctx, const nrphy_pdcch_pdu_t* pdu, void* grid, uint32_t nof_ports,
                             uint32_t nof_subc);
/* pdcch_encoder::encode (R/include/srsran/phy/upper/channel_processors/pdcch_encoder.h:33-57) alone: payload bits
 * (one per byte) -> E = rm_length rate-matched bits (one per byte); host spans, blocking. */
int nrphy_pdcch_encode_host(nrphy_ctx_t* ctx, const uint8_t* payload, uint32_t payload_size, uint32_t rnti,
                            uint32_t rm_length, uint8_t* encoded);

/* ---- other downlink grid writers: SS/PBCH block processor -----------------------------
 * Replaces ssb_processor::process (R/include/srsran/phy/upper/channel_processors/ssb_processor.h:35-92; impl
 * R/lib/phy/upper/channel_processors/ssb_processor_impl.cpp:29-107) with pbch_encoder_impl (payload generation,
 * scrambling, CRC24C, polar coding, rate matching: pbch_encoder_impl.cpp:38-186), pbch_modulator_impl
 * (pbch_modulator_impl.cpp:29-109), dmrs_pbch_processor_impl, pss_processor_impl and sss_processor_impl
 * (R/lib/phy/upper/signal_processors/).  The fields are ssb_processor::pdu_t; the slot is given as numerology, system
 * frame number and slot within the frame (slot_point). */
typedef struct nrphy_ssb_pdu {
  uint32_t numerology;       /* of the slot: 0 = 15 kHz ... */
  uint32_t sfn;
  uint32_t slot_index;       /* slot within the radio frame */
  uint32_t phys_cell_id;     /* 0..1007 */
  float    beta_pss_dB;      /* PSS power relative to SSS */
  uint32_t ssb_idx;
  uint32_t L_max;            /* 4, 8 or 64 */
  uint32_t common_scs;       /* subCarrierSpacingCommon as a numerology: 0 = 15 kHz, 1 = 30, 2 = 60, 3 = 120, 4 = 240 */
  uint32_t subcarrier_offset; /* k_SSB */
  uint32_t offset_to_pointA;
  uint32_t pattern_case;     /* 0..4 = case A..E */
  uint8_t  bch_payload[32];  /* one bit per byte: 24 MIB bits (+ 8 the encoder regenerates) */
  uint32_t nof_ports;
  uint8_t  ports[NRPHY_MAX_PORTS]; /* grid ports that carry the block */
} nrphy_ssb_pdu_t;
/* Also refused: a block whose four symbols would run past symbol 13 of the slot (pattern case E, blocks starting at symbol 12). */
int nrphy_ssb_validate(const nrphy_ssb_pdu_t* pdu);
/* n blocks into device grids, as nrphy_pdcch_process. */
int nrphy_ssb_process(nrphy_ctx_t* ctx, uint32_t n, const nrphy_ssb_pdu_t* pdus, const uint32_t* grid_index, void* d_grid,
                      uint32_t grid_nof_ports, uint32_t grid_nof_subc, void* stream);
int nrphy_ssb_process_host(nrphy_ctx_t* ctx, const nrphy_ssb_pdu_t* pdu, void* grid, uint32_t nof_ports,
                           uint32_t nof_subc);
/* pbch_encoder::encode alone: the 864 rate-matched bits (one per byte) of the block's PBCH; host span, blocking. */
int nrphy_pbch_encode_host(nrphy_ctx_t* ctx, const nrphy_ssb_pdu_t* pdu, uint8_t* encoded);

/* ---- receive side ("next" row): LDPC rate dematcher --------------------------
 * Replaces ldpc_rate_dematcher::rate_dematch (R/include/srsran/phy/upper/channel_coding/ldpc/
 * ldpc_rate_dematcher.h; impl R/lib/phy/upper/channel_coding/ldpc/ldpc_rate_dematcher_impl.cpp:43-256):
 * rm_length soft bits as received -> the codeblock's soft buffer of (66 or 50) * Zc int8 LLRs (the
 * codeblock without its first 2*Zc bits), which the LDPC decoder reads.  new_data != 0: first
 * transmission, the buffer is rebuilt (filler bits +infinity = 127, bits not received 0); otherwise the
 * soft bits are added to what the buffer holds (HARQ combining, saturating LLR sum).  The fields are
 * those of codeblock_metadata the reference reads: tb_common {base_graph, lifting_size, rv, mod (as bits
 * per symbol, 1 = BPSK), Nref} and cb_specific.nof_filler_bits, plus the input length.  Results are
 * those of the reference's generic implementation bit for bit, including which soft bits it leaves
 * untouched (so the buffer is an in/out argument in both modes); its AVX2 implementation treats an
 * infinite soft bit like a finite one when combining. */
typedef struct nrphy_ldpc_rate_dematcher_cfg {
  uint32_t base_graph;
  uint32_t lifting_size;
  uint32_t rv;
  uint32_t qm;
  uint32_t nref;
  uint32_t nof_filler_bits;
  uint32_t rm_length;
} nrphy_ldpc_rate_dematcher_cfg_t;
/* n_cb codeblocks that share the configuration: input i at d_in + i * in_stride_bytes, soft buffer i at
 * d_soft + i * soft_stride_bytes.  Asynchronous on `stream`; capturable except for extreme repetition
 * (rm_length of dozens of buffer lengths), where a longer operation list goes through a stream-ordered
 * allocation of the call's own. */
int nrphy_ldpc_rate_dematch(nrphy_ctx_t* ctx, const nrphy_ldpc_rate_dematcher_cfg_t* cfg, uint32_t n_cb,
                            const int8_t* d_in, uint32_t in_stride_bytes, int8_t* d_soft, uint32_t soft_stride_bytes,
                            int new_data, void* stream);
/* Host-span form for one codeblock (blocking); soft_buffer is read and written. */
int nrphy_ldpc_rate_dematch_host(nrphy_ctx_t* ctx, const nrphy_ldpc_rate_dematcher_cfg_t* cfg, const int8_t* in,
                                 int8_t* soft_buffer, int new_data);

/* ---- receive side ("next" row): LDPC decoder ------------------------------
 * Replaces ldpc_decoder::decode (R/include/srsran/phy/upper/channel_coding/ldpc/ldpc_decoder.h;
 * impl R/lib/phy/upper/channel_coding/ldpc/ldpc_decoder_impl.cpp:60-126 with the message kernels of
 * ldpc_decoder_generic.cpp:30-128): layered scaled min-sum on int8 log-likelihood ratios (finite range
 * +-120, +-127 = certain), early stop when the hard bits pass the CRC.  The fields are
 * ldpc_decoder::configuration: codeblock metadata (base graph, lifting size, filler bits, CRC) and
 * algorithm details (max_iterations, scaling_factor in (0, 1)).  crc_poly: 0 = no early stop, 16 =
 * CRC16, 0x24A = CRC24A, 0x24B = CRC24B.  nof_llr soft bits per codeblock: the codeblock without its
 * first 2*Zc (punctured) bits, as the rate dematcher delivers it, between (Kb + 2) * Zc and
 * (N_full - 2) * Zc of them.  Results are bit-identical to the reference's generic implementation; its
 * AVX2 implementation uses other intermediate arithmetic and agrees only once both have converged. */
typedef struct nrphy_ldpc_decoder_cfg {
  uint32_t base_graph;
  uint32_t lifting_size;
  uint32_t nof_filler_bits;
  uint32_t crc_poly;
  uint32_t nof_llr;
  uint32_t max_iterations;
  float    scaling_factor;
} nrphy_ldpc_decoder_cfg_t;
/* n_cb codeblocks that share the configuration.  d_llr: codeblock i at i * llr_stride_bytes.  d_out:
 * the Kb*Zc hard bits of codeblock i, packed MSB first, at i * out_stride_bytes.  d_iterations (may be
 * NULL): per codeblock the iteration after which the CRC passed, 0 when it did not (or no CRC given).
 * d_scratch: nrphy_ldpc_decoder_scratch_bytes() bytes of device memory the CALLER owns for the duration of the call
 * (the decoder's check-to-variable records: a pool of slots shared by the workgroups resident at once, so its size
 * stops growing with the batch -- 0.2 GB at most); calls in flight at the same time need a scratch each.
 * After nrphy_ldpc_decoder_prepare() for the configuration (it uploads the decoder's graph and CRC weights; a call
 * without it does so itself, once, with an allocation and a blocking copy) the call neither allocates nor
 * synchronises and can be captured in a hipGraph. */
int nrphy_ldpc_decoder_scratch_bytes(nrphy_ctx_t* ctx, const nrphy_ldpc_decoder_cfg_t* cfg, uint32_t n_cb, uint64_t* bytes);
int nrphy_ldpc_decoder_prepare(nrphy_ctx_t* ctx, const nrphy_ldpc_decoder_cfg_t* cfg);
int nrphy_ldpc_decode(nrphy_ctx_t* ctx, const nrphy_ldpc_decoder_cfg_t* cfg, uint32_t n_cb, const int8_t* d_llr,
                      uint32_t llr_stride_bytes, uint8_t* d_out, uint32_t out_stride_bytes, uint32_t* d_iterations,
                      void* d_scratch, void* stream);
/* Host-span form for one codeblock (blocking). */
int nrphy_ldpc_decode_host(nrphy_ctx_t* ctx, const nrphy_ldpc_decoder_cfg_t* cfg, const int8_t* llr,
                           uint8_t* message_packed, uint32_t* iterations);

/* One codeblock through rate dematcher and decoder, host spans, one round trip: the operation of the
 * per-codeblock accelerator seam hal::hw_accelerator_pusch_dec::{configure,enqueue,dequeue}_operation +
 * read_operation_outputs (R/include/srsran/hal/phy/upper/channel_processors/pusch/hw_accelerator_pusch_dec.h:
 * 36-110; caller R/lib/phy/upper/channel_processors/pusch/pusch_decoder_hw_impl.cpp:180-345).  llr: the
 * dm->rm_length soft bits of the codeblock; soft_buffer: its HARQ buffer of (66 or 50) * Zc LLRs, read
 * and written; message_packed: Kb * Zc hard bits; *iterations: as nrphy_ldpc_decode.  crc_poly 0 runs
 * max_iterations without a check. */
int nrphy_pusch_decode_codeblock_host(nrphy_ctx_t* ctx, const nrphy_ldpc_rate_dematcher_cfg_t* dm, uint32_t crc_poly,
                                      uint32_t max_iterations, float scaling_factor, const int8_t* llr,
                                      int8_t* soft_buffer, int new_data, uint8_t* message_packed, uint32_t* iterations);

/* ---- receive side ("next" row): PUSCH (UL-SCH) decoder, transport-block level ----
 * Replaces pusch_decoder::new_data ... on_end_softbits (R/include/srsran/phy/upper/channel_processors/pusch/
 * pusch_decoder.h; impl R/lib/phy/upper/channel_processors/pusch/pusch_decoder_impl.cpp:94-497 with
 * ldpc_segmenter_rx and pusch_codeblock_decoder.cpp:28-71) for a batch of transport blocks that share one
 * configuration, everything resident in HBM: segmentation of the codeword LLRs, rate dematching of every
 * codeblock into its HARQ soft buffer, LDPC decoding of the codeblocks whose CRC has not passed yet,
 * concatenation, transport-block CRC.  The fields are pusch_decoder::configuration (base_graph, rv, mod,
 * Nref, nof_layers, nof_ldpc_iterations, use_early_stop, new_data) plus the transport-block size and the
 * number of channel symbols (codeword soft bits / bits per symbol). */
typedef struct nrphy_pusch_decoder_cfg {
  uint32_t base_graph;
  uint32_t qm;
  uint32_t rv;
  uint32_t nof_layers;
  uint32_t nref;            /* limited-buffer size N_ref in bits, 0 = none */
  uint32_t tb_size_bytes;
  uint32_t nof_ch_symbols;  /* G / qm */
  uint32_t max_iterations;
  uint32_t use_early_stop;
  uint32_t new_data;
} nrphy_pusch_decoder_cfg_t;
/* HARQ state the caller keeps per batch between transmissions (sizes from nrphy_pusch_decoder_sizes):
 * d_soft  = n_tb * soft_bytes_per_tb  int8 soft buffers, [tb][codeblock][(66 or 50) * Zc];
 * d_state = n_tb-dependent codeblock state (CRC flags, decoded messages, iteration counts), state_bytes(n_tb).
 * Neither needs initialising before a new_data call.  d_scratch = scratch_bytes of device memory owned by the caller
 * for the duration of one call (the LDPC decoder's records, see nrphy_ldpc_decode); it carries nothing between calls. */
int nrphy_pusch_decoder_sizes(nrphy_ctx_t* ctx, const nrphy_pusch_decoder_cfg_t* cfg, uint32_t n_tb, uint64_t* soft_bytes_per_tb,
                              uint64_t* state_bytes, uint64_t* scratch_bytes, uint32_t* nof_codeblocks);
/* Uploads what the configuration needs once (decoder graph, CRC weights): afterwards nrphy_pusch_decode_batch neither
 * allocates nor synchronises (capturable). */
int nrphy_pusch_decoder_prepare(nrphy_ctx_t* ctx, const nrphy_pusch_decoder_cfg_t* cfg);
/* d_llr: codeword LLRs of transport block i at i * llr_stride_bytes (nof_ch_symbols * qm of them, in the
 * order the demodulator delivers them).  d_tb: transport block i at i * tb_stride_bytes (written whenever
 * all its codeblock CRCs pass; valid when its tb_crc_ok is 1).  d_result: 4 words per transport block --
 * tb_crc_ok, codeblocks whose CRC passed, sum and maximum of the LDPC iterations of the codeblocks decoded
 * in this call (a failed decode counts max_iterations).  Asynchronous on `stream`. */
int nrphy_pusch_decode_batch(nrphy_ctx_t* ctx, const nrphy_pusch_decoder_cfg_t* cfg, uint32_t n_tb, const int8_t* d_llr,
                             uint64_t llr_stride_bytes, int8_t* d_soft, uint8_t* d_state, void* d_scratch, uint8_t* d_tb,
                             uint32_t tb_stride_bytes, uint32_t* d_result, void* stream);

/* ---- receive side of seam C ("next" row): OFDM demodulator ---------------
 * Replaces ofdm_symbol_demodulator::demodulate / ofdm_slot_demodulator::demodulate
 * (R/include/srsran/phy/lower/modulation/ofdm_demodulator.h; impl
 * R/lib/phy/lower/modulation/ofdm_demodulator_impl.cpp:98-171) for every port of nof_grids slots:
 * d_iq [grid][port][slot_stride] complex float (the layout nrphy_ofdm_run writes) -> d_grid
 * [grid][port][14][12*bw_rb] cbf16.  The plan's configuration doubles as ofdm_demodulator_configuration
 * (numerology, bw_rb, dft_size, cp, scale, center_freq_hz); window_offset is its
 * nof_samples_window_offset (must be below the shortest cyclic prefix).  slot_index as in nrphy_ofdm_run. */
int nrphy_ofdm_demod_run(nrphy_ofdm_plan_t* plan, uint32_t nof_grids, const float* d_iq, const uint32_t* slot_index,
                         uint32_t window_offset, void* d_grid, void* stream);
/* Host-span whole-slot form: iq holds nof_ports x nrphy_ofdm_slot_size(cfg, slot_index) complex samples,
 * port after port; grid receives [nof_ports][14][12*bw_rb] cbf16 (blocking). */
int nrphy_ofdm_demodulate_slot_host(nrphy_ofdm_plan_t* plan, const float* iq, uint32_t slot_index,
                                    uint32_t window_offset, void* grid);
/* Host-span form of ofdm_symbol_demodulator::demodulate for one symbol of one port: input = the symbol's
 * cyclic prefix + dft_size samples, symbol_index counted within the subframe; grid_row receives the
 * 12*bw_rb cbf16 values of that OFDM symbol (blocking). */
int nrphy_ofdm_demodulate_symbol_host(nrphy_ofdm_plan_t* plan, const float* input, uint32_t input_size,
                                      uint32_t symbol_index, uint32_t window_offset, void* grid_row);

/* ---- lower-PHY tail: amplitude controller, radio sample format, fronthaul compression ----
 * Amplitude controller: replaces amplitude_controller::process (R/include/srsran/phy/lower/amplitude_controller/
 * amplitude_controller.h:52-66; impl amplitude_controller_clipping_impl.cpp:31-68 and _scaling_impl.cpp:28-37) for
 * n_buffers baseband buffers of nof_samples complex floats (what the lower PHY hands over per port):
 * out = in * 10^(input_gain_dB / 20), then, with clipping enabled, real and imaginary parts limited to
 * +-full_scale_lin * 10^(ceiling_dBFS / 20).  kind 1 is the scaling implementation (gain only, no measurements).
 * The device leaves the raw measurements per buffer in d_stats (may be NULL): sum of |x|^2 and largest |x|^2 after
 * the gain and before clipping, number of clipped real / imaginary parts; nrphy_amplitude_metrics() turns them into
 * amplitude_controller_metrics on the host, carrying the running counters of the reference's object.  The reference
 * skips clipping when the measured power is not a normal number (all-zero, NaN): for such buffers clipping changes
 * nothing unless the ceiling itself is denormal, which is refused. */
typedef struct nrphy_amplitude_cfg {
  uint32_t kind;            /* 0 amplitude_controller_clipping_impl, 1 amplitude_controller_scaling_impl */
  uint32_t enable_clipping;
  float    input_gain_dB;
  float    full_scale_lin;
  float    ceiling_dBFS;
} nrphy_amplitude_cfg_t;
typedef struct nrphy_amplitude_stats { /* device side, one per buffer */
  float    sum_power;
  float    peak_power;
  uint32_t nof_clipped;
  uint32_t nof_samples;
} nrphy_amplitude_stats_t;
typedef struct nrphy_amplitude_metrics { /* amplitude_controller_metrics */
  float    avg_power_fs;
  float    peak_power_fs;
  float    papr_lin;
  float    gain_dB;
  uint64_t nof_processed_samples; /* running totals: pass the same struct to every call for one controller */
  uint64_t nof_clipped_samples;
  double   clipping_probability;
  uint32_t clipping_enabled;
  uint32_t reserved_;
} nrphy_amplitude_metrics_t;
/* Buffer i at d_in + i * in_stride / d_out + i * out_stride (strides in complex samples; in place allowed).
 * Asynchronous on `stream`, capturable (d_stats is cleared by the call itself with a memset node). */
int nrphy_amplitude_control(nrphy_ctx_t* ctx, const nrphy_amplitude_cfg_t* cfg, uint32_t n_buffers, uint32_t nof_samples,
                            const float* d_in, size_t in_stride, float* d_out, size_t out_stride,
                            nrphy_amplitude_stats_t* d_stats, void* stream);
/* Host arithmetic of amplitude_controller_clipping_impl::process on the measurements of ONE buffer; `metrics` is read
 * (running counters) and written. */
int nrphy_amplitude_metrics(const nrphy_amplitude_cfg_t* cfg, const nrphy_amplitude_stats_t* stats,
                            nrphy_amplitude_metrics_t* metrics);
/* One buffer from and to host memory (blocking); metrics may be NULL. */
int nrphy_amplitude_control_host(nrphy_ctx_t* ctx, const nrphy_amplitude_cfg_t* cfg, const float* in, uint32_t nof_samples,
                                 float* out, nrphy_amplitude_metrics_t* metrics);

/* Radio sample format: complex float -> complex int16 (I, Q interleaved), out = round_to_nearest_even(in * scale)
 * saturated to int16 -- srsvec::convert(span<const cf_t>, float, span<int16_t>) (R/lib/srsvec/conversion.cpp:29-65,
 * 323-328), which the radio layers call on every transmit buffer.  The reference's vector loop converts 16 values at
 * a time this way; the last (2 * nof_samples) mod 16 values of a buffer go through std::round (ties away from zero),
 * and so do they here.  Strides in complex samples. */
int nrphy_iq_convert_ci16(nrphy_ctx_t* ctx, uint32_t n_buffers, uint32_t nof_samples, const float* d_in, size_t in_stride,
                          float scale, int16_t* d_out, size_t out_stride, void* stream);
int nrphy_iq_convert_ci16_host(nrphy_ctx_t* ctx, const float* in, uint32_t nof_samples, float scale, int16_t* out);

/* The two above fused into the OFDM modulator's store: nrphy_ofdm_run with the slot leaving the device as complex
 * int16 (4 bytes per sample instead of 8: the IQ write is 71 % of the modulator's traffic).  Every sample takes the
 * path modulator -> amplitude controller (gain, clipping per buffer = per (grid, port) slot) -> conversion, in the
 * reference's order of roundings.  d_iq: [grid][port][slot_stride] complex int16; d_stats: [grid][port] or NULL.
 * Every sample is converted as the reference's vector loop does it (round to nearest even, saturate).  The reference's scalar tail
 * -- the last (2 n mod 16) floats of ONE conversion call round half away from zero and wrap instead of saturating -- has no
 * counterpart here: where it falls depends on how the caller of the reference cuts its buffers, not on the slot
 * (nrphy_iq_convert_ci16 reproduces it per call).
 * With d_stats the plan keeps one 16-byte record per workgroup in a buffer of its own that grows with the largest
 * nof_grids seen (a synchronous reallocation on growth only): run the largest batch once before capturing the call in a
 * hipGraph, and keep the runs of one plan ordered (Conventions). */
typedef struct nrphy_iq_wire_cfg {
  nrphy_amplitude_cfg_t amplitude;
  float                 ci16_scale;
} nrphy_iq_wire_cfg_t;
int nrphy_ofdm_run_ci16(nrphy_ofdm_plan_t* plan, uint32_t nof_grids, const void* d_grid, const uint32_t* slot_index,
                        const nrphy_iq_wire_cfg_t* cfg, int16_t* d_iq, nrphy_amplitude_stats_t* d_stats, void* stream);

/* Open Fronthaul IQ compression of resource-grid PRBs (split 7.2: the grid, not the time-domain signal, leaves the
 * DU).  Replaces iq_compressor::compress (R/include/srsran/ofh/compression/iq_compressor.h; impl
 * R/lib/ofh/compression/iq_compression_none_impl.cpp:31-55 and iq_compression_bfp_impl.cpp:31-98 with quantizer.h and
 * compressed_prb_packer.cpp) and the serialisation of the result in ofh_uplane_message_builder_impl.cpp:137-144: per
 * PRB [udCompParam: the BFP exponent, one byte, BFP only] + 24 samples of data_width bits packed MSB first.  One
 * row = one compress() call = the PRBs of one OFDM symbol of one port; results are those of the reference built for
 * AVX2 (its 16-lane conversion loop rounds to nearest even and saturates, the tail of a call rounds half away). */
typedef struct nrphy_ofh_compression_cfg {
  uint32_t type;        /* 0 none, 1 BFP */
  uint32_t data_width;  /* 1..16 */
  float    iq_scaling;
} nrphy_ofh_compression_cfg_t;
/* Bytes per compressed PRB: 3 * data_width (+ 1 for BFP). */
uint32_t nrphy_ofh_compressed_prb_bytes(const nrphy_ofh_compression_cfg_t* cfg);
/* n_rows rows of nof_prb PRBs: row r reads 12 * nof_prb cbf16 at d_prbs + r * row_stride (in cbf16 words) and writes
 * nof_prb records at d_out + r * out_row_stride bytes.  A batch of whole grids is n_rows = grids * ports * 14,
 * row_stride = 12 * nof_prb.  Asynchronous on `stream`, capturable. */
int nrphy_ofh_compress(nrphy_ctx_t* ctx, const nrphy_ofh_compression_cfg_t* cfg, uint32_t n_rows, uint32_t nof_prb,
                       const void* d_prbs, size_t row_stride, uint8_t* d_out, size_t out_row_stride, void* stream);
int nrphy_ofh_compress_host(nrphy_ctx_t* ctx, const nrphy_ofh_compression_cfg_t* cfg, uint32_t nof_prb, const void* prbs,
                            uint8_t* out);

/* Open Fronthaul IQ decompression: the receive half.  Replaces iq_decompressor::decompress
 * (R/lib/ofh/compression/iq_compression_none_impl.cpp:56-73, iq_compression_bfp_impl.cpp:98-135 with quantizer.h,
 * compressed_prb_unpacker.cpp and to_bf16 of R/include/srsran/adt/bf16.h:39-56; the reference's SIMD classes delegate
 * decompress to these, so there is one behaviour).  The records are the ones nrphy_ofh_compress writes.  Per value: v = the
 * data_width-bit field sign-extended; none: float(v) / float(2^(data_width - 1) - 1); BFP: float(v * scaler) / 32767.0f in
 * 32-bit integer arithmetic, scaler = (int16_t)(1 << udCompParam) as the reference built by gcc evaluates it -- 2^e for
 * e <= 14, -32768 for e = 15 (the sign flip included), 0 for 16 <= e <= 30.  For e >= 31 the reference is undefined; this
 * library's rule is scaler = 0.  The division is IEEE single precision, correctly rounded; the result is rounded to bf16 as
 * to_bf16 does.  Every result is byte for byte the reference's.
 * Widths: BFP 1..16, none 2..16.  none with 1 bit has a quantiser gain of 0 and the reference produces NaN and infinities
 * whose bit patterns differ between hosts: NRPHY_ERR_ARGUMENT.  cfg->iq_scaling is not used (the reference's decompressors
 * ignore theirs).
 * n_rows rows of nof_prb PRBs: row r reads nof_prb records at d_in + r * in_row_stride bytes (any byte alignment; only
 * the rows' own bytes are read) and writes 12 * nof_prb cbf16 at d_prbs + r * row_stride (in cbf16 words; d_prbs 4-byte
 * aligned).  Asynchronous on `stream`, capturable.  The host form goes through the context's staging like every _host
 * call. */
int nrphy_ofh_decompress(nrphy_ctx_t* ctx, const nrphy_ofh_compression_cfg_t* cfg, uint32_t n_rows, uint32_t nof_prb,
                         const uint8_t* d_in, size_t in_row_stride /* bytes */, void* d_prbs, size_t row_stride /* cbf16 words */,
                         void* stream);
int nrphy_ofh_decompress_host(nrphy_ctx_t* ctx, const nrphy_ofh_compression_cfg_t* cfg, uint32_t nof_prb, const uint8_t* in,
                              void* prbs);

/* Open Fronthaul uplink receive: the sections of decoded user-plane messages -- of any number of messages, slots and
 * cells -- decompressed from packet payload in device memory straight into the receive grid
 * [nof_grids][grid_nof_ports][14][grid_nof_subc] cbf16 that nrphy_pusch_chest_run, nrphy_pucch_run and nrphy_pf2_run read.
 * Replaces uplane_message_decoder_impl::decode_iq_data + uplane_rx_symbol_data_flow_writer::write_to_resource_grid
 * (R/lib/ofh/receiver/ofh_uplane_rx_symbol_data_flow_writer.cpp:53-80).  Header parsing, the sequence and window checks
 * and the context repositories stay with the caller: one descriptor per section says where its records are and where
 * they belong. */
typedef struct nrphy_ofh_ul_section {
  uint64_t payload_offset; /* byte offset in d_payload of the section's first PRB record */
  uint32_t grid_index;     /* the uplink slot context */
  uint16_t port;           /* resource-grid port = position of the eAxC in the cell's list */
  uint16_t symbol;         /* 0..13 */
  uint16_t start_prb;      /* as decoded from the section header, 0..1023 */
  uint16_t nof_prbs;       /* as decoded, after the reference's "0 means ru_nof_prbs, start 0" rule; 1..MAX_NOF_PRBS */
  uint8_t  type;           /* 0 none, 1 BFP: the section's udCompHdr (static or dynamic compression alike) */
  uint8_t  data_width;
  uint16_t reserved_;      /* 0 */
} nrphy_ofh_ul_section_t;
/* Clipping is the reference's, with du_nof_prbs = grid_nof_subc / 12: a section with start_prb >= du_nof_prbs writes
 * nothing, any other writes min(nof_prbs, du_nof_prbs - start_prb) PRBs from subcarrier 12 * start_prb on; every other
 * resource element of every grid is left untouched.
 * nrphy_ofh_ul_validate is host only (no device work).  NRPHY_ERR_ARGUMENT for: an unknown type, a width outside the
 * ranges of nrphy_ofh_decompress, symbol >= 14, port >= grid_nof_ports, grid_index >= nof_grids, nof_prbs of 0 or above
 * 275 (MAX_NOF_PRBS), a non-zero reserved_, grid_nof_subc that is no multiple of 12, a section whose nof_prbs records --
 * all of them as sent, not only the clipped part (check_iq_data_size) -- do not lie inside [0, payload_bytes), and two
 * sections of one call whose clipped ranges share a resource element: the reference writes sections in order, one launch
 * cannot, so a caller with duplicates makes two calls on the same stream.
 * nrphy_ofh_ul_write_grid validates, then launches; n = 0 is NRPHY_OK with no work.  `sections` is a host array, copied
 * at the call into staging that lives in stream order, as nrphy_grid_put does: asynchronous on `stream`, NOT capturable.
 * The kernel reads no byte outside the sections' records and writes nothing outside the clipped ranges.  d_grid is 4-byte
 * aligned; d_payload may have any alignment. */
int nrphy_ofh_ul_validate(uint32_t n, const nrphy_ofh_ul_section_t* sections, uint64_t payload_bytes, uint32_t nof_grids,
                          uint32_t grid_nof_ports, uint32_t grid_nof_subc);
int nrphy_ofh_ul_write_grid(nrphy_ctx_t* ctx, uint32_t n, const nrphy_ofh_ul_section_t* sections, const uint8_t* d_payload,
                            uint64_t payload_bytes, void* d_grid, uint32_t nof_grids, uint32_t grid_nof_ports,
                            uint32_t grid_nof_subc, void* stream);

/* The same into the PRACH buffer that nrphy_prach_run reads in place (the tensor nrphy_prach_plan_create describes:
 * sym_offset, port_stride, symbol_stride).  Replaces uplane_prach_symbol_data_flow_writer::write_to_prach_buffer
 * (R/lib/ofh/receiver/ofh_uplane_prach_symbol_data_flow_writer.cpp:56-112): its range arithmetic -- the PRACH's PRBs, the two
 * skip conditions, the PRBs to write, start_re, the trimming of the last PRB, iq_start_re, iq_size_re -- is done on the
 * host per section in the reference's order and integer widths, from the two values of the reference's prach_context that
 * the caller passes.  Resource elements [iq_start_re, iq_start_re + iq_size_re) of the section are decompressed to cbf16
 * as above, each half is widened to float (srsvec::convert(cf, cbf16)), and element i goes to
 * d_symbols[dst_offset + start_re + i]. */
typedef struct nrphy_ofh_ul_prach_section {
  nrphy_ofh_ul_section_t section;   /* grid_index, port, symbol unused by the arithmetic: must be 0 */
  uint64_t dst_offset;              /* element (complex f32) of d_symbols where RE 0 of this (port, symbol, occasion) lives */
  uint32_t prach_nof_re;            /* prach_context::get_prach_nof_re(): 839 or 139 */
  uint32_t offset_to_first_re;      /* prach_context::get_prach_offset_to_first_re() */
} nrphy_ofh_ul_prach_section_t;
/* Refused like nrphy_ofh_ul_validate where that applies (type, width, nof_prbs, reserved_, the records inside the
 * payload), and: non-zero grid_index, port or symbol, prach_nof_re other than 139 or 839, a range of the section's samples
 * that the reference's subspan would refuse, a destination range outside [0, symbols_elems), destinations of one call
 * that overlap.  d_symbols is 8-byte aligned.  Asynchronous on `stream`, not capturable (the host array is staged as
 * above). */
int nrphy_ofh_ul_prach_validate(uint32_t n, const nrphy_ofh_ul_prach_section_t* sections, uint64_t payload_bytes,
                                uint64_t symbols_elems);
int nrphy_ofh_ul_write_prach(nrphy_ctx_t* ctx, uint32_t n, const nrphy_ofh_ul_prach_section_t* sections, const uint8_t* d_payload,
                             uint64_t payload_bytes, void* d_symbols, uint64_t symbols_elems, void* stream);

/* Open Fronthaul uplink frame receiver: received Ethernet frames in device-visible memory -- of any number of slots and
 * cells -- to the receive grid, with no host step on the frames' bytes.  Replaces, for a batch of frames,
 * message_receiver_impl::process_new_frame (R/lib/ofh/receiver/ofh_message_receiver.cpp:59-118) with
 * vlan_frame_decoder_impl, ecpri::packet_decoder_{use,ignore}_header_payload_size, sequence_id_checker_impl (or the dummy),
 * uplane_peeker, uplane_message_decoder_{static,dynamic}_compression_impl, data_flow_uplane_uplink_data_impl's filter and
 * uplane_rx_symbol_data_flow_writer::write_to_resource_grid.  What stays with the caller: the control plane (it says what it
 * announced through nrphy_ofh_rx_expect_t), update_rx_window_statistics, the re_written bookkeeping and symbol-complete
 * notifications, logging -- all from the per-frame records -- and the PRACH writes (nrphy_ofh_ul_write_prach from the
 * records of status 22: its range arithmetic needs the prach_context). */
typedef struct nrphy_ofh_rx_cfg {            /* message_receiver_config + what the decoders are constructed with */
  uint8_t  mac_dst[6], mac_src[6];           /* should_ethernet_frame_be_filtered compares these two and eth_type */
  uint16_t eth_type, reserved_;              /* reserved_: 0 */
  uint32_t vlan_tag_present;                 /* 0: the NIC stripped the tag (14-byte header, as the reference assumes); 1: a 4-byte
                                                802.1Q tag follows the addresses and is skipped, TCI not compared (18 bytes) */
  uint32_t ignore_ecpri_payload_size;        /* 1: packet_decoder_ignore_header_payload_size; 0: ..._use_header_payload_size */
  uint32_t seq_id_check;                     /* 1: sequence_id_checker_impl; 0: the dummy (always 0) */
  uint32_t numerology;                       /* 0..4 */
  uint32_t nof_symbols;                      /* 14 or 12 */
  uint32_t ru_nof_prbs;                      /* 1..275 */
  uint32_t static_compression;               /* 1: the two cfgs below go into every section; 0: udCompHdr + reserved byte per section */
  uint32_t n_ul_eaxc, n_prach_eaxc;          /* 0..4 each (MAX_NOF_SUPPORTED_EAXC) */
  uint16_t ul_eaxc[4], prach_eaxc[4];        /* below 32 (MAX_SUPPORTED_EAXC_ID_VALUE), distinct within a list */
  nrphy_ofh_compression_cfg_t compression;       /* filter index 0; iq_scaling unused; ignored with static_compression = 0 */
  nrphy_ofh_compression_cfg_t prach_compression; /* filter indices 1..7 */
} nrphy_ofh_rx_cfg_t;
typedef struct nrphy_ofh_rx_frame {          /* one received frame: bytes [offset, offset + length) of d_frames, any alignment */
  uint64_t offset;
  uint32_t length;
  uint32_t reserved_;                        /* 0 */
} nrphy_ofh_rx_frame_t;
typedef struct nrphy_ofh_rx_expect {         /* one (slot, eAxC) for which a control-plane message was sent: both repositories */
  uint32_t grid_index;                       /* the uplink slot context's grid */
  uint16_t sfn8;                             /* 0..255: slot.sfn() % 256, the key of uplink_cplane_context_repository */
  uint16_t eaxc;                             /* one of ul_eaxc */
  uint16_t prb_start, nof_prb;               /* ul_cplane_context */
  uint16_t context_symbols;                  /* bit s: uplink_context_repository::get(slot, s) is not empty */
  uint8_t  subframe, slot;                   /* 0..9, 0..2^numerology - 1 */
  uint8_t  filter_index;                     /* 0..7: radio_hdr.filter_index */
  uint8_t  start_symbol, nof_symbols;        /* radio_hdr.start_symbol, ul_cplane_context::nof_symbols */
  uint8_t  reserved_;                        /* 0 */
} nrphy_ofh_rx_expect_t;
/* status: 0 accepted and written; 22 a PRACH message decoded, nothing written; any other value names the first of the
 * reference's checks, in the reference's order, that dropped the frame:
 *    1 shorter than 64 bytes                          2 a MAC address or the Ethernet type differs
 *    3 eCPRI revision not 1, or concatenation         4 (payload-size mode) the payload size exceeds what follows the common
 *                                                       header; library rule: or is below 5 (no message byte; below 4 the
 *                                                       reference's subspan is ill-formed)
 *    5 eCPRI message type not IQ data                 6 pc_id in neither eAxC list
 *    7 sequence identifier from the past              8 peek_slot_symbol_point fails (under 4 bytes, subframe, slot)
 *    9 filter index reserved (8..15)                 10 not uplink
 *   11 payload version not 1                         12 symbol >= nof_symbols
 *   13 reserved dynamic compression type (7..15)     14 a second complete section (the decoder's result list is full)
 *   15 no section decoded                            16 library rule: dynamic types 2..6, or none with 1 bit (the reference
 *                                                       has no decompressor for them)
 *   17 no expectation for (sfn8, subframe, slot, eAxC), or the symbol outside its range, or another filter index
 *   18 every-other-RB mode                           19 the symbol-increment bit
 *   20 the section's PRBs outside [prb_start, prb_start + nof_prb)
 *   21 the symbol's bit of context_symbols is clear
 * The sequence checker (7) sees every frame that passed 1..6, in batch order per eAxC and across calls in stream order, and
 * is updated by it also when a later check drops the frame.  Filter indices 1..7 end at 22 after 16; index 0 goes on to 17.
 * Fields that decoding did not reach are 0: nothing is filled up to status 5; eaxc and seq_id from 6 on; seq_skipped (the
 * checker's return value: negative for 7, the number of potentially lost messages otherwise) from 7 on; sfn8, subframe, slot,
 * symbol and filter_index from 9 on; the section (start_prb and nof_prbs after the "0 means ru_nof_prbs, start 0" rule,
 * type, data_width, payload_offset) for 0 and from 16 on; expect_index, grid_index and port (the eAxC's position in ul_eaxc)
 * for 0 and 18..21; nof_prbs_written (write_to_resource_grid's clipping to grid_nof_subc / 12, as nrphy_ofh_ul_write_grid
 * documents it) for 0. */
typedef struct nrphy_ofh_rx_record {
  uint64_t payload_offset;                   /* byte of d_frames of the section's first PRB record */
  uint32_t status;
  int32_t  seq_skipped;
  uint32_t grid_index, expect_index;
  uint16_t eaxc, seq_id;                     /* pc_id and the 16-bit seq_id field (the checker takes seq_id >> 8) */
  uint16_t start_prb, nof_prbs, nof_prbs_written, port, sfn8;
  uint8_t  filter_index, subframe, slot, symbol, type, data_width;
  uint8_t  reserved_[4];
} nrphy_ofh_rx_record_t;
typedef struct nrphy_ofh_rx nrphy_ofh_rx_t;
/* The object owns the device-resident checker state (initialized + one counter per configured eAxC), the per-(grid, port,
 * symbol, PRB) ownership words a batch needs for "later message wins" (grown to the largest grid batch seen), and refers to
 * its context.  reset returns the checker to "first packet is always valid", in stream order.  One object serves one
 * stream of frames: its calls are issued from one thread at a time and take effect in stream order. */
int nrphy_ofh_rx_create(nrphy_ctx_t* ctx, const nrphy_ofh_rx_cfg_t* cfg, nrphy_ofh_rx_t** rx);
int nrphy_ofh_rx_destroy(nrphy_ofh_rx_t* rx);
int nrphy_ofh_rx_reset(nrphy_ofh_rx_t* rx, void* stream);
/* Host only (no device work).  NRPHY_ERR_ARGUMENT for: a configuration outside the ranges above (a non-zero reserved_,
 * flags above 1, eAxC values of 32 or more or repeated within a list, more than 4 of them), under static compression a
 * compression or prach_compression that nrphy_ofh_decompress refuses, non-zero reserved fields of a descriptor, a frame
 * range outside [0, frames_bytes), two frame ranges that overlap, grid_nof_subc that is no multiple of 12,
 * n_ul_eaxc > grid_nof_ports, an expectation with eaxc not in ul_eaxc, grid_index >= nof_grids, sfn8 >= 256,
 * subframe >= 10, slot >= 1 << numerology, filter_index > 7, start_symbol + nof_symbols > cfg->nof_symbols or
 * prb_start + nof_prb > 275, and two expectations with the same (sfn8, subframe, slot, eaxc). */
int nrphy_ofh_rx_validate(const nrphy_ofh_rx_cfg_t* cfg, uint32_t n_frames, const nrphy_ofh_rx_frame_t* frames, uint32_t n_expect,
                          const nrphy_ofh_rx_expect_t* expects, uint64_t frames_bytes, uint32_t nof_grids, uint32_t grid_nof_ports,
                          uint32_t grid_nof_subc);
/* Validates, stages the two host arrays in stream order (as nrphy_ofh_ul_write_grid and nrphy_grid_put do) and does three
 * launches with no host step or synchronisation between them: (1) one thread per frame parses and runs every stateless check;
 * (2) one workgroup walks the records per eAxC through the sequence checker, finalises the statuses, and the accepted frames
 * claim their PRBs, the largest frame index winning; (3) one wave per (frame, 16 PRBs) decompresses -- the arithmetic of
 * nrphy_ofh_decompress -- and stores the PRBs its frame owns at [grid_index][port][symbol][12 * start_prb ...] of d_grid
 * [nof_grids][grid_nof_ports][14][grid_nof_subc] cbf16.  When accepted frames cover the same PRB of the same (grid, port,
 * symbol), the later one in batch order stays, as when the reference takes the frames one after another.  Asynchronous on
 * `stream`, NOT capturable; n_frames = 0 is NRPHY_OK with no work.  The kernels read no byte of d_frames outside the frames'
 * own ranges, whatever the bytes in a frame claim, and write only d_records (n_frames records, in frame order, 8-byte
 * aligned) and the resource elements of accepted sections.  d_grid is 4-byte aligned; d_frames has any alignment. */
int nrphy_ofh_rx_run(nrphy_ofh_rx_t* rx, uint32_t n_frames, const nrphy_ofh_rx_frame_t* frames, uint32_t n_expect,
                     const nrphy_ofh_rx_expect_t* expects, const uint8_t* d_frames, uint64_t frames_bytes, void* d_grid,
                     uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc, nrphy_ofh_rx_record_t* d_records,
                     void* stream);
/* Host-span form for one frame and one grid (blocking): `frame` is the frame's `length` bytes, `grid` the host copy of one
 * grid [grid_nof_ports][14][grid_nof_subc] cbf16, read and written in place, so every expectation's grid_index must be 0;
 * `record` receives the frame's record (its payload_offset counts from the frame's first byte).  The checker state is the
 * object's, as for nrphy_ofh_rx_run.  Through the context's staging like every _host call. */
int nrphy_ofh_rx_host(nrphy_ofh_rx_t* rx, const uint8_t* frame, uint32_t length, uint32_t n_expect, const nrphy_ofh_rx_expect_t* expects,
                      void* grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc, nrphy_ofh_rx_record_t* record);

/* Open Fronthaul downlink transmit: OFDM symbols of the device-resident downlink grid
 * [nof_grids][grid_nof_ports][14][grid_nof_subc] cbf16 (what every downlink writer here produces) to complete, ready-to-send
 * Ethernet frames in device (or pinned) memory, byte for byte those of
 * data_flow_uplane_downlink_data_impl::enqueue_section_type_1_message
 * (R/lib/ofh/transmitter/ofh_data_flow_uplane_downlink_data_impl.cpp) with vlan_frame_builder_impl, ecpri::packet_builder_impl, the
 * static or the dynamic user-plane message builder and the AVX2 compressors.  One descriptor is one OFDM symbol of one eAxC;
 * one launch takes any number of them, of any slots, cells and compressions.  The control plane, the frame pool and the send
 * stay with the caller.
 * A symbol's ru_nof_prbs PRBs are cut into fragments of floor((mtu - headers) / record bytes) PRBs (the last one shorter),
 * headers = 18 (VLAN Ethernet) + 8 (eCPRI) + 8 or 10 (radio application and section header, + udCompHdr and a reserved byte
 * for the dynamic builder).  Fragment f is one frame at frame_offset + f * frame_stride:
 *   dst MAC, src MAC, 0x8100, tci, eth_type | 0x10, 0x00 (iq_data), payload size (all after these four bytes), eaxc,
 *   (seq_id + f) mod 256, 0x80 | 0x90, sfn & 0xFF, subframe << 4 | slot >> 2, (slot & 3) << 6 | symbol | 0x00,
 *   start_prb >> 8, start_prb & 0xFF, nof_prbs (0 above 255) | [data_width << 4 | type (low 8 bits), 0x00] | the PRB records
 * and zeros up to 64 bytes when it is shorter.  The records of a fragment are those of nrphy_ofh_compress for ONE row that
 * consists of the fragment's PRBs -- the reference calls compress() per fragment, and where the vector loop of a call ends
 * decides the rounding of its last values -- so they differ from a slice of a whole-symbol row.  PRBs at or beyond
 * grid_nof_subc / 12 are zero samples.  The reference's `symbol_end = symbol_range.length()` loop bound is not reproduced: the
 * caller passes one descriptor per symbol. */
typedef struct nrphy_ofh_dl_flow {          /* data_flow_uplane_downlink_data_impl_config + its builders: one per cell/compression */
  uint8_t  mac_dst[6], mac_src[6];
  uint16_t tci, eth_type;                   /* vlan_frame_params */
  uint32_t mtu;                             /* bytes of one frame buffer, Ethernet header included (eth_frame_pool's mtu) */
  uint32_t ru_nof_prbs;                     /* 1..275 */
  uint32_t static_compression;              /* 1: static builder, no udCompHdr (OFH header 8 B); 0: dynamic (10 B) */
  nrphy_ofh_compression_cfg_t compression;  /* type none|BFP, data_width, iq_scaling: as nrphy_ofh_compress */
} nrphy_ofh_dl_flow_t;
typedef struct nrphy_ofh_dl_fragment {
  uint16_t start_prb, nof_prbs;
  uint32_t frame_bytes;                     /* frame_buffer::set_size: max(64, headers + records) */
} nrphy_ofh_dl_fragment_t;
typedef struct nrphy_ofh_dl_symbol {        /* one OFDM symbol of one eAxC */
  uint64_t frame_offset;  /* byte offset in d_frames of this symbol's first frame; fragment f at + f * frame_stride */
  uint32_t flow, grid_index;
  uint16_t port, eaxc;    /* grid port; eCPRI pc_id */
  uint16_t sfn;
  uint8_t  subframe, slot /* subframe_slot_index */, symbol, seq_id /* of the first fragment */;
  uint8_t  reserved_[2];  /* 0 */
} nrphy_ofh_dl_symbol_t;
/* The reference's fragmentation of one symbol of `flow` (ofh_uplane_fragment_size_calculator driven with mtu - headers as
 * the data flow drives it): up to `max` entries to `out`, the number of fragments to *n.  Host only.  It depends on the flow
 * alone, so every frame's place and length are known before the launch.  NRPHY_ERR_ARGUMENT for a flow that
 * nrphy_ofh_dl_validate refuses and for max below the number of fragments (*n is set all the same). */
int nrphy_ofh_dl_fragments(const nrphy_ofh_dl_flow_t* flow, uint32_t max, nrphy_ofh_dl_fragment_t* out, uint32_t* n);
/* Host only (no device work).  NRPHY_ERR_ARGUMENT for: an unknown compression type, a width outside 8..16 or an iq_scaling
 * that is not finite (what nrphy_ofh_compress refuses), ru_nof_prbs of 0 or above 275, static_compression above 1, mtu
 * above 9600 (MAX_ETH_FRAME_LENGTH), below 64 (the reference pads inside the buffer) or below headers + one PRB record (the
 * reference would ask its pool for frames for ever), grid_nof_subc that is no multiple of 12 or above 12 * ru_nof_prbs of a
 * flow a descriptor uses (the reference's first() would assert), flow >= n_flows, grid_index >= nof_grids,
 * port >= grid_nof_ports, symbol >= 14, subframe >= 10, slot >= 16, sfn >= 1024, non-zero reserved_ bytes, frame_stride
 * below a used flow's mtu or no multiple of 16, a symbol's frames -- frame_bytes of each -- not inside [0, frames_bytes),
 * and frames of two descriptors that overlap. */
int nrphy_ofh_dl_validate(uint32_t n_flows, const nrphy_ofh_dl_flow_t* flows, uint32_t n, const nrphy_ofh_dl_symbol_t* symbols,
                          uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc, uint64_t frames_bytes,
                          uint32_t frame_stride);
/* Validates, stages the two host arrays' digest in stream order (as nrphy_ofh_ul_write_grid and nrphy_grid_put do) and does
 * ONE launch for the whole batch: asynchronous on `stream`, NOT capturable.  n = 0 is NRPHY_OK with no work.  The kernel
 * writes frame_bytes bytes of every frame and no other byte of d_frames, as aligned 16-byte stores wherever a frame's
 * address allows; it reads the grid rows of the descriptors only.  d_grid and d_frames are 16-byte aligned. */
int nrphy_ofh_dl_write_frames(nrphy_ctx_t* ctx, uint32_t n_flows, const nrphy_ofh_dl_flow_t* flows, uint32_t n,
                              const nrphy_ofh_dl_symbol_t* symbols, const void* d_grid, uint32_t nof_grids, uint32_t grid_nof_ports,
                              uint32_t grid_nof_subc, uint8_t* d_frames, uint64_t frames_bytes, uint32_t frame_stride, void* stream);
/* Host-span form for one symbol (blocking): `row` is the symbol's grid_nof_subc cbf16 on the host, so symbol->flow,
 * grid_index and port must be 0; `frames` is a host buffer of frames_bytes of which only the frames' own bytes are
 * written.  Through the context's staging like every _host call. */
int nrphy_ofh_dl_frames_host(nrphy_ctx_t* ctx, const nrphy_ofh_dl_flow_t* flow, const nrphy_ofh_dl_symbol_t* symbol, const void* row,
                             uint32_t grid_nof_subc, uint8_t* frames, uint64_t frames_bytes, uint32_t frame_stride);

/* dft_processor::run (R/include/srsran/phy/generic_functions/dft_processor.h:34-73; generic impl
 * dft_processor_generic_impl.cpp:14-218).  Unnormalised DFT of `size` complex floats, `batch` of them
 * back to back.  inverse != 0 uses exp(+j...).  Sizes: every size of the reference's generic implementation
 * (dft_processor_generic_impl.cpp:190-208) -- 128, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096, 4608, 6144
 * (one workgroup per transform, in LDS; these are also the sizes nrphy_ofdm_plan_create accepts) and 9216, 12288,
 * 18432, 24576, 36864, 49152 (the PRACH sizes: a radix-3/6/12 column pass through a scratch copy of the batch,
 * allocated and released in stream order by the call, then LDS transforms of 3072 or 4096 points). */
int nrphy_dft_run(nrphy_ctx_t* ctx, uint32_t size, int inverse, uint32_t batch, const float* d_in, float* d_out,
                  void* stream);
/* Host-span form of dft_processor::run for one transform (blocking). */
int nrphy_dft_run_host(nrphy_ctx_t* ctx, uint32_t size, int inverse, const float* in, float* out);

/* ---- seams A and C on ONE device-resident grid: the downlink slot pipeline ----------------------------------------
 * What the reference does per slot -- the upper PHY's channel processors fill a resource grid
 * (R/lib/phy/upper/downlink_processor_single_executor_impl.cpp:52-215: configure_resource_grid, process_pdcch / _pdsch /
 * _ssb / _nzp_csi_rs, finish_processing_pdus -> send_resource_grid), the grid is handed to the lower PHY
 * (pdxch_processor_request_handler::handle_request, R/lib/phy/lower/processors/downlink/pdxch/pdxch_processor_impl.cpp:
 * 97-112) and the real-time thread asks for it one OFDM symbol at a time (pdxch_processor_baseband::process_symbol,
 * pdxch_processor_impl.cpp:47-95, calling ofdm_symbol_modulator::modulate per port) -- with the grid staying in HBM
 * from the first channel written to the last sample modulated: per slot the transport blocks go down and the IQ comes up,
 * the grid crosses PCIe only if the host asks for it (nrphy_dl_slot_read_grid).
 *
 * A pool owns `depth` slots, each with a stream, a device grid, pinned staging for transport blocks + plan tables and a
 * pinned IQ buffer.  Everything a slot is asked to do is enqueued on its stream in call order; no call allocates device
 * memory or waits for the device unless it says so (the control-channel writers and the sparse put stage their descriptors
 * through a stream-ordered allocation, as their stand-alone forms do).  Calls on ONE slot are serialised by the library (a lock per slot);
 * different slots may be driven from different threads.
 *
 *   nrphy_dl_slot_open      resource_grid::set_all_zero + a free slot: NRPHY_ERR_CAPACITY when all `depth` slots are open
 *   nrphy_dl_slot_pdsch     seam A for n PDUs of the slot (one plan, one launch; may be called more than once per slot --
 *                           pdsch_processor::process arrives PDU by PDU): the transport blocks are copied at the call
 *   nrphy_dl_slot_pdcch / _ssb / _csi_rs / _put    the other grid writers, as nrphy_pdcch_process ... on the slot's grid
 *   nrphy_dl_slot_load_grid a grid computed elsewhere (host span) replaces the slot's grid: seam C alone
 *   nrphy_dl_slot_modulate  seam C, submitted at grid hand-over: every symbol of every port of the slot is modulated
 *                           (nrphy_ofdm_run, or nrphy_ofdm_run_ci16 for a pool created with iq_format 1), ONE
 *                           device-to-host copy brings the IQ into the slot's pinned buffer, then `done(user, status,
 *                           slot_id)` runs on a thread of the HIP runtime (it must not call HIP or this library except
 *                           nrphy_dl_slot_iq / _poll).  Once per open.
 *   nrphy_dl_slot_poll      NRPHY_OK: the IQ is on the host; NRPHY_ERR_NOT_READY: not yet (or no modulate submitted);
 *                           an error code: the slot's stream failed.  An atomic load: what process_symbol calls.
 *   nrphy_dl_slot_wait      blocks until the modulate submitted for the slot has completed, returns its status
 *   nrphy_dl_slot_iq        pinned host samples of `port`: nof_samples = nrphy_ofdm_slot_size(cfg, slot index) complex
 *                           values (float32 pairs, or int16 pairs), symbols back to back, cyclic prefix first; valid from
 *                           completion until the slot is closed.  Pointer arithmetic only.
 *   nrphy_dl_slot_read_grid blocking: everything enqueued so far, then the grid [nof_ports][14][12 * bw_rb] cbf16 to the
 *                           host (resource_grid::get_reader() on a device-mirrored grid)
 *   nrphy_dl_slot_close     gives the slot back; waits for what it still has in flight
 * Statuses: NRPHY_ERR_ARGUMENT for a slot id that is not open or a call out of order (modulate twice, a writer after
 * modulate), NRPHY_ERR_INVALID_PDU as nrphy_pdsch_plan_create, NRPHY_ERR_CAPACITY when the slot's staging cannot take the
 * transport blocks (max_tb_bytes is per slot, all PDSCH calls together). */
typedef struct nrphy_dl_slots nrphy_dl_slots_t;
typedef void (*nrphy_dl_slot_done_fn)(void* user, int status, uint32_t slot_id);
typedef struct nrphy_dl_slots_cfg {
  nrphy_ofdm_config_t ofdm;         /* the lower PHY's modulator configuration (pdxch_processor_factories.cpp:41-48) */
  uint32_t            nof_ports;    /* grid ports = transmit ports */
  uint32_t            depth;        /* slots that can be open at once, 1..64 (the reference's request pool holds 16) */
  uint32_t            max_tb_bytes; /* transport-block bytes per slot, all PDUs together */
  uint32_t            iq_format;    /* 0 = complex float32 (baseband_gateway_buffer), 1 = complex int16 after the amplitude controller */
  nrphy_iq_wire_cfg_t wire;         /* iq_format 1 only */
} nrphy_dl_slots_cfg_t;
int nrphy_dl_slots_create(nrphy_ctx_t* ctx, const nrphy_dl_slots_cfg_t* cfg, nrphy_dl_slots_t** pool);
int nrphy_dl_slots_destroy(nrphy_dl_slots_t* pool); /* waits for everything in flight, then frees */
int nrphy_dl_slots_wait_free(nrphy_dl_slots_t* pool); /* blocks while all `depth` slots are open */
int nrphy_dl_slot_open(nrphy_dl_slots_t* pool, uint32_t* slot_id);
int nrphy_dl_slot_close(nrphy_dl_slots_t* pool, uint32_t slot_id);
int nrphy_dl_slot_pdsch(nrphy_dl_slots_t* pool, uint32_t slot_id, uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus,
                        const uint8_t* const* tbs);
int nrphy_dl_slot_put(nrphy_dl_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_grid_re_t* entries);
int nrphy_dl_slot_load_grid(nrphy_dl_slots_t* pool, uint32_t slot_id, const void* grid);
int nrphy_dl_slot_modulate(nrphy_dl_slots_t* pool, uint32_t slot_id, uint32_t subframe_slot_index, nrphy_dl_slot_done_fn done,
                           void* user);
int nrphy_dl_slot_poll(nrphy_dl_slots_t* pool, uint32_t slot_id);
int nrphy_dl_slot_wait(nrphy_dl_slots_t* pool, uint32_t slot_id);
const void* nrphy_dl_slot_iq(nrphy_dl_slots_t* pool, uint32_t slot_id, uint32_t port, uint32_t* nof_samples);
/* Wire-format pools (iq_format 1): the amplitude controller's raw measurements of the slot's buffer of `port` (sum and peak of
 * |x|^2 after the gain and before clipping, clipped parts, samples) in pinned host memory, valid like nrphy_dl_slot_iq;
 * nrphy_amplitude_metrics() turns them into amplitude_controller_metrics, what downlink_processor_baseband_impl reports per
 * buffer (R/lib/phy/lower/processors/downlink/downlink_processor_baseband_impl.cpp:238-264).  NULL for a float pool. */
const nrphy_amplitude_stats_t* nrphy_dl_slot_amplitude_stats(nrphy_dl_slots_t* pool, uint32_t slot_id, uint32_t port);
int nrphy_dl_slot_read_grid(nrphy_dl_slots_t* pool, uint32_t slot_id, void* grid);
/* For callers that keep more of the chain on the device: the slot's grid in HBM and the stream its work is ordered on. */
void* nrphy_dl_slot_device_grid(nrphy_dl_slots_t* pool, uint32_t slot_id);
void* nrphy_dl_slot_stream(nrphy_dl_slots_t* pool, uint32_t slot_id);
int nrphy_dl_slot_pdcch(nrphy_dl_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_pdcch_pdu_t* pdus);
int nrphy_dl_slot_ssb(nrphy_dl_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_ssb_pdu_t* pdus);
int nrphy_dl_slot_csi_rs(nrphy_dl_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_csi_rs_cfg_t* cfgs);

/* ---- receive side: UL-SCH information (TS 38.212 Section 6.3.2.4) ---------------------------------------------------------------
 * Replaces get_ulsch_information (R/include/srsran/ran/pusch/ulsch_info.h; impl R/lib/ran/pusch/ulsch_info.cpp:30-360 with
 * get_sch_segmentation_info, R/lib/ran/sch/sch_segmentation.cpp:30-63): the rate-matching sizes of a PUSCH that carries UL-SCH,
 * HARQ-ACK, CSI part 1 and CSI part 2 -- what nrphy_ulsch_demux_cfg_t, nrphy_uci_decoder_cfg_t and nrphy_pusch_decoder_cfg_t take
 * as inputs.  The fields are ulsch_configuration and ulsch_information.  Host arithmetic only; the float expressions keep the
 * reference's order of operations (the function is named ul_sch: the symbols with "ulsch" in them are the demultiplexer's). */
typedef struct nrphy_ulsch_info_cfg {
  uint32_t tbs_bits;                    /* transport-block size in bits; 0 = no UL-SCH */
  uint32_t modulation;                  /* NRPHY_MOD_* */
  float    target_code_rate;            /* R x 1024, in (0, 1024) */
  uint32_t nof_harq_ack_bits, nof_csi_part1_bits, nof_csi_part2_bits; /* O^ACK, O^CSI-1, O^CSI-2 */
  float    alpha_scaling;               /* alpha */
  float    beta_offset_harq_ack, beta_offset_csi_part1, beta_offset_csi_part2;
  uint32_t nof_rb;
  uint32_t start_symbol_index, nof_symbols;
  uint32_t dmrs_type;                   /* 1 or 2 */
  uint32_t dmrs_symbol_mask;            /* bit l = symbol l carries DM-RS; every bit inside [start, start + nof) */
  uint32_t nof_cdm_groups_without_data; /* type 1: 1..2, type 2: 1..3 */
  uint32_t nof_layers;                  /* 1..4 */
  uint32_t contains_dc;                 /* 0 or 1: the allocation overlaps the DC subcarrier */
} nrphy_ulsch_info_cfg_t;
typedef struct nrphy_ulsch_info {
  uint32_t has_sch;                     /* tbs_bits > 0; the six segmentation fields below are 0 without it */
  uint32_t tb_crc_bits, base_graph, nof_cb, nof_filler_bits_per_cb, lifting_size, nof_bits_per_cb; /* sch_information */
  uint32_t nof_ul_sch_bits, nof_harq_ack_bits, nof_harq_ack_rvd, nof_csi_part1_bits, nof_csi_part2_bits; /* G^UL-SCH, G^ACK, G^ACK_rvd, G^CSI-1, G^CSI-2 */
  uint32_t nof_harq_ack_re, nof_csi_part1_re, nof_csi_part2_re; /* Q'_ACK, Q'_CSI-1, Q'_CSI-2 */
  uint32_t nof_dc_overlap_bits;
} nrphy_ulsch_info_t;
/* NRPHY_OK, or NRPHY_ERR_ARGUMENT for what the reference asserts on -- a code rate outside (0, 1), CDM groups the DM-RS type does
 * not allow, no DM-RS symbol or one outside the allocation -- for sizes the structures cannot hold (an unknown modulation, more
 * than 275 PRB or 4 layers, symbols beyond the slot, a UCI part above 1706 bits, alpha or a beta offset that is negative or not
 * finite), and where the reference's unsigned subtractions would wrap: ceil(alpha N_RE) below the RE HARQ-ACK took, or more UCI RE
 * than the allocation has. */
int nrphy_ul_sch_info(const nrphy_ulsch_info_cfg_t* cfg, nrphy_ulsch_info_t* out);

/* ---- receive side: PUSCH processor ------------------------------------------------------------------------------------------------
 * Replaces pusch_processor::process (R/include/srsran/phy/upper/channel_processors/pusch/pusch_processor.h; impl
 * R/lib/phy/upper/channel_processors/pusch/pusch_processor_impl.cpp:115-298) and pusch_pdu_validator::is_valid: from the received
 * grid to the transport block and its CRC verdict, the HARQ-ACK and CSI part 1 payloads with their status, and the
 * channel_state_information record -- nrphy_pusch_chest_run, nrphy_pusch_demod_run, nrphy_ulsch_demux_run, nrphy_uci_decoder_run
 * and nrphy_pusch_decode_batch with the configurations nrphy_pusch_proc_derive gives, on one stream with no host step, followed
 * by one launch that writes a nrphy_pusch_result_t per PDU.  A PDU with a CSI part 2 description is refused here and taken by
 * nrphy_pusch_csi2_* (the next section).  Not covered, and refused: DM-RS type 2.  The EVM and the EVM-based SINR are not part
 * of these calls either -- they keep refusing NRPHY_PUSCH_SINR_EVM and reporting has_evm = 0 -- but of nrphy_pusch_evm_* below,
 * which take the EVM from the demodulator (nrphy_pusch_demod_run_evm).  Transform precoding is never enabled by these calls, as
 * in the reference's processor of this release; nrphy_pusch_tp_* below enable it per PDU. */
#define NRPHY_PUSCH_SINR_CHANNEL_ESTIMATOR 0u /* channel_state_information::sinr_type */
#define NRPHY_PUSCH_SINR_POST_EQUALIZATION 1u
#define NRPHY_PUSCH_SINR_EVM 2u               /* nrphy_pusch_evm_* with enable_evm = 1 only; refused by nrphy_pusch_proc_* */
typedef struct nrphy_pusch_pdu {              /* pusch_processor::pdu_t */
  uint32_t numerology, slot_index;            /* slot within the frame: < 10 * 2^numerology */
  uint32_t rnti, n_id;                        /* data scrambling: c_init = rnti * 2^15 + n_id */
  uint32_t scrambling_id, n_scid;             /* DM-RS */
  uint32_t modulation;                        /* mcs_descr: NRPHY_MOD_QPSK .. NRPHY_MOD_QAM256; NRPHY_MOD_PI2_BPSK with nrphy_pusch_tp_* */
  float    target_code_rate;                  /* mcs_descr: R x 1024 */
  uint32_t has_codeword;                      /* 0: no UL-SCH (tb_size_bytes must be 0 then); 1: rv, ldpc_base_graph, new_data hold */
  uint32_t rv, ldpc_base_graph, new_data;
  uint32_t tb_size_bytes;                     /* the size of `data` */
  uint32_t tbs_lbrm_bytes;                    /* > 0 */
  uint32_t nof_harq_ack, nof_csi_part1;       /* uci: payload bits, 0 = none */
  uint32_t nof_csi_part2_entries;             /* uci.csi_part2_size.entries.size(): 0 for nrphy_pusch_proc_*, nrphy_pusch_csi2_desc_t::nof_entries for nrphy_pusch_csi2_* */
  float    alpha_scaling, beta_offset_harq_ack, beta_offset_csi_part1, beta_offset_csi_part2;
  uint32_t start_symbol_index, nof_symbols;
  uint32_t dmrs_type;                         /* must be 1 */
  uint32_t dmrs_symbol_mask;
  uint32_t nof_cdm_groups_without_data;       /* must be 2 */
  uint32_t nof_tx_layers;                     /* 1 or 2 */
  uint32_t nof_rx_ports;                      /* 1..4 */
  uint32_t rx_ports[NRPHY_MAX_PORTS];         /* grid port of receive port i */
  uint32_t dc_position;                       /* grid subcarrier of DC, or NRPHY_PUSCH_CHEST_NO_DC */
  uint32_t reserved_;
  uint64_t prb_mask[NRPHY_PRB_WORDS];         /* freq_alloc.get_prb_mask(bwp_start_rb, bwp_size_rb): allocated PRBs, grid-indexed */
} nrphy_pusch_pdu_t;
typedef struct nrphy_pusch_proc_options {     /* pusch_processor_impl::configuration and the factory's choices */
  uint32_t dec_nof_iterations;                /* > 0 */
  uint32_t dec_enable_early_stop;             /* 0 or 1 */
  uint32_t csi_sinr_calc_method;              /* NRPHY_PUSCH_SINR_CHANNEL_ESTIMATOR or _POST_EQUALIZATION */
  uint32_t equalizer;                         /* NRPHY_EQ_ZF, NRPHY_EQ_MMSE (one layer only) */
} nrphy_pusch_proc_options_t;
/* The configurations of the five stages for one PDU.  uci[]: the messages present, HARQ-ACK before CSI part 1 (nof_uci of them). */
typedef struct nrphy_pusch_proc_derived {
  nrphy_ulsch_info_t        info;
  nrphy_pusch_chest_cfg_t   chest;            /* scaling = (float)10^(3 / 20) for two CDM groups without data */
  nrphy_pusch_demod_cfg_t   demod;
  nrphy_ulsch_demux_cfg_t   demux;            /* read only when nof_uci > 0: without UCI the UL-SCH stream is the demodulator's output */
  nrphy_uci_decoder_cfg_t   uci[2];
  nrphy_pusch_decoder_cfg_t decoder;          /* read only when has_decoder: nref from tbs_lbrm_bytes and the codeblocks of ldpc_base_graph */
  uint32_t                  nof_uci, has_decoder;
  uint32_t                  codeword_bits;    /* soft bits the demodulator writes */
  uint32_t                  nof_sch_bits;     /* soft bits of the UL-SCH stream (the demultiplexer's, or codeword_bits without UCI) */
} nrphy_pusch_proc_derived_t;
typedef struct nrphy_pusch_result {           /* one per PDU */
  uint32_t has_sch;                           /* the PDU has a codeword; the five fields below are 0 without one */
  uint32_t tb_crc_ok, nof_codeblocks, nof_codeblocks_ok, ldpc_iterations_sum, ldpc_iterations_max;
  uint32_t harq_ack_status, csi_part1_status; /* NRPHY_UCI_STATUS_*; UNKNOWN when the PDU carries none */
  uint32_t nof_harq_ack, nof_csi_part1;       /* payload bits, one per byte ... */
  uint64_t harq_ack_offset, csi_part1_offset; /* ... at these bytes of d_uci_bits */
  /* channel_state_information (channel_estimate::get_channel_state_information over layer 0 of the PDU's receive ports) */
  float    sinr_dB;                           /* the one of the next two that csi_sinr_calc_method selects */
  float    sinr_ch_estimator_dB, sinr_post_eq_dB;
  float    epre_dB, rsrp_dB;
  float    time_alignment_s;                  /* of the receive port with the best SNR */
  float    cfo_hz;                            /* of that port; 0 with has_cfo = 0 */
  uint32_t has_cfo;                           /* 0 with a single DM-RS symbol: the reference's optional is empty */
  uint32_t has_evm;                           /* 1 from nrphy_pusch_evm_* with enable_evm = 1, else 0 */
  float    evm;                               /* the demodulator's EVM (nrphy_pusch_demod_run_evm); 0 with has_evm = 0 */
} nrphy_pusch_result_t;
typedef struct nrphy_pusch_proc_plan nrphy_pusch_proc_plan_t;
/* NRPHY_OK, or NRPHY_ERR_ARGUMENT for what pusch_processor_validator_impl and assert_pdu refuse and for what any of the five stage
 * validators refuses for the derived configuration: a DM-RS type other than 1; CDM groups without data other than 2; layers outside
 * 1..2; tbs_lbrm_bytes 0; dc_position neither NRPHY_PUSCH_CHEST_NO_DC nor inside the grid; no rx port, more than 4, one outside the
 * grid or repeated; PRBs beyond the grid or none; symbols beyond the slot; a DM-RS symbol outside the allocation or none; a
 * modulation outside QPSK..256-QAM; rv above 3, a base graph other than 1 or 2, a codeword without bytes or bytes without a
 * codeword; sizes nrphy_ul_sch_info refuses, UCI soft bits the placement or the UCI decoder cannot take, an UL-SCH the decoder
 * cannot take; a CSI part 2 description; a PDU with neither a codeword nor a UCI bit; no decoder iteration; csi_sinr_calc_method
 * NRPHY_PUSCH_SINR_EVM (accepted by nrphy_pusch_evm_validate with enable_evm = 1 only) or unknown; an unknown equaliser or MMSE
 * with two layers.  No device work. */
int nrphy_pusch_proc_validate(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_proc_options_t* options, uint32_t grid_nof_ports,
                              uint32_t grid_nof_subc);
/* The stage configurations of a PDU nrphy_pusch_proc_validate accepts (the grid only bounds the checks).  No device work. */
int nrphy_pusch_proc_derive(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_proc_options_t* options, uint32_t grid_nof_ports,
                            uint32_t grid_nof_subc, nrphy_pusch_proc_derived_t* out);
/* The sizes of the PDU's HARQ blocks, those nrphy_pusch_decoder_sizes(cfg, 1, ...) gives for the derived decoder configuration;
 * both 0 for a PDU without codeword.  No device work: a caller lays out its arena before it makes a plan. */
int nrphy_pusch_proc_harq_bytes(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_proc_options_t* options, uint64_t* soft_bytes,
                                uint64_t* state_bytes);
/* n PDUs over a batch of grids [nof_grids][grid_nof_ports][14][grid_nof_subc] cbf16; PDU i reads grid grid_index[i].  Each PDU
 * with a codeword owns one soft block at byte harq_soft_offset[i] and one state block at byte harq_state_offset[i] (a multiple of
 * 64) of the caller's arena d_harq, which the caller keys by (rnti, HARQ process) across slots; the decoder's state layout is per
 * batch, not per transport block, so the plan decodes each PDU as a batch of one.  Its transport block goes to byte tb_offset[i]
 * of d_tb, its UCI payload to byte uci_offset[i] of d_uci_bits: nof_harq_ack bytes, then nof_csi_part1 bytes, one bit each.  The
 * three HARQ / transport-block arrays are not read for a PDU without codeword and may be NULL when no PDU has one; uci_offset
 * likewise for UCI.  Validates every PDU, derives everything, creates the stage plans, prepares the decoders and allocates the
 * plan's workspace: channel estimates, noise variances, measurements, codeword soft bits, the demultiplexed streams, SINR,
 * decoder results and scratch (blocking). */
int nrphy_pusch_proc_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_pdu_t* pdus, const nrphy_pusch_proc_options_t* options,
                                 const uint32_t* grid_index, uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                                 const uint64_t* harq_soft_offset, const uint64_t* harq_state_offset, const uint64_t* tb_offset,
                                 const uint64_t* uci_offset, nrphy_pusch_proc_plan_t** plan);
int nrphy_pusch_proc_plan_destroy(nrphy_pusch_proc_plan_t* plan);
int nrphy_pusch_proc_plan_harq_bytes(const nrphy_pusch_proc_plan_t* plan, uint32_t i, uint64_t* soft_bytes, uint64_t* state_bytes);
/* d_result: [n], 8-byte aligned.  d_harq (64-byte aligned), d_tb (both may be NULL when no PDU has a codeword), d_uci_bits (may be
 * NULL when no PDU has UCI).  The launch
 * order is the hand-written chain's: estimator; demodulator; demultiplexer, when a PDU of the plan has UCI; UCI decoder;
 * transport-block decoders, PDU after PDU; the result kernel, one wavefront per PDU, no atomics and no scratch, every sum in a
 * fixed order.  Asynchronous on `stream`; allocates nothing and touches no host memory (capturable; two runs give identical
 * bytes).  Runs of one plan must be ordered: the plan owns its workspace. */
int nrphy_pusch_proc_run(nrphy_pusch_proc_plan_t* plan, const void* d_grid, void* d_harq, uint8_t* d_tb, uint8_t* d_uci_bits,
                         nrphy_pusch_result_t* d_result, void* stream);
/* One PDU from and to host memory (blocking, on the GPU): grid [grid_nof_ports][14][grid_nof_subc] cbf16; harq_soft and harq_state
 * (the sizes of nrphy_pusch_proc_harq_bytes; NULL without codeword) are read and written, so a retransmission finds what the
 * transmission before it left; tb [tb_size_bytes] and uci_bits [nof_harq_ack + nof_csi_part1] may be NULL where the PDU has none.
 * Makes and releases a plan inside the call. */
int nrphy_pusch_proc_host(nrphy_ctx_t* ctx, const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_proc_options_t* options, const void* grid,
                          uint32_t grid_nof_ports, uint32_t grid_nof_subc, int8_t* harq_soft, uint8_t* harq_state, uint8_t* tb,
                          uint8_t* uci_bits, nrphy_pusch_result_t* result);
/* The processor with the EVM: pusch_processor_impl built over a demodulator that has an EVM calculator, and
 * pusch_processor_notifier_adaptor.h:154-163.  The three calls take the arguments of their nrphy_pusch_proc_* namesakes with the
 * options below, and there is one implementation: nrphy_pusch_proc_* are these calls with enable_evm = 0, and with enable_evm = 0
 * every result byte is theirs.  enable_evm above 1 or a non-zero reserved_ is NRPHY_ERR_ARGUMENT; NRPHY_PUSCH_SINR_EVM is
 * accepted only with enable_evm = 1.  With enable_evm = 1 the demodulator stage is nrphy_pusch_demod_run_evm, every record has
 * has_evm = 1 and the demodulator's EVM -- a PDU without codeword too --, and sinr_dB follows csi_sinr_calc_method: with
 * NRPHY_PUSCH_SINR_EVM it is -20 log10f(evm) - 3.7f, evaluated in float in the result kernel, +inf for an EVM of 0.  The plan is
 * a nrphy_pusch_proc_plan_t: nrphy_pusch_proc_run, nrphy_pusch_proc_plan_destroy and nrphy_pusch_proc_plan_harq_bytes take it
 * as they are.  nrphy_pusch_csi2_* keeps has_evm = 0. */
typedef struct nrphy_pusch_evm_options {
  nrphy_pusch_proc_options_t proc;
  uint32_t enable_evm;                        /* 0 or 1 */
  uint32_t reserved_;                         /* 0 */
} nrphy_pusch_evm_options_t;
int nrphy_pusch_evm_validate(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_evm_options_t* options, uint32_t grid_nof_ports,
                             uint32_t grid_nof_subc);
int nrphy_pusch_evm_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_pdu_t* pdus, const nrphy_pusch_evm_options_t* options,
                                const uint32_t* grid_index, uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                                const uint64_t* harq_soft_offset, const uint64_t* harq_state_offset, const uint64_t* tb_offset,
                                const uint64_t* uci_offset, nrphy_pusch_proc_plan_t** plan);
int nrphy_pusch_evm_host(nrphy_ctx_t* ctx, const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_evm_options_t* options, const void* grid,
                         uint32_t grid_nof_ports, uint32_t grid_nof_subc, int8_t* harq_soft, uint8_t* harq_state, uint8_t* tb,
                         uint8_t* uci_bits, nrphy_pusch_result_t* result);
/* The processor with transform precoding (DFT-s-OFDM): what the reference's releases after 24.04 do for a pusch_processor::pdu_t
 * whose dmrs is a dmrs_transform_precoding_configuration{n_rs_id}.  The calls take the arguments of their nrphy_pusch_evm_*
 * (nrphy_pusch_proc_*) namesakes and one descriptor per PDU, and there is one implementation: nrphy_pusch_evm_* and
 * nrphy_pusch_proc_* are these calls without descriptors (tp / tps == NULL), every byte as before; a descriptor with
 * transform_precoding = 0 is no descriptor.  A plan, and a slot, may mix PDUs with and without transform precoding.  With
 * transform_precoding = 1: the estimator stage is created with the low-PAPR DM-RS {1, n_rs_id} (nrphy_pusch_chest_plan_create_ex;
 * the PDU's scrambling_id is ignored), the derived demodulator configuration has transform_precoding = 1 and the demodulator
 * plan is created with NRPHY_PUSCH_DEMOD_TRANSFORM_PRECODING | NRPHY_PUSCH_DEMOD_PI2_BPSK; NRPHY_MOD_PI2_BPSK is accepted as the
 * PDU's modulation, and then qm = 1 in the demodulator, demultiplexer and decoder configurations and the UCI decoder's modulation
 * is pi/2-BPSK.  HARQ-ACK and CSI part 1 on the PUSCH and the EVM (enable_evm = 1, measured after the deprecoder) work as without
 * transform precoding.  NRPHY_ERR_ARGUMENT also for: pi/2-BPSK without transform precoding; transform precoding with two layers,
 * with n_scid other than 0, with a number of PRBs nrphy_transform_precoding_nof_prb_valid rejects or with n_rs_id above 1007;
 * transform_precoding above 1; everything the stage validators refuse; a CSI part 2 description (nrphy_pusch_csi2_* takes no
 * descriptor: CSI part 2 with transform precoding is not covered).  nrphy_pusch_tp_derive also writes the estimator's low-PAPR
 * description to lp_out (may be NULL).  The plan is a nrphy_pusch_proc_plan_t: nrphy_pusch_proc_run,
 * nrphy_pusch_proc_plan_destroy and nrphy_pusch_proc_plan_harq_bytes take it as they are. */
typedef struct nrphy_pusch_tp_desc {
  uint32_t transform_precoding;               /* 0 or 1 */
  uint32_t n_rs_id;                           /* 0..1007: dmrs_transform_precoding_configuration::n_rs_id */
} nrphy_pusch_tp_desc_t;
int nrphy_pusch_tp_validate(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_tp_desc_t* tp, const nrphy_pusch_evm_options_t* options,
                            uint32_t grid_nof_ports, uint32_t grid_nof_subc);
int nrphy_pusch_tp_derive(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_tp_desc_t* tp, const nrphy_pusch_evm_options_t* options,
                          uint32_t grid_nof_ports, uint32_t grid_nof_subc, nrphy_pusch_proc_derived_t* out,
                          nrphy_pusch_chest_lowpapr_t* lp_out);
int nrphy_pusch_tp_harq_bytes(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_tp_desc_t* tp, const nrphy_pusch_evm_options_t* options,
                              uint64_t* soft_bytes, uint64_t* state_bytes);
int nrphy_pusch_tp_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_pdu_t* pdus, const nrphy_pusch_tp_desc_t* tps,
                               const nrphy_pusch_evm_options_t* options, const uint32_t* grid_index, uint32_t nof_grids,
                               uint32_t grid_nof_ports, uint32_t grid_nof_subc, const uint64_t* harq_soft_offset,
                               const uint64_t* harq_state_offset, const uint64_t* tb_offset, const uint64_t* uci_offset,
                               nrphy_pusch_proc_plan_t** plan);
int nrphy_pusch_tp_host(nrphy_ctx_t* ctx, const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_tp_desc_t* tp,
                        const nrphy_pusch_evm_options_t* options, const void* grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                        int8_t* harq_soft, uint8_t* harq_state, uint8_t* tb, uint8_t* uci_bits, nrphy_pusch_result_t* result);

/* ---- receive side: PUSCH processor with CSI part 2 ---------------------------------------------------------------------------------
 * What pusch_processor_impl::process does with pdu.uci.csi_part2_size (pusch_processor_impl.cpp:57-86 and
 * pusch_processor_notifier_adaptor.h:268): once CSI part 1 has decoded `valid`, uci_part2_get_size
 * (R/lib/ran/uci/uci_part2_size_calculator.cpp) turns its payload into the size of part 2; a size above 0 redoes
 * get_ulsch_information, tells the demultiplexer (set_csi_part2) and the decoder (set_nof_softbits), and part 2 is decoded.  An
 * invalid part 1 or a size of 0 leaves the PDU as if it had no part 2: what nrphy_pusch_proc_run computes.
 *
 * Nothing is sized on the device.  A description has at most 2 entries of at most 4 index bits, so a PDU has few possible sizes:
 * the plan enumerates the distinct ones ("variants": 0 = no part 2, then the non-zero sizes ascending), derives for each the UL-SCH
 * information, the demultiplexer's placement, the UCI decoder's code and the transport-block decoder's length on the host with the
 * code of the stages, and the run chooses among them on the device: the launches of nrphy_pusch_proc_run up to the UCI decoder;
 * one launch that evaluates every description on its decoded part 1 and writes a select word per PDU; one demultiplexer launch,
 * one UCI decoder launch and the rate-dematcher launches of every variant, of which only the selected ones act; one LDPC decode
 * and one assembly per PDU; the result kernels.  One stream, no host step, no allocation.
 *
 * Part 2 is placed as TS 38.212 Section 6.2.7 places it and as a UE transmits it: from the first symbol without DM-RS on.  The
 * reference's demultiplexer is a stream and starts placing part 2 in the symbol that holds the last part 1 RE
 * (ulsch_demultiplex_impl.cpp:241-251, 539-543); the two differ only when part 1 spans several symbols that also hold REs reserved
 * for HARQ-ACK of at most 2 bits.  Refused: a description on a PDU without codeword (G^CSI-1 itself depends on whether part 2 is
 * present there, which the reference does not handle either), and what NRPHY_PUSCH_CSI2_MAX_SIZES bounds. */
#define NRPHY_PUSCH_CSI2_MAX_ENTRIES 2u     /* uci_part2_size_description::max_nof_entries */
#define NRPHY_PUSCH_CSI2_MAX_PARAMETERS 2u  /* ::max_nof_parameters */
#define NRPHY_PUSCH_CSI2_MAX_ENTRY_BITS 4u  /* ::max_nof_entry_bits: the widths of an entry's parameters sum to at most this */
#define NRPHY_PUSCH_CSI2_MAX_SIZES 16u      /* distinct non-zero sizes of one PDU (two full entries could give up to 256 sums: refused) */
#define NRPHY_PUSCH_CSI2_MAX_VARIANTS 17u   /* "no part 2" and the sizes */
typedef struct nrphy_pusch_csi2_entry {     /* uci_part2_size_description::entry */
  uint32_t nof_parameters;                  /* 0..2; the index is the concatenation of the parameters, the first one highest */
  uint32_t offset[NRPHY_PUSCH_CSI2_MAX_PARAMETERS]; /* of the parameter in the CSI part 1 payload: that bit is its most significant */
  uint32_t width[NRPHY_PUSCH_CSI2_MAX_PARAMETERS];  /* bits; offset + width <= nof_csi_part1 */
  uint32_t map_size;                        /* 1 << sum of the widths */
  uint32_t map[1u << NRPHY_PUSCH_CSI2_MAX_ENTRY_BITS]; /* index -> bits this entry adds to part 2 */
} nrphy_pusch_csi2_entry_t;
typedef struct nrphy_pusch_csi2_desc {      /* pusch_processor::pdu_t::uci.csi_part2_size */
  uint32_t                 nof_entries;     /* 0..2; 0 = no description */
  nrphy_pusch_csi2_entry_t entries[NRPHY_PUSCH_CSI2_MAX_ENTRIES];
} nrphy_pusch_csi2_desc_t;
typedef struct nrphy_pusch_csi2_result {    /* one per PDU, next to its nrphy_pusch_result_t */
  uint32_t status;                          /* NRPHY_UCI_STATUS_*; UNKNOWN (0) where no part 2 was extracted */
  uint32_t nof_csi_part2;                   /* payload bits, one per byte ... */
  uint64_t csi_part2_offset;                /* ... at this byte of d_uci_bits; both 0 where no part 2 was extracted */
  uint32_t nof_enc_bits;                    /* G^CSI-2 */
  uint32_t nof_ul_sch_bits;                 /* G^UL-SCH the transport block was decoded with */
  uint32_t variant;                         /* the row of nrphy_pusch_csi2_variants that was selected; 0 = no part 2 */
  uint32_t reserved_;
} nrphy_pusch_csi2_result_t;
typedef struct nrphy_pusch_csi2_plan nrphy_pusch_csi2_plan_t;
/* uci_part2_get_size: csi_part1_bits [nof_csi_part1], one bit per byte.  NRPHY_ERR_ARGUMENT for a description that
 * nrphy_pusch_csi2_validate would refuse for its structure alone.  Host arithmetic, no device. */
int nrphy_pusch_csi2_size(const nrphy_pusch_csi2_desc_t* desc, const uint8_t* csi_part1_bits, uint32_t nof_csi_part1, uint32_t* size);
/* NRPHY_OK, or NRPHY_ERR_ARGUMENT for: everything nrphy_pusch_proc_validate refuses for the PDU with nof_csi_part2_entries 0;
 * pdu->nof_csi_part2_entries != desc->nof_entries; more than 2 entries or 2 parameters; an entry's widths summing above 4;
 * map_size != 1 << sum of the widths; offset + width > nof_csi_part1; a description with nof_csi_part1 0 or without codeword; a
 * size above 1706; more than NRPHY_PUSCH_CSI2_MAX_SIZES distinct non-zero sizes; any size for which nrphy_ul_sch_info, the
 * placement (no soft bit left for part 2 included), the UCI decoder or the transport-block decoder refuses the configuration.  A
 * description with nof_entries 0 is the PDU without part 2.  No device work. */
int nrphy_pusch_csi2_validate(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_csi2_desc_t* desc, const nrphy_pusch_proc_options_t* options,
                              uint32_t grid_nof_ports, uint32_t grid_nof_subc);
/* The variant table of an accepted PDU: *nof_variants rows (1..NRPHY_PUSCH_CSI2_MAX_VARIANTS), sizes[0] = 0 and infos[0] the UL-SCH
 * information without part 2, then the distinct non-zero sizes ascending, each with its information.  sizes and infos have room for
 * NRPHY_PUSCH_CSI2_MAX_VARIANTS rows.  With these a caller can drive the stages by hand. */
int nrphy_pusch_csi2_variants(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_csi2_desc_t* desc, const nrphy_pusch_proc_options_t* options,
                              uint32_t grid_nof_ports, uint32_t grid_nof_subc, uint32_t* nof_variants, uint32_t* sizes,
                              nrphy_ulsch_info_t* infos);
/* As nrphy_pusch_proc_harq_bytes: the sizes do not depend on the variant. */
int nrphy_pusch_csi2_harq_bytes(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_csi2_desc_t* desc,
                                const nrphy_pusch_proc_options_t* options, uint64_t* soft_bytes, uint64_t* state_bytes);
/* nrphy_pusch_proc_plan_create with descs[n] (PDUs with and without description mix; pdus[i].nof_csi_part2_entries must equal
 * descs[i].nof_entries) and csi2_offset[n]: PDU i's part 2 payload goes to byte csi2_offset[i] of d_uci_bits, as many bytes as the
 * size that was selected, at most the largest of its sizes.  csi2_offset is not read for a PDU without description and may be NULL
 * when no PDU has one. */
int nrphy_pusch_csi2_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_pdu_t* pdus, const nrphy_pusch_csi2_desc_t* descs,
                                 const nrphy_pusch_proc_options_t* options, const uint32_t* grid_index, uint32_t nof_grids,
                                 uint32_t grid_nof_ports, uint32_t grid_nof_subc, const uint64_t* harq_soft_offset,
                                 const uint64_t* harq_state_offset, const uint64_t* tb_offset, const uint64_t* uci_offset,
                                 const uint64_t* csi2_offset, nrphy_pusch_csi2_plan_t** plan);
int nrphy_pusch_csi2_plan_destroy(nrphy_pusch_csi2_plan_t* plan);
/* The arguments of nrphy_pusch_proc_run and d_csi2_result: [n], 8-byte aligned.  For a PDU without description the
 * nrphy_pusch_result_t and every output byte are those of nrphy_pusch_proc_run.  The variants that are not selected write nothing:
 * not the soft buffers, not d_uci_bits, no status.  Asynchronous on `stream`; allocates nothing and touches no host memory.
 * Runs of one plan must be ordered. */
int nrphy_pusch_csi2_run(nrphy_pusch_csi2_plan_t* plan, const void* d_grid, void* d_harq, uint8_t* d_tb, uint8_t* d_uci_bits,
                         nrphy_pusch_result_t* d_result, nrphy_pusch_csi2_result_t* d_csi2_result, void* stream);
/* One PDU from and to host memory (blocking, on the GPU), as nrphy_pusch_proc_host.  csi2_bits: room for the largest size of the
 * description (NULL without one); the bytes behind the selected size keep the caller's.  csi2_result->csi_part2_offset is 0. */
int nrphy_pusch_csi2_host(nrphy_ctx_t* ctx, const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_csi2_desc_t* desc,
                          const nrphy_pusch_proc_options_t* options, const void* grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                          int8_t* harq_soft, uint8_t* harq_state, uint8_t* tb, uint8_t* uci_bits, uint8_t* csi2_bits,
                          nrphy_pusch_result_t* result, nrphy_pusch_csi2_result_t* csi2_result);


/* ---- receive side: OFDM demodulation of a run of symbols, from float or int16 samples --------------------------------------------
 * puxch_processor_impl::process_symbol (R/lib/phy/lower/processors/uplink/puxch/puxch_processor_impl.cpp:30-81) demodulates every
 * port of ONE symbol into the slot's grid as soon as its samples are in.  nrphy_ofdm_demod_run with a range: the layout is the
 * same -- d_iq [grid][port][slot_stride] samples, d_grid [grid][port][14][12 * bw_rb] cbf16 -- but only symbols [first_symbol,
 * first_symbol + nof_symbols) of every (grid, port) are read and only their grid rows are written; the samples of the other
 * symbols need not be valid.  NRPHY_IQ_CI16: a sample is two int16 (re, im), 4 bytes, at the same sample index, and each component
 * becomes float(x) * gain with gain = 1.0f / iq_scale formed once in single precision, the product rounded on its own, as
 * srsvec::convert(span<const int16_t>, float scale, span<cf_t>) does (R/lib/srsvec/conversion.cpp:67-129); the radio's samples
 * cross PCIe at 4 bytes.  iq_scale is ignored for NRPHY_IQ_CF32.  NRPHY_ERR_ARGUMENT, with no launch, for nof_symbols == 0 or a
 * range beyond the slot's symbols (12 with extended cyclic prefix), an unknown iq_format, for ci16 an iq_scale that is not positive
 * and finite, and a window offset not below the shortest cyclic prefix; nof_grids == 0 is NRPHY_OK with no launch.  Asynchronous
 * on `stream`. */
#define NRPHY_IQ_CF32 0u
#define NRPHY_IQ_CI16 1u
int nrphy_ofdm_demod_symbols(nrphy_ofdm_plan_t* plan, uint32_t nof_grids, const void* d_iq, uint32_t iq_format, float iq_scale,
                             const uint32_t* d_slot_index, uint32_t first_symbol, uint32_t nof_symbols, uint32_t window_offset,
                             void* d_grid, void* stream);

/* ---- the uplink slot pipeline: baseband samples to PUSCH, PUCCH and SRS results on one device-resident grid ----------------------
 * The receive-side twin of nrphy_dl_slots_*.  What the reference does per uplink slot -- the lower PHY demodulates symbol after
 * symbol into the slot's grid (puxch_processor_impl::process_symbol, puxch_processor_impl.cpp:30-97) and the upper PHY runs
 * process_pusch, process_pucch and process_srs on that grid (R/lib/phy/upper/uplink_processor_impl.cpp:86-170) -- with the grid
 * staying in HBM: per slot the samples go down and the results come up.
 *
 * A pool owns `depth` slots, each with a stream, a device grid, pinned sample staging and a device and a pinned result block sized
 * from the max_* fields.  Everything a slot is asked to do is enqueued on its stream in call order; no call allocates device
 * memory or waits for the device unless it says so -- except that a receiver call makes its plan with the stand-alone
 * *_plan_create, which allocates and uploads (blocking), under the context's host lock.  Calls on ONE slot are serialised by the
 * library (a lock per slot); different slots may be driven from different threads.
 *
 *   nrphy_ul_slot_open       a free slot (NRPHY_ERR_CAPACITY when all `depth` are open) for slot subframe_slot_index of the
 *                            subframe; its grid is zeroed on its stream, so symbols never delivered read as zero
 *   nrphy_ul_slot_samples    process_symbol for a run of symbols: port_samples[port] is a host span of those symbols' samples
 *                            (cyclic prefix + dft_size each, back to back) in the pool's format; copied into the pinned staging
 *                            at the symbols' place (a memcpy on the calling thread), then one host-to-device copy per port and
 *                            one nrphy_ofdm_demod_symbols launch.  Runs must be contiguous and in order, starting at 0.
 *   nrphy_ul_slot_load_grid  a host grid replaces the slot's grid; all symbols count as delivered
 *   nrphy_ul_slot_device_grid / _stream / _symbols_written   split 7.2: the caller runs nrphy_ofh_rx_run or
 *                            nrphy_ofh_ul_write_grid on the slot's stream into the slot's grid and declares that symbols
 *                            [0, upto) are there (upto may only grow, up to the symbols a slot has: 12 with extended CP)
 *   nrphy_ul_slot_pusch      process_pusch for n PDUs: nrphy_pusch_proc_plan_create + _run on the slot's grid and stream, with
 *                            the caller's HARQ arena (the offsets are those of nrphy_pusch_proc_plan_create)
 *   nrphy_ul_slot_pf01      process_pucch, formats 0 and 1: nrphy_pucch_run
 *   nrphy_ul_slot_pf2        process_pucch, format 2: nrphy_pf2_run
 *   nrphy_ul_slot_srs        process_srs: nrphy_srs_run
 *   nrphy_ul_slot_finish     once per open: after everything enqueued so far, ONE device-to-host copy brings the slot's result
 *                            block into pinned memory, then `done(user, status, slot_id)` runs on a thread of the HIP runtime (it
 *                            must not call HIP or this library except the accessors and nrphy_ul_slot_poll)
 *   nrphy_ul_slot_poll / _wait / _close   as the downlink's; close waits for what is in flight and destroys the slot's plans
 *   nrphy_ul_slot_read_grid  blocking: everything enqueued so far, then the grid [nof_ports][14][12 * bw_rb] cbf16 to the host
 * Each receiver call may come more than once per slot (PDUs arrive one by one): results append in call order, index i of an
 * accessor counts over all calls of its kind, and totals are bounded by the max_* fields (NRPHY_ERR_CAPACITY).  A receiver call
 * is accepted only when the last symbol of every allocation it reads has been delivered (else NRPHY_ERR_ARGUMENT), which is what
 * lets a PUCCH of symbols 0-1 run after the first two symbols.  A PDU the stand-alone plan call refuses gives that call's
 * status.  NRPHY_ERR_ARGUMENT for use out of order: samples not contiguous, anything after finish except poll, wait, the
 * accessors, read_grid and close, finish twice, an id that is not open.  A refused call enqueues nothing.
 *
 * Accessors (nrphy_ul_slot_pusch_results, _tb, _pusch_uci, _pf01_results, _format2_results, _sounding_results): pointer arithmetic
 * into the pinned result block, valid from completion until close.  Transport block i starts on a 4-byte boundary and holds zeros
 * where the CRC failed; the UCI bits of PDU i (_pusch_uci) are nof_harq_ack then nof_csi_part1 bytes, one bit each, and
 * harq_ack_offset / csi_part1_offset of its result are relative to them, as nrphy_pusch_proc_host gives them.  _format2_results
 * copies the status and the channel state information of format 2 PUCCH i out and points at its message bits;
 * _sounding_results are the records of nrphy_ul_slot_srs. */
typedef struct nrphy_ul_slots nrphy_ul_slots_t;
typedef void (*nrphy_ul_slot_done_fn)(void* user, int status, uint32_t slot_id);
typedef struct nrphy_ul_slots_cfg {
  nrphy_ofdm_config_t ofdm;       /* the lower PHY's demodulator configuration */
  uint32_t nof_ports;             /* grid ports = receive ports of the radio */
  uint32_t depth;                 /* slots open at once, 1..64 */
  uint32_t iq_format;             /* NRPHY_IQ_CF32 / NRPHY_IQ_CI16 */
  float    iq_scale;              /* ci16 only */
  uint32_t window_offset;
  uint32_t max_pusch, max_pucch, max_pf2, max_srs;   /* per slot, all calls together */
  uint32_t max_tb_bytes, max_uci_bits;               /* per slot, all PUSCH (and PF2 payload) together */
} nrphy_ul_slots_cfg_t;
/* d_harq: the caller's HARQ arena on the device (64-byte aligned; NULL if no PUSCH will carry a codeword). */
int nrphy_ul_slots_create(nrphy_ctx_t* ctx, const nrphy_ul_slots_cfg_t* cfg, void* d_harq, nrphy_ul_slots_t** pool);
int nrphy_ul_slots_destroy(nrphy_ul_slots_t* pool); /* waits for everything in flight, then frees */
int nrphy_ul_slots_wait_free(nrphy_ul_slots_t* pool); /* blocks while all `depth` slots are open */
int nrphy_ul_slot_open(nrphy_ul_slots_t* pool, uint32_t subframe_slot_index, uint32_t* slot_id);
int nrphy_ul_slot_close(nrphy_ul_slots_t* pool, uint32_t slot_id);
int nrphy_ul_slot_samples(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t first_symbol, uint32_t nof_symbols,
                          const void* const* port_samples);
int nrphy_ul_slot_load_grid(nrphy_ul_slots_t* pool, uint32_t slot_id, const void* grid);
void* nrphy_ul_slot_device_grid(nrphy_ul_slots_t* pool, uint32_t slot_id);
void* nrphy_ul_slot_stream(nrphy_ul_slots_t* pool, uint32_t slot_id);
int nrphy_ul_slot_symbols_written(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t upto);
int nrphy_ul_slot_pusch(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_pusch_pdu_t* pdus,
                        const nrphy_pusch_proc_options_t* options, const uint64_t* harq_soft_offset, const uint64_t* harq_state_offset);
/* nrphy_ul_slot_pusch with the options of nrphy_pusch_evm_plan_create: the same operation, the results append to the same list,
 * and a slot may mix both calls. */
int nrphy_pusch_evm_slot(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_pusch_pdu_t* pdus,
                         const nrphy_pusch_evm_options_t* options, const uint64_t* harq_soft_offset, const uint64_t* harq_state_offset);
/* nrphy_pusch_evm_slot with the descriptors of nrphy_pusch_tp_plan_create (tps may be NULL): the same operation, the results append
 * to the same list, and a slot may mix all three calls. */
int nrphy_pusch_tp_slot(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_pusch_pdu_t* pdus,
                        const nrphy_pusch_tp_desc_t* tps, const nrphy_pusch_evm_options_t* options, const uint64_t* harq_soft_offset,
                        const uint64_t* harq_state_offset);
int nrphy_ul_slot_pf01(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_pucch_cfg_t* cfgs);
int nrphy_ul_slot_pf2(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_pf2_cfg_t* cfgs);
int nrphy_ul_slot_srs(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_srs_cfg_t* cfgs);
int nrphy_ul_slot_finish(nrphy_ul_slots_t* pool, uint32_t slot_id, nrphy_ul_slot_done_fn done, void* user);
int nrphy_ul_slot_poll(nrphy_ul_slots_t* pool, uint32_t slot_id);
int nrphy_ul_slot_wait(nrphy_ul_slots_t* pool, uint32_t slot_id);
int nrphy_ul_slot_read_grid(nrphy_ul_slots_t* pool, uint32_t slot_id, void* grid);
const nrphy_pusch_result_t* nrphy_ul_slot_pusch_results(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t* n);
const uint8_t* nrphy_ul_slot_tb(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t i, uint32_t* nbytes);
const uint8_t* nrphy_ul_slot_pusch_uci(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t i, uint32_t* nbits);
const nrphy_pucch_result_t* nrphy_ul_slot_pf01_results(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t* n);
int nrphy_ul_slot_format2_results(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t i, const uint8_t** message, uint32_t* nbits,
                              uint32_t* status, nrphy_pf2_csi_t* csi);
const nrphy_srs_result_t* nrphy_ul_slot_sounding_results(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t* n);

/* ---- receive side: the OFDM PRACH demodulator from float or int16 samples -------------------------------------------------------
 * nrphy_prach_demod_run with a sample format.  The plan is the same: its element offsets (in_offset, in_port_stride) count samples
 * in either format.  NRPHY_IQ_CF32 is exactly nrphy_prach_demod_run (iq_scale is ignored).  NRPHY_IQ_CI16: a sample is two int16
 * (re, im), 4 bytes, at the same sample index (d_iq 4-byte aligned), and each component becomes float(x) * gain with gain = 1.0f /
 * iq_scale formed once in single precision, the product rounded on its own before the first butterfly, as
 * srsvec::convert(span<const int16_t>, float scale, span<cf_t>) does (R/lib/srsvec/conversion.cpp:67-129); everything behind the
 * load is the same code, so the two formats give the same bytes on equal values, on the single transform and on the split one.
 * NRPHY_ERR_ARGUMENT, with no launch, for an unknown iq_format and for ci16 an iq_scale that is not positive and finite.
 * Asynchronous on `stream`; allocates nothing, touches no host memory, uses no atomics (capturable). */
int nrphy_prach_window_demod_run(nrphy_prach_demod_plan_t* plan, const void* d_iq, uint32_t iq_format, float iq_scale,
                                 void* d_symbols, void* stream);

/* ---- the PRACH window pipeline: baseband samples to detected preambles ------------------------------------------------------------
 * What the reference's lower PHY does per PRACH occasion -- prach_processor_worker appends symbol after symbol to a window buffer
 * until get_prach_window_duration samples are there, then demodulates into the prach_buffer and notifies
 * (R/lib/phy/lower/processors/uplink/prach/prach_processor_worker.cpp:31-162) -- and what the upper PHY does with that buffer
 * (prach_detector::detect), with the buffer staying in HBM: per window the samples go down, in the radio's own format, and the
 * detections come up.  The sibling of nrphy_ul_slots_* for the one uplink channel whose window is not a slot.
 *
 * A pool owns `depth` windows, each with a stream, pinned and device sample staging of max_window_samples per port in the pool's
 * format, a device prach_buffer sized from the max_* fields, and a device and a pinned result block.  Everything a window is asked
 * to do is enqueued on its stream in call order; no call allocates device memory or waits for the device unless it says so --
 * except an open whose configurations differ from the window's last, below.  Calls on ONE window are serialised by the library
 * (a lock per window); different windows may be driven from different threads.
 *
 *   nrphy_prach_window_open     prach_processor_worker::handle_request: a free window (NRPHY_ERR_CAPACITY when all `depth` are
 *                               open) for one PRACH context, given as the demodulator's and the detector's configuration.  Both
 *                               must pass nrphy_prach_demod_validate / nrphy_prach_validate and agree (NRPHY_ERR_ARGUMENT): one
 *                               format; detect->ra_scs the spacing the format and the PUSCH numerology give; one nof_rx_ports;
 *                               demod->srate_hz the pool's.  PRACH port p takes its samples from radio port radio_port[p], which
 *                               must be below nof_radio_ports.  NRPHY_ERR_CAPACITY for more samples, ports or occasions than the
 *                               pool's max_* fields.  The window length is window_samples of nrphy_prach_demod_sizes.  The window
 *                               has one demodulator plan and one detector plan with an item per (td, fd) occasion, td outer,
 *                               reading the window's buffer in place.  PRACH configuration is cell-static: a window keeps the
 *                               plans of its last open and reuses them when both configurations and the port map are byte-equal;
 *                               only an open that differs makes new plans (an allocation and a blocking upload each, under the
 *                               context's host lock) and frees the old ones.  The buffer is zeroed on the window's stream.
 *   nrphy_prach_window_samples  accumulate_samples: radio_port_samples[r] is a host span of nof_samples samples of radio port r in
 *                               the pool's format (only the mapped ports are read).  *taken = min(window length - collected,
 *                               nof_samples) of them, from the front, are copied into the pinned staging behind what is there (a
 *                               memcpy on the calling thread), then one host-to-device copy per PRACH port.  taken may be 0 or
 *                               fewer than offered: that is no error.  The call that completes the window also enqueues
 *                               nrphy_prach_window_demod_run, nrphy_prach_run (no metric), ONE device-to-host copy of the result
 *                               block, and `done(user, status, window_id)` on a thread of the HIP runtime (it must not call HIP or
 *                               this library except the accessors and nrphy_prach_window_poll).  After that, NRPHY_ERR_ARGUMENT.
 *   nrphy_prach_window_device_buffer / _stream / _buffer_written   split 7.2: the caller runs nrphy_ofh_ul_write_prach on the
 *                               window's stream into the window's buffer (C-contiguous [port][td][fd][symbol][L_RA] complex f32 in
 *                               the dimensions of the open), then _buffer_written enqueues the detector, the result copy and the
 *                               callback.  Once per open; refused after a samples call, and a samples call after it is refused.
 *   nrphy_prach_window_poll / _wait / _close   as the slot pools': poll never blocks (NRPHY_ERR_NOT_READY until done), wait
 *                               blocks for a window whose detector is enqueued (NRPHY_ERR_ARGUMENT for one still collecting),
 *                               close waits for what is in flight and frees the window (its plans stay for the next open)
 *   nrphy_prach_window_read_buffer   blocking: everything enqueued so far, then the buffer to the host
 * NRPHY_ERR_ARGUMENT for an id that is not open.  A refused call enqueues nothing.
 * A device error in a samples or _buffer_written call that has begun to enqueue ends the window: the call returns the error, nothing
 * more is accepted, poll and wait give NRPHY_ERR_DEVICE and `done` does not run; close gives the window back.
 *
 * Accessors, valid from completion with status NRPHY_OK until close (NULL before, and for a window that failed):
 * nrphy_prach_window_results gives the n = nof_td * nof_fd result headers, td outer
 * (occasion = td * nof_fd + fd); nrphy_prach_window_preambles the 64 records of one occasion, as nrphy_prach_run writes them.
 * nrphy_prach_windows_plans_made counts the plan pairs the pool has made since it was created. */
typedef struct nrphy_prach_windows nrphy_prach_windows_t;
typedef void (*nrphy_prach_window_done_fn)(void* user, int status, uint32_t window_id);
typedef struct nrphy_prach_windows_cfg {
  uint32_t srate_hz;              /* the radio's sampling rate: every open's demod->srate_hz */
  uint32_t nof_radio_ports;       /* receive ports of the radio, 1..64 */
  uint32_t depth;                 /* windows open at once, 1..16 */
  uint32_t iq_format;             /* NRPHY_IQ_CF32 / NRPHY_IQ_CI16 */
  uint32_t max_window_samples;    /* per port */
  float    iq_scale;              /* ci16 only */
  uint32_t max_ports;             /* PRACH ports per window, 1..4 */
  uint32_t max_td_occasions;      /* 1..7 */
  uint32_t max_fd_occasions;      /* 1..8 */
} nrphy_prach_windows_cfg_t;
int nrphy_prach_windows_create(nrphy_ctx_t* ctx, const nrphy_prach_windows_cfg_t* cfg, nrphy_prach_windows_t** pool);
int nrphy_prach_windows_destroy(nrphy_prach_windows_t* pool); /* waits for everything in flight, then frees */
int nrphy_prach_windows_wait_free(nrphy_prach_windows_t* pool); /* blocks while all `depth` windows are open */
uint64_t nrphy_prach_windows_plans_made(nrphy_prach_windows_t* pool);
int nrphy_prach_window_open(nrphy_prach_windows_t* pool, const nrphy_prach_demod_cfg_t* demod, const uint32_t* radio_port,
                            const nrphy_prach_cfg_t* detect, nrphy_prach_window_done_fn done, void* user, uint32_t* window_id);
int nrphy_prach_window_close(nrphy_prach_windows_t* pool, uint32_t window_id);
int nrphy_prach_window_samples(nrphy_prach_windows_t* pool, uint32_t window_id, uint32_t nof_samples,
                               const void* const* radio_port_samples, uint32_t* taken);
void* nrphy_prach_window_device_buffer(nrphy_prach_windows_t* pool, uint32_t window_id);
void* nrphy_prach_window_stream(nrphy_prach_windows_t* pool, uint32_t window_id);
int nrphy_prach_window_buffer_written(nrphy_prach_windows_t* pool, uint32_t window_id);
int nrphy_prach_window_poll(nrphy_prach_windows_t* pool, uint32_t window_id);
int nrphy_prach_window_wait(nrphy_prach_windows_t* pool, uint32_t window_id);
int nrphy_prach_window_read_buffer(nrphy_prach_windows_t* pool, uint32_t window_id, void* symbols);
const nrphy_prach_result_t* nrphy_prach_window_results(nrphy_prach_windows_t* pool, uint32_t window_id, uint32_t* n);
const nrphy_prach_preamble_t* nrphy_prach_window_preambles(nrphy_prach_windows_t* pool, uint32_t window_id, uint32_t occasion);

#ifdef __cplusplus
}
#endif
#endif /* MI355_NRPHY_H */
