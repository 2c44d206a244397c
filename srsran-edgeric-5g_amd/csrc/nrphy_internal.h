// Internal declarations shared by the host side (nrphy_host.cpp, pdsch_plan_build.cpp and every *_host.cpp) and the HIP kernels of libmi355nrphy.so.
// Not part of the ABI (that is include/mi355_nrphy.h).
#pragma once

#include "mi355_nrphy.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nrphy {

// ---- LDPC base graphs -------------------------------------------------------------------------------------
// One lifted graph per (base graph, lifting size): 2 x 51 graphs, built once per context from the
// 3GPP TS 38.212 Tables 5.3.2-2/-3 edge list (nr_ldpc_bg.inc).  The role of the reference's
// ldpc_graph_impl array (R/lib/phy/upper/channel_coding/ldpc/ldpc_graph_impl.cpp:29-65), laid out for the GPU:
// per check row a contiguous run of packed edges (column * Zc << 16 | shift), the identity column of extension rows
// dropped, plus the three numbers that describe the dual-diagonal core (see ldpc_device.h).
constexpr int NOF_LIFTING_SIZES = 51;
constexpr int NOF_GRAPHS        = 2 * NOF_LIFTING_SIZES;
constexpr int MAX_BG_ROWS       = 46;
constexpr int MAX_BG_EDGES      = 316;

struct LiftedGraph {
  uint16_t row_ptr[MAX_BG_ROWS + 2]; // edges of row m: [row_ptr[m], row_ptr[m+1])
  uint16_t core_b;                   // P^b p0 = sum(aux): the odd shift out of column Kb
  uint16_t core_s0;                  // shift of (row 0, column Kb)
  uint16_t core_s3;                  // shift of (row 3, column Kb)
  uint16_t core_mid;                 // 1: row 1 has the third edge of column Kb (BG1); 2: row 2 (BG2)
  uint32_t edge[MAX_BG_EDGES];       // (column * Zc) << 16 | lifted shift; core rows: systematic columns only
};

// ---- Polar codes ---------------------------------------------------------------------------------------------------
// TS 38.212 Table 5.4.1.1-1, the sub-block interleaver pattern P(i): the one copy that the downlink (PDCCH, PBCH) and uplink (UCI)
// constructions and kernels initialise their tables from.
#define NR_POLAR_SUBBLOCK_PATTERN                                                                                       \
  {0, 1, 2, 4, 3, 5, 6, 7, 8, 16, 9, 17, 10, 18, 11, 19, 12, 20, 13, 21, 14, 22, 15, 23, 24, 25, 26, 28, 27, 29, 30, 31}

// ---- Gold sequence tables -----------------------------------------------------------------------------------
// x2 jump matrices: row r of (M2)^(2^k) as a 31-bit mask, k = 0..GOLD_JUMP_BITS-1 (state bit j = x2(n + j)).
constexpr int GOLD_JUMP_BITS  = 24;
constexpr int GOLD_X1_WORDS   = 1 << 16; // x1(n + 1600) for n < 2^21 bits, MSB-first words

constexpr uint32_t SCR_PARTS = 4; // workgroups sharing the scrambling sequence of one PDU (prologue)

constexpr int CRC_POW_WORDS = 288;     // >= 8448 / 32 + 1

struct GoldTables {
  uint32_t x2_jump[GOLD_JUMP_BITS][32];
  // x2_head[t][w]: mask over the 31-bit state giving bit t of word w of the next 31 words (w < 31): the first 992
  // sequence bits are linear in the state, so 31 lanes produce the 31 seed words of the word recurrence in parallel.
  uint32_t x2_head[32][32];
  uint32_t crc24b_pow32[CRC_POW_WORDS]; // x^(32 m) mod g_CRC24B(x): places a lane's partial CB-CRC
  uint32_t crc24b_table[256];           // byte table of CRC24B: (b x^24) mod g
  // crc24b_mul[m][n][v] = (v x^(4n)) x^(32 m) mod g: a lane's partial CB-CRC times x^(32 m), one look-up per nibble
  // of the partial instead of a 24-step shift-and-add multiplication.
  uint32_t crc24b_mul[CRC_POW_WORDS][6][16];
  // Modulation tables (TS 38.211 Section 5.1): qam_lut[Qm/2 - 1][index of Qm bits, first bit in the MSB] = the
  // un-normalised odd-integer symbol of the reference's ci8 table, as floats (re, im).
  float2 qam_lut[4][256];
};

// ---- PDSCH plan ---------------------------------------------------------------------------------------------
constexpr int RE_CHUNK = 512; // data RE handled by one wavefront
// Scratch region of a codeblock wave during LDPC encoding: doubled systematic blocks (2 * 22 * 12 words), the core rows'
// scratch (80 words), then the graph rows (codeblock_build_device.h, CbShared).
#define NRPHY_CB_U_GRAPH_OFFSET (2 * 22 * 12 + 80)

enum SymKind : uint32_t { SYM_NONE = 0, SYM_CONTIGUOUS = 1, SYM_TABLE = 2 };

// Everything the device needs to know about one PDU (derived on the host at plan creation).
struct PduDev {
  uint64_t tb_offset;      // byte offset of the transport block in d_tb (multiple of 4)
  uint64_t cw_bit_offset;  // bit offset of the codeword in the tap buffers (multiple of 32)
  uint32_t tb_bytes;
  uint32_t grid_index;
  uint32_t graph;          // index into the lifted graph array
  uint32_t zc;
  uint32_t kb;             // 22 or 10
  uint32_t K;              // Kb * Zc
  uint32_t info_bits;      // K' - L_cb
  uint32_t filler;         // F
  uint32_t tb_crc_bits;    // 16 or 24
  uint32_t cb_crc_bits;    // 0 or 24
  uint32_t zero_pad;
  uint32_t C;
  uint32_t n_short;
  uint32_t e_short;
  uint32_t e_long;
  uint32_t n_cb;
  uint32_t k0;
  uint32_t nof_rows;       // parity rows to compute (>= 4): enough for every bit rate matching reads
  uint32_t qm;
  uint32_t nof_layers;
  uint32_t nof_ports;
  uint32_t c_init;         // scrambling sequence initialisation
  uint32_t item_first;     // index of the PDU's first work item in the plan's (bucket-sorted) work list; its items follow in codeblock / chunk order
  uint32_t seed_first;     // seed slot of that first item; the others follow.  PDUs whose scrambling sequence and codeword layout are the same share their slots
  uint32_t scr_words;      // words of the scrambling sequence the prologue walks: ceil(G / 32) + read-ahead + a seed's length
  uint32_t scr_word_offset; // words form (PdschLaunch::scr_as_words): the first word of the PDU's sequence in scr_seq; PDUs that share the sequence share it
  uint32_t nof_re;
  uint32_t weights_offset; // floats: data weights (scaled) [nof_prg][P][L][2] in the plan's weight array
  uint32_t dmrs_weights_offset; // floats: unscaled weights, same shape
  uint32_t nof_prg;
  uint32_t prg_size_subc;
  // RE mapping: data RE r of OFDM symbol l sits on subcarrier
  //   SYM_CONTIGUOUS: sym_arg[l] + r,   SYM_TABLE: re_table[sym_arg[l] + r]
  uint32_t sym_re_start[NRPHY_NSYMB + 1]; // prefix count of data RE before symbol l
  uint32_t sym_kind[NRPHY_NSYMB];
  uint32_t sym_arg[NRPHY_NSYMB];
  // DM-RS
  uint32_t dmrs_symbol_mask;
  uint32_t dmrs_zero_other_group; // 1: CDM group 1 is reserved but unused by this PDU -> the DM-RS waves write its zeros
  uint32_t dmrs_c_init[NRPHY_NSYMB];
  uint32_t dmrs_ref_rb;
  uint32_t dmrs_seq_offset; // word offset of the DM-RS sequences (one per DM-RS symbol, in symbol order); PDUs that ask for the same ones share them
  uint32_t dmrs_seq_words;  // words per DM-RS symbol: sequence bits [0, 12 * (end_prb - dmrs_ref_rb))
  float    dmrs_amplitude;
  uint32_t prb_mask[2 * NRPHY_PRB_WORDS];
  uint32_t first_prb;
  uint32_t end_prb;
  uint32_t crc_first;       // the PDU's transport-block CRC shares: tb_crc_part[crc_first .. crc_first + crc_count)
  uint32_t crc_count;
};

// One wavefront of the codeblock kernel: RE [re_begin, re_begin + re_count) of codeblock cb of PDU pdu.
struct CbWork {
  uint32_t pdu;
  uint32_t cb;
  uint32_t re_begin; // first RE of the chunk, counted within the codeblock
  uint32_t re_count;
};

// One workgroup of the DM-RS kernel: OFDM symbol `symbol` of PDU `pdu`.
constexpr int DMRS_PRB_CHUNK = 32; // PRBs per DM-RS wavefront
// Transport-block CRC: one 256-thread workgroup reduces a 16 KiB region of the transport block.
#ifndef NRPHY_CRC_WORDS_PER_THREAD
#define NRPHY_CRC_WORDS_PER_THREAD 16
#endif
constexpr uint32_t TB_CRC_REGION_WORDS = 256 * NRPHY_CRC_WORDS_PER_THREAD;
constexpr uint32_t TB_CRC_REGION_BYTES = 4 * TB_CRC_REGION_WORDS;

// Tables of the transport-block CRC, per polynomial ([0] CRC24A, [1] CRC16).  A workgroup takes a 16 KiB region in four
// rounds of 16-byte loads: thread t owns the words 1024 i + 4 t + j (round i, j = 0..3).  It folds the four words of a round
// with Horner's rule in x^32 (table y32), the four rounds with y1k = x^(32 * 1024); the 256 partials, 128 bits apart, are
// folded by 64 lanes with y8k = x^(128 * 64), and a workgroup that walks several regions steps from one to the next with
// yz = x^(8 * TB_CRC_REGION_BYTES).  y[k][b] = (b x^(8k)) y mod g, so that a 32-bit partial advances with four independent
// look-ups.
struct TbCrcTables {
  uint32_t y32[2][4][256];
  uint32_t y1k[2][4][256];
  uint32_t y8k[2][4][256];
  uint32_t yz[2][4][256];
  uint32_t lane[2][64]; // x^(128 (63 - l)) mod g
};

struct DmrsWork {
  uint32_t pdu;
  uint32_t symbol;
  uint32_t prb_begin;
  uint32_t prb_end;
};

// One 256-thread workgroup of the sequence role: wave 0 walks words [first, first + count) of the PDU's scrambling sequence
// and stores them (words form) or the seeds of the work items that start there (seeds form); the PDU's first workgroup also generates its DM-RS sequences
// (waves 1-3, with_dmrs).  Long sequences are split over up to SCR_PARTS workgroups when the plan has few of them.  Only the
// first PDU that asks for a sequence gets work: a PDU that shares its scrambling sequence but not its DM-RS has one entry
// with count == 0 and with_dmrs set.
struct ScrWork {
  uint32_t pdu;
  uint32_t first;
  uint32_t count;
  uint32_t with_dmrs;
};

// One 256-thread workgroup of the TB-CRC role: regions [region, region + count) (16 KiB each) of the PDU's transport
// block, one after the other with the next region's words requested while the current one is reduced.  A region is
// reduced as if the transport block were zero-extended to the region's end; `factor` = x^(order + 8 (bytes - end of the
// LAST region)) mod g (a negative exponent for the last region of the block: x is invertible mod g) turns the workgroup's
// running remainder into its share of the CRC.
struct CrcWork {
  uint32_t pdu;
  uint32_t region;
  uint32_t factor;
  uint32_t count;
};
constexpr uint32_t TB_CRC_MAX_REGIONS_PER_WORK = 8;
constexpr uint32_t TB_CRC_TARGET_WORK          = 1024; // workgroups of the TB-CRC role a big batch aims at (4 per compute unit)

// Grid words no PDU of the plan maps must read as zero (resource_grid::set_all_zero in the reference).  Instead of
// clearing whole grids and overwriting most of them, the plan lists the uncovered runs and a few waves of the
// codeblock launch write zeros there: every grid word is written exactly once per run.
struct ZeroSeg {
  uint16_t symbol;
  uint16_t k0;
  uint16_t count;
  uint16_t pad_;
};
constexpr uint32_t ZERO_LONG_RUN = 32; // runs at least this long are cleared by the whole wave, shorter ones by one lane
struct ZeroWork {
  uint32_t grid;
  uint32_t port;
  uint32_t seg_begin;
  uint32_t seg_count; // segments [seg_begin, seg_begin + seg_count): the first seg_long of them are long runs
  uint32_t seg_long;
};

struct PdschLaunch {
  const ZeroWork*    zero_work;
  const ZeroSeg*     zero_segs;
  uint32_t           n_zero_work;     // zero-fill waves appended to the codeblock launch (0: caller cleared the grids)
  uint32_t           n_dmrs_in_launch; // DM-RS waves appended to the codeblock launch (0: separate launch)
  uint32_t*          scr;             // DM-RS sequences c(n) of every PDU, MSB-first words (prologue -> DM-RS waves)
  // The plan's distinct scrambling sequences (prologue -> codeblock waves), in one of two forms for the whole launch:
  //   seeds  [seed slot][32]: the first 31 words of the x2 part of the sequence from every work item's first word on
  //          (PduDev::seed_first; the codeblock waves expand them, gold_expand_seed_wave, and add the x1 table's words);
  //   words  the PduDev::scr_words words of every sequence, c = x1 ^ x2 (PduDev::scr_word_offset): taken while all of them fit
  //          an L2 (pdsch_plan_build.cpp, SCR_WORDS_BUDGET_BYTES), read by the codeblock waves like the x1 table.
  uint32_t*          scr_seq;
  uint32_t           scr_as_words;    // 1: words, 0: seeds
  const PduDev*      pdus;
  const CbWork*      work;
  const DmrsWork*    dmrs_work;
  const CrcWork*     crc_work;
  const ScrWork*     scr_work;
  uint32_t           n_scr_work;
  const TbCrcTables* tbcrc;
  uint32_t           n_crc_work;
  const float*       weights;
  const uint16_t*    re_table;
  const LiftedGraph* graphs;
  const GoldTables*  gold;
  const uint32_t*    x1_words;
  uint32_t*          tb_crc_part; // [n_crc_work] share of every 16 KiB region in its PDU's CRC, rewritten by every run
  uint32_t           n_pdu;
  uint32_t           n_work;
  uint32_t           work_base;      // index of work[0] in the plan's whole work list (a bucket launch starts inside it): PduDev::item_first counts from there
  uint32_t           n_dmrs_work;
  uint32_t           grid_nof_ports;
  uint32_t           grid_nof_subc;
  uint32_t           lds_lin_words;  // dynamic LDS carve of the codeblock kernel (words, multiples of 4): the codeblock ...
  uint32_t           lds_u_words;    // ... and the scratch region its stages share (codeblock_build_device.h, CbShared)
  uint32_t           profile_stage; // 0 = run everything; n > 0 = codeblock waves stop after stage n (NRPHY_PROFILE_STAGE)
  // 1: this run clears what it does not map (zero_grids): the DM-RS waves then also clear the resource elements of a CDM group
  // that is reserved (no data) but carries no pilots of the PDU; 0: like the reference's mapper, they leave those alone --
  // whatever another writer of the slot put there stays.
  uint32_t           zero_fill;
};

// Kernel launchers (defined in the .hip files).
hipError_t launch_prologue(const PdschLaunch& p, const uint8_t* d_tb, hipStream_t stream);
// Work items are sorted by bucket = (modulation order, layers): one output-stage specialisation each.
constexpr uint32_t CB_BUCKETS        = 16;
constexpr uint32_t CB_MIXED_MAX_WORK = 4096; // a mixed plan below this many work items takes the one-launch mixed kernel
inline uint32_t cb_bucket(uint32_t qm, uint32_t nof_layers)
{
  return (qm / 2u - 1u) * 4u + (nof_layers - 1u);
}
bool       codeblocks_take_bucket_launches(const PdschLaunch& p, const uint32_t* bucket_begin, int dispatch, uint32_t* nof_buckets);
hipError_t launch_codeblocks(const PdschLaunch& p, const uint32_t* bucket_begin, int dispatch, const uint8_t* d_tb,
                             uint32_t* d_grid, uint32_t* d_cw_rm, uint32_t* d_cw_scr, const hipStream_t* streams, uint32_t n_streams);
hipError_t launch_dmrs(const PdschLaunch& p, uint32_t* d_grid, hipStream_t stream);
hipError_t launch_ldpc_encode(const LiftedGraph* graphs, uint32_t graph, uint32_t kb, uint32_t zc, uint32_t n_cb,
                              const uint8_t* d_msg, uint32_t msg_stride, uint32_t out_bits, uint8_t* d_out,
                              uint32_t out_stride, hipStream_t stream);

// ---- LDPC decoder ("next" row, receive side) -------------------------------------------------------------------
// The whole lifted graph of one (base graph, lifting size) for the decoder: every edge of every check row in
// adjacency order (ascending variable index, the order that breaks ties between equal minima).
struct DecoderGraph {
  uint32_t row_ptr[MAX_BG_ROWS + 2]; // 32-bit: read with scalar loads (a 16-bit element goes through a vector load and a round trip to L2)
  uint32_t pair_ptr[MAX_BG_ROWS + 2]; // rows of two edges before row m: sum of ceil(degree / 2) (messages per edge in LDS)
  uint32_t quad_ptr[MAX_BG_ROWS + 2]; // rows of four edges before row m: sum of ceil(degree / 4) (the table of soft-bit addresses)
  uint32_t edge[MAX_BG_EDGES]; // (variable node * Zc) << 16 | lifted shift
};

constexpr uint32_t DEC_CRC_TABLE_WORDS = 8 * 16; // early-stop CRC: eight nibble tables per message word

struct LdpcDecodeLaunch {
  const DecoderGraph* graph;
  const uint32_t*     pair_addr;  // even lifting sizes: soft-bit addresses of (edge, pair of checks), [row of four edges][lane][4]; else null
  const int8_t*       llr;        // per codeblock: nof_llr soft bits (the codeblock without its first 2 Zc bits)
  uint2*              scratch;    // nof_slots slots of slot_bytes each: a codeblock's check records (8 bytes per check and layer) or its messages per edge
  uint32_t*           slot_flags;  // one word per slot (0 = free), all clear at launch; unused when every codeblock has a slot of its own
  uint32_t            nof_slots;  // >= the workgroups of this kernel the device can hold at once, <= codeblocks
  uint32_t            slot_bytes; // of one slot
  uint8_t*            out;        // per codeblock: Kb * Zc hard bits, packed MSB first
  uint32_t*           iterations; // per codeblock: iterations until the CRC passed, 0 = it did not (may be null)
  const uint32_t*     crc_weight; // per 32-bit word of the message DEC_CRC_TABLE_WORDS words: [nibble k][value v] = (v x^(4k)) x^(bits after the word) mod the CRC polynomial
  const uint8_t*      skip;       // per codeblock (may be null): non-zero = leave it alone (decoded earlier)
  uint8_t*            ok_flags;   // per codeblock (may be null): set to 1 when the CRC passed
  uint32_t            crc_at_end; // 1: check the CRC once, after max_iterations (no early stop)
  uint32_t            zc, bg_k, nof_nodes, nof_layers_max;
  uint32_t            nof_llr, llr_stride, out_stride, nof_filler;
  uint32_t            crc_poly, crc_order; // order 0: no early stop
  uint32_t            max_iterations;
  float               scaling_factor;
  // Two checks per lane with the messages per edge in LDS: in = the LDS bytes that takes for the layers the caller expects
  // (0: not wanted); launch_ldpc_decode() turns it into the launch's LDS size, or 0 when the messages stay in the slots.
  // Each codeblock decides by the layers its own soft bits ask for whether it fits.
  uint32_t            lm_lds_bytes;
  uint32_t            lds_tail_off;     // set by launch_ldpc_decode(): where the kernel's flags and scaling table sit in its LDS
  // How the message kernels scale a minimum m = 0 .. 120 to round(m * scaling_factor): 2 = (m * scale_fixed + 256) >> 9 in
  // 16-bit arithmetic, 1 = (unsigned)(m * scaling_factor + 0.5f), 0 = the table in LDS -- the cheapest the host has verified.
  uint32_t            scale_arithmetic;
  uint32_t            scale_fixed;
  // The context's knobs (Tunables) for launch_ldpc_decode(), -1 = not set; no kernel reads them.  pairs 0: one check per lane
  // whatever the lifting size; ldsmsg 0: messages never in LDS, 2: wherever a workgroup's LDS can hold them.
  int                 knob_pairs, knob_ldsmsg;
};
hipError_t launch_ldpc_decode(const LdpcDecodeLaunch& p, uint32_t n_cb, hipStream_t stream);

// ---- LDPC rate dematcher ("next" row, receive side) ---------------------------------------------------------------
enum DematchKind : uint32_t { DEMATCH_ZERO = 0, DEMATCH_FILL, DEMATCH_COPY, DEMATCH_COMBINE };
// One step of the reference's walk over the soft buffer: positions [begin, begin + count) are cleared, set to
// +infinity, or take / add elements [src, src + count) of the deinterleaved input.
struct DematchOp {
  uint32_t kind, begin, count, src;
};
constexpr uint32_t MAX_DEMATCH_OPS = 60;
struct DematchLaunch {
  const int8_t* in;  // per codeblock: rm_length soft bits as received
  int8_t*       out; // per codeblock: the soft buffer, block_length soft bits
  uint32_t      in_stride, out_stride, block_length, qm, cols, n_ops;
  uint32_t      in_stride_outer, out_stride_outer; // a second batch dimension (transport blocks of codeblocks)
  uint32_t      skip_load; // the operations write every soft bit of the block: the old contents need not be read
  uint32_t      disjoint;  // no two operations touch the same soft bit: they can run in any order, element by element
  const DematchOp* ops_ext; // the list in device memory when it has more than MAX_DEMATCH_OPS entries, else null
  // Null: unconditional.  Else the launch acts only when *select == select_value (every workgroup tests it and the others return
  // at once): one of several launches of which a word written earlier on the stream picks one.
  const uint32_t*  select       = nullptr;
  uint32_t         select_value = 0;
  DematchOp        ops[MAX_DEMATCH_OPS];
};
hipError_t launch_ldpc_dematch(const DematchLaunch& p, uint32_t n_cb, hipStream_t stream, uint32_t n_outer = 1);

// ---- PUSCH decoder: transport-block assembly ("next" row, receive side) --------------------------------------------
struct PuschAssembleLaunch {
  const uint8_t* cb_msg;      // [n_tb][C][msg_stride] decoded messages, packed MSB first
  uint8_t*       cb_ok;       // [n_tb][C] codeblock CRC flags (cleared when the transport-block CRC fails)
  const uint32_t* cb_iter;    // [n_tb][C] iterations of this call's decodes (0: failed or skipped)
  const uint8_t* skipped;     // [n_tb][C] 1 where this call did not run the decoder (CRC ok since an earlier transmission)
  uint8_t*       tb;          // [n_tb][tb_stride] transport blocks out
  uint32_t*      result;      // [n_tb][4]: tb_crc_ok, codeblocks with CRC ok, sum and max of iterations over decoded codeblocks
  const uint32_t* crc_weight; // [PUSCH_ASSEMBLE_THREADS] x^(8 * bytes behind run t of the block) mod CRC24A (the byte-wise form: unaligned blocks)
  const TbCrcTables* tbcrc;   // the context's TB-CRC tables and ...
  uint32_t       crc_factor;  // ... x^(24 + 8 (tb_bytes - end of the last 16 KiB region)) mod CRC24A (the form by regions)
  uint32_t       C, msg_stride, tb_stride, tb_bytes, cb_info_bits, max_iterations;
};
constexpr uint32_t PUSCH_ASSEMBLE_THREADS = 1024;
hipError_t launch_pusch_assemble(const PuschAssembleLaunch& p, uint32_t n_tb, hipStream_t stream);

// ---- NZP-CSI-RS ("next" row: other downlink grid writers) -------------------------------------------------------------
constexpr uint32_t CSI_RS_MAX_SEQ_WORDS = 128; // 2 * (3 * 275 skipped + 3 * 275 used) bits and some
// One CDM group of one signal (rows 1-5 have one OFDM symbol per group).
struct CsiRsWork {
  uint32_t grid_index, symbol, c_init;
  uint32_t advance, seq_len;          // sequence elements skipped / used
  uint32_t rb_begin, rb_stride, re_mask, n_re_prb;
  uint32_t nof_ports, first_layer, group_size;
  uint32_t weights_offset;            // floats: [nof_ports][nof_ports] complex of the signal
  float    amplitude;                 // config amplitude / sqrt(2)
};
struct CsiRsLaunch {
  const CsiRsWork*  work;
  const float*      weights;
  const GoldTables* gold;
  const uint32_t*   x1_words;
  uint32_t*         grid;
  uint32_t          grid_nof_ports, grid_nof_subc;
};
hipError_t launch_csi_rs(const CsiRsLaunch& p, uint32_t n_work, hipStream_t stream);
hipError_t launch_llr_descramble(const GoldTables* gold, const uint32_t* x1_words, const uint32_t* d_c_init, uint32_t n_cw,
                                 uint32_t length, const int8_t* d_in, size_t in_stride, int8_t* d_out, size_t out_stride,
                                 hipStream_t stream);
// ---- soft demodulator ("next" row, receive side) ---------------------------------------------------------------------
constexpr uint32_t DEMOD_MAX_PAIRS = 4;
struct DemodLaunch {
  uint32_t modulation; // NRPHY_MOD_*
  uint32_t span_len;   // symbols per span
  uint32_t nof_vector; // leading symbols of a span that take the reference's vector arithmetic
  float    range, scale; // quantisation range limit and 120 / range
  float    qam16_gain, qam16_threshold; // 4 / sqrt(10), 2 / sqrt(10)
  uint32_t nof_intervals[DEMOD_MAX_PAIRS];
  float    width[DEMOD_MAX_PAIRS], rcp_width[DEMOD_MAX_PAIRS];
  float    slope[DEMOD_MAX_PAIRS][16], intercept[DEMOD_MAX_PAIRS][16];
};
hipError_t launch_demodulate_soft(const DemodLaunch& p, uint32_t nof_spans, const float* d_symbols, const float* d_noise,
                                  int8_t* d_llr, hipStream_t stream);
// The host side of nrphy_demodulate_soft: parameters of a modulation for spans of span_len symbols (false: not one it demaps).
bool demod_params(uint32_t modulation, uint32_t span_len, DemodLaunch& p);

// ---- channel equaliser and PUSCH demodulator (receive side) -------------------------------------------------------------
constexpr uint32_t PUSCH_DEMOD_THREADS = 256; // a work item is up to this many data RE of one OFDM symbol, one per lane
struct PuschDemodDesc {                       // one PUSCH of a plan
  uint32_t grid_index, nof_rx_ports, nof_layers, qm;
  uint32_t equalizer, c_init, prb_first, dmrs_re_per_prb; // prb_first: its allocated PRBs at prbs[prb_first ...]
  uint32_t rx_ports[NRPHY_MAX_PORTS];
  uint8_t  dmrs_subc[NRPHY_NRE];              // the data subcarriers of a PRB on DM-RS symbols, ascending
  uint32_t item_first, nof_items;
  uint64_t ce_offset;                         // elements of d_ch_est
};
struct PuschDemodItem {
  uint32_t pusch, symbol, dmrs;               // dmrs != 0: the symbol carries DM-RS
  uint32_t re_first, count;                   // data RE [re_first, re_first + count) of the symbol
  uint32_t bit_offset;                        // codeword bit of the first soft bit of the item
  uint32_t span_pos, nof_vector;              // equalised symbols of the OFDM symbol before the item; the span's vector part
};
// ---- transform precoding: run-time mixed-radix transform of 12 * M_rb points (dft_mixed_device.h) ------------------------
constexpr uint32_t MIXED_DFT_THREADS    = 256;  // threads of the workgroup that runs one transform, whatever its size
constexpr uint32_t MIXED_DFT_MAX_POINTS = 3240; // 12 * 270, the largest valid transform-precoding size
constexpr uint32_t MIXED_DFT_MAX_STAGES = 8;    // 2916 = 4 * 3^6 takes 7
struct MixedDftPlan {
  uint32_t      n, nof_stages;
  uint8_t       radix[MIXED_DFT_MAX_STAGES];    // each of {2, 3, 4, 5}; their product is n
  const float2* twiddle;                        // exp(+j 2 pi k / n), k < n
  float         scale;                          // 1 / sqrt(n) as the reference rounds it: 1.0F / std::sqrt((float)n)
};
// The stage list of n = 12 * nof_prb points (twiddle left null); false when nof_prb is not a valid transform-precoding size.
bool       mixed_dft_stages(uint32_t nof_prb, MixedDftPlan& plan);
hipError_t launch_transform_deprecode(const MixedDftPlan& plan, uint32_t batch, const float2* in, float2* out, hipStream_t stream);

struct PuschTpItem {                          // one OFDM symbol of a transform-precoded PUSCH: one workgroup
  uint32_t pusch, symbol, count;              // count = 12 * M_rb data RE, the transform's size
  uint32_t bit_offset, nof_vector;            // as in PuschDemodItem
  uint32_t dft;                               // its entry of PuschDemodLaunch::dft
};
struct PuschEvmDesc {                         // one PUSCH of a plan, for the EVM: its OFDM symbols with data, ascending
  uint32_t nof_symbols;
  uint32_t item_first[NRPHY_NSYMB + 1];       // symbol k's partial sums are [item_first[k], item_first[k + 1]) of evm_partial
  uint32_t count[NRPHY_NSYMB];                // n_s = data RE x layers: the block evm_calculator::calculate is handed
};
struct PuschDemodLaunch {
  const PuschDemodDesc* desc;
  const PuschDemodItem* items;
  const PuschTpItem*    tp_items;             // their partial sums follow those of `items`
  const MixedDftPlan*   dft;                  // one per distinct transform size of the plan
  const uint16_t*       prbs;
  const DemodLaunch*    demod;                // [5]: QPSK, 16-QAM, 64-QAM, 256-QAM, pi/2-BPSK
  const GoldTables*     gold;
  const uint32_t*       x1_words;
  const uint32_t*       grid;
  const uint32_t*       ch;
  const float*          noise;                // [pusch][NRPHY_MAX_PORTS]
  int8_t*               llr;
  uint64_t              llr_stride;
  double*               partial;              // [item][2]: sum and count of the finite equalised noise variances
  float*                sinr;                 // may be null
  uint32_t              grid_nof_ports, grid_nof_subc, n_pusch, n_items, n_tp_items;
  // The EVM (nrphy_pusch_demod_run_evm); evm null: not computed, and nothing below is read.
  const PuschEvmDesc*   evm_desc;
  double*               evm_partial;          // [item]: sum of |m - x|^2 over the item's equalised symbols
  float*                evm;                  // [pusch]
  float                 evm_scale[5];         // the mapper's float scale per entry of `demod`
};
hipError_t launch_pusch_demod(const PuschDemodLaunch& p, hipStream_t stream);
struct EqualizeLaunch {
  uint32_t        algorithm, n_batch, nof_re, nof_layers, nof_rx_ports;
  float           tx_scaling;
  const uint32_t* rx;
  const uint32_t* ch;
  const float*    noise;
  float*          eq;
  float*          eq_nvars;
};
hipError_t launch_channel_equalize(const EqualizeLaunch& p, hipStream_t stream);
// ---- PUSCH DM-RS channel estimator (receive side) -----------------------------------------------------------------------
constexpr uint32_t PUSCH_CHEST_TA_WINDOW  = 144;  // time_alignment_estimator_dft_impl: (144 / 2) * 4096 / 2048 bins per side
constexpr uint32_t PUSCH_CHEST_MAX_LAYERS = 2;
struct PuschChestDesc {                        // one PUSCH of a plan
  uint32_t grid_index, nof_rx_ports, nof_layers, nprb;
  uint32_t prb_first;                          // its allocated PRBs at prbs[prb_first ...]
  uint32_t first_symbol, nof_symbols, nof_dmrs; // nof_dmrs: DM-RS symbols, dmrs_symbol[0 .. nof_dmrs)
  uint32_t nwords;                             // Gold words per DM-RS symbol (from c(0), up to the last allocated PRB)
  uint32_t ntaps, nof_v;                       // FIR taps (5, 11, 15) and virtual pilots per side
  uint32_t dc;                                 // grid subcarrier whose estimate is zeroed (NRPHY_PUSCH_CHEST_NO_DC: none)
  uint32_t scs_hz;
  uint32_t rx_ports[NRPHY_MAX_PORTS];
  uint32_t dmrs_symbol[NRPHY_NSYMB];
  union {
    uint32_t c_init[NRPHY_NSYMB];              // Gold DM-RS: per DM-RS symbol
    struct {                                   // low-PAPR DM-RS (low_papr_device.h): the same sequence on every DM-RS symbol
      uint32_t circle;                         // 8 (tables), 62 (5 PRB) or 2 N_zc: the size of the unit circle
      uint32_t u;                              // n_rs_id mod 30
      uint32_t n_zc, q;                        // 6 nprb >= 36: largest prime below it and the Zadoff-Chu root
      int8_t   phi[24];                        // 1 .. 4 PRB: phi(n) of group u
    } lp;
  };
  float    epoch[NRPHY_NSYMB];                 // symbol start epochs (initialize_symbol_start_epochs), in symbols
  float    taps[16];
  float    beta, ls_scale;                     // ls_scale = 1 / (nof_dmrs * beta), in float
  uint64_t ce_offset;                          // elements of d_ch_est
  uint64_t row_offset;                         // words of the scratch rows: [port][layer][12 nprb]
};
struct PuschChestLaunch {
  const PuschChestDesc*     desc;
  const uint32_t*           jobs;              // (pusch << 8) | (port << 4) | layer
  const uint16_t*           prbs;
  const float2*             twiddle;           // the context's e^{j 2 pi i / 2048}, i < 2048
  const GoldTables*         gold;
  const uint32_t*           x1_words;
  const uint32_t*           grid;
  uint32_t*                 ch;
  float*                    noise_vars;        // [pusch][NRPHY_MAX_PORTS]
  nrphy_pusch_chest_meas_t* meas;              // [pusch][NRPHY_MAX_PORTS][PUSCH_CHEST_MAX_LAYERS], may be null
  uint32_t*                 rows;              // scratch: interpolated rows, cbf16
  float2*                   rot;               // scratch: [job][14] CFO phasors
  uint32_t                  grid_nof_ports, grid_nof_subc, n_jobs;
};
// The first n_gold jobs are of PUSCHs with Gold DM-RS, the others of PUSCHs with low-PAPR DM-RS (desc.lp).
hipError_t launch_pusch_chest(const PuschChestLaunch& p, uint32_t n_gold, hipStream_t stream);
// The first kernel alone, for p.n_jobs low-PAPR jobs (launch_pusch_chest calls it; pusch_chest_lowpapr_kernels.hip).
void launch_pusch_chest_lowpapr(const PuschChestLaunch& p, hipStream_t stream);
// out[n] = the low-PAPR DM-RS of desc[0], n < 6 nprb.
hipError_t launch_pusch_lowpapr_sequence(const PuschChestDesc* desc, float2* out, hipStream_t stream);
// ---- PRACH detector (receive side) ----------------------------------------------------------------------------------------
constexpr uint32_t PRACH_L_LONG = 839, PRACH_L_SHORT = 139, PRACH_N_LONG = 1024, PRACH_N_SHORT = 256;
struct PrachTables {                           // per context
  float2 cexp_long[4 * PRACH_L_LONG];          // polar(sqrtf(L), float(2 pi) float(i) / float(4 L)): complex_exponential_table
  float2 cexp_short[4 * PRACH_L_SHORT];
  float2 tw_long[PRACH_N_LONG];                // exp(+j 2 pi k / N)
  float2 tw_short[PRACH_N_SHORT];
};
struct PrachSequence {                         // what the generator needs for one preamble or root
  uint16_t u, factor, offset, shift;           // sequence number, u^-1 mod L, phase index of y[0], cyclic shift C_v
};
struct PrachDesc {                             // one occasion of a plan
  uint64_t sym_offset;                         // elements of d_symbols
  double   sample_rate_hz;                     // N x spacing
  uint32_t is_long, nof_symbols, nof_rx_ports;
  uint32_t n_cs, nof_shifts, nof_sequences;
  uint32_t win_width, win_margin, max_delay;   // correlation samples
  uint32_t delay_end;                          // a delay is reported below ceil(float(max_delay) * 0.8)
  uint32_t start, end;                         // monitored preambles [start, end)
  uint32_t group_log2;                         // lanes per window: the smallest power of two >= win_width, at most 64
  float    threshold;
  float    modsq_scale, win_scale;             // 1 / float(N L L), float(N) / float(L)
  float    time_resolution_s, time_advance_max_s;
  PrachSequence seq[NRPHY_PRACH_MAX_PREAMBLES]; // the root of sequence i (shift 0)
};
struct PrachLaunch {
  const PrachDesc*        desc;
  const uint32_t*         jobs_long;           // (occasion << 8) | sequence
  const uint32_t*         jobs_short;
  const PrachTables*      tables;
  const float2*           symbols;
  nrphy_prach_result_t*   result;              // [n]
  nrphy_prach_preamble_t* preambles;           // [n][64]
  float*                  metric;              // [n][64][metric_stride], may be null
  uint32_t*               rssi_ok;             // scratch [n]: the RSSI is a normal number
  uint64_t                port_stride, symbol_stride;
  uint32_t                n, n_jobs_long, n_jobs_short, metric_stride;
};
hipError_t launch_prach_detect(const PrachLaunch& p, hipStream_t stream);
// y[n], n < L, of one sequence into d_y (blocking forms only).
hipError_t launch_prach_generate(const PrachTables* tables, PrachSequence seq, uint32_t is_long, float2* d_y, hipStream_t stream);
// ---- OFDM PRACH demodulator (receive side) --------------------------------------------------------------------------------
struct PrachDemodDesc {                        // one configuration of a plan
  const float2* tw_total;                      // exp(+j 2 pi k / dft_size), the context's table
  uint64_t      fd_stride;
  uint32_t      n1, n_total;                   // dft_size = n_total = n1 x the LDS transform's size
  uint32_t      seq_len, spacing, span;        // L_RA; bins between frequency-domain occasions; (nof_fd - 1) spacing + L_RA
  uint32_t      first_bin, first_bin_lds;      // bin of element 0 of occasion 0, and the same modulo the LDS transform's size
};
struct PrachDemodJob {                         // one workgroup: a symbol of (item, port, time-domain occasion)
  uint64_t in_offset, out_offset;              // first sample of the symbol; element 0 of frequency-domain occasion 0
  uint32_t desc, reserved;
};
struct PrachDemodLaunch {
  const PrachDemodDesc* desc;
  const PrachDemodJob*  jobs;                  // the jobs of this transform size
  const float2*         tw_lds;                // the table of the LDS transform's size
  const void*           samples;               // complex f32, or complex int16 (ci16): the offsets count samples in either
  float2*               symbols;
  uint32_t              n_jobs;
  uint32_t              ci16;                  // NRPHY_IQ_CI16
  float                 iq_gain;               // ci16: 1.0f / iq_scale, rounded once on the host
};
hipError_t launch_prach_demod(uint32_t lds_size, const PrachDemodLaunch& p, hipStream_t stream);
// ---- PUCCH formats 0 and 1 (receive side) ---------------------------------------------------------------------------------
struct PucchTables {                           // per plan
  float2 base[30][NRPHY_NRE];                  // exp(j phi(n) pi / 4) of group u: the reference's 8-entry exponential table
  float2 shift[24];                            // polar(1, float(2 pi) float(i) / 24): cyclic shift alpha n = entry (2 alpha n) % 24
  float2 occ[7][7][7];                         // w_i(m) of length N at [N - 1][i][m]: polar(1, TWOPI phi / N)
};
struct PucchDesc {                             // one PUCCH of a plan
  uint32_t format, grid_index, nof_rx_ports;
  uint32_t first_symbol, nof_symbols;
  uint32_t prb[2];                             // grid PRB of the first and of the second hop (equal without hopping)
  uint32_t hopping;                            // format 1: 1 = the second hop starts at first_symbol + nof_symbols / 2
  uint32_t u, occ;                             // sequence group n_id % 30; time-domain OCC index
  uint32_t nof_harq_ack, sr_opportunity;
  uint32_t scs_khz;
  float    cfo_dt[2];                          // per hop: epoch of its second DM-RS symbol minus that of its first, in symbols
  uint8_t  rx_ports[NRPHY_MAX_PORTS];
  uint8_t  alpha[NRPHY_NSYMB];                 // (m_0 + n_cs(l)) % 12 of allocation symbol l - first_symbol (m_cs = 0)
  uint8_t  pad_[2];
  uint64_t ce_offset;                          // elements of d_ch_est
};
struct PucchLaunch {
  const PucchDesc*          desc;
  const PucchTables*        tables;
  const uint32_t*           grid;
  nrphy_pucch_result_t*     result;            // [n]
  nrphy_pusch_chest_meas_t* meas;              // [n][NRPHY_MAX_PORTS], may be null
  uint32_t*                 ch;                // may be null
  uint32_t                  grid_nof_ports, grid_nof_subc, n;
};
hipError_t launch_pucch(const PucchLaunch& p, hipStream_t stream);
// ---- PUCCH format 2 (receive side) ------------------------------------------------------------------------------------------
constexpr uint32_t PF2_MAX_PRB = 16, PF2_MAX_SYMBOLS = 2;
constexpr uint32_t PF2_PILOTS_PER_PRB = 4, PF2_DATA_PER_PRB = 8; // subcarriers 1, 4, 7, 10 carry DM-RS, the other eight data
constexpr uint32_t PF2_TW_WORDS = 1024;                       // e^{j 2 pi i / 4096}, i < 1024: the other quadrants by symmetry
struct Pf2Desc {                                              // one PUCCH of a plan
  uint32_t grid_index, nof_rx_ports, nprb, prb0;              // prb0: first grid PRB (bwp_start_rb + starting_prb)
  uint32_t first_symbol, nof_symbols;
  uint32_t c_init_dmrs[PF2_MAX_SYMBOLS];                      // per symbol of the allocation
  uint32_t c_init_data;                                       // rnti 2^15 + n_id
  uint32_t dmrs_words;                                        // Gold words per symbol, from c(0) up to the last pilot's bits
  uint32_t ntaps, nof_v;                                      // FIR taps (3, 7, 11) and virtual pilots per side (4, 3, 5)
  uint32_t scs_hz;
  uint32_t nof_vector;                                        // leading data REs that take the demapper's vector arithmetic
  uint32_t rx_ports[NRPHY_MAX_PORTS];
  float    epoch[PF2_MAX_SYMBOLS];                            // start epochs of the allocation's symbols, in symbols
  float    taps[12];
  float    ls_scale;                                          // 1 / nof_symbols, in float
  uint32_t pad_;
  uint64_t llr_offset;                                        // bytes of d_llr
  uint64_t ce_offset;                                         // elements of d_ch_est
};
struct Pf2Launch {
  const Pf2Desc*            desc;
  const float2*             twiddle;                          // the context's e^{j 2 pi i / 4096}: its first PF2_TW_WORDS are read
  const GoldTables*         gold;
  const uint32_t*           x1_words;
  const uint32_t*           grid;
  int8_t*                   llr;
  nrphy_pf2_csi_t*          csi;                              // [n]
  nrphy_pusch_chest_meas_t* meas;                             // [n][NRPHY_MAX_PORTS], may be null
  uint32_t*                 ch;                               // may be null
  float                     demod_range, demod_scale;         // the QPSK demapper's quantisation range and 120 / range
  uint32_t                  grid_nof_ports, grid_nof_subc, n;
};
hipError_t launch_pf2(const Pf2Launch& p, hipStream_t stream);
// ---- SRS channel estimator (receive side) ----------------------------------------------------------------------------------
constexpr uint32_t SRS_DFT_SIZE    = 4096;                    // the time alignment estimator's inverse DFT
constexpr uint32_t SRS_MAX_SEQ     = 272 * NRPHY_NRE / 2;     // 1632: C_SRS 63, B_SRS 0, comb 2
constexpr uint32_t SRS_CEXP_SIZE   = 1024;                    // the compensation's unit circle
constexpr uint32_t SRS_CS_SIZE     = 24;                      // the cyclic shifts' unit circle
constexpr uint32_t SRS_PATHS       = NRPHY_MAX_PORTS * NRPHY_MAX_PORTS; // workgroups per SRS: [rx][tx]
struct SrsDesc {                                              // one SRS of a plan
  uint32_t grid_index, nof_rx_ports, nof_tx_ports;
  uint32_t first_symbol, nof_symbols;
  uint32_t comb, M;                                           // sequence length, common to the antenna ports
  uint32_t window;                                            // searched bins on each side: floor(max_ta scs 4096)
  uint32_t n_zc, q;                                           // M >= 36: largest prime below M and the Zadoff-Chu root
  uint32_t scs_hz;
  float    symbol_scale;                                      // float(1.0 / nof_symbols)
  uint32_t rx_ports[NRPHY_MAX_PORTS];
  uint32_t k0[NRPHY_MAX_PORTS];                               // first subcarrier of antenna port p
  uint32_t cs_step[NRPHY_MAX_PORTS];                          // n_cs 24 / n_cs_max of antenna port p
  int8_t   phi[24];                                           // M = 12, 24: phi(n) of group u
};
struct SrsLaunch {
  const SrsDesc*      desc;
  const float2*       twiddle;                                // the context's exp(+j 2 pi k / 4096)
  const float2*       cs_table;                               // [SRS_CS_SIZE] polar(1, float(2 pi) n / 24)
  const float2*       cexp_table;                             // [SRS_CEXP_SIZE]
  const uint32_t*     grid;
  nrphy_srs_result_t* result;                                 // [n]
  uint32_t            grid_nof_ports, grid_nof_subc, n;
};
hipError_t launch_srs(const SrsLaunch& p, hipStream_t stream);
// out[n] = the sequence of antenna port `port` of desc[0], n < M.
hipError_t launch_srs_sequence(const SrsDesc* desc, const float2* cs_table, uint32_t port, uint32_t M, float2* out, hipStream_t stream);
hipError_t launch_grid_put(const uint32_t* d_index, const uint32_t* d_value, uint32_t n, uint32_t* d_grid, hipStream_t stream);

// A codeword of the UL-SCH demultiplexer and a message of the UCI decoder may name a select word and a value (UlschCwDesc,
// UciMsgDesc): its workgroups act only when the word holds the value.  This is the word of those that name none.
constexpr uint32_t NO_SELECT_WORD = 0xFFFFFFFFu;

// ---- UCI decoder (receive side: short blocks and polar) -------------------------------------------------------------------
// One wavefront per message.  A polar code (K, E) is built once per plan: its offsets index the plan's tab16 and ops tables.
constexpr uint32_t UCI_NO_CODE = 0xFFFFFFFFu;
enum UciOp : uint32_t { UCI_OP_F = 0, UCI_OP_G = 1, UCI_OP_RATE1 = 2, UCI_OP_XOR = 3 }; // op word: kind | stage << 2 | position << 6
struct UciCodeDesc {
  uint32_t n, K, E;                            // code length 2^n, bits of a block (filler + message + CRC), soft bits of a block
  uint32_t mode;                               // 0 repetition, 1 puncturing, 2 shortening
  uint32_t nof_ops, ops_offset;                // the decoder's walk over the tree, in order
  uint32_t ch_offset;                          // tab16[E]: input position of position i behind the channel de-interleaver
  uint32_t info_offset;                        // tab16[K]: decoder output position of block bit k (parity-check positions left out)
  uint32_t crc_offset;                         // tab16[K]: x^(K - 1 - k) mod g, the share of block bit k in the CRC remainder
  uint32_t crc_size;
};
struct UciMsgDesc {
  uint32_t A, E;
  uint32_t bps;                                // bits per symbol of the modulation (messages of 1 and 2 bits)
  uint32_t code;                               // index of the polar code, UCI_NO_CODE for a short block
  uint32_t nof_blocks;
  uint32_t pad_;
  uint64_t llr_offset, message_offset;
  uint32_t select_word, select_value;          // NO_SELECT_WORD: unconditional, else the message runs only when select[select_word] == select_value
};
struct UciLaunch {
  const UciMsgDesc*  msg;
  const UciCodeDesc* code;
  const uint16_t*    tab16;
  const uint32_t*    ops;
  const int8_t*      llr;
  uint8_t*           message;
  uint32_t*          status;
  uint32_t           n;
  const uint32_t*    select = nullptr;         // the words UciMsgDesc::select_word indexes; null when no message names one
};
hipError_t launch_uci_decoder(const UciLaunch& p, hipStream_t stream);

// ---- UL-SCH demultiplexer (ulsch_kernels.hip) ---------------------------------------------------------------------------------
// One descriptor per codeword.  map[map_offset + r]: where input RE r goes (ulsch_placement_host.h); special[special_offset + i]:
// the REs that take a placeholder correction or a second destination.  `unit`: bytes a thread moves at once (1, 4 or 16: the
// largest that divides bits_per_re and every offset).
constexpr uint32_t ULSCH_THREADS = 256, ULSCH_UNITS_PER_THREAD = 4;
// Map entry of an input RE: stream << 29 | flags | RE index within the stream.
constexpr uint32_t ULSCH_MAP_ZERO_BIT   = 1u << 28; // the stream receives zeros (the RE was punctured by HARQ-ACK of 1 or 2 bits)
constexpr uint32_t ULSCH_MAP_SKIP_BIT   = 1u << 27; // written by a special entry instead (placeholder corrections)
constexpr uint32_t ULSCH_MAP_INDEX_MASK = ULSCH_MAP_SKIP_BIT - 1u;
struct UlschCwDesc {
  uint64_t in_offset, out_offset[4];
  uint32_t nof_re, bits_per_re, qm, unit;
  uint32_t map_offset, special_offset, nof_special, c_init;
  uint32_t first_block, nof_copy_blocks; // the codeword's blocks: copy blocks first, then the special ones
  uint32_t select_word, select_value;    // NO_SELECT_WORD: unconditional, else the codeword's blocks act only when select[select_word] == select_value
};
struct UlschSpecialDev {
  uint32_t src, dst, stream, fix;
};
struct UlschLaunch {
  const UlschCwDesc*     cw;
  const uint32_t*        block_cw; // codeword of every block
  const uint32_t*        map;
  const UlschSpecialDev* special;
  const GoldTables*      gold;
  const uint32_t*        x1_words;
  const int8_t*          in;
  int8_t*                out[4];
  uint32_t               nof_blocks;
  uint32_t               ptr_unit; // 16, 4 or 1: what the alignment of the five pointers allows
  const uint32_t*        select = nullptr; // the words UlschCwDesc::select_word indexes; null when no codeword names one
};
hipError_t launch_ulsch_demux(const UlschLaunch& p, hipStream_t stream);

// ---- PUSCH processor: the result kernel (pusch_proc_kernels.hip) ---------------------------------------------------------------
// One descriptor per PDU: where the stages of the run left what its record is made of.
constexpr uint32_t PUSCH_PROC_NO_STATUS = 0xFFFFFFFFu;
struct PuschProcDesc {
  uint32_t nof_rx_ports;
  uint32_t has_sch, nof_codeblocks;
  uint32_t harq_status, csi1_status;     // index into the UCI decoder's statuses, PUSCH_PROC_NO_STATUS without that part
  uint32_t nof_harq_ack, nof_csi_part1;
  uint32_t sinr_method;                  // NRPHY_PUSCH_SINR_*
  uint64_t harq_ack_offset, csi_part1_offset;
  uint32_t has_evm, reserved_;           // the demodulator ran with the EVM (nrphy_pusch_evm_*): one value over a plan
};
struct PuschProcLaunch {
  const PuschProcDesc*            desc;
  const nrphy_pusch_chest_meas_t* meas;    // [n][NRPHY_MAX_PORTS][NRPHY_PUSCH_CHEST_MAX_LAYERS]
  const float*                    sinr_db; // [n] post-equalisation
  const uint32_t*                 dec;     // [n][4] the decoder's result words
  const uint32_t*                 status;  // the UCI decoder's statuses
  nrphy_pusch_result_t*           result;  // [n]
  uint32_t                        n;
  const float*                    evm;     // [n] the demodulator's EVM; read where the descriptor has has_evm
};
hipError_t launch_pusch_proc_result(const PuschProcLaunch& p, hipStream_t stream);

// ---- PUSCH processor with CSI part 2: the select and result kernels (pusch_csi2_kernels.hip) -----------------------------------
// One descriptor per PDU of a plan, also for those without description (nof_entries 0, one variant).  Variant v > 0 of a PDU is
// part 2 of size[v] bits; its UCI decoder status is variant_status[status_base + v - 1].
struct PuschCsi2Desc {
  uint32_t nof_entries, nof_variants;
  uint32_t csi1_status;                  // index into the processor's UCI statuses; PUSCH_PROC_NO_STATUS without description
  uint32_t status_base;
  uint64_t csi1_offset, csi2_offset;     // bytes of d_uci_bits: the decoded CSI part 1 payload, the place of part 2
  uint32_t nof_parameters[NRPHY_PUSCH_CSI2_MAX_ENTRIES];
  uint32_t offset[NRPHY_PUSCH_CSI2_MAX_ENTRIES][NRPHY_PUSCH_CSI2_MAX_PARAMETERS];
  uint32_t width[NRPHY_PUSCH_CSI2_MAX_ENTRIES][NRPHY_PUSCH_CSI2_MAX_PARAMETERS];
  uint32_t map[NRPHY_PUSCH_CSI2_MAX_ENTRIES][1u << NRPHY_PUSCH_CSI2_MAX_ENTRY_BITS];
  uint32_t size[NRPHY_PUSCH_CSI2_MAX_VARIANTS], nof_enc[NRPHY_PUSCH_CSI2_MAX_VARIANTS], nof_ul_sch[NRPHY_PUSCH_CSI2_MAX_VARIANTS];
  uint32_t pad_;
};
struct PuschCsi2Launch {
  const PuschCsi2Desc*       desc;
  const uint32_t*            status;         // the processor's UCI statuses (HARQ-ACK, CSI part 1)
  uint32_t*                  variant_status; // the statuses of the part 2 messages, one per (PDU, variant > 0)
  const uint8_t*             uci_bits;
  uint32_t*                  select;         // [n] the variant of every PDU
  nrphy_pusch_csi2_result_t* result;         // [n] (the result kernel)
  uint32_t                   n;
};
hipError_t launch_pusch_csi2_select(const PuschCsi2Launch& p, hipStream_t stream);
hipError_t launch_pusch_csi2_result(const PuschCsi2Launch& p, hipStream_t stream);

// ---- PDCCH and SS/PBCH block ("next" row: other downlink grid writers) --------------------------------------------------
// One wavefront per DCI.  Offsets index the launch's shared tables: tab16 (gather table of the polar input, PRB list),
// bytes (payload bits, one per byte), words (CRC weights), weights (floats).
struct PdcchWork {
  uint32_t grid_index;
  uint32_t A, E, N;        // payload bits, rate-matched bits, polar code length
  uint32_t mode;           // bit selection: 0 repetition, 1 puncturing, 2 shortening
  uint32_t rnti, crc_const; // crc_const: the share of the 24 leading ones in the CRC
  uint32_t c_init_data;
  uint32_t start_symbol, duration, n_prb, ref_rb, top_prb; // top_prb: highest allocated PRB + 1
  uint32_t nof_ports, prg_size_subc;
  uint32_t dmrs_c_init[3];
  float    data_amp, dmrs_amp;
  uint32_t weights_offset, src_offset, prb_offset, payload_offset, crcw_offset, enc_offset;
};
// One wavefront per SS/PBCH block.
struct SsbWork {
  uint32_t grid_index, l0, k0, pci;
  uint32_t a_bits;     // PBCH payload a_0 .. a_31 after the interleaver G, a_0 in the MSB
  uint32_t scr_mask;   // positions of a that are scrambled, position 0 in the MSB
  uint32_t scr_adv;    // M v: offset of the payload scrambling sequence
  uint32_t ssb_adv;    // (ssb_idx mod 8) * 864: offset of the PBCH scrambling sequence
  uint32_t dmrs_c_init;
  uint32_t m_pss, m0, m1;
  float    pss_amp;
  uint32_t nof_ports;
  uint8_t  ports[NRPHY_MAX_PORTS];
  uint32_t src_offset, crcw_offset, enc_offset;
};
struct DlControlLaunch {
  const PdcchWork*  pdcch;
  const SsbWork*    ssb;
  const float*      weights;
  const uint16_t*   tab16;
  const uint8_t*    bytes;
  const uint32_t*   words;
  const GoldTables* gold;
  const uint32_t*   x1_words;
  uint32_t*         grid; // null: encode only
  uint8_t*          enc;  // null, or the rate-matched bits (one per byte) of every work item at its enc_offset
  uint32_t          grid_nof_ports, grid_nof_subc;
};
hipError_t launch_pdcch(const DlControlLaunch& p, uint32_t n, hipStream_t stream);
hipError_t launch_ssb(const DlControlLaunch& p, uint32_t n, hipStream_t stream);

// ---- OFDM ---------------------------------------------------------------------------------------------------
struct OfdmLaunch {
  uint32_t       dft_size;
  uint32_t       rg_size;     // 12 * bw_rb
  uint32_t       nof_ports;
  uint32_t       nsymb;       // symbols per slot
  uint32_t       slot_stride; // samples per (grid, port) in the output
  const float2*  twiddle;     // exp(+j 2 pi k / N), k < N
  const float2*  phase;       // [symbols per subframe] phase compensation * scale
  const float2*  window_phase; // demodulator with a window offset: [dft_size] exp(+j 2 pi offset i / N), else unused
  const uint32_t* cp_len;     // [symbols per subframe]
  const uint32_t* sym_offset; // [symbols per subframe] start of the symbol within its slot (samples)
  uint32_t       probe;       // NRPHY_OFDM_PROBE: timing-only runs with the loads and/or stores range-checked away
  // Wire-format output (nrphy_ofdm_run_ci16): amplitude controller + int16 conversion fused into the store; d_iq then
  // points at complex int16 samples.
  uint32_t       wire = 0, wire_clip = 0;
  float          wire_gain = 1.f, wire_ceiling = 0.f, wire_scale = 1.f;
  float          wire_limit = 0.f; // sample powers up to this neither clip nor saturate: min(ceiling, largest x with x * scale <= 32767)^2
  nrphy_amplitude_stats_t* wire_stats = nullptr; // [grid][port], may be null
  uint4*         wire_partials = nullptr; // [grid][port][workgroup]: {sum power, peak power, clipped, -} of one workgroup
};

// ---- lower-PHY tail ("next" row: amplitude controller, radio sample format, fronthaul compression) ----------------------
struct AmplitudeLaunch {
  const float* in;
  float*       out;
  size_t       in_stride, out_stride; // complex samples between buffers
  uint32_t     nof_samples, measure, clip;
  float        gain, ceiling;
  nrphy_amplitude_stats_t* stats; // per buffer, cleared by the caller; may be null
};
hipError_t launch_amplitude(const AmplitudeLaunch& p, uint32_t n_buffers, hipStream_t stream);
hipError_t launch_convert_ci16(const float* in, size_t in_stride, int16_t* out, size_t out_stride, uint32_t n_buffers,
                               uint32_t nof_samples, float scale, hipStream_t stream);
struct OfhCompressLaunch {
  const uint32_t* prbs;      // cbf16 words
  uint8_t*        out;
  size_t          row_stride, out_row_stride; // words / bytes between rows
  uint32_t        nof_prb, data_width, bfp, whole_span;
  float           scale;     // quantiser gain * iq_scaling
};
hipError_t launch_ofh_compress(const OfhCompressLaunch& p, uint32_t n_rows, hipStream_t stream);
// ---- Open Fronthaul uplink receive (ofh_ul_kernels.hip) -----------------------------------------------------------------
constexpr uint32_t OFH_UL_PRBS_PER_WG = 16; // records per workgroup (one wave: three resource elements per lane)
struct OfhDecompressLaunch {
  const uint8_t* in;
  uint32_t*      prbs;      // cbf16 words
  size_t         in_row_stride, row_stride; // bytes / words between rows
  uint32_t       nof_prb, data_width, bfp;
};
hipError_t launch_ofh_decompress(const OfhDecompressLaunch& p, uint32_t n_rows, hipStream_t stream);
// One run of records and the resource elements of it that are written: elements [re_skip, re_skip + nof_re) counted from
// the first record at payload byte `src` go to destination elements dst, dst + 1, ... (cbf16 words of the grid, complex
// floats of the PRACH buffer).  Workgroups first_chunk ... of the launch take OFH_UL_PRBS_PER_WG records each.
struct OfhUlItem {
  uint64_t src, dst;
  uint32_t nof_re, re_skip, first_chunk;
  uint16_t data_width, bfp;
};
hipError_t launch_ofh_ul_sections(const OfhUlItem* d_items, uint32_t n, uint32_t nof_chunks, const uint8_t* d_payload, void* d_dst,
                                  bool prach, hipStream_t stream);
// ---- Open Fronthaul uplink frame receiver (ofh_rx_kernels.hip) ----------------------------------------------------------
constexpr uint32_t OFH_RX_MAX_EAXC = 8; // distinct values of ul_eaxc and prach_eaxc together: one checker lane each
// What the three launches of nrphy_ofh_rx_run share.  state[k]: bit 8 = initialized, bits 0..7 = the counter of eaxc[k].
// own[((grid * ports + port) * 14 + symbol) * grid_prbs + prb]: the largest (frame index + 1) that claimed the PRB, 0 = none.
struct OfhRxLaunch {
  const nrphy_ofh_rx_frame_t*  frames;
  const nrphy_ofh_rx_expect_t* expects;
  const uint8_t*               d_frames;
  nrphy_ofh_rx_record_t*       records;
  uint32_t*                    grid;
  uint32_t*                    state;
  uint32_t*                    own;
  uint32_t n_frames, n_expect, grid_nof_ports, grid_nof_subc, chunks_per_frame;
  uint32_t eth_header, eth_type, ignore_size, seq_id_check, numerology, nof_symbols, ru_nof_prbs, static_compression;
  uint32_t n_ul_eaxc, n_prach_eaxc, n_eaxc;
  uint16_t ul_eaxc[4], prach_eaxc[4], eaxc[OFH_RX_MAX_EAXC];
  uint8_t  mac[12];                // destination, source
  uint8_t  type[2], data_width[2]; // static compression: [0] data route, [1] PRACH route
};
hipError_t launch_ofh_rx(const OfhRxLaunch& p, hipStream_t stream);
// ---- Open Fronthaul downlink transmit (ofh_dl_kernels.hip) --------------------------------------------------------------
constexpr uint32_t OFH_DL_MAX_HEADER = 36; // VLAN Ethernet 18 + eCPRI 8 + radio application, section and udCompHdr 10
// One OFDM symbol of one eAxC as the kernel reads it.  Its fragments are frames of `stride` bytes apart from byte
// `frame` of d_frames on; all but the last hold prbs_per_frag PRBs.  A workgroup takes one window of `window` bytes of one
// frame, cut at 16-byte boundaries of the frame's address: windows_per_frag for every fragment but the last, workgroups
// first_wg ... of the launch in fragment order.
struct OfhDlSymbol {
  uint64_t frame;         // byte offset in d_frames of fragment 0
  uint64_t row;           // cbf16 word of the grid where the symbol's row starts
  uint32_t first_wg, stride, window, windows_per_frag;
  uint16_t nof_frags, prbs_per_frag, nof_prbs, grid_prbs; // ru_nof_prbs; PRBs the grid row has (the others are zeros)
  uint8_t  data_width, bfp, whole_span, header_bytes;
  float    scale;         // quantiser gain * iq_scaling
  uint8_t  header[OFH_DL_MAX_HEADER]; // of fragment 0; the kernel sets size, sequence, start and number of PRBs per fragment
  uint32_t pad_;
};
static_assert(sizeof(OfhDlSymbol) == 88, "read as words by the kernel");
hipError_t launch_ofh_dl_frames(const OfhDlSymbol* d_symbols, uint32_t n, uint32_t nof_wgs, const uint32_t* d_grid, uint8_t* d_frames,
                                hipStream_t stream);
hipError_t launch_ofdm(const OfdmLaunch& p, uint32_t nof_grids, const uint32_t* d_grid, const uint32_t* d_slot_index,
                       float2* d_iq, hipStream_t stream);
// OFDM demodulation (the receive-side mirror of launch_ofdm): `p.phase` is the receive table (conjugate phase x scale),
// window_offset = nof_samples_window_offset of the reference's demodulator configuration.  Symbols [first_symbol, first_symbol +
// nof_symbols) of every (grid, port) are read and written; d_iq holds complex float, or complex int16 widened by `gain`.
struct OfdmDemodRange {
  uint32_t first_symbol, nof_symbols;
  bool     ci16;
  float    gain; // ci16: 1 / iq_scale
};
hipError_t launch_ofdm_demod(const OfdmLaunch& p, uint32_t nof_grids, const void* d_iq, const OfdmDemodRange& range,
                             const uint32_t* d_slot_index, uint32_t window_offset, uint32_t* d_grid, hipStream_t stream);
// size = n1 * n2: n1 = 1 for the sizes one workgroup transforms in LDS (128 ... 6144, what the OFDM kernels take), else
// a radix-n1 column pass through global memory in front of n1 LDS transforms of size n2 (9216 ... 49152).
bool       dft_split(uint32_t size, uint32_t* n1, uint32_t* n2);
bool       dft_size_supported(uint32_t size);
inline bool dft_size_in_lds(uint32_t size)
{
  uint32_t n1 = 0, n2 = 0;
  return dft_split(size, &n1, &n2) && n1 == 1;
}
// twiddle: exp(+j 2 pi k / size); split sizes also need the table of n2 and `batch` transforms of scratch.
hipError_t launch_dft(uint32_t size, int inverse, uint32_t batch, const float2* twiddle, const float2* twiddle_n2,
                      float2* d_tmp, const float2* d_in, float2* d_out, hipStream_t stream);

} // namespace nrphy
