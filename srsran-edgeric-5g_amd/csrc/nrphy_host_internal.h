// Host-side internals shared by the translation units behind the C ABI (nrphy_host.cpp, every *_host.cpp, pdsch_plan_build.cpp,
// pdsch_async.cpp, dl_slot_async.cpp): the context, its staging buffers, small helpers.  Not part of the ABI.
#pragma once

#include "nrphy_internal.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

using namespace nrphy;

#define HIP_TRY(expr)                                                                                                  \
  do {                                                                                                                 \
    if ((expr) != hipSuccess) {                                                                                        \
      return NRPHY_ERR_DEVICE;                                                                                         \
    }                                                                                                                  \
  } while (0)

// The helpers below are inline in every translation unit that uses them; hidden, so that none becomes a symbol of the library.
#pragma GCC visibility push(hidden)

// Remainder arithmetic in GF(2)[x] / poly on the host (plan-time constants of the CRC kernels).
struct CrcField {
  uint32_t poly, order;
  uint32_t mul(uint32_t a, uint32_t b) const // a below 2^order, b any 32-bit polynomial
  {
    const uint32_t top = 1U << order;
    uint32_t       r   = 0;
    for (int k = 31; k >= 0; --k) {
      r <<= 1;
      if (r & top) {
        r ^= poly;
      }
      if ((b >> k) & 1U) {
        r ^= a;
      }
    }
    return r;
  }
  uint32_t xpow(int64_t e) const // x^e mod g; g(0) = 1 makes x invertible: x^-1 = (g - 1) / x
  {
    uint32_t base = (e >= 0) ? 2U : (poly >> 1);
    uint64_t n    = (uint64_t)(e >= 0 ? e : -e);
    uint32_t r    = 1;
    while (n) {
      if (n & 1U) {
        r = mul(r, base);
      }
      base = mul(base, base);
      n >>= 1;
    }
    return r;
  }
};
inline const CrcField CRC24A_FIELD = {0x1864CFBU, 24};
inline const CrcField CRC16_FIELD  = {0x11021U, 16};

// The LDPC lifting sizes in ascending order (TS 38.212 Table 5.3.2-1) and the place of one among them (-1: not a lifting size).
inline constexpr uint16_t LIFTING_SIZES[NOF_LIFTING_SIZES] = {
    2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13,  14,  15,  16,  18,  20,  22,  24,  26,  28,  30,  32,  36,  40, 44,
    48, 52, 56, 60, 64, 72, 80, 88, 96, 104, 112, 120, 128, 144, 160, 176, 192, 208, 224, 240, 256, 288, 320, 352, 384};

inline int lifting_position(unsigned zc)
{
  for (int i = 0; i != NOF_LIFTING_SIZES; ++i) {
    if (LIFTING_SIZES[i] == zc) {
      return i;
    }
  }
  return -1;
}

inline unsigned divide_ceil(unsigned a, unsigned b)
{
  return (a + b - 1) / b;
}

inline bool mask_test(const uint64_t* w, unsigned i)
{
  return (w[i >> 6] >> (i & 63)) & 1U;
}

inline int mask_lowest(const uint64_t* w)
{
  for (unsigned i = 0; i != 64 * NRPHY_PRB_WORDS; ++i) {
    if (mask_test(w, i)) {
      return (int)i;
    }
  }
  return -1;
}

inline int mask_highest(const uint64_t* w)
{
  int hi = -1;
  for (unsigned i = 0; i != 64 * NRPHY_PRB_WORDS; ++i) {
    if (mask_test(w, i)) {
      hi = (int)i;
    }
  }
  return hi;
}

template <typename T>
inline hipError_t upload(T** dptr, const void* src, size_t bytes)
{
  *dptr = nullptr;
  if (bytes == 0) {
    bytes = 16;
    hipError_t e = hipMalloc((void**)dptr, bytes);
    return e;
  }
  hipError_t e = hipMalloc((void**)dptr, bytes);
  if (e != hipSuccess) {
    return e;
  }
  return hipMemcpy(*dptr, src, bytes, hipMemcpyHostToDevice);
}

// All tables of a plan in ONE device allocation filled by ONE copy (a plan of a single PDU used to spend most of its
// creation time in a dozen hipMalloc / hipMemcpy pairs).  add() registers a table; commit() allocates, copies and
// points every registered device pointer into the block, followed by `scratch_bytes` of uninitialised device memory.
class DeviceArena
{
public:
  template <typename T>
  void add(T** dptr, const void* src, size_t bytes)
  {
    items.push_back({(void**)dptr, src, bytes, total});
    total += (bytes + 255) & ~(size_t)255;
  }
  size_t bytes() const { return std::max<size_t>(total, 256); }
  // The same layout in memory the caller owns: the tables are written to `h_base`, the device pointers point into
  // `d_base`; copying [h_base, h_base + bytes()) there is the caller's business (no HIP call here).
  void place(uint8_t* h_base, uint8_t* d_base)
  {
    for (const Item& it : items) {
      if (it.bytes != 0) {
        std::memcpy(h_base + it.offset, it.src, it.bytes);
      }
      *it.dptr = d_base + it.offset;
    }
  }
  hipError_t commit(void** base, size_t scratch_bytes, void** scratch)
  {
    std::vector<uint8_t> staging(std::max<size_t>(total, 256), 0);
    for (const Item& it : items) {
      if (it.bytes != 0) {
        std::memcpy(&staging[it.offset], it.src, it.bytes);
      }
    }
    hipError_t e = hipMalloc(base, staging.size() + scratch_bytes);
    if (e != hipSuccess) {
      return e;
    }
    for (const Item& it : items) {
      *it.dptr = (uint8_t*)*base + it.offset;
    }
    *scratch = (uint8_t*)*base + staging.size();
    return hipMemcpy(*base, staging.data(), staging.size(), hipMemcpyHostToDevice);
  }

private:
  struct Item {
    void**      dptr;
    const void* src;
    size_t      bytes, offset;
  };
  std::vector<Item> items;
  size_t            total = 0;
};

#pragma GCC visibility pop

// Environment knobs (INTEGRATION.md section 5 lists them): A/B and test aids, none changes a result.  Read ONCE, when the
// context is created -- never on a submit path, where several threads of the host may be running -- so a process that wants
// another setting creates another context.  -1 / 0 = not set.
struct Tunables {
  int      cb_dispatch     = 0;  // NRPHY_CB_DISPATCH: 1 = the mixed codeblock kernel, 2 = one launch per bucket, 0 = by plan shape
  int      crc_regions     = 0;  // NRPHY_CRC_REGIONS: 16 KiB regions per TB-CRC workgroup (0: by batch size)
  int      scr_parts_big   = 0;  // NRPHY_SCR_PARTS_BIG: parts per scrambling sequence in a batch of 128 PDUs or more (0: 1)
  int      scr_words       = -1; // NRPHY_SCR_WORDS: 0 = scrambling sequences always as seeds, 1 = always as words (-1: words within the L2 budget)
  int      decoder_pairs   = -1; // NRPHY_DECODER_PAIRS=0: one check per lane whatever the lifting size
  int      decoder_ldsmsg  = -1; // NRPHY_DECODER_LDSMSG: 0 = messages never in LDS, 2 = wherever a workgroup's LDS can hold them
  bool     decoder_slots_all = false; // NRPHY_DECODER_SLOTS_ALL=1: a scratch slot per codeblock (no pooling)
  // Profiling variants only (profiles/make_variant.sh ... -DNRPHY_PROBES): read and consulted under that flag alone, 0 without
  // it (the members are always there, so that the context has one layout in both builds); set, the outputs are INCOMPLETE.
  uint32_t profile_stage   = 0;  // NRPHY_PROFILE_STAGE: the codeblock waves stop after a stage
  uint32_t ofdm_probe      = 0;  // NRPHY_OFDM_PROBE: bit 0 drops the IQ stores, bit 1 the grid loads, bit 2 takes the grids first to last
};
Tunables read_tunables();

// Lifted graph of base graph `bg` (1 or 2) at lifting size `zc`, as the encoder's kernels read it (nrphy_host.cpp).
void build_lifted_graph(unsigned bg, unsigned zc, LiftedGraph& g);

enum ScratchSlot { SCRATCH_TB = 0, SCRATCH_GRID, SCRATCH_CW_RM, SCRATCH_CW_SCR, SCRATCH_IQ, SCRATCH_SMALL,
                   SCRATCH_DECODER, SCRATCH_RX, SCRATCH_COUNT };

struct nrphy_ctx {
  int          device   = 0;
  Tunables     tune;
  uint32_t     nof_cus  = 256; // compute units of the device (sizes the decoder's scratch pool)
  hipStream_t  stream   = nullptr;
  LiftedGraph* d_graphs = nullptr;
  GoldTables*  d_gold   = nullptr;
  TbCrcTables* d_tbcrc  = nullptr;
  uint32_t*    d_x1     = nullptr;
  std::map<uint32_t, float2*> d_twiddle; // exp(+j 2 pi k / N) per DFT size, built on first use (under host_mutex)
  PrachTables* d_prach = nullptr;        // PRACH generator's exponentials and the detector's twiddles, built on first use
  DecoderGraph* d_dec_graph[NOF_GRAPHS] = {}; // decoder graphs, built on first use
  uint32_t*     d_dec_addr[NOF_GRAPHS]  = {}; // ... and, for even lifting sizes, the soft-bit addresses of every (edge, pair of checks)
  std::map<uint64_t, uint32_t*> d_dec_crc;     // early-stop CRC weights per (polynomial, message length)
  std::map<uint32_t, uint32_t*> d_tb_crc_w;    // transport-block CRC weights of the PUSCH assembly kernel per block size
  std::vector<LiftedGraph> graphs; // host copy (plan creation sizes the LDS staging of graph rows from it)
  // Device staging of the host-span entry points (*_host): grow-only buffers, one call at a time per context.
  // One lock for everything context-owned and shared: the staging buffers below and the lazily built tables.  Every getter
  // of such a table (get_twiddle, the decoder's graphs and CRC weights, the PUSCH TB-CRC weights, the PRACH tables) takes it
  // itself, no caller has to.  The host-span entry points (*_host) hold it for the whole call (HostCall below), so two of
  // them never interleave on a buffer; it is recursive because they are built from device-pointer calls that take it briefly.
  std::recursive_mutex host_mutex;
  void*      scratch[SCRATCH_COUNT]       = {};
  size_t     scratch_bytes[SCRATCH_COUNT] = {};
};

// The context's table exp(+j 2 pi k / size) of a size nrphy_dft_run supports, built on first use with the context's device
// current; null for another size or when the upload fails.  It lives as long as the context.
const float2* get_twiddle(nrphy_ctx* ctx, uint32_t size);
// The same table for any size >= 1 (the transform-precoding sizes 12 * M_rb); the two share the context's tables.
const float2* get_twiddle_table(nrphy_ctx* ctx, uint32_t size);
// The deprecoder of nof_prb PRBs with the context's twiddle table (built on first use, device current): false for an invalid
// size or a failed upload.  transform_precoder_host.cpp.
bool transform_deprecode_plan(nrphy_ctx* ctx, uint32_t nof_prb, MixedDftPlan& plan);

#pragma GCC visibility push(hidden)

// Amplitude controller parameters as the reference's constructors derive them
// (amplitude_controller_clipping_impl.h:52-62, amplitude_controller_scaling_impl.h); false for a configuration to refuse.
// Defined in ofdm_host.cpp (the wire-format modulator), used by lower_phy_host.cpp too.
struct AmplitudeParams {
  float gain, ceiling;
  bool  measure, clip;
};
bool amplitude_params(const nrphy_amplitude_cfg_t& c, AmplitudeParams& a);

// Staging buffer `slot` of the context with room for `bytes` (reallocated only when it has to grow).
inline void* ctx_scratch(nrphy_ctx* ctx, ScratchSlot slot, size_t bytes)
{
  if (bytes > ctx->scratch_bytes[slot]) {
    (void)hipFree(ctx->scratch[slot]);
    ctx->scratch[slot]       = nullptr;
    ctx->scratch_bytes[slot] = 0;
    const size_t want        = (bytes + (bytes >> 2) + 4095) & ~(size_t)4095;
    if (hipMalloc(&ctx->scratch[slot], want) != hipSuccess) {
      return nullptr;
    }
    ctx->scratch_bytes[slot] = want;
  }
  return ctx->scratch[slot];
}

// The one way a blocking host-span entry point (*_host) gets the lock, the device and its device memory: what
// include/mi355_nrphy.h promises about all of them.  From construction to return it holds ctx->host_mutex, with ctx->device
// made current.  Device memory comes from the context's grow-only staging: mem() for a whole slot, carve() for several
// 256-byte aligned pieces of one slot with every size given at once, because growth frees the old buffer.  For the same
// reason a call asks for a slot once, and a host form never calls another host form (none does).  Both return null when the
// device could not be made current, so NRPHY_ERR_DEVICE on null covers that too.  sync() is the success path's one
// hipStreamSynchronize.  A return before it -- HIP_TRY's included -- drains ctx->stream in the destructor: no copy into a
// caller's span or into a local of the entry point outlives the call (a container that an asynchronous copy targets is
// declared before the HostCall, so that it is destroyed after the drain).
class HostCall
{
public:
  explicit HostCall(nrphy_ctx* c) : ctx(c), lock(c->host_mutex), device_set(hipSetDevice(c->device) == hipSuccess) {}
  HostCall(const HostCall&)            = delete;
  HostCall& operator=(const HostCall&) = delete;
  ~HostCall()
  {
    if (!drained) {
      (void)hipStreamSynchronize(ctx->stream);
    }
  }
  template <typename T = void>
  T* mem(ScratchSlot slot, size_t bytes)
  {
    return device_set ? (T*)ctx_scratch(ctx, slot, bytes) : nullptr;
  }
  template <size_t N>
  bool carve(ScratchSlot slot, const size_t (&bytes)[N], uint8_t* (&piece)[N])
  {
    size_t offset[N + 1] = {};
    for (size_t i = 0; i != N; ++i) {
      offset[i + 1] = offset[i] + ((bytes[i] + 255) & ~(size_t)255);
    }
    uint8_t* base = mem<uint8_t>(slot, offset[N]);
    for (size_t i = 0; i != N; ++i) {
      piece[i] = base ? base + offset[i] : nullptr;
    }
    return base != nullptr;
  }
  hipError_t sync()
  {
    drained = true;
    return hipStreamSynchronize(ctx->stream);
  }

private:
  nrphy_ctx*                            ctx;
  std::lock_guard<std::recursive_mutex> lock;
  bool                                  device_set;
  bool                                  drained = false;
};

// Device staging that lives for ONE device-pointer call on the caller's stream: host-built work lists a kernel of this call
// reads.  Allocated and released in stream order (hipMallocAsync / hipFreeAsync), so calls in flight on different streams
// never share a buffer and nothing waits for the device.  Usage: alloc(), copy + launch on the same stream, then the
// destructor frees.  The host-span forms do not use it: they block anyway and reuse the context's staging (HostCall).
class StreamStaging
{
public:
  explicit StreamStaging(hipStream_t s) : stream(s) {}
  StreamStaging(const StreamStaging&)            = delete;
  StreamStaging& operator=(const StreamStaging&) = delete;
  ~StreamStaging()
  {
    if (ptr != nullptr) {
      (void)hipFreeAsync(ptr, stream);
    }
  }
  void* alloc(size_t bytes)
  {
    if (hipMallocAsync(&ptr, std::max<size_t>(bytes, 16), stream) != hipSuccess) {
      ptr = nullptr;
    }
    return ptr;
  }

private:
  hipStream_t stream;
  void*       ptr = nullptr;
};

#pragma GCC visibility pop
