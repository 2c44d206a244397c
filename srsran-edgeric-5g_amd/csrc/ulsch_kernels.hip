// UL-SCH demultiplexer: the descrambled soft bits of PUSCH codewords to the UL-SCH, HARQ-ACK, CSI part 1 and CSI part 2 streams
// (ulsch_demultiplex_impl::demux_current_ofdm_symbol, R/lib/phy/upper/channel_processors/pusch/ulsch_demultiplex_impl.cpp:474-590).
// The placement is a table the host made (ulsch_placement_host.h): the kernel is a gather.  Copy blocks move the codeword in
// units of 16, 4 or 1 bytes, consecutive threads consecutive units of the input, so loads are coalesced and stores are coalesced
// within every run of REs that share a stream (UCI takes every d-th RE of a few symbols; everything else is one long run).
// The few REs that need more than a copy -- HARQ-ACK of 1 or 2 bits, which also leaves zeros behind, and the placeholder
// corrections of on_uci_placeholder_1bit / _2bit -- are left out by the copy blocks and done by the codeword's special blocks,
// one thread per RE and layer, with the Gold bits of the soft bits' positions from the jump-ahead matrices.
#include "bits_device.h"

namespace nrphy {

namespace {

template <class T>
__device__ __forceinline__ void ulsch_copy_block(const UlschLaunch& p, const UlschCwDesc& cw, uint32_t block)
{
  constexpr uint32_t U       = sizeof(T);
  const uint32_t     per_re  = cw.bits_per_re / U;
  const uint32_t     n_units = cw.nof_re * per_re;
  const int8_t*      in      = p.in + cw.in_offset;
  const uint32_t*    map     = p.map + cw.map_offset;
  T                  v[ULSCH_UNITS_PER_THREAD];
  uint32_t           e[ULSCH_UNITS_PER_THREAD], part[ULSCH_UNITS_PER_THREAD];
#pragma unroll
  for (uint32_t i = 0; i != ULSCH_UNITS_PER_THREAD; ++i) {
    const uint32_t u = (block * ULSCH_UNITS_PER_THREAD + i) * ULSCH_THREADS + threadIdx.x;
    e[i]             = ULSCH_MAP_SKIP_BIT;
    part[i]          = 0;
    v[i]             = T{};
    if (u < n_units) {
      const uint32_t re = u / per_re;
      part[i]           = u - re * per_re;
      e[i]              = map[re];
      v[i]              = reinterpret_cast<const T*>(in)[u];
    }
  }
#pragma unroll
  for (uint32_t i = 0; i != ULSCH_UNITS_PER_THREAD; ++i) {
    if ((e[i] & ULSCH_MAP_SKIP_BIT) == 0) {
      const uint32_t s   = e[i] >> 29;
      int8_t*        dst = p.out[s] + cw.out_offset[s] + (uint64_t)(e[i] & ULSCH_MAP_INDEX_MASK) * cw.bits_per_re + part[i] * U;
      *reinterpret_cast<T*>(dst) = (e[i] & ULSCH_MAP_ZERO_BIT) ? T{} : v[i];
    }
  }
}

// c(pos + j), j < 8, in bit j: the scrambling sequence at the soft bits of one modulation symbol.
__device__ __forceinline__ uint32_t ulsch_gold_bits(const UlschLaunch& p, uint32_t c_init, uint32_t pos)
{
  uint32_t       state  = c_init & 0x7FFFFFFFu;
  const uint32_t offset = 1600u + pos;
  for (uint32_t k = 0; k != GOLD_JUMP_BITS; ++k) {
    if ((offset >> k) & 1u) {
      uint32_t next = 0;
      for (uint32_t r = 0; r != 31; ++r) {
        next |= (__popc(p.gold->x2_jump[k][r] & state) & 1u) << r;
      }
      state = next;
    }
  }
  uint32_t x1 = 0;
  for (uint32_t j = 0; j != 8; ++j) {
    const uint32_t n = pos + j;
    x1 |= ((p.x1_words[n >> 5] >> (31u - (n & 31u))) & 1u) << j;
  }
  return (state ^ x1) & 0xFFu;
}

__device__ __forceinline__ void ulsch_special_block(const UlschLaunch& p, const UlschCwDesc& cw, uint32_t block)
{
  const uint32_t layers = cw.bits_per_re / cw.qm;
  const uint32_t item   = block * ULSCH_THREADS + threadIdx.x;
  if (item >= cw.nof_special * layers) {
    return;
  }
  const UlschSpecialDev sp    = p.special[cw.special_offset + item / layers];
  const uint32_t        layer = item % layers;
  const uint32_t        pos   = sp.src * cw.bits_per_re + layer * cw.qm; // of the symbol's first soft bit in the codeword
  const int8_t*         src   = p.in + cw.in_offset + pos;
  int8_t*               dst   = p.out[sp.stream] + cw.out_offset[sp.stream] + (uint64_t)sp.dst * cw.bits_per_re + layer * cw.qm;
  uint32_t              flip  = 0; // bit j: soft bit j changes sign
  if (sp.fix != 0) {
    const uint32_t c = ulsch_gold_bits(p, cw.c_init, pos);
    flip             = c & ~3u; // placeholder x: the scrambling is reverted
    if (sp.fix == 1) {
      flip |= ((c ^ (c >> 1)) & 1u) << 1; // placeholder y: the second bit takes the first one's mask
    }
  }
  for (uint32_t j = 0; j != cw.qm; ++j) {
    const int8_t x = src[j];
    dst[j]         = ((flip >> j) & 1u) ? (int8_t)-x : x;
  }
}

} // namespace

__global__ __launch_bounds__(ULSCH_THREADS) void ulsch_demux_kernel(UlschLaunch p)
{
  const uint32_t     c     = p.block_cw[blockIdx.x];
  const UlschCwDesc& cw    = p.cw[c];
  const uint32_t     block = blockIdx.x - cw.first_block;
  // A codeword that names a select word acts only when the word holds its value (workgroup-uniform: scalar loads of a kernel
  // argument and of the block's descriptor).
  if (p.select != nullptr && cw.select_word != NO_SELECT_WORD && p.select[cw.select_word] != cw.select_value) {
    return;
  }
  if (block >= cw.nof_copy_blocks) { // workgroup-uniform
    ulsch_special_block(p, cw, block - cw.nof_copy_blocks);
    return;
  }
  const uint32_t unit = cw.unit < p.ptr_unit ? cw.unit : p.ptr_unit;
  // The block count was sized for cw.unit; with a smaller one (unaligned pointers) every block walks its share in steps.
  const uint32_t steps = cw.unit / unit;
  for (uint32_t s = 0; s != steps; ++s) {
    if (unit == 16) {
      ulsch_copy_block<uint4>(p, cw, block * steps + s);
    } else if (unit == 4) {
      ulsch_copy_block<uint32_t>(p, cw, block * steps + s);
    } else {
      ulsch_copy_block<uint8_t>(p, cw, block * steps + s);
    }
  }
}

hipError_t launch_ulsch_demux(const UlschLaunch& p, hipStream_t stream)
{
  if (p.nof_blocks == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(ulsch_demux_kernel, dim3(p.nof_blocks), dim3(ULSCH_THREADS), 0, stream, p);
  return hipGetLastError();
}

} // namespace nrphy
