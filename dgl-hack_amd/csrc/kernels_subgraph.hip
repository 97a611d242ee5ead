// Ordered CSR row-and-column slice on the device (DGLGraph.subgraph): the reference's
// CSRSliceMatrix loop (src/array/cpu/spmat_op_impl.cc:495-542) restated so that no id leaves
// the GPU, no atomic orders the output and a hub row does not serialise.  include/dglmi.h
// states the contract; this file is one way to meet it.
//
// The work is the G gathered positions: position p is one CSR entry of one selected row,
// goff (the running sum of the selected rows' degrees) says which.  Positions are cut into
// tiles of kSliceTile = 1024; a block of four wavefronts owns a tile and each wavefront owns
// four consecutive 64-position words of it, so a word is exactly one ballot.
//
// Resolving a position.  A wavefront's 256 positions are consecutive, so their row slots lie
// between the slot of the first and the slot of the last: those two searches run over all of
// goff with wave-uniform arguments (every lane reads the same addresses), and the per-lane
// search that follows runs between them -- zero steps inside a hub row, a few where rows are
// short.
//
// Count.  Each lane loads its entry's column and looks it up in the relabel table (marked with
// the selected nodes' positions, INT32_MAX elsewhere).  The ballot of a word is its 64 keep
// bits; lane 0 stores it to the bitmap.  The wavefront's four popcounts add up in a register,
// meet in LDS, and thread 0 adds the four wave counts in wave order into tile_cnt[t].
//
// Fill, after the caller's running sum over tile_cnt.  The bitmap is the only membership
// record read: sixteen lanes load the tile's words and leave their popcounts in LDS; a kept
// position's output rank is the tile's base, plus the popcounts of the earlier words, plus
// the number of set bits below its own lane (v_mbcnt).  Ranks ascend with positions, so the
// output is in (slot, CSR order) whatever the schedule.  Only kept lanes resolve their
// position again and touch the CSR, the table (for the destination's new id) and the output.
//
// G itself is read on the device (goff[S], clamped to the capacity the caller sized the
// bitmap for): the host launches one block per tile of the capacity and blocks past G leave
// at once, which spares the call a second readback.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace dglmi {
namespace {

constexpr int kSliceBlock = 256;
constexpr int kSliceWaves = kSliceBlock / 64;
constexpr int kSliceWaveWords = 4;                            // 64-position words per wavefront
constexpr int kSliceTileWords = kSliceWaves * kSliceWaveWords;  // 16
constexpr int kSliceTile = kSliceTileWords * 64;              // 1024 positions
constexpr int32_t kSliceFree = 0x7fffffff;                    // the relabel table's sentinel

struct SliceArgs {
  SampleCsr c;
  const int32_t* nodes;  // S selected rows
  int64_t S;
  const int64_t* goff;   // S + 1 running degrees
  const int32_t* table;  // table[v] = position of v in nodes, kSliceFree when absent
  int64_t table_len;
  int64_t max_pos;       // capacity: the bitmap holds ceil(max_pos / 64) words
};

__device__ __forceinline__ int64_t slice_total(const SliceArgs& a) {
  const int64_t g = a.goff[a.S];
  return g < 0 ? 0 : (g < a.max_pos ? g : a.max_pos);
}

// the slot bounds of the positions w0 .. w1 of one wavefront (wave-uniform)
__device__ __forceinline__ void slice_bounds(const SliceArgs& a, int64_t w0, int64_t w1,
                                             int64_t* lo, int64_t* hi) {
  *lo = seg_of_row(a.goff, 0, a.S - 1, w0);
  *hi = seg_of_row(a.goff, *lo, a.S - 1, w1);
}

// position p -> its slot and its CSR entry; -1 when the row has no such entry
__device__ __forceinline__ int64_t slice_entry(const SliceArgs& a, int64_t lo, int64_t hi, int64_t p,
                                               int64_t* slot) {
  const int64_t i = seg_of_row(a.goff, lo, hi, p);
  *slot = i;
  const int64_t row = a.nodes[i];
  if (row < 0 || row >= a.c.num_rows) return -1;
  const int64_t start = a.c.indptr[row];
  const int64_t k = p - a.goff[i];
  return k >= 0 && k < a.c.indptr[row + 1] - start ? start + k : -1;
}

__global__ void __launch_bounds__(kSliceBlock)
k_slice_count(SliceArgs a, uint64_t* __restrict__ keep, int64_t* __restrict__ tile_cnt) {
  __shared__ int wave_cnt[kSliceWaves];
  const int64_t G = slice_total(a);
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * kSliceTile;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t w0 = t0 + static_cast<int64_t>(wave) * (kSliceWaveWords * 64);
  int cnt = 0;
  if (w0 < G) {  // wave-uniform
    const int64_t wl = w0 + kSliceWaveWords * 64 - 1;
    int64_t lo, hi;
    slice_bounds(a, w0, wl < G ? wl : G - 1, &lo, &hi);
    for (int k = 0; k < kSliceWaveWords; ++k) {
      const int64_t base = w0 + k * 64;
      if (base >= G) break;  // wave-uniform
      const int64_t p = base + lane;
      bool kept = false;
      if (p < G) {
        int64_t slot;
        const int64_t e = slice_entry(a, lo, hi, p, &slot);
        if (e >= 0) {
          const int64_t col = a.c.indices[e];
          kept = col >= 0 && col < a.table_len && a.table[col] != kSliceFree;
        }
      }
      const uint64_t bits = __ballot(kept);
      if (lane == 0) keep[base >> 6] = bits;
      cnt += __popcll(bits);
    }
  }
  if (lane == 0) wave_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t sum = 0;
    for (int w = 0; w < kSliceWaves; ++w) sum += wave_cnt[w];
    tile_cnt[blockIdx.x] = sum;
  }
}

__global__ void __launch_bounds__(kSliceBlock)
k_slice_fill(SliceArgs a, const uint64_t* __restrict__ keep, const int64_t* __restrict__ tile_scan,
             int64_t num_out, int32_t* __restrict__ new_src, int32_t* __restrict__ new_dst,
             int64_t* __restrict__ parent_eid) {
  __shared__ int word_pop[kSliceTileWords];
  const int64_t G = slice_total(a);
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * kSliceTile;
  if (t0 >= G) return;  // block-uniform: before the barrier
  if (threadIdx.x < kSliceTileWords) {
    const int64_t base = t0 + static_cast<int64_t>(threadIdx.x) * 64;
    word_pop[threadIdx.x] = base < G ? __popcll(keep[base >> 6]) : 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t w0 = t0 + static_cast<int64_t>(wave) * (kSliceWaveWords * 64);
  if (w0 >= G) return;
  int64_t rank0 = blockIdx.x > 0 ? tile_scan[blockIdx.x - 1] : 0;  // inclusive scan: the tile's base
  for (int j = 0; j < wave * kSliceWaveWords; ++j) rank0 += word_pop[j];
  const int64_t wl = w0 + kSliceWaveWords * 64 - 1;
  int64_t lo, hi;
  slice_bounds(a, w0, wl < G ? wl : G - 1, &lo, &hi);
  for (int k = 0; k < kSliceWaveWords; ++k) {
    const int64_t base = w0 + k * 64;
    if (base >= G) break;
    const uint64_t bits = keep[base >> 6];
    if ((bits >> lane) & 1) {
      const int below = __builtin_amdgcn_mbcnt_hi(
          static_cast<uint32_t>(bits >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(bits), 0u));
      const int64_t rank = rank0 + below;
      int64_t slot;
      const int64_t e = slice_entry(a, lo, hi, base + lane, &slot);
      if (e >= 0 && rank >= 0 && rank < num_out) {
        const int64_t col = a.c.indices[e];
        new_src[rank] = static_cast<int32_t>(slot);
        new_dst[rank] = col >= 0 && col < a.table_len ? a.table[col] : -1;
        parent_eid[rank] = a.c.data[e];
      }
    }
    rank0 += word_pop[wave * kSliceWaveWords + k];
  }
}

}  // namespace

int subgraph_tile() { return kSliceTile; }

int64_t subgraph_tiles(int64_t max_pos) { return (max_pos + kSliceTile - 1) / kSliceTile; }

void launch_slice_count(const SampleCsr& c, const int32_t* nodes, int64_t S, const int64_t* goff,
                        const int32_t* table, int64_t table_len, int64_t max_pos, uint64_t* keep,
                        int64_t* tile_cnt, hipStream_t s) {
  const int64_t tiles = subgraph_tiles(max_pos);
  if (tiles == 0) return;
  const SliceArgs a{c, nodes, S, goff, table, table_len, max_pos};
  hipLaunchKernelGGL(k_slice_count, dim3(static_cast<unsigned>(tiles)), dim3(kSliceBlock), 0, s, a,
                     keep, tile_cnt);
}

void launch_slice_fill(const SampleCsr& c, const int32_t* nodes, int64_t S, const int64_t* goff,
                       const int32_t* table, int64_t table_len, int64_t max_pos,
                       const uint64_t* keep, const int64_t* tile_scan, int64_t num_out,
                       int32_t* new_src, int32_t* new_dst, int64_t* parent_eid, hipStream_t s) {
  const int64_t tiles = subgraph_tiles(max_pos);
  if (tiles == 0 || num_out == 0) return;
  const SliceArgs a{c, nodes, S, goff, table, table_len, max_pos};
  hipLaunchKernelGGL(k_slice_fill, dim3(static_cast<unsigned>(tiles)), dim3(kSliceBlock), 0, s, a,
                     keep, tile_scan, num_out, new_src, new_dst, parent_eid);
}

}  // namespace dglmi
