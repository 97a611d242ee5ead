// Neighbour sampling and block relabelling on the device (dgl.sampling.sample_neighbors,
// dgl.to_block, dgl.in_subgraph / out_subgraph): the reference's per-row CPU loop
// (src/array/cpu/rowwise_pick.h:68-110, src/graph/transform/to_bipartite.cc:39-56) restated
// so that no node or edge id leaves the GPU.  include/dglmi.h states the contract; this file
// is one way to meet it.
//
// The sampler.  A seed is served by a group of G lanes, G the smallest power of two that is
// at least the fan-out and at least 4, so a wavefront serves 64 / G seeds.  Lane t of a group
// computes draw t (one Philox4x32-10 block per lane: four lanes share a block's counter but
// not a register, which costs arithmetic and saves a shuffle).  With replacement the draw is
// the pick.  Without, and with more neighbours than the fan-out, Floyd's subset algorithm
// resolves the picks in `fanout` steps of one broadcast and one compare inside the group:
// step t takes lane t's candidate, or j_t when an earlier step already holds it.  The picks
// are then ranked by counting (fan-out broadcasts again): lane t writes its pick at
// offsets[seed] + rank.  Every cross-lane operation runs for every lane of the wavefront --
// the loops' bounds are launch-uniform and a group without work carries sentinels -- so no
// group-level branch surrounds a shuffle or a ballot.
//
// No LDS, no atomics, no float arithmetic: the sample is a function of the arguments alone.
//
// The gather (take-all) walks output positions, not rows: one lane per output entry finds its
// row by binary search in the offsets, so a hub row is spread over as many lanes as it has
// entries.
//
// The relabel.  An int32 table of one entry per node holds INT32_MAX between calls.  Pass 1
// takes the minimum position of every node with a non-returning atomicMin (an integer
// minimum does not depend on the order of arrival); pass 2 flags the positions that own
// their node's entry; the caller scans the flags; pass 3 writes the new ids; pass 4 stores
// the sentinel back into exactly the entries pass 1 touched.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace dglmi {
namespace {

constexpr int kSampleBlock = 256;
constexpr int kSampleMaxFanout = 64;  // one group is at most one wavefront
constexpr int32_t kRelabelFree = 0x7fffffff;

__device__ __forceinline__ uint32_t sample_draw(uint64_t seed, uint64_t ctr, int64_t slot, int t) {
  const uint64_t c = ctr + static_cast<uint64_t>(t >> 2);
  const uint64_t s = static_cast<uint64_t>(slot);
  const Philox4 r = philox4x32_10(Philox4{static_cast<uint32_t>(c), static_cast<uint32_t>(c >> 32),
                                          static_cast<uint32_t>(s), static_cast<uint32_t>(s >> 32)},
                                  static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
  const int k = t & 3;
  return k == 0 ? r.x : k == 1 ? r.y : k == 2 ? r.z : r.w;
}

// floor(r * n / 2^32) for n < 2^32
__device__ __forceinline__ int64_t sample_scale(uint32_t r, int64_t n) {
  return static_cast<int64_t>((static_cast<uint64_t>(r) * static_cast<uint64_t>(n)) >> 32);
}

// the degree of row `row`, 0 for a row outside the CSR
__device__ __forceinline__ int64_t row_degree(const IdxPtr& indptr, int64_t num_rows, int64_t row,
                                              int64_t* start) {
  if (row < 0 || row >= num_rows) {
    *start = 0;
    return 0;
  }
  const int64_t s = indptr[row];
  const int64_t d = indptr[row + 1] - s;
  *start = s;
  return d > 0 ? d : 0;
}

// cnt[0] = 0, cnt[i + 1] = the number of picks of seed slot i (fanout < 0: the whole row)
__global__ void __launch_bounds__(kSampleBlock)
k_sample_count(IdxPtr indptr, int64_t num_rows, const int32_t* __restrict__ seeds, int64_t num_seeds,
               int fanout, int replace, int64_t* __restrict__ cnt) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kSampleBlock + threadIdx.x;
  if (i == 0) cnt[0] = 0;
  if (i >= num_seeds) return;
  int64_t start;
  const int64_t deg = row_degree(indptr, num_rows, seeds[i], &start);
  int64_t c = deg;
  if (fanout >= 0) c = deg == 0 ? 0 : (replace ? fanout : (deg < fanout ? deg : fanout));
  cnt[i + 1] = c;
}

template <int G>
__global__ void __launch_bounds__(kSampleBlock)
k_sample_pick(IdxPtr indptr, const int32_t* __restrict__ indices, IdxPtr data, int64_t num_rows,
              const int32_t* __restrict__ seeds, int64_t num_seeds, int fanout, int replace,
              uint64_t rng_seed, uint64_t rng_ctr, const int64_t* __restrict__ offsets,
              int64_t num_out, int32_t* __restrict__ out_nbr, int64_t* __restrict__ out_eid) {
  constexpr int64_t kNone = INT64_MAX;
  const int g = threadIdx.x & (G - 1);
  const int64_t slot = (static_cast<int64_t>(blockIdx.x) * kSampleBlock + threadIdx.x) / G;
  const bool live = slot < num_seeds;
  int64_t start = 0;
  const int64_t deg = live ? row_degree(indptr, num_rows, seeds[slot], &start) : 0;
  const bool mine = g < fanout;  // this lane owns draw g
  const uint32_t r = mine ? sample_draw(rng_seed, rng_ctr, slot, g) : 0u;

  int64_t pos = kNone;  // this lane's pick: a position inside the row
  int cnt = 0;
  if (deg > 0) {
    if (replace) {
      cnt = fanout;
      if (mine) pos = sample_scale(r, deg);
    } else if (deg <= fanout) {
      cnt = static_cast<int>(deg);
      if (g < deg) pos = g;
    } else {
      cnt = fanout;
    }
  }
  if (!replace) {
    // Floyd: step t picks p_t = floor(r_t (j_t + 1) / 2^32), j_t = deg - fanout + t, or j_t
    // when an earlier step holds p_t.  Only groups with deg > fanout keep the result.
    const bool floyd = deg > fanout;
    const int64_t j = deg - fanout + g;
    const int64_t cand = floyd && mine ? sample_scale(r, j + 1) : kNone;
    int64_t fin = kNone;
    const int base = (threadIdx.x & 63) & ~(G - 1);
    for (int t = 0; t < fanout; ++t) {
      const int64_t c = __shfl(cand, t, G);
      const uint64_t hits = __ballot(floyd && g < t && fin == c);
      const uint64_t in_group = G == 64 ? hits : (hits >> base) & ((uint64_t(1) << (G & 63)) - 1);
      if (g == t) fin = in_group != 0 ? j : c;
    }
    if (floyd && mine) pos = fin;
  }
  // rank by counting: the picks of a seed ascend by position, equal picks by draw
  int rank = 0;
  for (int t = 0; t < fanout; ++t) {
    const int64_t v = __shfl(pos, t, G);
    rank += (v < pos || (v == pos && t < g)) ? 1 : 0;
  }
  if (pos != kNone && rank < cnt) {
    const int64_t o = offsets[slot] + rank;
    if (o >= 0 && o < num_out) {
      out_nbr[o] = indices[start + pos];
      out_eid[o] = data[start + pos];
    }
  }
}

// one lane per output entry: its row is the last i with offsets[i] <= p
__global__ void __launch_bounds__(kSampleBlock)
k_gather_rows(IdxPtr indptr, const int32_t* __restrict__ indices, IdxPtr data, int64_t num_rows,
              const int32_t* __restrict__ rows, int64_t n, const int64_t* __restrict__ offsets,
              int64_t num_out, int32_t* __restrict__ out_nbr, int64_t* __restrict__ out_eid) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kSampleBlock + threadIdx.x;
  if (p >= num_out) return;
  const int64_t i = seg_of_row(offsets, 0, n - 1, p);
  int64_t start;
  const int64_t deg = row_degree(indptr, num_rows, rows[i], &start);
  const int64_t k = p - offsets[i];
  if (k < 0 || k >= deg) return;
  out_nbr[p] = indices[start + k];
  out_eid[p] = data[start + k];
}

// ---- block relabel -------------------------------------------------------------------
// position p: destination p for p < S (skipped unless include_dst), edge p - S otherwise
__device__ __forceinline__ int32_t relabel_node(const int32_t* dst_nodes, const int32_t* src, int64_t S,
                                                int64_t p, int include_dst, int64_t num_nodes) {
  int32_t v;
  if (p < S) {
    if (!include_dst) return -1;
    v = dst_nodes[p];
  } else {
    v = src[p - S];
  }
  return v >= 0 && v < num_nodes ? v : -1;
}

__global__ void __launch_bounds__(kSampleBlock)
k_relabel_min(int32_t* __restrict__ table, int64_t num_nodes, const int32_t* __restrict__ dst_nodes,
              int64_t S, const int32_t* __restrict__ src, int64_t P, int include_dst) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kSampleBlock + threadIdx.x;
  if (p >= P) return;
  const int32_t v = relabel_node(dst_nodes, src, S, p, include_dst, num_nodes);
  if (v >= 0) atomicMin(&table[v], static_cast<int32_t>(p));  // result unused: no return
}

__global__ void __launch_bounds__(kSampleBlock)
k_relabel_flag(const int32_t* __restrict__ table, int64_t num_nodes,
               const int32_t* __restrict__ dst_nodes, int64_t S, const int32_t* __restrict__ src,
               int64_t P, int include_dst, int32_t* __restrict__ flags) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kSampleBlock + threadIdx.x;
  if (p >= P) return;
  const int32_t v = relabel_node(dst_nodes, src, S, p, include_dst, num_nodes);
  flags[p] = v >= 0 && table[v] == static_cast<int32_t>(p) ? 1 : 0;
}

__global__ void __launch_bounds__(kSampleBlock)
k_relabel_write(const int32_t* __restrict__ table, int64_t num_nodes,
                const int32_t* __restrict__ dst_nodes, int64_t S, const int32_t* __restrict__ src,
                int64_t P, int include_dst, const int32_t* __restrict__ flags,
                const int32_t* __restrict__ scan, int64_t* __restrict__ src_nodes,
                int32_t* __restrict__ new_src, int64_t* __restrict__ counts) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kSampleBlock + threadIdx.x;
  if (p == 0) {
    counts[0] = P > 0 ? scan[P - 1] : 0;
    counts[1] = S > 0 && P >= S ? scan[S - 1] : 0;
  }
  if (p >= P) return;
  const int32_t v = relabel_node(dst_nodes, src, S, p, include_dst, num_nodes);
  int32_t id = -1;
  if (v >= 0) {
    const int32_t owner = table[v];
    if (owner >= 0 && owner < P) id = scan[owner] - 1;
  }
  if (p >= S) new_src[p - S] = id;
  if (id >= 0 && flags[p]) src_nodes[id] = v;
}

__global__ void __launch_bounds__(kSampleBlock)
k_relabel_reset(int32_t* __restrict__ table, int64_t num_nodes, const int32_t* __restrict__ dst_nodes,
                int64_t S, const int32_t* __restrict__ src, int64_t P, int include_dst) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kSampleBlock + threadIdx.x;
  if (p >= P) return;
  const int32_t v = relabel_node(dst_nodes, src, S, p, include_dst, num_nodes);
  if (v >= 0) table[v] = kRelabelFree;
}

unsigned blocks_for(int64_t n) { return static_cast<unsigned>((n + kSampleBlock - 1) / kSampleBlock); }

}  // namespace

int sample_max_fanout() { return kSampleMaxFanout; }

int sample_group_width(int fanout) {
  int g = 4;
  while (g < fanout) g <<= 1;
  return g;
}

void launch_sample_count(const SampleCsr& c, const int32_t* seeds, int64_t num_seeds, int fanout,
                         int replace, int64_t* cnt, hipStream_t s) {
  hipLaunchKernelGGL(k_sample_count, dim3(blocks_for(num_seeds > 0 ? num_seeds : 1)),
                     dim3(kSampleBlock), 0, s, c.indptr, c.num_rows, seeds, num_seeds, fanout, replace,
                     cnt);
}

void launch_sample_pick(const SampleCsr& c, const int32_t* seeds, int64_t num_seeds, int fanout,
                        int replace, uint64_t rng_seed, uint64_t rng_ctr, const int64_t* offsets,
                        int64_t num_out, int32_t* out_nbr, int64_t* out_eid, hipStream_t s) {
  if (num_seeds == 0 || num_out == 0 || fanout == 0) return;
  const int G = sample_group_width(fanout);
  const dim3 grid(blocks_for(num_seeds * G)), block(kSampleBlock);
#define DGLMI_PICK(W)                                                                           \
  hipLaunchKernelGGL(k_sample_pick<W>, grid, block, 0, s, c.indptr, c.indices, c.data, c.num_rows, \
                     seeds, num_seeds, fanout, replace, rng_seed, rng_ctr, offsets, num_out,    \
                     out_nbr, out_eid)
  switch (G) {
    case 4: DGLMI_PICK(4); break;
    case 8: DGLMI_PICK(8); break;
    case 16: DGLMI_PICK(16); break;
    case 32: DGLMI_PICK(32); break;
    default: DGLMI_PICK(64); break;
  }
#undef DGLMI_PICK
}

void launch_gather_rows(const SampleCsr& c, const int32_t* rows, int64_t n, const int64_t* offsets,
                        int64_t num_out, int32_t* out_nbr, int64_t* out_eid, hipStream_t s) {
  if (n == 0 || num_out == 0) return;
  hipLaunchKernelGGL(k_gather_rows, dim3(blocks_for(num_out)), dim3(kSampleBlock), 0, s, c.indptr,
                     c.indices, c.data, c.num_rows, rows, n, offsets, num_out, out_nbr, out_eid);
}

void launch_relabel_mark(int32_t* table, int64_t num_nodes, const int32_t* dst_nodes, int64_t S,
                         const int32_t* src, int64_t E, int include_dst, int32_t* flags,
                         hipStream_t s) {
  const int64_t P = S + E;
  if (P == 0) return;
  const dim3 grid(blocks_for(P)), block(kSampleBlock);
  hipLaunchKernelGGL(k_relabel_min, grid, block, 0, s, table, num_nodes, dst_nodes, S, src, P,
                     include_dst);
  hipLaunchKernelGGL(k_relabel_flag, grid, block, 0, s, table, num_nodes, dst_nodes, S, src, P,
                     include_dst, flags);
}

void launch_relabel_write(int32_t* table, int64_t num_nodes, const int32_t* dst_nodes, int64_t S,
                          const int32_t* src, int64_t E, int include_dst, const int32_t* flags,
                          const int32_t* scan, int64_t* src_nodes, int32_t* new_src, int64_t* counts,
                          hipStream_t s) {
  const int64_t P = S + E;
  const dim3 grid(blocks_for(P > 0 ? P : 1)), block(kSampleBlock);
  hipLaunchKernelGGL(k_relabel_write, grid, block, 0, s, table, num_nodes, dst_nodes, S, src, P,
                     include_dst, flags, scan, src_nodes, new_src, counts);
  if (P == 0) return;
  hipLaunchKernelGGL(k_relabel_reset, grid, block, 0, s, table, num_nodes, dst_nodes, S, src, P,
                     include_dst);
}

}  // namespace dglmi
