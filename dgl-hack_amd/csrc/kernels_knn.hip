// k nearest neighbours inside the segments of a batch (dgl.knn_graph / segmented_knn_graph):
// squared distances and the selection of the k smallest in one kernel, so the (N, M)
// distance matrix of the reference (transform.py:45-141: pairwise_squared_distance, topk,
// a host copy, scipy) never exists.
//
// The walk.  One 256-lane workgroup owns kKnnTQ consecutive rows (its queries) whatever
// the segment sizes, as the segment walk of kernels_segment.hip does: a batch of 8-40 point
// sets fills a tile.  Its candidates run from the segment start of its first row to the
// segment end of its last row; a query masks the candidates outside its own [lo, hi).
// Candidates stream through LDS in tiles of kKnnTC rows and features in chunks of kKnnDC,
// both tiles stored feature-major so that a lane reads its four queries and its four
// candidates of one feature with one 16-byte LDS read each.  Lane (qy, cx) of the 16 x 16
// lane grid accumulates the 4 x 4 distances of queries 4 qy .. and candidates 4 cx ..:
// per feature a rounded subtraction, a rounded square and a rounded add, features in
// ascending order (the build's -ffp-contract=off), so d(i, j) is a function of x alone.
//
// The selection.  Every (distance, row) pair is one 64-bit key: the distance's bits (it is
// never negative, so its bits order as it does; any NaN becomes 0xffffffff, after +inf)
// above the row id.  Unsigned order on keys is the contract's strict total order.  A query
// keeps its k smallest keys sorted in LDS; an empty slot is the all-ones key, above every
// real one.  After a candidate tile's distances are complete a lane tests its candidates
// against the query's current k-th key; a survivor leaves its distance in an LDS tile and
// its bit in the query's 64-bit survivor mask (an LDS integer or: the order of arrival
// cannot matter).  After a barrier each wavefront inserts the survivors of 16 of the
// queries, in candidate order, a query's list held across its 64 lanes (hence k <= 64).
// Once a list is full the expected number of survivors is about k ln(M / k) per query over
// the whole walk.
//
// No float atomics, no global atomics, no scratch, no workspace; the result is the same
// bits on every run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace dglmi {
namespace {

constexpr int kKnnBlock = 256;
constexpr int kKnnTQ = 64;    // queries per workgroup
constexpr int kKnnTC = 64;    // candidates per LDS tile
constexpr int kKnnDC = 16;    // features per LDS chunk
constexpr int kKnnMaxK = 64;  // lists of 64 x (k | 1) keys: 33 KB of the 64 KB at k = 64
constexpr int kKnnRow = kKnnTQ + 4;  // floats per feature row of a tile: 16-byte aligned, and
                                     // a wavefront's transposing stores spread over the banks
constexpr int kKnnDRow = kKnnTC + 1; // floats per query row of the survivor distances
constexpr uint64_t kKnnEmpty = ~uint64_t(0);

__device__ __forceinline__ uint64_t knn_key(float d, int32_t row) {
  const uint32_t b = d != d ? 0xffffffffu : __float_as_uint(d);
  return (static_cast<uint64_t>(b) << 32) | static_cast<uint32_t>(row);
}

// lane l's value of v in lane l + 1 (lane 0 gets 0): the DPP wavefront shift, a register
// move where __shfl_up is an LDS-crossbar round trip per insertion
__device__ __forceinline__ uint32_t knn_lane_below(uint32_t v) {
  return static_cast<uint32_t>(
      __builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

// rows r0 .. r0 + 63, features f0 .. f0 + len - 1 of x into tile[f][row]; rows outside
// [0, N) read nothing and leave zeros (they are masked, but must not be fetched)
__device__ __forceinline__ void knn_load(const float* __restrict__ x, int64_t N, int64_t D,
                                         int64_t r0, int64_t f0, int len, float* tile, int tid) {
  if (len == D) {
    // whole rows: the tile's rows are one contiguous run of 64 D floats
    for (int idx = tid; idx < kKnnTQ * len; idx += kKnnBlock) {
      const int r = idx / len, f = idx - r * len;
      const int64_t row = r0 + r;
      tile[f * kKnnRow + r] = row < N ? x[row * D + f] : 0.0f;
    }
  } else {
    // kKnnDC or fewer floats of every row: 16 lanes a row, 16 rows a pass
    const int f = tid & (kKnnDC - 1);
    for (int r = tid / kKnnDC; r < kKnnTQ; r += kKnnBlock / kKnnDC) {
      const int64_t row = r0 + r;
      if (f < len) tile[f * kKnnRow + r] = row < N ? x[row * D + f0 + f] : 0.0f;
    }
  }
}

__device__ __forceinline__ void knn_accumulate(const float4& q, const float4& c, float (&acc)[4][4]) {
  const float qv[4] = {q.x, q.y, q.z, q.w};
  const float cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t = qv[i] - cv[j];
      acc[i][j] += t * t;
    }
  }
}

__global__ void __launch_bounds__(kKnnBlock)
k_knn_select(const float* __restrict__ x, const int64_t* __restrict__ offsets, int64_t B, int64_t N,
             int64_t D, int k, int32_t* __restrict__ nbr, float* __restrict__ dist) {
  extern __shared__ __align__(16) unsigned char knn_lds[];
  __shared__ float sh_q[kKnnDC * kKnnRow];
  __shared__ float sh_c[kKnnDC * kKnnRow];
  __shared__ float sh_d[kKnnTQ * kKnnDRow];
  __shared__ unsigned int sh_mask[kKnnTQ][2];
  __shared__ int32_t sh_lo[kKnnTQ], sh_hi[kKnnTQ];
  uint64_t* lists = reinterpret_cast<uint64_t*>(knn_lds);  // [kKnnTQ][ks]
  const int ks = k | 1;  // odd: the inserting lanes' lists start in different banks

  const int tid = threadIdx.x;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kKnnTQ;
  const int nq = N - r0 < kKnnTQ ? static_cast<int>(N - r0) : kKnnTQ;

  for (int i = tid; i < kKnnTQ * ks; i += kKnnBlock) lists[i] = kKnnEmpty;
  if (tid < kKnnTQ) {
    sh_mask[tid][0] = 0;
    sh_mask[tid][1] = 0;
    int64_t lo = 0, hi = 0;
    if (tid < nq) {
      const int64_t s = seg_of_row(offsets, 0, B - 1, r0 + tid);
      lo = offsets[s];
      hi = offsets[s + 1];
      lo = lo < 0 ? 0 : (lo > N ? N : lo);
      hi = hi < lo ? lo : (hi > N ? N : hi);
    }
    sh_lo[tid] = static_cast<int32_t>(lo);
    sh_hi[tid] = static_cast<int32_t>(hi);
  }
  __syncthreads();
  const int64_t cbeg = sh_lo[0], cend = sh_hi[nq - 1];

  const int qy = tid >> 4, cx = tid & 15;
  const int wave = tid >> 6, lane = tid & 63;
  int32_t qlo[4], qhi[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    qlo[i] = sh_lo[qy * 4 + i];
    qhi[i] = sh_hi[qy * 4 + i];
  }
  const bool q_once = D <= kKnnDC;  // the query tile is whole rows: staged once
  if (q_once) knn_load(x, N, D, r0, 0, static_cast<int>(D), sh_q, tid);

  for (int64_t c0 = cbeg; c0 < cend; c0 += kKnnTC) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
    }
    for (int64_t f0 = 0; f0 < D; f0 += kKnnDC) {
      const int len = D - f0 < kKnnDC ? static_cast<int>(D - f0) : kKnnDC;
      __syncthreads();  // the tiles' readers, and the previous tile's insertions, are done
      if (!q_once) knn_load(x, N, D, r0, f0, len, sh_q, tid);
      knn_load(x, N, D, c0, f0, len, sh_c, tid);
      __syncthreads();
      if (len == kKnnDC) {
        // four features in flight: unrolled whole, the 16 features' LDS reads are all
        // hoisted and the kernel takes 200 VGPRs (two waves per SIMD)
#pragma unroll 4
        for (int f = 0; f < kKnnDC; ++f)
          knn_accumulate(*reinterpret_cast<const float4*>(sh_q + f * kKnnRow + qy * 4),
                         *reinterpret_cast<const float4*>(sh_c + f * kKnnRow + cx * 4), acc);
      } else {
        for (int f = 0; f < len; ++f)
          knn_accumulate(*reinterpret_cast<const float4*>(sh_q + f * kKnnRow + qy * 4),
                         *reinterpret_cast<const float4*>(sh_c + f * kKnnRow + cx * 4), acc);
      }
    }
    // survivors of this tile: below the query's k-th key, inside the query's segment
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = qy * 4 + i;
      const uint64_t thr = lists[q * ks + k - 1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = cx * 4 + j;
        const int64_t row = c0 + c;
        if (row >= qlo[i] && row < qhi[i] && knn_key(acc[i][j], static_cast<int32_t>(row)) < thr) {
          sh_d[q * kKnnDRow + c] = acc[i][j];
          atomicOr(&sh_mask[q][c >> 5], 1u << (c & 31));
        }
      }
    }
    __syncthreads();
    // Each wavefront inserts for 16 of the queries, one query at a time with the list
    // across its lanes (k <= 64): lane j holds entry j, the survivor's place is the
    // number of entries below it (they are a prefix: the list is sorted), and the entries
    // from there on move up one lane.  A few instructions per survivor and no dependent
    // LDS round trip; one lane walking its list entry by entry took 0.5 ms of the 32 x
    // 1024-point shapes (scripts/bench_knn.py) against 0.02 ms of distance arithmetic.
    // the 32 mask words of the wavefront's 16 queries: one LDS read, then lane reads
    const uint32_t mw =
        lane < 32 ? reinterpret_cast<const uint32_t*>(sh_mask)[wave * (kKnnTQ / 2) + lane] : 0u;
    if (__ballot(mw != 0) == 0) continue;
    for (int qi = 0; qi < kKnnTQ / 4; ++qi) {
      const int q = wave * (kKnnTQ / 4) + qi;
      uint64_t m = (static_cast<uint64_t>(static_cast<uint32_t>(
                        __builtin_amdgcn_readlane(static_cast<int>(mw), 2 * qi + 1))) << 32) |
                   static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(mw), 2 * qi));
      if (m == 0) continue;
      uint64_t mine = lane < k ? lists[q * ks + lane] : kKnnEmpty;
      // lane c: the key bits of candidate c's distance (read only where c survived)
      const uint32_t kb = static_cast<uint32_t>(knn_key(sh_d[q * kKnnDRow + lane], 0) >> 32);
      while (m) {
        const int c = __builtin_ctzll(m);
        m &= m - 1;
        const uint64_t key =
            (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(kb, c))) << 32) |
            static_cast<uint32_t>(c0 + c);
        const int pos = __popcll(__ballot(mine < key));
        if (pos >= k) continue;  // an earlier survivor of this tile moved the bar
        const uint32_t up_lo = knn_lane_below(static_cast<uint32_t>(mine));
        const uint32_t up_hi = knn_lane_below(static_cast<uint32_t>(mine >> 32));
        if (lane == pos) mine = key;
        else if (lane > pos) mine = (static_cast<uint64_t>(up_hi) << 32) | up_lo;
      }
      if (lane < k) lists[q * ks + lane] = mine;
    }
    if (lane < 32) reinterpret_cast<uint32_t*>(sh_mask)[wave * (kKnnTQ / 2) + lane] = 0u;
  }
  __syncthreads();
  // the tile's rows are consecutive: nq k entries, one contiguous run of each output
  const int64_t out0 = r0 * k;
  for (int i = tid; i < nq * k; i += kKnnBlock) {
    const int q = i / k, j = i - q * k;
    const uint64_t key = lists[q * ks + j];
    const uint32_t b = static_cast<uint32_t>(key >> 32);
    const bool empty = key == kKnnEmpty;
    nbr[out0 + i] = empty ? -1 : static_cast<int32_t>(static_cast<uint32_t>(key));
    if (dist != nullptr)
      dist[out0 + i] = empty ? __uint_as_float(0x7f800000u)
                             : __uint_as_float(b == 0xffffffffu ? 0x7fc00000u : b);
  }
}

}  // namespace

int knn_max_k() { return kKnnMaxK; }

void knn_tile(int64_t D, int k, int* tq, int* tc, int* dc) {
  (void)D;
  (void)k;
  *tq = kKnnTQ;
  *tc = kKnnTC;
  *dc = kKnnDC;
}

void launch_knn_select(const float* x, const int64_t* offsets, int64_t num_segments, int64_t N,
                       int64_t D, int k, int32_t* nbr, float* dist, hipStream_t s) {
  if (N == 0) return;
  const unsigned grid = static_cast<unsigned>((N + kKnnTQ - 1) / kKnnTQ);
  const size_t lds = static_cast<size_t>(kKnnTQ) * (k | 1) * sizeof(uint64_t);
  hipLaunchKernelGGL(k_knn_select, dim3(grid), dim3(kKnnBlock), lds, s, x, offsets, num_segments, N,
                     D, k, nbr, dist);
}

}  // namespace dglmi
