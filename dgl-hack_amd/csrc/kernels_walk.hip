// Random walks and PinSAGE visit counts on the device (dgl.sampling.random_walk,
// RandomWalkNeighborSampler / PinSAGESampler): the reference's OpenMP loop over seeds
// (src/graph/sampling/randomwalks/randomwalks_cpu.h:47-61, metapath_randomwalk.h:61-98) and
// its to_simple(return_counts) + select_topk + gather (python/dgl/sampling/pinsage.py:103-117)
// restated so that no node id leaves the GPU.  include/dglmi.h states the two contracts; this
// file is one way to meet them.
//
// The walk.  A walk is a chain of dependent loads -- indptr[v], indptr[v + 1], indices[.] --
// with nothing to share inside it, so one lane owns one walk and the parallelism is walks in
// flight: 64-lane workgroups (one wavefront), few registers, 32 of them per CU.  The
// relations' CSRs travel in the kernel argument (WalkTable); the relation of a step is
// launch-uniform, so its row is read with scalar loads.  One Philox4x32-10 block per lane and
// step gives the pick (x) and the restart draw (y).  The loop over steps has launch-uniform
// bounds and every lane runs all of it: a finished lane carries -1 and loads nothing, and no
// wavefront-level branch surrounds the barrier of the staged variant.
//
// Stores.  A lane that stores its own trace row writes 8 bytes at a stride of (L + 1) * 8: 64
// partial lines per wave-instruction (k_walk<false>, variant 1).  The staged variant
// (k_walk<true>, variant 2) keeps kWalkChunk columns of the wavefront's 64 rows in LDS,
// column-major with a padded column so both the per-lane writes and the flush's reads are
// free of bank conflicts, and flushes them row by row: kWalkChunk * 8 contiguous bytes per
// row, and the whole 64 * (L + 1) * 8-byte region in one contiguous sweep when L + 1 <=
// kWalkChunk (a wavefront's rows are adjacent).
//
// The visit counts.  A group of T lanes serves one seed slot: it loads the slot's W
// candidates into an LDS array of P = the next power of two >= max(W, 64) unsigned keys
// (ignored entries become the top sentinel), sorts it (bitonic), finds the run heads, gets
// each head's run length by a binary search for the run's end, builds one 64-bit key
// (~count, id) per head -- sentinel elsewhere -- sorts those and writes the first K.  Every
// group of a workgroup runs the same number of stages whatever its slot holds, so the
// workgroup barriers are uniform; a group past the last slot sorts sentinels and stores
// nothing.  No atomics, no float arithmetic: the same bits on every run.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace dglmi {
namespace {

constexpr int kWalkBlock = 64;   // one wavefront: the staged variant's barrier is wave-wide
constexpr int kWalkChunk = 8;    // columns staged per flush
constexpr int kWalkColPad = 72;  // LDS column stride in entries: 72 = 8 mod 32 (64-bit banks)

template <bool STAGED>
__global__ void __launch_bounds__(kWalkBlock)
k_walk(WalkTable tab, const int32_t* __restrict__ metapath, int64_t L,
       const int32_t* __restrict__ seeds, int64_t num_walks, const uint64_t* __restrict__ restart,
       uint64_t rng_seed, uint64_t rng_ctr, int64_t* __restrict__ traces) {
  __shared__ int64_t stage[STAGED ? kWalkChunk * kWalkColPad : 1];
  const int lane = threadIdx.x;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kWalkBlock;
  const int64_t i = i0 + lane;
  const bool live = i < num_walks;
  const int64_t row_len = L + 1;
  int64_t rows_here = num_walks - i0;  // the wavefront's rows inside the output
  if (rows_here > kWalkBlock) rows_here = kWalkBlock;
  const uint32_t k0 = static_cast<uint32_t>(rng_seed), k1 = static_cast<uint32_t>(rng_seed >> 32);
  const uint64_t slot = static_cast<uint64_t>(i);

  int64_t v = live ? static_cast<int64_t>(seeds[i]) : -1;
  bool alive = live;
  for (int64_t c0 = 0; c0 < row_len; c0 += kWalkChunk) {
    const int cw = static_cast<int>(row_len - c0 < kWalkChunk ? row_len - c0 : kWalkChunk);
    for (int k = 0; k < cw; ++k) {
      const int64_t col = c0 + k;
      if (col > 0) {
        const int64_t t = col - 1;
        // launch-uniform: scalar loads
        const int rel = tab.num_rels == 1 ? 0 : metapath[t];
        const uint64_t stop_below = restart != nullptr ? restart[t] : 0;
        int64_t next = -1;
        if (alive) {
          int64_t deg = 0, start = 0;
          if (rel >= 0 && rel < tab.num_rels) {
            const WalkRel& r = tab.rel[rel];
            if (v >= 0 && v < r.num_rows) {
              const IdxPtr ip{r.indptr, r.wide};
              start = ip[v];
              deg = ip[v + 1] - start;
            }
            if (deg > 0) {
              const uint64_t c = rng_ctr + static_cast<uint64_t>(t);
              const Philox4 d = philox4x32_10(
                  Philox4{static_cast<uint32_t>(c), static_cast<uint32_t>(c >> 32),
                          static_cast<uint32_t>(slot), static_cast<uint32_t>(slot >> 32)},
                  k0, k1);
              const int64_t pos =
                  static_cast<int64_t>((static_cast<uint64_t>(d.x) * static_cast<uint64_t>(deg)) >> 32);
              next = static_cast<int64_t>(r.indices[start + pos]);
              if (static_cast<uint64_t>(d.y) < stop_below) alive = false;
            }
          }
          if (deg <= 0) alive = false;
        }
        v = next;
      }
      if constexpr (STAGED) {
        stage[k * kWalkColPad + lane] = v;
      } else {
        if (live) traces[i * row_len + col] = v;
      }
    }
    if constexpr (STAGED) {
      __syncthreads();
      // entry e of the chunk: row e / cw, column c0 + e % cw -- cw * 8 contiguous bytes per row
      const int n = static_cast<int>(rows_here) * cw;
      for (int e = lane; e < n; e += kWalkBlock) {
        const int row = e / cw;
        const int k = e - row * cw;
        traces[(i0 + row) * row_len + c0 + k] = stage[k * kWalkColPad + row];
      }
      __syncthreads();
    }
  }
}

// ---- visit counts ------------------------------------------------------------------------
constexpr int kVisitBlock = 256;
constexpr int kVisitMaxK = 64;
constexpr int kVisitMinWidth = 64;    // >= kVisitMaxK: the first K keys always exist
constexpr int kVisitMaxWidth = 4096;
constexpr uint32_t kVisitNoId = 0xffffffffu;
constexpr uint64_t kVisitNoKey = ~uint64_t(0);

// lanes that serve one seed slot at padded width P
constexpr int visit_group(int P) { return P <= 256 ? 64 : (P == 512 ? 128 : 256); }

// ascending bitonic sort of a[0 .. P) by the T lanes of a group (lane g); every lane of the
// workgroup calls it with the same P and T
template <typename Key, int P, int T>
__device__ __forceinline__ void visit_sort(Key* a, int g) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = g; p < P / 2; p += T) {
        const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const int hi = lo | j;
        const Key x = a[lo], y = a[hi];
        const bool up = (lo & k) == 0;
        if ((x > y) == up) {
          a[lo] = y;
          a[hi] = x;
        }
      }
      __syncthreads();
    }
  }
}

template <int P>
__global__ void __launch_bounds__(kVisitBlock)
k_visit_topk(const int64_t* __restrict__ traces, int64_t row_len, int64_t num_seeds,
             int64_t walks_per_seed, int64_t col0, int64_t col_step, int ncols, int W, int K,
             int32_t* __restrict__ out_nbr, int32_t* __restrict__ out_cnt,
             int32_t* __restrict__ out_num) {
  constexpr int T = visit_group(P);
  constexpr int S = kVisitBlock / T;  // seed slots per workgroup
  __shared__ uint32_t ids[S][P];
  __shared__ uint64_t keys[S][P];
  const int grp = threadIdx.x / T;
  const int g = threadIdx.x - grp * T;
  const int64_t s = static_cast<int64_t>(blockIdx.x) * S + grp;
  const bool live = s < num_seeds;
  uint32_t* a = ids[grp];
  uint64_t* b = keys[grp];

  for (int e = g; e < P; e += T) {
    uint32_t id = kVisitNoId;
    if (live && e < W) {
      const int w = e / ncols;
      const int c = e - w * ncols;
      const int64_t x = traces[(s * walks_per_seed + w) * row_len + col0 + c * col_step];
      if (x >= 0 && x < static_cast<int64_t>(0x7fffffff)) id = static_cast<uint32_t>(x);
    }
    a[e] = id;
  }
  __syncthreads();
  visit_sort<uint32_t, P, T>(a, g);
  // run heads: (~count, id); the run's end is the first position whose id is larger
  for (int e = g; e < P; e += T) {
    const uint32_t id = a[e];
    uint64_t key = kVisitNoKey;
    if (id != kVisitNoId && (e == 0 || a[e - 1] != id)) {
      int lo = e + 1, hi = P;  // the first position in [e + 1, P] with a[.] > id
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] > id) hi = mid;
        else lo = mid + 1;
      }
      const uint32_t cnt = static_cast<uint32_t>(lo - e);
      key = (static_cast<uint64_t>(~cnt) << 32) | id;
    }
    b[e] = key;
  }
  __syncthreads();
  visit_sort<uint64_t, P, T>(b, g);
  if (!live) return;
  for (int j = g; j < K; j += T) {  // K <= kVisitMinWidth <= P
    const uint64_t key = b[j];
    const bool have = key != kVisitNoKey;
    out_nbr[s * K + j] = have ? static_cast<int32_t>(static_cast<uint32_t>(key)) : -1;
    out_cnt[s * K + j] = have ? static_cast<int32_t>(~static_cast<uint32_t>(key >> 32)) : 0;
    if (have && (j + 1 == K || b[j + 1] == kVisitNoKey)) out_num[s] = j + 1;
    if (!have && j == 0) out_num[s] = 0;
  }
}

int visit_padded(int64_t W) {
  int P = kVisitMinWidth;
  while (P < W) P <<= 1;
  return P;
}

}  // namespace

int walk_max_relations() { return kWalkMaxRels; }
int walk_stage_chunk() { return kWalkChunk; }

void launch_walk(const WalkTable& tab, const int32_t* metapath, int64_t L, const int32_t* seeds,
                 int64_t num_walks, const uint64_t* restart, uint64_t rng_seed, uint64_t rng_ctr,
                 bool staged, int64_t* traces, hipStream_t s) {
  if (num_walks == 0) return;
  const dim3 grid(static_cast<unsigned>((num_walks + kWalkBlock - 1) / kWalkBlock)), block(kWalkBlock);
  if (staged) {
    hipLaunchKernelGGL(k_walk<true>, grid, block, 0, s, tab, metapath, L, seeds, num_walks, restart,
                       rng_seed, rng_ctr, traces);
  } else {
    hipLaunchKernelGGL(k_walk<false>, grid, block, 0, s, tab, metapath, L, seeds, num_walks, restart,
                       rng_seed, rng_ctr, traces);
  }
}

int visit_max_k() { return kVisitMaxK; }
int visit_max_width() { return kVisitMaxWidth; }

void visit_tile(int64_t W, int* padded, int* seeds_per_wg) {
  const int P = visit_padded(W);
  *padded = P;
  *seeds_per_wg = kVisitBlock / visit_group(P);
}

void launch_visit_topk(const int64_t* traces, int64_t row_len, int64_t num_seeds,
                       int64_t walks_per_seed, int64_t col0, int64_t col_step, int ncols, int K,
                       int32_t* out_nbr, int32_t* out_cnt, int32_t* out_num, hipStream_t s) {
  if (num_seeds == 0) return;
  const int W = static_cast<int>(walks_per_seed) * ncols;
  const int P = visit_padded(W);
  const int S = kVisitBlock / visit_group(P);
  const dim3 grid(static_cast<unsigned>((num_seeds + S - 1) / S)), block(kVisitBlock);
#define DGLMI_VISIT(PW)                                                                          \
  hipLaunchKernelGGL(k_visit_topk<PW>, grid, block, 0, s, traces, row_len, num_seeds,            \
                     walks_per_seed, col0, col_step, ncols, W, K, out_nbr, out_cnt, out_num)
  switch (P) {
    case 64: DGLMI_VISIT(64); break;
    case 128: DGLMI_VISIT(128); break;
    case 256: DGLMI_VISIT(256); break;
    case 512: DGLMI_VISIT(512); break;
    case 1024: DGLMI_VISIT(1024); break;
    case 2048: DGLMI_VISIT(2048); break;
    default: DGLMI_VISIT(4096); break;
  }
#undef DGLMI_VISIT
}

}  // namespace dglmi
