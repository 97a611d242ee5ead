// Ordered graph traversal on the device (dgl.traversal: BFS node / edge frontiers and
// topological frontiers): the reference's sequential queue loops (src/graph/traversal.h)
// restated as level-synchronous kernels that give the queue's own order.  include/dglmi.h
// states the contract; this file is one way to meet it.
//
// The queue is the output: q[head .. tail) is the frontier being expanded and new nodes are
// appended at tail.  gq, parallel to q, holds the running sum of the frontier's degrees
// (gq[head + i] = the first gathered position of slot i), so gathered position p is one CSR
// entry of one frontier row and a lane finds its row by a search in gq: a hub row spreads
// over many wavefronts.  st (the level state) carries head, tail, the level number, G and
// the counts the host reads back.
//
// Order without a sort.  BFS: every position whose column is unvisited does
// atomicMin(key[col], p); the position that finds its own p in key[col] afterwards is the
// column's first occurrence, and ranking those positions in ascending p (ballot bitmap,
// popcounts, v_mbcnt, as in kernels_subgraph.hip) appends the columns in the order the
// sequential queue discovers them.  Topological: every position decrements remaining[col];
// then positions whose column reached 0 do atomicMax(key[col], p), so the winner is the
// sequential loop's last decrement.  A key is claimed at one level only (a BFS column is
// visited afterwards, a topological column has no in-edge left), so keys are never reset.
// Integer min / max / add commute: the result does not depend on the schedule.
//
// Wide route, one level: k_claim (topological: twice), k_count, k_scan_tiles (one
// workgroup), k_fill, k_advance (one workgroup: moves the state and turns the new frontier's
// degrees into their running sum).  Tiles are kTile = 1024 positions, a block of four
// wavefronts per tile, four 64-position words per wavefront.  No workgroup waits on another:
// every dependency is a kernel boundary.
//
// Narrow route: k_narrow, one workgroup of sixteen wavefronts, runs whole levels while the
// frontier has at most kNarrowLimit = 4096 rows and positions -- the running sum in LDS, the
// same claim / count / emit phases over the same word layout separated by __syncthreads()
// and __threadfence(), then the state update -- and goes on to the next level in the same
// launch, up to kMaxLevels levels.  A chain of hundreds of one-node levels costs a handful of
// launches.  Data that other phases of the same launch wrote (q, key, visited, remaining)
// is read with agent-scope atomic loads, which do not take a stale line from the L1.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace dglmi {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kWaveWords = 4;                    // 64-position words per wavefront
constexpr int kTileWords = kWaves * kWaveWords;  // 16
constexpr int kTile = kTileWords * 64;           // 1024 positions
constexpr int kWgBlock = 1024;                   // the single-workgroup kernels
constexpr int kWgWaves = kWgBlock / 64;
constexpr int kNarrowLimit = 4 * kTile;          // kWgBlock lanes x kWaveWords positions
constexpr int kNarrowWords = kNarrowLimit / 64;
constexpr int kMaxLevels = 128;
static_assert(kNarrowLimit == kWgBlock * kWaveWords, "one narrow lane owns kWaveWords positions");

template <typename T>
__device__ __forceinline__ T ld(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename K>
struct Trav {
  SampleCsr c;       // the walked CSR (square: num_rows nodes)
  int kind;
  int64_t* st;       // kTraverseStateWords
  int64_t* sections;
  int64_t cap_sections;
  int32_t* q;
  int64_t* gq;
  int64_t cap_q;
  int64_t* eids;     // BFS edges only
  int64_t cap_e;
  K* key;
  uint32_t* visited; // BFS
  int32_t* rem;      // topological
  uint64_t* keep;
  int64_t* tile_cnt;
  int64_t cap_pos;   // keep holds ceil(cap_pos / 64) words, tile_cnt ceil(cap_pos / kTile)
};

__device__ __forceinline__ void key_min(int32_t* k, int64_t p) { atomicMin(k, static_cast<int32_t>(p)); }
__device__ __forceinline__ void key_min(int64_t* k, int64_t p) {
  atomicMin(reinterpret_cast<long long*>(k), static_cast<long long>(p));
}
__device__ __forceinline__ void key_max(int32_t* k, int64_t p) { atomicMax(k, static_cast<int32_t>(p)); }
__device__ __forceinline__ void key_max(int64_t* k, int64_t p) {
  atomicMax(reinterpret_cast<long long*>(k), static_cast<long long>(p));
}

template <typename K>
__device__ __forceinline__ bool topo(const Trav<K>& a) { return a.kind == kTraverseTopo; }

__device__ __forceinline__ int64_t row_degree(const SampleCsr& c, int64_t v) {
  return v >= 0 && v < c.num_rows ? c.indptr[v + 1] - c.indptr[v] : 0;
}

// the positions that slot `slot` of the frontier at `head` contributes: its row's degree,
// and 0 for a BFS source that an earlier slot already holds (k_bfs_mark left the first slot
// in key): the repeated row's columns all occur earlier and can win nothing
template <typename K>
__device__ __forceinline__ int64_t slot_degree(const Trav<K>& a, int64_t head, int64_t slot,
                                               bool sources) {
  const int64_t v = ld(a.q + head + slot);
  if (v < 0 || v >= a.c.num_rows) return 0;
  if (sources && !topo(a) && static_cast<int64_t>(ld(a.key + v)) != slot) return 0;
  return row_degree(a.c, v);
}

// position p -> its CSR entry (-1: none); off = the frontier's running sum (S values)
template <typename K>
__device__ __forceinline__ int64_t entry_of(const Trav<K>& a, const int64_t* off, const int32_t* f,
                                            int64_t lo, int64_t hi, int64_t p) {
  const int64_t i = seg_of_row(off, lo, hi, p);
  const int64_t row = f[i];
  if (row < 0 || row >= a.c.num_rows) return -1;
  const int64_t start = a.c.indptr[row];
  const int64_t k = p - off[i];
  return k >= 0 && k < a.c.indptr[row + 1] - start ? start + k : -1;
}

template <typename K>
__device__ __forceinline__ bool seen(const Trav<K>& a, int64_t v) {
  return (ld(a.visited + (v >> 5)) >> (v & 31)) & 1u;
}

// may column v join the next frontier at this level?
template <typename K>
__device__ __forceinline__ bool is_open(const Trav<K>& a, int64_t v) {
  return topo(a) ? ld(a.rem + v) == 0 : !seen(a, v);
}

// pass 0: BFS claim / topological decrement; pass 1: topological claim
template <typename K>
__device__ __forceinline__ void claim(const Trav<K>& a, int pass, int64_t col, int64_t p) {
  if (col < 0 || col >= a.c.num_rows) return;
  if (!topo(a)) {
    if (!seen(a, col)) key_min(a.key + col, p);
  } else if (pass == 0) {
    atomicSub(a.rem + col, 1);
  } else if (ld(a.rem + col) == 0) {
    key_max(a.key + col, p);
  }
}

template <typename K>
__device__ __forceinline__ bool wins(const Trav<K>& a, int64_t col, int64_t p) {
  return col >= 0 && col < a.c.num_rows && is_open(a, col) && static_cast<int64_t>(ld(a.key + col)) == p;
}

// append column col (found at CSR entry e) at queue index out
template <typename K>
__device__ __forceinline__ void emit(const Trav<K>& a, int64_t out, int64_t col, int64_t e) {
  if (out < 0 || out >= a.cap_q) return;
  a.q[out] = static_cast<int32_t>(col);
  a.gq[out] = row_degree(a.c, col);  // k_advance / k_narrow turn these into the running sum
  if (!topo(a)) atomicOr(a.visited + (col >> 5), 1u << (col & 31));
  const int64_t oe = out - a.st[kTravSources];
  if (a.kind == kTraverseBfsEdges && oe >= 0 && oe < a.cap_e) a.eids[oe] = a.c.data[e];
}

__device__ __forceinline__ int below(uint64_t bits) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(bits >> 32),
                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(bits), 0u));
}

// inclusive running sum over the workgroup's lanes in lane order; lds: one value per wave
template <int kW>
__device__ __forceinline__ int64_t block_scan(int64_t v, int64_t* lds, int64_t* total) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t t = __shfl_up(static_cast<long long>(v), d);
    if (lane >= d) v += t;
  }
  __syncthreads();  // the previous call's readers are done with lds
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  int64_t base = 0, all = 0;
  for (int w = 0; w < kW; ++w) {
    const int64_t x = lds[w];
    if (w < wave) base += x;
    all += x;
  }
  *total = all;
  return v + base;
}

__device__ __forceinline__ int64_t clamp_pos(int64_t g, int64_t cap) {
  return g < 0 ? 0 : (g < cap ? g : cap);
}

// ---- wide route -----------------------------------------------------------------------
template <typename K>
struct WaveSpan {  // the positions of one wavefront of a tile and their slot bounds
  int64_t w0, G, lo, hi, head;
  bool work;
};

template <typename K>
__device__ __forceinline__ WaveSpan<K> wave_span(const Trav<K>& a) {
  WaveSpan<K> s;
  s.G = clamp_pos(a.st[kTravG], a.cap_pos);
  s.head = a.st[kTravHead];
  const int64_t S = a.st[kTravTail] - s.head;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  s.w0 = static_cast<int64_t>(blockIdx.x) * kTile + static_cast<int64_t>(wave) * (kWaveWords * 64);
  s.work = s.w0 < s.G && S > 0 && s.head >= 0 && s.head + S <= a.cap_q;
  s.lo = s.hi = 0;
  if (s.work) {
    const int64_t wl = s.w0 + kWaveWords * 64 - 1;
    s.lo = seg_of_row(a.gq + s.head, 0, S - 1, s.w0);
    s.hi = seg_of_row(a.gq + s.head, s.lo, S - 1, wl < s.G ? wl : s.G - 1);
  }
  return s;
}

template <typename K>
__global__ void __launch_bounds__(kBlock) k_claim(Trav<K> a, int pass) {
  const WaveSpan<K> s = wave_span(a);
  if (!s.work) return;
  const int lane = threadIdx.x & 63;
  for (int k = 0; k < kWaveWords; ++k) {
    const int64_t p = s.w0 + k * 64 + lane;
    if (p >= s.G) break;
    const int64_t e = entry_of(a, a.gq + s.head, a.q + s.head, s.lo, s.hi, p);
    if (e >= 0) claim(a, pass, a.c.indices[e], p);
  }
}

template <typename K>
__global__ void __launch_bounds__(kBlock) k_count(Trav<K> a) {
  __shared__ int wave_cnt[kWaves];
  const WaveSpan<K> s = wave_span(a);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int cnt = 0;
  if (s.work) {
    for (int k = 0; k < kWaveWords; ++k) {
      const int64_t base = s.w0 + k * 64;
      if (base >= s.G) break;  // wave-uniform
      const int64_t p = base + lane;
      bool kept = false;
      if (p < s.G) {
        const int64_t e = entry_of(a, a.gq + s.head, a.q + s.head, s.lo, s.hi, p);
        kept = e >= 0 && wins(a, a.c.indices[e], p);
      }
      const uint64_t bits = __ballot(kept);
      if (lane == 0) a.keep[base >> 6] = bits;
      cnt += __popcll(bits);
    }
  }
  if (lane == 0) wave_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t sum = 0;
    for (int w = 0; w < kWaves; ++w) sum += wave_cnt[w];
    a.tile_cnt[blockIdx.x] = sum;
  }
}

// one workgroup: tile_cnt -> its inclusive running sum in place; st[Cnt] = the total
template <typename K>
__global__ void __launch_bounds__(kWgBlock) k_scan_tiles(Trav<K> a) {
  __shared__ int64_t lds[kWgWaves];
  const int64_t G = clamp_pos(a.st[kTravG], a.cap_pos);
  const int64_t tiles = (G + kTile - 1) / kTile;
  int64_t carry = 0;
  for (int64_t t0 = 0; t0 < tiles; t0 += kWgBlock) {
    const int64_t t = t0 + threadIdx.x;
    int64_t total;
    const int64_t v = block_scan<kWgWaves>(t < tiles ? a.tile_cnt[t] : 0, lds, &total);
    if (t < tiles) a.tile_cnt[t] = carry + v;
    carry += total;
  }
  if (threadIdx.x == 0) a.st[kTravCnt] = carry;
}

// nodes = true: the "positions" are the node ids themselves (topological frontier 0)
template <typename K>
__global__ void __launch_bounds__(kBlock) k_fill(Trav<K> a, bool nodes) {
  __shared__ int word_pop[kTileWords];
  const int64_t G = clamp_pos(a.st[kTravG], a.cap_pos);
  const int64_t t0 = static_cast<int64_t>(blockIdx.x) * kTile;
  if (t0 >= G) return;  // block-uniform: before the barrier
  if (threadIdx.x < kTileWords) {
    const int64_t base = t0 + static_cast<int64_t>(threadIdx.x) * 64;
    word_pop[threadIdx.x] = base < G ? __popcll(a.keep[base >> 6]) : 0;
  }
  __syncthreads();
  WaveSpan<K> s{};
  if (!nodes) {
    s = wave_span(a);
    if (!s.work) return;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t w0 = t0 + static_cast<int64_t>(wave) * (kWaveWords * 64);
  if (w0 >= G) return;
  int64_t rank0 = a.st[kTravTail] + (blockIdx.x > 0 ? a.tile_cnt[blockIdx.x - 1] : 0);
  for (int j = 0; j < wave * kWaveWords; ++j) rank0 += word_pop[j];
  for (int k = 0; k < kWaveWords; ++k) {
    const int64_t base = w0 + k * 64;
    if (base >= G) break;
    const uint64_t bits = a.keep[base >> 6];
    if ((bits >> lane) & 1) {
      const int64_t out = rank0 + below(bits);
      if (nodes) {
        emit(a, out, base + lane, 0);
      } else {
        const int64_t e = entry_of(a, a.gq + s.head, a.q + s.head, s.lo, s.hi, base + lane);
        if (e >= 0) emit(a, out, a.c.indices[e], e);
      }
    }
    rank0 += word_pop[wave * kWaveWords + k];
  }
}

// one workgroup: the st[Cnt] nodes appended at tail become the frontier -- their degrees in
// gq become the running sum, G its total -- or the traversal is done
template <typename K>
__global__ void __launch_bounds__(kWgBlock) k_advance(Trav<K> a) {
  __shared__ int64_t lds[kWgWaves];
  const int64_t tail = a.st[kTravTail];
  const int64_t level = a.st[kTravLevel];
  int64_t cnt = a.st[kTravCnt];
  if (tail < 0 || cnt < 0 || tail + cnt > a.cap_q || level >= a.cap_sections) cnt = 0;
  const bool sources = level == 0;
  const bool stop = cnt == 0 || a.st[kTravBad] != 0;
  int64_t carry = 0;
  if (!stop) {
    constexpr int kPer = 4;
    for (int64_t i0 = 0; i0 < cnt; i0 += kWgBlock * kPer) {
      int64_t d[kPer], sum = 0;
      const int64_t i = i0 + static_cast<int64_t>(threadIdx.x) * kPer;
      for (int j = 0; j < kPer; ++j) {
        d[j] = i + j < cnt ? (sources ? slot_degree(a, tail, i + j, true) : a.gq[tail + i + j]) : 0;
        sum += d[j];
      }
      int64_t total;
      int64_t run = carry + block_scan<kWgWaves>(sum, lds, &total) - sum;
      for (int j = 0; j < kPer; ++j) {
        if (i + j < cnt) a.gq[tail + i + j] = run;
        run += d[j];
      }
      carry += total;
    }
  }
  __syncthreads();  // every lane has read the state
  if (threadIdx.x == 0) {
    if (stop) {
      a.st[kTravDone] = 1;
    } else {
      a.sections[level] = cnt;
      a.st[kTravLevel] = level + 1;
      a.st[kTravHead] = tail;
      a.st[kTravTail] = tail + cnt;
      a.st[kTravG] = carry;
    }
  }
}

// ---- frontier 0 -----------------------------------------------------------------------
template <typename K>
__global__ void __launch_bounds__(kBlock) k_init(Trav<K> a, IdxPtr opp_indptr, int64_t num_sources) {
  const int64_t N = a.c.num_rows;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < N) {
    if (topo(a)) {
      a.key[i] = static_cast<K>(-1);
      a.rem[i] = static_cast<int32_t>(opp_indptr[i + 1] - opp_indptr[i]);
    } else {
      a.key[i] = static_cast<K>(sizeof(K) == 8 ? INT64_MAX : INT32_MAX);
    }
  }
  if (!topo(a) && i < (N + 31) / 32) a.visited[i] = 0;
  if (i < kTraverseStateWords) {
    int64_t v = 0;
    if (i == kTravSources) v = num_sources;
    if (i == kTravCnt) v = topo(a) ? 0 : num_sources;
    if (i == kTravG) v = topo(a) ? N : 0;  // k_fill(nodes): one position per node
    a.st[i] = v;
  }
}

// BFS: the sources verbatim; key keeps the first slot of every source
template <typename K>
__global__ void __launch_bounds__(kBlock)
k_bfs_mark(Trav<K> a, const int32_t* __restrict__ source, int64_t num_sources) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= num_sources || i >= a.cap_q) return;
  const int64_t v = source[i];
  a.q[i] = static_cast<int32_t>(v);
  if (v < 0 || v >= a.c.num_rows) {
    atomicAdd(reinterpret_cast<unsigned long long*>(a.st + kTravBad), 1ull);
    return;
  }
  key_min(a.key + v, i);
  atomicOr(a.visited + (v >> 5), 1u << (v & 31));
}

// topological: the bitmap of the nodes without an opposite edge, a tile of nodes per block
template <typename K>
__global__ void __launch_bounds__(kBlock) k_topo_roots(Trav<K> a) {
  __shared__ int wave_cnt[kWaves];
  const int64_t N = a.c.num_rows;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t w0 = static_cast<int64_t>(blockIdx.x) * kTile + static_cast<int64_t>(wave) * (kWaveWords * 64);
  int cnt = 0;
  for (int k = 0; k < kWaveWords; ++k) {
    const int64_t base = w0 + k * 64;
    if (base >= N) break;
    const int64_t v = base + lane;
    const uint64_t bits = __ballot(v < N && a.rem[v] == 0);
    if (lane == 0) a.keep[base >> 6] = bits;
    cnt += __popcll(bits);
  }
  if (lane == 0) wave_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t sum = 0;
    for (int w = 0; w < kWaves; ++w) sum += wave_cnt[w];
    a.tile_cnt[blockIdx.x] = sum;
  }
}

// ---- narrow route ---------------------------------------------------------------------
template <typename K>
__global__ void __launch_bounds__(kWgBlock) k_narrow(Trav<K> a) {
  __shared__ int64_t off[kNarrowLimit];
  __shared__ int32_t front[kNarrowLimit];
  __shared__ uint64_t words[kNarrowWords];
  __shared__ int word_base[kNarrowWords];
  __shared__ int64_t lds[kWgWaves];
  __shared__ int total_cnt;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int64_t head = a.st[kTravHead], tail = a.st[kTravTail], level = a.st[kTravLevel];
  if (a.st[kTravDone] != 0 || head < 0 || tail > a.cap_q) return;
  for (int it = 0; it < kMaxLevels; ++it) {  // bounded: the launch always ends
    const int64_t S = tail - head;
    if (S <= 0 || S > kNarrowLimit || level >= a.cap_sections) return;  // block-uniform
    // the frontier and the running sum of its degrees, in LDS and in gq
    int64_t d[kWaveWords], sum = 0;
    const int64_t i = static_cast<int64_t>(threadIdx.x) * kWaveWords;
    for (int j = 0; j < kWaveWords; ++j) {
      d[j] = i + j < S ? slot_degree(a, head, i + j, level == 1) : 0;
      sum += d[j];
    }
    int64_t G;
    int64_t run = block_scan<kWgWaves>(sum, lds, &G) - sum;
    for (int j = 0; j < kWaveWords; ++j) {
      if (i + j < S) {
        off[i + j] = run;
        front[i + j] = ld(a.q + head + i + j);
        a.gq[head + i + j] = run;
      }
      run += d[j];
    }
    if (threadIdx.x == 0) a.st[kTravG] = G;
    __syncthreads();
    if (G > kNarrowLimit || G > a.cap_pos) return;  // the wide route's level: gq is in place
    // resolve this lane's positions once
    int64_t col[kWaveWords], ent[kWaveWords];
    const int64_t w0 = static_cast<int64_t>(wave) * (kWaveWords * 64);
    for (int k = 0; k < kWaveWords; ++k) {
      const int64_t p = w0 + k * 64 + lane;
      ent[k] = p < G ? entry_of(a, off, front, 0, S - 1, p) : -1;
      col[k] = ent[k] >= 0 ? a.c.indices[ent[k]] : -1;
    }
    for (int pass = 0; pass < (topo(a) ? 2 : 1); ++pass) {
      for (int k = 0; k < kWaveWords; ++k)
        if (ent[k] >= 0) claim(a, pass, col[k], w0 + k * 64 + lane);
      __threadfence();
      __syncthreads();
    }
    for (int k = 0; k < kWaveWords; ++k) {
      const uint64_t bits = __ballot(ent[k] >= 0 && wins(a, col[k], w0 + k * 64 + lane));
      if (lane == 0) words[wave * kWaveWords + k] = bits;
    }
    __syncthreads();
    if (wave == 0) {  // kNarrowWords == 64: one word per lane
      const int pop = __popcll(words[lane]);
      int inc = pop;
      for (int dd = 1; dd < 64; dd <<= 1) {
        const int t = __shfl_up(inc, dd);
        if (lane >= dd) inc += t;
      }
      word_base[lane] = inc - pop;
      if (lane == 63) total_cnt = inc;
    }
    __syncthreads();
    const int cnt = total_cnt;
    for (int k = 0; k < kWaveWords; ++k) {
      const uint64_t bits = words[wave * kWaveWords + k];
      if ((bits >> lane) & 1) emit(a, tail + word_base[wave * kWaveWords + k] + below(bits), col[k], ent[k]);
    }
    __threadfence();
    __syncthreads();  // the level's writes are out; LDS may be reused
    if (cnt == 0 || tail + cnt > a.cap_q) {
      if (threadIdx.x == 0) a.st[kTravDone] = 1;
      return;
    }
    if (threadIdx.x == 0) {
      a.sections[level] = cnt;
      a.st[kTravLevel] = level + 1;
      a.st[kTravHead] = tail;
      a.st[kTravTail] = tail + cnt;
      a.st[kTravCnt] = cnt;
    }
    head = tail;
    tail += cnt;
    level += 1;
  }
  // the cap: the next frontier's running sum and G are not computed yet; do it so that the
  // state the host reads is whole
  {
    const int64_t S = tail - head;
    int64_t d[kWaveWords], sum = 0;
    const int64_t i = static_cast<int64_t>(threadIdx.x) * kWaveWords;
    for (int j = 0; j < kWaveWords; ++j) {
      d[j] = i + j < S ? slot_degree(a, head, i + j, false) : 0;
      sum += d[j];
    }
    int64_t G;
    int64_t run = block_scan<kWgWaves>(sum, lds, &G) - sum;
    for (int j = 0; j < kWaveWords; ++j) {
      if (i + j < S) a.gq[head + i + j] = run;
      run += d[j];
    }
    if (threadIdx.x == 0) a.st[kTravG] = G;
  }
}

unsigned grid_of(int64_t n, int per) { return static_cast<unsigned>((n + per - 1) / per); }

template <typename K>
Trav<K> make_trav(const SampleCsr& c, int kind, const TraverseBuffers& b) {
  Trav<K> a;
  a.c = c;
  a.kind = kind;
  a.st = b.st;
  a.sections = b.sections;
  a.cap_sections = b.cap_sections;
  a.q = b.q;
  a.gq = b.gq;
  a.cap_q = b.cap_q;
  a.eids = b.eids;
  a.cap_e = b.cap_e;
  a.key = static_cast<K*>(b.key);
  a.visited = b.visited;
  a.rem = b.rem;
  a.keep = b.keep;
  a.tile_cnt = b.tile_cnt;
  a.cap_pos = b.cap_pos;
  return a;
}

template <typename K>
void init_impl(const SampleCsr& c, const IdxPtr& opp, int kind, const int32_t* source,
               int64_t num_sources, const TraverseBuffers& b, hipStream_t s) {
  const Trav<K> a = make_trav<K>(c, kind, b);
  const int64_t N = c.num_rows;
  const int64_t n0 = N > kTraverseStateWords ? N : kTraverseStateWords;
  hipLaunchKernelGGL(k_init<K>, dim3(grid_of(n0, kBlock)), dim3(kBlock), 0, s, a, opp, num_sources);
  if (kind == kTraverseTopo) {
    if (N > 0) {
      const unsigned tiles = grid_of(N, kTile);
      hipLaunchKernelGGL(k_topo_roots<K>, dim3(tiles), dim3(kBlock), 0, s, a);
      hipLaunchKernelGGL(k_scan_tiles<K>, dim3(1), dim3(kWgBlock), 0, s, a);
      hipLaunchKernelGGL(k_fill<K>, dim3(tiles), dim3(kBlock), 0, s, a, true);
    }
  } else if (num_sources > 0) {
    hipLaunchKernelGGL(k_bfs_mark<K>, dim3(grid_of(num_sources, kBlock)), dim3(kBlock), 0, s, a, source,
                       num_sources);
  }
  hipLaunchKernelGGL(k_advance<K>, dim3(1), dim3(kWgBlock), 0, s, a);
}

template <typename K>
void step_impl(const SampleCsr& c, int kind, bool narrow, int64_t num_pos, const TraverseBuffers& b,
               hipStream_t s) {
  const Trav<K> a = make_trav<K>(c, kind, b);
  if (narrow) {
    hipLaunchKernelGGL(k_narrow<K>, dim3(1), dim3(kWgBlock), 0, s, a);
    return;
  }
  const unsigned tiles = grid_of(num_pos, kTile);
  if (tiles > 0) {
    hipLaunchKernelGGL(k_claim<K>, dim3(tiles), dim3(kBlock), 0, s, a, 0);
    if (kind == kTraverseTopo) hipLaunchKernelGGL(k_claim<K>, dim3(tiles), dim3(kBlock), 0, s, a, 1);
    hipLaunchKernelGGL(k_count<K>, dim3(tiles), dim3(kBlock), 0, s, a);
  }
  hipLaunchKernelGGL(k_scan_tiles<K>, dim3(1), dim3(kWgBlock), 0, s, a);
  if (tiles > 0) hipLaunchKernelGGL(k_fill<K>, dim3(tiles), dim3(kBlock), 0, s, a, false);
  hipLaunchKernelGGL(k_advance<K>, dim3(1), dim3(kWgBlock), 0, s, a);
}

}  // namespace

int traverse_tile() { return kTile; }
int traverse_narrow_limit() { return kNarrowLimit; }
int traverse_max_levels() { return kMaxLevels; }

void launch_traverse_init(const SampleCsr& c, const IdxPtr& opp_indptr, int kind,
                          const int32_t* source, int64_t num_sources, const TraverseBuffers& b,
                          hipStream_t s) {
  if (c.indptr.wide) init_impl<int64_t>(c, opp_indptr, kind, source, num_sources, b, s);
  else init_impl<int32_t>(c, opp_indptr, kind, source, num_sources, b, s);
}

void launch_traverse_step(const SampleCsr& c, int kind, bool narrow, int64_t num_pos,
                          const TraverseBuffers& b, hipStream_t s) {
  if (c.indptr.wide) step_impl<int64_t>(c, kind, narrow, num_pos, b, s);
  else step_impl<int32_t>(c, kind, narrow, num_pos, b, s);
}

}  // namespace dglmi
