// Weighted neighbour sampling and row-wise top-k on the device
// (dgl.sampling.sample_neighbors(prob=...), dgl.sampling.select_topk): the reference's
// per-row CPU loops (src/array/cpu/rowwise_sampling.cc, rowwise_topk.cc) restated so that no
// id leaves the GPU.  include/dglmi.h states the contract (DGLMISampleNeighborsWeighted,
// DGLMISelectTopk); this file is one way to meet it.
//
// As in kernels_sample.hip a seed is served by a group of G lanes, G the smallest power of
// two that is at least the fan-out (or k) and at least 4.  The group walks its row in tiles
// of G entries, lane g reading entry tile + g.
//
// k smallest (select_walk): top-k and the unreplaced sample are the same selection, by
// (uint64 key, position).  Lane j of the group holds the j-th smallest entry seen so far.
// A tile's entries are compared with the k-th (one broadcast); the survivors, found by one
// ballot, are inserted one at a time: a broadcast of the survivor, a shift by one lane of
// the held list, and a compare per lane.  The ballot's loop ends when no group of the
// wavefront has a survivor left, so its trip count is wavefront-uniform.
//
// With replacement (k_weighted_replace): three walks of the row.  The first two are
// lane-strided integer reductions (maximum of the weights' bits, sum of the quantised
// weights); the third scans each tile's quantised weights inside the group, and lane t
// finds the entry of its own target in the scanned tile by bisection with log2 G
// variable-lane shuffles.
//
// Every shuffle, ballot and vote runs for all 64 lanes: no thread returns early, the tile
// loops end on a wavefront-wide vote, and a group without work carries sentinels.  No LDS, no
// atomics; the weights are handled as bit patterns and integers, and the one float operation
// is the correctly rounded fp64 division of the unreplaced key.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace dglmi {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kNoPos = 0xffffffffu;  // a row's positions stay below 2^32 - 1
constexpr uint64_t kSign = uint64_t(1) << 63;
constexpr uint64_t kExpMask = uint64_t(0x7ff) << 52;
constexpr uint64_t kMinSampled = uint64_t(1023 - 900) << 52;  // 2^-900 as fp64 bits

__device__ __forceinline__ int64_t w_row_degree(const IdxPtr& indptr, int64_t num_rows, int64_t row,
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

__device__ __forceinline__ Philox4 w_block(uint64_t seed, uint64_t c, int64_t slot) {
  const uint64_t s = static_cast<uint64_t>(slot);
  return philox4x32_10(Philox4{static_cast<uint32_t>(c), static_cast<uint32_t>(c >> 32),
                               static_cast<uint32_t>(s), static_cast<uint32_t>(s >> 32)},
                       static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
}

// r(i, p) of DGLMISampleNeighbors for a 64-bit p
__device__ __forceinline__ uint32_t w_draw32(uint64_t seed, uint64_t ctr, int64_t slot, int64_t p) {
  const Philox4 r = w_block(seed, ctr + (static_cast<uint64_t>(p) >> 2), slot);
  const int k = static_cast<int>(p & 3);
  return k == 0 ? r.x : k == 1 ? r.y : k == 2 ? r.z : r.w;
}

// R_t: words (x, y) for even t, (z, w) for odd t of the block at counter ctr + (t >> 1)
__device__ __forceinline__ uint64_t w_draw64(uint64_t seed, uint64_t ctr, int64_t slot, int t) {
  const Philox4 r = w_block(seed, ctr + static_cast<uint64_t>(t >> 1), slot);
  const uint32_t lo = (t & 1) ? r.z : r.x, hi = (t & 1) ? r.w : r.y;
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

// the fp64 bit pattern of a float's value, from the float's bits: exact, sign included, and
// independent of the denormal mode (a subnormal float is a normal double)
__device__ __forceinline__ uint64_t f32_bits_to_f64_bits(uint32_t b) {
  const uint64_t sign = static_cast<uint64_t>(b >> 31) << 63;
  const uint32_t ex = (b >> 23) & 0xffu, man = b & 0x7fffffu;
  if (ex == 0xffu) return sign | kExpMask | (static_cast<uint64_t>(man) << 29);
  if (ex != 0) return sign | (static_cast<uint64_t>(ex - 127 + 1023) << 52) | (static_cast<uint64_t>(man) << 29);
  if (man == 0) return sign;
  const int n = 31 - __clz(static_cast<int>(man));  // man = 1.xxx * 2^n, value man * 2^-149
  return sign | (static_cast<uint64_t>(n - 149 + 1023) << 52) |
         (static_cast<uint64_t>(man ^ (1u << n)) << (52 - n));
}

struct WeightArg {
  const void* p;
  int64_t n;  // entries; an edge id outside [0, n) has no weight
  int code;   // DGLMI_WEIGHT_*
};

// the weight of parent edge `eid` as fp64 bits when it is eligible for sampling, else 0
__device__ __forceinline__ uint64_t sample_weight_bits(const WeightArg& w, int64_t eid) {
  if (eid < 0 || eid >= w.n) return 0;
  uint64_t b;
  if (w.code == DGLMI_WEIGHT_F32) {
    const uint32_t f = static_cast<const uint32_t*>(w.p)[eid];
    if ((f >> 31) != 0 || (f & 0x7f800000u) == 0x7f800000u || f == 0) return 0;
    b = f32_bits_to_f64_bits(f);
  } else {
    b = static_cast<const uint64_t*>(w.p)[eid];
    if ((b >> 63) != 0 || (b & kExpMask) == kExpMask) return 0;
  }
  return b >= kMinSampled ? b : 0;
}

// the top-k key: an order-preserving uint64 image of the weight, complemented for descending;
// a NaN, or an edge without a weight, takes the largest key in both directions
__device__ __forceinline__ uint64_t topk_key(const WeightArg& w, int64_t eid, int ascending) {
  if (eid < 0 || eid >= w.n) return ~uint64_t(0);
  uint64_t img;
  if (w.code == DGLMI_WEIGHT_I32) {
    img = static_cast<uint64_t>(static_cast<int64_t>(static_cast<const int32_t*>(w.p)[eid])) ^ kSign;
  } else if (w.code == DGLMI_WEIGHT_I64) {
    img = static_cast<const uint64_t*>(w.p)[eid] ^ kSign;
  } else {
    uint64_t b = w.code == DGLMI_WEIGHT_F32
                     ? f32_bits_to_f64_bits(static_cast<const uint32_t*>(w.p)[eid])
                     : static_cast<const uint64_t*>(w.p)[eid];
    if ((b & ~kSign) > kExpMask) return ~uint64_t(0);  // NaN
    if (b == kSign) b = 0;                             // -0.0 counts as +0.0
    img = (b >> 63) != 0 ? ~b : (b | kSign);
  }
  return ascending ? img : ~img;
}

// E(r): -log2((r + 1/2) / 2^32) in 40 fractional bits, by repeated squaring
__device__ __forceinline__ uint64_t exp_key(uint32_t r) {
  const uint64_t y = 2 * static_cast<uint64_t>(r) + 1;
  const int n = 63 - __clzll(static_cast<long long>(y));
  uint64_t m = y << (63 - n);
  uint64_t bits = 0;
#pragma unroll 4
  for (int i = 0; i < 40; ++i) {
    const uint64_t hi = __umul64hi(m, m), lo = m * m;
    const uint64_t one = hi >> 63;  // (m m) >> 63 has reached 2^64
    m = one ? hi : ((hi << 1) | (lo >> 63));
    bits = (bits << 1) | one;
  }
  return (uint64_t(33) << 40) - ((static_cast<uint64_t>(n) << 40) + bits);
}

// floor(w 2^(31 - e)) for eligible fp64 bits `b` (0: not eligible), `emax` the biased exponent
// of the row's largest weight
__device__ __forceinline__ uint64_t quantise(uint64_t b, int emax) {
  if (b == 0) return 0;
  const int sh = 22 + emax - static_cast<int>(b >> 52);
  const uint64_t m = (b & ((uint64_t(1) << 52) - 1)) | (uint64_t(1) << 52);
  return sh >= 53 ? 0 : m >> sh;
}

__device__ __forceinline__ bool entry_less(uint64_t ak, uint32_t ap, uint64_t bk, uint32_t bp) {
  return ak < bk || (ak == bk && ap < bp);
}

// cnt[0] = 0, cnt[i + 1] = the number of picks of seed slot i; G lanes count a row's eligible
// entries
__global__ void __launch_bounds__(kBlock)
k_weighted_count(IdxPtr indptr, IdxPtr data, int64_t num_rows, const int32_t* __restrict__ seeds,
                 int64_t num_seeds, int fanout, int replace, int G, WeightArg w,
                 int64_t* __restrict__ cnt) {
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int g = static_cast<int>(tid & (G - 1));
  const int64_t slot = tid / G;
  const bool live = slot < num_seeds;
  int64_t start = 0;
  const int64_t deg = live ? w_row_degree(indptr, num_rows, seeds[slot], &start) : 0;
  int64_t nz = 0;
  for (int64_t p = g; p < deg; p += G) nz += sample_weight_bits(w, data[start + p]) != 0 ? 1 : 0;
  for (int m = G >> 1; m > 0; m >>= 1) nz += __shfl_xor(nz, m, 64);
  if (tid == 0) cnt[0] = 0;
  if (live && g == 0)
    cnt[slot + 1] = nz == 0 ? 0 : (replace ? fanout : (nz < fanout ? nz : fanout));
}

// The k entries of the row first in (key, position) order, lane j of the group holding the
// j-th.  TOPK: the key is the weight's image and the picks are listed in that order.
// Otherwise: the key is E(r) / w over the eligible entries, and the picks are listed by
// position.
template <int G, bool TOPK>
__global__ void __launch_bounds__(kBlock)
k_select_walk(IdxPtr indptr, const int32_t* __restrict__ indices, IdxPtr data, int64_t num_rows,
              const int32_t* __restrict__ seeds, int64_t num_seeds, int k, WeightArg w, int ascending,
              uint64_t rng_seed, uint64_t rng_ctr, const int64_t* __restrict__ offsets,
              int64_t num_out, int32_t* __restrict__ out_nbr, int64_t* __restrict__ out_eid) {
  const int lane = threadIdx.x & 63;
  const int g = lane & (G - 1);
  const int base = lane & ~(G - 1);
  const int64_t slot = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) / G;
  const bool live = slot < num_seeds;
  int64_t start = 0;
  const int64_t deg = live ? w_row_degree(indptr, num_rows, seeds[slot], &start) : 0;
  const int64_t cnt = live ? offsets[slot + 1] - offsets[slot] : 0;
  // fewer picks than k: every eligible entry is taken and no key is needed
  const bool keyed = TOPK || cnt >= k;

  uint64_t hk = ~uint64_t(0);  // held entry: (key, position), kNoPos for none
  uint32_t hp = kNoPos;
  for (int64_t tb = 0; __any(tb < deg); tb += G) {
    const int64_t p = tb + g;
    uint64_t ck = ~uint64_t(0);
    uint32_t cp = kNoPos;
    if (p < deg) {
      const int64_t eid = data[start + p];
      if (TOPK) {
        ck = topk_key(w, eid, ascending);
        cp = static_cast<uint32_t>(p);
      } else {
        const uint64_t wb = sample_weight_bits(w, eid);
        if (wb != 0) {
          cp = static_cast<uint32_t>(p);
          ck = 0;
          if (keyed) {
            const double e = static_cast<double>(exp_key(w_draw32(rng_seed, rng_ctr, slot, p)));
            ck = static_cast<uint64_t>(__double_as_longlong(e / __longlong_as_double(static_cast<long long>(wb))));
          }
        }
      }
    }
    const uint64_t tk = __shfl(hk, k - 1, G);
    const uint32_t tp = __shfl(hp, k - 1, G);
    bool surv = cp != kNoPos && entry_less(ck, cp, tk, tp);
    for (;;) {
      const uint64_t all = __ballot(surv);
      if (all == 0) break;
      const uint64_t mine = G == 64 ? all : (all >> base) & ((uint64_t(1) << (G & 63)) - 1);
      const int src = mine != 0 ? base + __builtin_ctzll(mine) : lane;
      const uint64_t xk = __shfl(ck, src, 64);
      const uint32_t xp = __shfl(cp, src, 64);
      const uint64_t uk = __shfl_up(hk, 1, G);
      const uint32_t up = __shfl_up(hp, 1, G);
      if (mine != 0) {
        if (entry_less(xk, xp, hk, hp)) {
          const bool shift = g > 0 && entry_less(xk, xp, uk, up);
          hk = shift ? uk : xk;
          hp = shift ? up : xp;
        }
        if (lane == src) surv = false;
      }
    }
  }

  int rank = g;
  if (!TOPK) {  // by position
    rank = 0;
    for (int t = 0; t < k; ++t) rank += __shfl(hp, t, G) < hp ? 1 : 0;
  }
  if (g < k && hp != kNoPos && rank < cnt) {
    const int64_t o = offsets[slot] + rank;
    if (o >= 0 && o < num_out) {
      out_nbr[o] = indices[start + hp];
      out_eid[o] = data[start + hp];
    }
  }
}

template <int G>
__global__ void __launch_bounds__(kBlock)
k_weighted_replace(IdxPtr indptr, const int32_t* __restrict__ indices, IdxPtr data, int64_t num_rows,
                   const int32_t* __restrict__ seeds, int64_t num_seeds, int fanout, WeightArg w,
                   uint64_t rng_seed, uint64_t rng_ctr, const int64_t* __restrict__ offsets,
                   int64_t num_out, int32_t* __restrict__ out_nbr, int64_t* __restrict__ out_eid) {
  constexpr int64_t kNone = INT64_MAX;
  const int g = threadIdx.x & (G - 1);
  const int64_t slot = (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) / G;
  const bool live = slot < num_seeds;
  int64_t start = 0;
  const int64_t deg = live ? w_row_degree(indptr, num_rows, seeds[slot], &start) : 0;

  uint64_t mx = 0;  // walk 1: the largest eligible weight (positive fp64 order by bits)
  for (int64_t p = g; p < deg; p += G) {
    const uint64_t b = sample_weight_bits(w, data[start + p]);
    mx = b > mx ? b : mx;
  }
  for (int m = G >> 1; m > 0; m >>= 1) {
    const uint64_t o = __shfl_xor(mx, m, 64);
    mx = o > mx ? o : mx;
  }
  const int emax = static_cast<int>(mx >> 52);

  uint64_t total = 0;  // walk 2: an integer sum, the same in any order
  for (int64_t p = g; p < deg; p += G) total += quantise(sample_weight_bits(w, data[start + p]), emax);
  for (int m = G >> 1; m > 0; m >>= 1) total += __shfl_xor(total, m, 64);

  const bool mine = g < fanout && total != 0;  // this lane owns draw g
  const uint64_t target = mine ? __umul64hi(w_draw64(rng_seed, rng_ctr, slot, g), total) : 0;

  int64_t pos = kNone;  // walk 3: the lowest position whose running sum exceeds the target
  uint64_t run = 0;
  for (int64_t tb = 0; __any(tb < deg); tb += G) {
    const int64_t p = tb + g;
    uint64_t sc = p < deg ? quantise(sample_weight_bits(w, data[start + p]), emax) : 0;
    for (int d = 1; d < G; d <<= 1) {
      const uint64_t v = __shfl_up(sc, d, G);
      if (g >= d) sc += v;
    }
    const uint64_t tile = __shfl(sc, G - 1, G);
    int lo = 0;  // the number of the tile's lanes 0 .. G - 2 whose running sum is <= target
    for (int step = G >> 1; step > 0; step >>= 1) {
      const uint64_t v = __shfl(sc, lo + step - 1, G);
      if (run + v <= target) lo += step;
    }
    if (mine && pos == kNone && target < run + tile) pos = tb + lo;
    run += tile;
  }

  // rank by counting: ascending position, equal picks by draw
  int rank = 0;
  for (int t = 0; t < fanout; ++t) {
    const int64_t v = __shfl(pos, t, G);
    rank += (v < pos || (v == pos && t < g)) ? 1 : 0;
  }
  if (pos != kNone && rank < fanout) {
    const int64_t o = offsets[slot] + rank;
    if (o >= 0 && o < num_out) {
      out_nbr[o] = indices[start + pos];
      out_eid[o] = data[start + pos];
    }
  }
}

unsigned w_blocks_for(int64_t n) { return static_cast<unsigned>((n + kBlock - 1) / kBlock); }

}  // namespace

void launch_weighted_count(const SampleCsr& c, const int32_t* seeds, int64_t num_seeds, int fanout,
                           int replace, const void* weight, int64_t num_weights, int code,
                           int64_t* cnt, hipStream_t s) {
  const int G = sample_group_width(fanout);
  const int64_t lanes = (num_seeds > 0 ? num_seeds : 1) * G;
  hipLaunchKernelGGL(k_weighted_count, dim3(w_blocks_for(lanes)), dim3(kBlock), 0, s, c.indptr, c.data,
                     c.num_rows, seeds, num_seeds, fanout, replace, G,
                     WeightArg{weight, num_weights, code}, cnt);
}

#define DGLMI_BY_GROUP(G, LAUNCH) \
  switch (G) {                    \
    case 4: LAUNCH(4); break;     \
    case 8: LAUNCH(8); break;     \
    case 16: LAUNCH(16); break;   \
    case 32: LAUNCH(32); break;   \
    default: LAUNCH(64); break;   \
  }

void launch_weighted_pick(const SampleCsr& c, const int32_t* seeds, int64_t num_seeds, int fanout,
                          int replace, const void* weight, int64_t num_weights, int code,
                          uint64_t rng_seed, uint64_t rng_ctr, const int64_t* offsets,
                          int64_t num_out, int32_t* out_nbr, int64_t* out_eid, hipStream_t s) {
  if (num_seeds == 0 || num_out == 0 || fanout == 0) return;
  const int G = sample_group_width(fanout);
  const dim3 grid(w_blocks_for(num_seeds * G)), block(kBlock);
  const WeightArg w{weight, num_weights, code};
  if (replace) {
#define DGLMI_REPLACE(W)                                                                          \
  hipLaunchKernelGGL(k_weighted_replace<W>, grid, block, 0, s, c.indptr, c.indices, c.data,       \
                     c.num_rows, seeds, num_seeds, fanout, w, rng_seed, rng_ctr, offsets, num_out, \
                     out_nbr, out_eid)
    DGLMI_BY_GROUP(G, DGLMI_REPLACE)
#undef DGLMI_REPLACE
  } else {
#define DGLMI_UNREPLACED(W)                                                                        \
  hipLaunchKernelGGL((k_select_walk<W, false>), grid, block, 0, s, c.indptr, c.indices, c.data,    \
                     c.num_rows, seeds, num_seeds, fanout, w, 1, rng_seed, rng_ctr, offsets,       \
                     num_out, out_nbr, out_eid)
    DGLMI_BY_GROUP(G, DGLMI_UNREPLACED)
#undef DGLMI_UNREPLACED
  }
}

void launch_select_topk(const SampleCsr& c, const int32_t* seeds, int64_t num_seeds, int k,
                        int ascending, const void* weight, int64_t num_weights, int code,
                        const int64_t* offsets, int64_t num_out, int32_t* out_nbr, int64_t* out_eid,
                        hipStream_t s) {
  if (num_seeds == 0 || num_out == 0 || k == 0) return;
  const int G = sample_group_width(k);
  const dim3 grid(w_blocks_for(num_seeds * G)), block(kBlock);
  const WeightArg w{weight, num_weights, code};
#define DGLMI_TOPK(W)                                                                            \
  hipLaunchKernelGGL((k_select_walk<W, true>), grid, block, 0, s, c.indptr, c.indices, c.data,   \
                     c.num_rows, seeds, num_seeds, k, w, ascending, uint64_t(0), uint64_t(0),    \
                     offsets, num_out, out_nbr, out_eid)
  DGLMI_BY_GROUP(G, DGLMI_TOPK)
#undef DGLMI_TOPK
}

#undef DGLMI_BY_GROUP

}  // namespace dglmi
