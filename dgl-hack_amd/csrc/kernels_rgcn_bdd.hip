// RelGraphConv with the block-diagonal-decomposition regulariser ("bdd") for many
// relations: aggregate per (destination, relation) segment, then transform.
//
//   out[v, b s_o + j] = sum_r sum_i W[r, b, i, j] a_{v,r}[b s_i + i],
//   a_{v,r} = sum_{e = (u -> v) of relation r} norm_e x[u]
//
// W_r is in * s_o floats (10 KB at 500 -> 500 with 100 bases) and a knowledge graph has
// hundreds of them: they do not fit in LDS (k_rgcn_fused's design), and the blocks
// (5 x 5) are far below an MFMA tile.  So:
//
//  * The walk (k_rgcn_bdd) runs over the CSR whose positions are stably regrouped by
//    (row, relation) (rgcn_bdd_build).  One wave owns kBddChunk consecutive positions;
//    lane l owns columns l, l + 64, .. of the gathered row and of the output row.  A
//    segment's sum a stays in registers; at a relation change or a row end the wave puts
//    a into its private LDS slot and every lane reads the s_i values its output columns
//    need, the matching s_i weights from global memory (consecutive lanes, consecutive j:
//    the weights live in L2 / Infinity Cache) and adds the products to its output
//    accumulators.  TRANSPOSED reads the same blocks as W[r, b, j, .] for the input
//    gradient over the (source, relation) out-CSR.
//  * Rows cut by a chunk boundary: the transform is linear, so a cut segment is
//    transformed in two parts; continuation chunks write carry records that k_rgcn_bdd_fixup
//    folds in chunk order (internal.h's segmented fixup protocol, CarryLayout).  Bias and
//    addend are added where the row is finished.  No floating-point atomics.
//  * The weight gradient (k_rgcn_bdd_wgrad) runs over the relation-major list of the same
//    segments: a workgroup takes kBddWgradChunk segments of one relation, re-aggregates
//    each a with the forward's gathers, stages a and grad_out[v] in LDS and keeps its
//    share of dW[r] (in * s_o elements over 256 lanes) in registers; one partial per
//    chunk, summed in chunk order by k_rgcn_bdd_wreduce (relations without edges: zeros).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "internal.h"

namespace dglmi {
namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kWavesPerBlock = kBlock / kWave;

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// NV: columns per lane (gathered and output rows up to 64 NV wide).  SI / SO: the
// weight's block shape at compile time, 0 = read from the arguments.
template <int NV, int SI, int SO, bool TRANSPOSED>
__global__ void __launch_bounds__(kBlock) k_rgcn_bdd(BddArgs a) {
  constexpr int U = NV >= 8 ? 2 : 4;  // source rows in flight per lane
  extern __shared__ float lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int64_t chunk = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  const int64_t K = kBddChunk;
  const int64_t nchunks = a.nnz > 0 ? (a.nnz + K - 1) / K : 1;
  if (chunk >= nchunks) return;
  const int si = SI ? SI : a.si, so = SO ? SO : a.so;
  const int64_t wi = a.wi, wo = a.wo;
  const int64_t wrel = (int64_t)a.nb * si * so;
  float* slot = lds + wave * wi;
  // output column c = lane + 64 k: which values of the slot and which weights it reads
  const int cnt = TRANSPOSED ? so : si;    // products per output column
  const int wstep = TRANSPOSED ? 1 : so;   // weight stride between them
  const int sout = TRANSPOSED ? si : so;   // output columns per block
  int aoff[NV], woff[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c = lane + kWave * k;
    const int b = c / sout, t = c - b * sout;
    aoff[k] = b * cnt;
    woff[k] = b * si * so + (TRANSPOSED ? t * so : t);
  }
  auto finish = [&](int64_t r, float* o, const float* acc, bool done) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int64_t c = lane + kWave * k;
      if (c < wo) {
        float v = acc[k];
        if (done && a.bias) v = v + a.bias[c];
        if (done && a.addend) v = v + a.addend[r * wo + c];
        o[c] = v;
      }
    }
  };
  const int64_t p0 = chunk * K;
  if (p0 < a.nnz) {
    const int64_t p1 = p0 + K < a.nnz ? p0 + K : a.nnz;
    const int n = static_cast<int>(p1 - p0);
    seg_reset(a.seg_cnt, chunk, lane);
    // the chunk's positions, one per lane
    const int64_t pl = p0 + (lane < n ? lane : n - 1);
    const int my_row = a.rows[pl], my_col = a.cols[pl], my_rel = a.rel[pl];
    const float my_norm = a.norm ? a.norm[pl] : 1.0f;
    int64_t cur = __shfl(my_row, 0);
    int cur_rel = __shfl(my_rel, 0);
    bool cont = p0 > 0 && a.rows[p0 - 1] == cur;
    bool dirty = false;
    float agg[NV], acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) agg[k] = acc[k] = 0.0f;
    auto transform = [&]() {
      if (!dirty) return;
      dirty = false;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int64_t c = lane + kWave * k;
        if (c < wi) slot[c] = agg[k];
        agg[k] = 0.0f;
      }
      wave_lds_sync();
      const float* w = a.W + cur_rel * wrel;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        if (lane + kWave * k < wo) {
          const float* wk = w + woff[k];
          const float* ak = slot + aoff[k];
          float s = acc[k];
          if constexpr (SI != 0) {
#pragma unroll
            for (int i = 0; i < cnt; ++i) s += ak[i] * wk[i * wstep];
          } else {
            for (int i = 0; i < cnt; ++i) s += ak[i] * wk[i * wstep];
          }
          acc[k] = s;
        }
      }
      wave_lds_sync();  // the slot is read before the next segment overwrites it
    };
    auto flush = [&]() {
      transform();
      const bool done = !cont && a.indptr[cur + 1] <= p1;
      finish(cur, cont ? a.carry + chunk * wo : a.out + cur * wo, acc, done);
#pragma unroll
      for (int k = 0; k < NV; ++k) acc[k] = 0.0f;
    };
    for (int t = 0; t < n; t += U) {
      float val[U][NV];
      int rr[U], tt[U];
      float nn[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = t + u < n ? t + u : n - 1;
        rr[u] = __shfl(my_row, q);
        tt[u] = __shfl(my_rel, q);
        nn[u] = __shfl(my_norm, q);
        const float* xr = a.x + (int64_t)__shfl(my_col, q) * wi;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          const int64_t c = lane + kWave * k;
          val[u][k] = c < wi ? xr[c] : 0.0f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u >= n) break;
        if (rr[u] != cur) {
          flush();
          cur = rr[u];
          cur_rel = tt[u];
          cont = false;
        } else if (tt[u] != cur_rel) {
          transform();
          cur_rel = tt[u];
        }
#pragma unroll
        for (int k = 0; k < NV; ++k) agg[k] += nn[u] * val[u][k];
        dirty = true;
      }
    }
    flush();
  }
  float zero[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) zero[k] = 0.0f;
  fill_empty_rows(a.indptr, a.num_rows, chunk, nchunks, kWave, lane,
                  [&](int64_t r) { finish(r, a.out + r * wo, zero, true); });
}

// folds a cut row's carries into its head in chunk order, then bias and addend
__global__ void __launch_bounds__(kBlock) k_rgcn_bdd_fixup(BddArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const FixupRole w =
      fixup_role(a, a.indptr, (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave);
  if (!w.work) return;
  const int64_t wo = a.wo;
  seg_fold(w, a.seg_cnt, kWave, lane, [&](bool head, int64_t c0, int64_t c1, int64_t step) {
    float* dst = head ? a.out + w.r * wo : a.carry + c0 * wo;
    for (int64_t k = lane; k < wo; k += kWave) {
      float acc = dst[k];
      for (int64_t c = head ? c0 : c0 + 1; c <= c1; c += step) acc += a.carry[c * wo + k];
      if (head && a.bias) acc = acc + a.bias[k];
      if (head && a.addend) acc = acc + a.addend[w.r * wo + k];
      dst[k] = acc;
    }
  });
}

// ---- weight gradient ----------------------------------------------------------
// ME: elements of dW[r] per lane (in * s_o <= 256 ME)
template <int ME>
__global__ void __launch_bounds__(kBlock) k_rgcn_bdd_wgrad(BddWgradArgs a) {
  constexpr int U = 4;
  constexpr int NQ = 4;  // gathered columns per lane (rows up to 1024 wide)
  extern __shared__ float lds[];
  const int t = threadIdx.x;
  const int64_t c = blockIdx.x;
  if (c >= a.chunk_ptr[a.R]) return;
  // the relation of chunk c: the last r with chunk_ptr[r] <= c (empty relations passed over)
  int64_t lo = 0, hi = a.R - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (a.chunk_ptr[mid] <= c) lo = mid;
    else hi = mid - 1;
  }
  const int64_t r = lo;
  const int64_t s0 = a.rel_seg[r] + (c - a.chunk_ptr[r]) * kBddWgradChunk;
  const int64_t s1 = s0 + kBddWgradChunk < a.rel_seg[r + 1] ? s0 + kBddWgradChunk : a.rel_seg[r + 1];
  const int64_t fi = a.fi, fo = a.fo;
  const int si = a.si, so = a.so;
  const int64_t nelem = fi * so;
  float* a_lds = lds;
  float* g_lds = lds + fi;
  // element e = t + 256 m of dW[r] = (b, i, j): a at b s_i + i = e / s_o, g at b s_o + j
  uint32_t off[ME];
  float acc[ME];
#pragma unroll
  for (int m = 0; m < ME; ++m) {
    const int64_t e = t + kBlock * m;
    const int64_t ea = e < nelem ? e : 0;
    const uint32_t ao = static_cast<uint32_t>(ea / so);
    const uint32_t go = static_cast<uint32_t>((ea / (si * so)) * so + ea % so);
    off[m] = ao | (go << 16);
    acc[m] = 0.0f;
  }
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t pos = a.seg_pos[s];
    const int64_t len = a.seg_first[s + 1] - a.seg_first[s];
    const int64_t v = a.seg_row[s];
    float av[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) av[q] = 0.0f;
    for (int64_t base = 0; base < len; base += U) {
      float val[U][NQ], nn[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t p = pos + (base + u < len ? base + u : len - 1);
        nn[u] = a.norm ? a.norm[p] : 1.0f;
        const float* xr = a.x + (int64_t)a.cols[p] * fi;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int64_t col = t + kBlock * q;
          val[u][q] = col < fi ? xr[col] : 0.0f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (base + u >= len) break;
#pragma unroll
        for (int q = 0; q < NQ; ++q) av[q] += nn[u] * val[u][q];
      }
    }
    float gv[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int64_t col = t + kBlock * q;
      gv[q] = col < fo ? a.g[v * fo + col] : 0.0f;
    }
    __syncthreads();  // the previous segment's products are done with the staging
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int64_t col = t + kBlock * q;
      if (col < fi) a_lds[col] = av[q];
      if (col < fo) g_lds[col] = gv[q];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < ME; ++m) acc[m] += a_lds[off[m] & 0xffffu] * g_lds[off[m] >> 16];
  }
  float* part = a.part + c * nelem;
#pragma unroll
  for (int m = 0; m < ME; ++m) {
    const int64_t e = t + kBlock * m;
    if (e < nelem) part[e] = acc[m];
  }
}

// dW[r] = its chunks' partials summed in chunk order (none: zeros)
__global__ void __launch_bounds__(kBlock) k_rgcn_bdd_wreduce(BddWgradArgs a, int64_t eblocks) {
  const int64_t r = blockIdx.x / eblocks;
  const int64_t e = (blockIdx.x - r * eblocks) * kBlock + threadIdx.x;
  const int64_t nelem = a.fi * a.so;
  if (e >= nelem) return;
  float s = 0.0f;
  for (int64_t c = a.chunk_ptr[r]; c < a.chunk_ptr[r + 1]; ++c) s += a.part[c * nelem + e];
  a.gw[r * nelem + e] = s;
}

// ---- per-graph state ------------------------------------------------------------
unsigned grid_of(int64_t n) {
  int64_t b = (n + kBlock - 1) / kBlock;
  return static_cast<unsigned>(std::min<int64_t>(std::max<int64_t>(b, 1), 16384));
}
int bits_for(int64_t n) {
  int b = 1;
  while ((int64_t(1) << b) < n && b < 31) ++b;
  return b;
}
#define BDD_FOR(i, n)                                                              \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n);        \
       i += (int64_t)gridDim.x * blockDim.x)

__global__ void k_bdd_rel_keys(const int32_t* __restrict__ eids, const int32_t* __restrict__ etypes,
                               int64_t n, int32_t* __restrict__ key, int32_t* __restrict__ val) {
  BDD_FOR(p, n) {
    key[p] = etypes[eids[p]];
    val[p] = static_cast<int32_t>(p);
  }
}
// row keys of the relation-major order, and its index as the second sort's payload
__global__ void k_bdd_row_keys(const int32_t* __restrict__ perm_a, const int32_t* __restrict__ rows,
                               int64_t n, int32_t* __restrict__ key, int32_t* __restrict__ val) {
  BDD_FOR(q, n) {
    key[q] = rows[perm_a[q]];
    val[q] = static_cast<int32_t>(q);
  }
}
// position b of the (row, relation) order holds relation-major index bq[b]
__global__ void k_bdd_fill(const int32_t* __restrict__ bq, const int32_t* __restrict__ perm_a,
                           const int32_t* __restrict__ indices, const int32_t* __restrict__ eids,
                           const int32_t* __restrict__ etypes, int64_t n, int32_t* __restrict__ cols,
                           int32_t* __restrict__ rel, int32_t* __restrict__ eid,
                           int32_t* __restrict__ inv) {
  BDD_FOR(b, n) {
    const int32_t q = bq[b];
    const int32_t p = perm_a[q];
    const int32_t e = eids[p];
    cols[b] = indices[p];
    eid[b] = e;
    rel[b] = etypes[e];
    if (inv) inv[q] = static_cast<int32_t>(b);
  }
}
__global__ void k_bdd_seg_flags(const int32_t* __restrict__ rel_a, const int32_t* __restrict__ row_a,
                                int64_t n, int32_t* __restrict__ flag) {
  BDD_FOR(q, n + 1)
    flag[q] = q < n && (q == 0 || rel_a[q] != rel_a[q - 1] || row_a[q] != row_a[q - 1]);
}
// the segment list (relation-major, destination order inside a relation) and each
// relation's first segment: index q opens every relation in (rel_a[q-1], rel_a[q]]
__global__ void k_bdd_seg_write(const int32_t* __restrict__ rel_a, const int32_t* __restrict__ row_a,
                                const int32_t* __restrict__ flag, const int32_t* __restrict__ scan,
                                const int32_t* __restrict__ inv, int64_t n, int64_t R,
                                int32_t* __restrict__ seg_pos, int32_t* __restrict__ seg_row,
                                int32_t* __restrict__ seg_first, int32_t* __restrict__ rel_seg) {
  BDD_FOR(q, n + 1) {
    const int32_t s = scan[q];
    if (q == n) {
      seg_first[s] = static_cast<int32_t>(n);
    } else if (flag[q]) {
      seg_pos[s] = inv[q];
      seg_row[s] = row_a[q];
      seg_first[s] = static_cast<int32_t>(q);
    }
    const int64_t lo = q == 0 ? 0 : (int64_t)rel_a[q - 1] + 1;
    const int64_t hi = q == n ? R : (int64_t)rel_a[q];
    for (int64_t r = lo; r <= hi; ++r) rel_seg[r] = s;
  }
}
__global__ void k_bdd_chunk_counts(const int32_t* __restrict__ rel_seg, int64_t R,
                                   int32_t* __restrict__ cnt) {
  BDD_FOR(r, R + 1)
    cnt[r] = r < R ? static_cast<int32_t>((rel_seg[r + 1] - rel_seg[r] + kBddWgradChunk - 1) /
                                          kBddWgradChunk)
                   : 0;
}
__global__ void k_bdd_norm(const float* __restrict__ norm, const int32_t* __restrict__ eid, int64_t n,
                           float* __restrict__ out) {
  BDD_FOR(p, n) out[p] = norm[eid[p]];
}

struct Temp {
  void* p = nullptr;
  hipStream_t s;
  hipError_t err;
  Temp(size_t bytes, hipStream_t stream) : s(stream) {
    err = hipMallocAsync(&p, std::max<size_t>(bytes, 256), s);
  }
  ~Temp() {
    if (p) (void)hipFreeAsync(p, s);
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};
#define BDD_TRY(e)                      \
  do {                                  \
    const hipError_t err_ = (e);        \
    if (err_ != hipSuccess) return err_; \
  } while (0)

hipError_t sort_pairs(const int32_t* kin, int32_t* kout, const int32_t* vin, int32_t* vout,
                      int64_t n, int bits, hipStream_t s) {
  size_t bytes = 0;
  BDD_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, kin, kout, vin, vout,
                                             static_cast<int>(n), 0, bits, s));
  Temp tmp(bytes, s);
  BDD_TRY(tmp.err);
  return hipcub::DeviceRadixSort::SortPairs(tmp.p, bytes, kin, kout, vin, vout, static_cast<int>(n),
                                            0, bits, s);
}
hipError_t exclusive_sum(const int32_t* in, int32_t* out, int64_t n, hipStream_t s) {
  size_t bytes = 0;
  BDD_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, static_cast<int>(n), s));
  Temp tmp(bytes, s);
  BDD_TRY(tmp.err);
  return hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, in, out, static_cast<int>(n), s);
}

}  // namespace

bool rgcn_bdd_ok(int64_t in, int64_t out, int64_t bases) {
  if (bases < 1 || in < 1 || out < 1 || in % bases || out % bases) return false;
  return in <= kBddMaxWidth && out <= kBddMaxWidth && in * (out / bases) <= kBddMaxWgradElems;
}

hipError_t rgcn_bdd_build(const BddBuild& b, hipStream_t s) {
  const int64_t n = b.nnz;
  if (n == 0) return hipSuccess;
  const unsigned grid = grid_of(n + 1);
  Temp key0(n * 4, s), val0(n * 4, s), rel_a(n * 4, s), perm_a(n * 4, s), row_a(n * 4, s), bq(n * 4, s);
  for (const Temp* t : {&key0, &val0, &rel_a, &perm_a, &row_a, &bq}) BDD_TRY(t->err);
  // stable sort by relation of positions already in row order: (relation, row) order
  hipLaunchKernelGGL(k_bdd_rel_keys, dim3(grid), dim3(kBlock), 0, s, b.eids, b.etypes, n,
                     key0.as<int32_t>(), val0.as<int32_t>());
  BDD_TRY(sort_pairs(key0.as<int32_t>(), rel_a.as<int32_t>(), val0.as<int32_t>(),
                     perm_a.as<int32_t>(), n, bits_for(b.num_rels), s));
  // then stably by row: (row, relation) order, original order inside a segment
  hipLaunchKernelGGL(k_bdd_row_keys, dim3(grid), dim3(kBlock), 0, s, perm_a.as<int32_t>(), b.rows, n,
                     key0.as<int32_t>(), val0.as<int32_t>());
  BDD_TRY(sort_pairs(key0.as<int32_t>(), row_a.as<int32_t>(), val0.as<int32_t>(), bq.as<int32_t>(), n,
                     bits_for(b.num_rows), s));
  // row_a now holds the sorted row keys (= the CSR's rows); the relation-major rows again:
  Temp inv(b.seg_pos ? n * 4 : 0, s);
  BDD_TRY(inv.err);
  hipLaunchKernelGGL(k_bdd_fill, dim3(grid), dim3(kBlock), 0, s, bq.as<int32_t>(), perm_a.as<int32_t>(),
                     b.indices, b.eids, b.etypes, n, b.cols, b.rel, b.eid,
                     b.seg_pos ? inv.as<int32_t>() : nullptr);
  if (b.seg_pos != nullptr) {
    hipLaunchKernelGGL(k_bdd_row_keys, dim3(grid), dim3(kBlock), 0, s, perm_a.as<int32_t>(), b.rows, n,
                       row_a.as<int32_t>(), val0.as<int32_t>());
    Temp flag((n + 1) * 4, s), scan((n + 1) * 4, s), cnt((b.num_rels + 1) * 4, s);
    for (const Temp* t : {&flag, &scan, &cnt}) BDD_TRY(t->err);
    hipLaunchKernelGGL(k_bdd_seg_flags, dim3(grid), dim3(kBlock), 0, s, rel_a.as<int32_t>(),
                       row_a.as<int32_t>(), n, flag.as<int32_t>());
    BDD_TRY(exclusive_sum(flag.as<int32_t>(), scan.as<int32_t>(), n + 1, s));
    hipLaunchKernelGGL(k_bdd_seg_write, dim3(grid), dim3(kBlock), 0, s, rel_a.as<int32_t>(),
                       row_a.as<int32_t>(), flag.as<int32_t>(), scan.as<int32_t>(), inv.as<int32_t>(),
                       n, b.num_rels, b.seg_pos, b.seg_row, b.seg_first, b.rel_seg);
    hipLaunchKernelGGL(k_bdd_chunk_counts, dim3(grid_of(b.num_rels + 1)), dim3(kBlock), 0, s,
                       b.rel_seg, b.num_rels, cnt.as<int32_t>());
    BDD_TRY(exclusive_sum(cnt.as<int32_t>(), b.chunk_ptr, b.num_rels + 1, s));
  }
  return hipGetLastError();
}

void launch_rgcn_bdd_norm(const float* norm, const int32_t* eid, int64_t n, float* out, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_bdd_norm, dim3(grid_of(n)), dim3(kBlock), 0, s, norm, eid, n, out);
}

int64_t rgcn_bdd_chunks(int64_t nnz) { return nnz > 0 ? (nnz + kBddChunk - 1) / kBddChunk : 1; }

namespace {
template <int NV, bool T>
void launch_walk_nv(const BddArgs& a, unsigned blocks, size_t lds, hipStream_t s) {
#define BDD_SQUARE(S)                                                                        \
  if (a.si == S && a.so == S) {                                                              \
    hipLaunchKernelGGL((k_rgcn_bdd<NV, S, S, T>), dim3(blocks), dim3(kBlock), lds, s, a);    \
    return;                                                                                  \
  }
  BDD_SQUARE(4)
  BDD_SQUARE(5)
  if constexpr (NV < 16) {  // at 16 columns per lane the unrolled 8 / 16 products spill
    BDD_SQUARE(8)
    BDD_SQUARE(16)
  }
#undef BDD_SQUARE
  hipLaunchKernelGGL((k_rgcn_bdd<NV, 0, 0, T>), dim3(blocks), dim3(kBlock), lds, s, a);
}
template <bool T>
void launch_walk(const BddArgs& a, hipStream_t s) {
  const int64_t w = std::max(a.wi, a.wo);
  const unsigned blocks =
      static_cast<unsigned>((rgcn_bdd_chunks(a.nnz) + kWavesPerBlock - 1) / kWavesPerBlock);
  const size_t lds = static_cast<size_t>(kWavesPerBlock * a.wi) * sizeof(float);
  if (w <= 64) launch_walk_nv<1, T>(a, blocks, lds, s);
  else if (w <= 128) launch_walk_nv<2, T>(a, blocks, lds, s);
  else if (w <= 256) launch_walk_nv<4, T>(a, blocks, lds, s);
  else if (w <= 512) launch_walk_nv<8, T>(a, blocks, lds, s);
  else launch_walk_nv<16, T>(a, blocks, lds, s);
  if (a.nnz > kBddChunk)
    hipLaunchKernelGGL(k_rgcn_bdd_fixup, dim3(blocks), dim3(kBlock), 0, s, a);
}
}  // namespace

void launch_rgcn_bdd(bool transposed, const BddArgs& a, hipStream_t s) {
  if (a.num_rows == 0) return;
  if (transposed) launch_walk<true>(a, s);
  else launch_walk<false>(a, s);
}

void launch_rgcn_bdd_wgrad(const BddWgradArgs& a, hipStream_t s) {
  const int64_t nelem = a.fi * a.so;
  if (a.num_chunks > 0) {
    const size_t lds = static_cast<size_t>(a.fi + a.fo) * sizeof(float);
    const unsigned blocks = static_cast<unsigned>(a.num_chunks);
    const int64_t me = (nelem + kBlock - 1) / kBlock;
#define BDD_ME(M)                                                                          \
  if (me <= M) {                                                                           \
    hipLaunchKernelGGL((k_rgcn_bdd_wgrad<M>), dim3(blocks), dim3(kBlock), lds, s, a);      \
  } else
    BDD_ME(1) BDD_ME(2) BDD_ME(4) BDD_ME(8) BDD_ME(16) BDD_ME(32) BDD_ME(64) {}
#undef BDD_ME
  }
  const int64_t eblocks = (nelem + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_rgcn_bdd_wreduce, dim3(static_cast<unsigned>(a.R * eblocks)), dim3(kBlock), 0,
                     s, a, eblocks);
}

}  // namespace dglmi
