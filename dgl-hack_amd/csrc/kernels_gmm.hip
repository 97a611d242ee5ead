// GMMConv (MoNet): Gaussian-mixture aggregation, aggregate first and project once.
//
//   A[v, k, :] = scale[v] sum_{e = (u -> v)} w_k(e) x[u, :]
//   w_k(e)     = exp(-1/2 g_k(e)),  g_k(e) = sum_d (pseudo[e, d] - mu[k, d])^2 inv_sigma[k, d]^2
//
// The reference projects every source row to K * out floats and gathers that per edge;
// sum and mean are linear, so here an edge gathers its `in` floats once and the projection
// is one dense GEMM on A (a library GEMM through torch).  Matrix instructions do not fit
// the walk itself: every edge has its own K scalars, the products are rank-1 updates of
// K x width accumulators with K <= 32 scalars that differ per edge, and the walk is bound
// by its gathers; the matrix work is the GEMM after it.
//
//  * k_gmm_aggregate: one wave owns kGmmChunk consecutive positions of a CSR (the in-CSR
//    for the forward, the out-CSR with x = grad_out for the input gradient).  Phase 1, one
//    position per lane: the lane reads its position's row, column and edge id, the `dim`
//    pseudo-coordinates of that EDGE ID and computes the K tile's weights, each once, into
//    the wave's LDS slot (slot[k * 64 + position]: conflict-free writes); mu and
//    inv_sigma^2 are staged in LDS once per workgroup.  Phase 2, positions in order: lane l
//    owns columns l, l + 64, .. (NV per lane) of the gathered row, keeps KT x NV
//    accumulators in registers, reads a position's KT weights as LDS broadcasts and has U
//    source rows in flight.  The (E, K) weight tensor is never stored.
//  * Register budget: KT * NV <= kGmmAccBudget = 32 accumulators per lane, chosen from the
//    compiler's resource report for gfx950.  At 64 the (NV, KT) = (2, 32), (4, 16) and
//    (8, 8) instances take 100 to 108 VGPRs, spill 336 bytes per lane to scratch and leave
//    4 waves per SIMD; at 32 every instance is free of scratch at 74 VGPRs or fewer and 6
//    to 8 waves per SIMD stay resident to hide the gathers' latency, which is what bounds
//    the walk.  K = 25 at width 64 is one tile, at width 128 two.  When K exceeds the tile
//    (32 / NV), gridDim.y walks the K tiles: a tile computes only its own weights and
//    gathers the rows again (from L2).  k_gmm_edge_grad also holds a dot product per
//    kernel and the butterfly's temporaries: its tile is 8 (NV <= 2) or 4 kernels (107 to
//    145 VGPRs, 3 to 4 waves per SIMD; 32 kernels took 235 VGPRs, one wave per SIMD), and
//    it walks the tiles inside the wave.
//  * Rows cut by a chunk boundary: internal.h's segmented fixup protocol (seg_reset,
//    fixup_role, seg_fold, CarryLayout) with records of K * width floats; k_gmm_fixup folds
//    them in chunk order.  The row scale (1 / in-degree for "mean") is applied where a
//    row is finished; rows without positions are written as zeros.
//  * k_gmm_edge_grad (in-CSR): a wave takes a contiguous range of chunks.  Per chunk and
//    K tile it keeps dA[v, k, :] of the current row in registers (KT x NV), gathers x[u]
//    per position and forms dw_k = <x[u], dA[v, k]> by a transposing butterfly over the
//    wave (KT values: KT + 6 - log2 KT shuffles, not 6 KT), stored in the LDS slot.  Then
//    one position per lane: w_k is recomputed, dg_k = dw_k w_k, dpseudo[eid] is written
//    (every edge id once).  Then lane j owns the (k, d) pairs j, j + 64, ..: it adds the
//    chunk's terms of dmu and dinv_sigma in position order from LDS.  One partial record
//    per wave (gmm_records(nnz) of them, at most kGmmMaxRecords, a function of nnz alone);
//    k_gmm_param_reduce adds the records in record order.
//  * No floating-point atomics; every sum has one fixed order: bit-reproducible.
//  * exp: HIP's expf (OCML exp_f32, documented maximum error 1 ulp in the HIP math API
//    reference), through gmm_weight in all three places, with g's operations in one order,
//    so forward and backward see the same w.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"

namespace dglmi {
namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kPad = kWave + 1;  // edge gradient: slot stride (lanes of different k, other banks)

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// w_k of one edge: ps its pseudo-coordinates, mu / s2 row k of mu and inv_sigma^2
__device__ __forceinline__ float gmm_weight(const float (&ps)[kGmmMaxDim], const float* mu,
                                            const float* s2, int dim) {
  float g = 0.0f;
#pragma unroll
  for (int d = 0; d < kGmmMaxDim; ++d) {
    if (d < dim) {
      const float t = ps[d] - mu[d];
      g += t * t * s2[d];
    }
  }
  return expf(-0.5f * g);
}

__device__ __forceinline__ void load_pseudo(const GmmArgs& a, int64_t eid, float (&ps)[kGmmMaxDim]) {
#pragma unroll
  for (int d = 0; d < kGmmMaxDim; ++d) ps[d] = d < a.dim ? a.pseudo[eid * a.dim + d] : 0.0f;
}

template <int NV, int KT>
__global__ void __launch_bounds__(kBlock) k_gmm_aggregate(GmmArgs a) {
  constexpr int U = NV >= 4 ? 2 : 4;  // source rows in flight per lane
  extern __shared__ float lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int K = a.K, dim = a.dim, KD = K * dim;
  for (int i = threadIdx.x; i < KD; i += kBlock) {
    const float sg = a.inv_sigma[i];
    lds[i] = a.mu[i];
    lds[KD + i] = sg * sg;
  }
  __syncthreads();
  const int64_t chunk = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  const int64_t nchunks = gmm_chunks(a.nnz);
  if (chunk >= nchunks) return;
  const int k0 = blockIdx.y * KT;
  const int kn = K - k0 < KT ? K - k0 : KT;
  float* slot = lds + 2 * KD + wave * (KT * kWave);
  const int64_t W = a.width, rec = (int64_t)K * W;
  auto store = [&](float* o, const float (&acc)[KT][NV], float scale) {
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      if (k < kn) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const int64_t c = lane + kWave * v;
          if (c < W) o[(k0 + k) * W + c] = acc[k][v] * scale;
        }
      }
    }
  };
  float acc[KT][NV];
#pragma unroll
  for (int k = 0; k < KT; ++k)
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[k][v] = 0.0f;
  const int64_t p0 = chunk * kGmmChunk;
  if (p0 < a.nnz) {
    const int64_t p1 = p0 + kGmmChunk < a.nnz ? p0 + kGmmChunk : a.nnz;
    const int n = static_cast<int>(p1 - p0);
    if (blockIdx.y == 0) seg_reset(a.seg_cnt, chunk, lane);
    // phase 1: the chunk's positions, one per lane, and their weights
    const int64_t pl = p0 + (lane < n ? lane : n - 1);
    const int my_row = a.rows[pl], my_col = a.cols[pl];
    float ps[kGmmMaxDim];
    load_pseudo(a, a.eids[pl], ps);
#pragma nounroll
    for (int k = 0; k < KT; ++k)
      slot[k * kWave + lane] =
          k < kn ? gmm_weight(ps, lds + (k0 + k) * dim, lds + KD + (k0 + k) * dim, dim) : 0.0f;
    wave_lds_sync();
    // phase 2: positions in order
    int64_t cur = __shfl(my_row, 0);
    bool cont = p0 > 0 && a.rows[p0 - 1] == cur;
    auto flush = [&]() {
      const bool done = !cont && a.indptr[cur + 1] <= p1;
      store(cont ? a.carry + chunk * rec : a.out + cur * rec, acc,
            done && a.row_scale ? a.row_scale[cur] : 1.0f);
#pragma unroll
      for (int k = 0; k < KT; ++k)
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[k][v] = 0.0f;
    };
    for (int t = 0; t < n; t += U) {
      float val[U][NV];
      int rr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = t + u < n ? t + u : n - 1;
        rr[u] = __shfl(my_row, q);
        const float* xr = a.x + (int64_t)__shfl(my_col, q) * W;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const int64_t c = lane + kWave * v;
          val[u][v] = c < W ? xr[c] : 0.0f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u >= n) break;
        if (rr[u] != cur) {
          flush();
          cur = rr[u];
          cont = false;
        }
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          const float w = slot[k * kWave + t + u];
#pragma unroll
          for (int v = 0; v < NV; ++v) acc[k][v] += w * val[u][v];
        }
      }
    }
    flush();
  }
  // acc is all zeros here
  fill_empty_rows(a.indptr, a.num_rows, chunk, nchunks, kWave, lane,
                  [&](int64_t r) { store(a.out + r * rec, acc, 1.0f); });
}

// folds a cut row's carries into its head in chunk order, then the row scale
__global__ void __launch_bounds__(kBlock) k_gmm_fixup(GmmArgs a) {
  fixup_float_records(a, a.indptr, (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave,
                      (int64_t)a.K * a.width, threadIdx.x & (kWave - 1));
}

// v[N] per lane -> the wave's sum of v[lane >> (6 - log2 N)] in every lane (a butterfly
// that halves the values a lane keeps at each of its first log2 N steps; fixed order)
template <int N>
__device__ __forceinline__ float wave_sum_transposed(float (&v)[N], int lane) {
  int off = kWave / 2;
#pragma unroll
  for (int n = N; n > 1; n >>= 1, off >>= 1) {
    const bool hi = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < n / 2; ++i) {
      const float send = hi ? v[i] : v[i + n / 2];
      const float keep = hi ? v[i + n / 2] : v[i];
      v[i] = keep + __shfl_xor(send, off);
    }
  }
  float r = v[0];
  for (; off >= 1; off >>= 1) r += __shfl_xor(r, off);
  return r;
}
constexpr int log2_of(int n) { return n <= 1 ? 0 : 1 + log2_of(n / 2); }

template <int NV, int KT>
__global__ void __launch_bounds__(kBlock) k_gmm_edge_grad(GmmArgs a, int64_t chunks_per_rec,
                                                          int64_t num_recs) {
  constexpr int U = NV >= 4 ? 2 : 4;
  constexpr int MP = kGmmMaxK * kGmmMaxDim / kWave;  // (k, d) pairs per lane
  constexpr int SH = 6 - log2_of(KT);                // lanes per value after the butterfly
  extern __shared__ float lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int K = a.K, dim = a.dim, KD = K * dim;
  float* mu = lds;
  float* sg = lds + KD;
  float* s2 = lds + 2 * KD;
  for (int i = threadIdx.x; i < KD; i += kBlock) {
    const float s = a.inv_sigma[i];
    mu[i] = a.mu[i];
    sg[i] = s;
    s2[i] = s * s;
  }
  __syncthreads();
  const int64_t rec = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (rec >= num_recs) return;
  float* slot = lds + 3 * KD + wave * ((K + dim) * kPad);  // dw, then dg: [k][position]
  float* pslot = slot + K * kPad;                          // pseudo: [d][position]
  const int64_t W = a.width, arow = (int64_t)K * W;
  const int64_t nchunks = gmm_chunks(a.nnz);
  float acc_mu[MP], acc_sg[MP];
#pragma unroll
  for (int m = 0; m < MP; ++m) acc_mu[m] = acc_sg[m] = 0.0f;
  const int64_t c_end = (rec + 1) * chunks_per_rec < nchunks ? (rec + 1) * chunks_per_rec : nchunks;
  for (int64_t chunk = rec * chunks_per_rec; chunk < c_end; ++chunk) {
    const int64_t p0 = chunk * kGmmChunk;
    const int64_t p1 = p0 + kGmmChunk < a.nnz ? p0 + kGmmChunk : a.nnz;
    const int n = static_cast<int>(p1 - p0);
    const int64_t pl = p0 + (lane < n ? lane : n - 1);
    const int my_row = a.rows[pl], my_col = a.cols[pl];
    const int64_t my_eid = a.eids[pl];
    float ps[kGmmMaxDim];
    load_pseudo(a, my_eid, ps);
    // dw_k = <x[u], dA[v, k]> of every position, one K tile after the other
    for (int k0 = 0; k0 < K; k0 += KT) {
      const int kn = K - k0 < KT ? K - k0 : KT;
      int64_t cur = -1;
      float da[KT][NV];
      for (int t = 0; t < n; t += U) {
        float val[U][NV];
        int rr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int q = t + u < n ? t + u : n - 1;
          rr[u] = __shfl(my_row, q);
          const float* xr = a.x + (int64_t)__shfl(my_col, q) * W;
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            const int64_t c = lane + kWave * v;
            val[u][v] = c < W ? xr[c] : 0.0f;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (t + u >= n) break;
          if (rr[u] != cur) {
            cur = rr[u];
            const float* dr = a.dA + cur * arow + (int64_t)k0 * W;
#pragma unroll
            for (int k = 0; k < KT; ++k)
#pragma unroll
              for (int v = 0; v < NV; ++v) {
                const int64_t c = lane + kWave * v;
                da[k][v] = k < kn && c < W ? dr[k * W + c] : 0.0f;
              }
          }
          float part[KT];
#pragma unroll
          for (int k = 0; k < KT; ++k) {
            float s = 0.0f;
#pragma unroll
            for (int v = 0; v < NV; ++v) s += val[u][v] * da[k][v];
            part[k] = s;
          }
          const float tot = wave_sum_transposed<KT>(part, lane);
          const int kk = lane >> SH;
          if ((lane & ((1 << SH) - 1)) == 0 && kk < kn) slot[(k0 + kk) * kPad + t + u] = tot;
        }
      }
    }
    wave_lds_sync();
    // one position per lane: dg_k = dw_k w_k, dpseudo of the lane's edge id
    float dps[kGmmMaxDim];
#pragma unroll
    for (int d = 0; d < kGmmMaxDim; ++d) dps[d] = 0.0f;
    if (lane < n) {
#pragma nounroll
      for (int k = 0; k < K; ++k) {
        const float dg = slot[k * kPad + lane] * gmm_weight(ps, mu + k * dim, s2 + k * dim, dim);
        slot[k * kPad + lane] = dg;
#pragma unroll
        for (int d = 0; d < kGmmMaxDim; ++d)
          if (d < dim) dps[d] -= dg * (ps[d] - mu[k * dim + d]) * s2[k * dim + d];
      }
#pragma unroll
      for (int d = 0; d < kGmmMaxDim; ++d) {
        if (d < dim) {
          if (a.dpseudo) a.dpseudo[my_eid * dim + d] = dps[d];
          pslot[d * kPad + lane] = ps[d];
        }
      }
    }
    wave_lds_sync();
    // lane j's (k, d) pairs: the chunk's terms in position order
#pragma unroll
    for (int m = 0; m < MP; ++m) {
      const int j = lane + kWave * m;
      if (j < KD) {
        const int k = j / dim, d = j - k * dim;
        const float mj = mu[j], sj = sg[j], s2j = s2[j];
        float am = acc_mu[m], as = acc_sg[m];
        for (int p = 0; p < n; ++p) {
          const float diff = pslot[d * kPad + p] - mj;
          const float t = slot[k * kPad + p] * diff;
          am += t * s2j;
          as -= t * diff * sj;
        }
        acc_mu[m] = am;
        acc_sg[m] = as;
      }
    }
    wave_lds_sync();  // the slots are read before the next chunk overwrites them
  }
  float* part = a.part + rec * 2 * KD;
#pragma unroll
  for (int m = 0; m < MP; ++m) {
    const int j = lane + kWave * m;
    if (j < KD) {
      part[j] = acc_mu[m];
      part[KD + j] = acc_sg[m];
    }
  }
}

// dmu / dinv_sigma = the records added in record order (none: zeros)
__global__ void __launch_bounds__(kWave) k_gmm_param_reduce(GmmArgs a, int64_t num_recs) {
  constexpr int UR = 8;  // loads in flight; the additions keep record order
  const int KD = a.K * a.dim;
  const int j = blockIdx.x * kWave + threadIdx.x;
  if (j >= 2 * KD) return;
  float s = 0.0f;
  int64_t r = 0;
  for (; r + UR <= num_recs; r += UR) {
    float v[UR];
#pragma unroll
    for (int i = 0; i < UR; ++i) v[i] = a.part[(r + i) * 2 * KD + j];
#pragma unroll
    for (int i = 0; i < UR; ++i) s += v[i];
  }
  for (; r < num_recs; ++r) s += a.part[r * 2 * KD + j];
  float* dst = j < KD ? a.dmu : a.dinv_sigma;
  if (dst) dst[j < KD ? j : j - KD] = s;
}

// the K tile: the smallest instance that holds K, capped by the register budget
constexpr int kt_cap(bool grad, int nv) {
  return grad ? (nv <= 2 ? 8 : 4) : (kGmmAccBudget / nv < kGmmMaxK ? kGmmAccBudget / nv : kGmmMaxK);
}
int kt_of(bool grad, int nv, int K) {
  const int cap = kt_cap(grad, nv);
  int kt = 4;
  while (kt < K && kt < cap) kt *= 2;
  return kt;
}

template <bool GRAD, int NV, int KT>
void launch_inst(const GmmArgs& a, hipStream_t s) {
  if constexpr (KT <= kt_cap(GRAD, NV)) {
    const int KD = a.K * a.dim;
    if constexpr (GRAD) {
      const int64_t recs = gmm_records(a.nnz);
      const size_t lds =
          sizeof(float) * static_cast<size_t>(3 * KD + kWavesPerBlock * (a.K + a.dim) * kPad);
      hipLaunchKernelGGL((k_gmm_edge_grad<NV, KT>),
                         dim3(static_cast<unsigned>((recs + kWavesPerBlock - 1) / kWavesPerBlock)),
                         dim3(kBlock), lds, s, a, gmm_chunks_per_record(a.nnz), recs);
    } else {
      const size_t lds = sizeof(float) * static_cast<size_t>(2 * KD + kWavesPerBlock * KT * kWave);
      const unsigned blocks =
          static_cast<unsigned>((gmm_chunks(a.nnz) + kWavesPerBlock - 1) / kWavesPerBlock);
      hipLaunchKernelGGL((k_gmm_aggregate<NV, KT>),
                         dim3(blocks, static_cast<unsigned>((a.K + KT - 1) / KT)), dim3(kBlock), lds,
                         s, a);
    }
  }
}
template <bool GRAD, int NV>
void launch_nv(const GmmArgs& a, hipStream_t s) {
  switch (kt_of(GRAD, NV, a.K)) {
    case 4: launch_inst<GRAD, NV, 4>(a, s); break;
    case 8: launch_inst<GRAD, NV, 8>(a, s); break;
    case 16: launch_inst<GRAD, NV, 16>(a, s); break;
    default: launch_inst<GRAD, NV, 32>(a, s); break;
  }
}
template <bool GRAD>
void launch_width(const GmmArgs& a, hipStream_t s) {
  switch (gmm_cols_per_lane(a.width)) {
    case 1: launch_nv<GRAD, 1>(a, s); break;
    case 2: launch_nv<GRAD, 2>(a, s); break;
    case 4: launch_nv<GRAD, 4>(a, s); break;
    default: launch_nv<GRAD, 8>(a, s); break;
  }
}

}  // namespace

void launch_gmm_aggregate(const GmmArgs& a, hipStream_t s) {
  if (a.num_rows == 0) return;
  launch_width<false>(a, s);
  if (a.nnz > kGmmChunk) {
    const unsigned blocks =
        static_cast<unsigned>((gmm_chunks(a.nnz) + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(k_gmm_fixup, dim3(blocks), dim3(kBlock), 0, s, a);
  }
}

void launch_gmm_edge_grad(const GmmArgs& a, hipStream_t s) {
  if (a.nnz > 0) launch_width<true>(a, s);
  if (a.dmu != nullptr || a.dinv_sigma != nullptr) {
    const int n2 = 2 * a.K * a.dim;
    hipLaunchKernelGGL(k_gmm_param_reduce, dim3(static_cast<unsigned>((n2 + kWave - 1) / kWave)),
                       dim3(kWave), 0, s, a, gmm_records(a.nnz));
  }
}

}  // namespace dglmi
