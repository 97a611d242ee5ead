// AtomicConv (ACNN): radial-filter aggregation, the filters computed where they are used.
//
//   out[v, t K + k] = sum_{e = (u -> v)} x[u, t] e_k(d_e)
//   e_k(d) = exp(-gamma_k (d - r_k)^2) f_k(d),  f_k(d) = 1/2 (cos(pi d / c_k) + 1) if d <= c_k else 0
//
// The reference builds three (K, E, 1) tensors for the filters, an (E, T K) message tensor
// and reduces it on degree buckets.  Here an edge contributes one distance and the T
// floats of its source; the (E, K) filter values are never stored.  The walk is bound by
// exp and cos (one of each per (edge, k)), not by its gathers, so the split of the work
// differs from the GMM walk's: A LANE OWNS A FILTER k, not a feature column.  It keeps
// gamma_k, r_k, c_k and pi / c_k in registers for its whole life (no parameter staging in
// LDS), the k-contiguous output out[v, t K + k] is one coalesced store per t, and in the
// backward the three parameter gradients are in-lane running sums, with no butterfly.
//
//  * k_atomic_aggregate<TT> (in-CSR): one wave owns kAtomicChunk = 64 consecutive
//    positions.  Phase 1, one position per lane: row, column, edge id, d = dist[eid], and
//    the position's T source values into the wave's LDS slot, slot[position * stride + t]
//    with stride = T | 1.  The stride is odd, so the 64 lanes' phase-1 writes of one t fall
//    in 64 different banks; in phase 2 the lanes of a group read ONE address (a broadcast)
//    and the G groups read G consecutive positions, G <= 64 addresses an odd stride apart:
//    different banks again.  Both phases are free of bank conflicts.
//    Phase 2: TT accumulators per lane (T rounded up to an instance, T <= 32), x[u, t] as
//    LDS broadcasts, e_k(d) computed once per (edge, k).  K > 64 walks tiles of 64 filters
//    over gridDim.y.  K <= 32: the wave splits into G = 64 / pow2ceil(K) lane groups; the
//    walk goes row span by row span, group j takes positions j, j + G, .. of the span, and
//    the G partials are added by a butterfly over the groups (one fixed association) once,
//    when the span ends.  Real ACNN grids have K = 5 .. 12: without the split 80 to 90 %
//    of the lanes would idle.
//  * Rows cut by a chunk boundary: internal.h's segmented fixup protocol (seg_reset,
//    fixup_role, seg_fold, CarryLayout) with records of T K floats, folded by
//    fixup_float_records as in k_gmm_fixup.  Rows without edges are written as zeros.
//  * k_atomic_edge_grad<TT> (in-CSR, same chunks, lane <-> k, the same groups): a wave takes
//    a contiguous range of chunks, one K tile of 64 after the other.  A group holds
//    g[v, t, k] of its position's row in TT registers (coalesced over k), forms dw_k =
//    sum_t x[u, t] g[v, t, k] in-lane, recomputes e_k, h_k and adds its terms of dgamma_k,
//    dr_k, dc_k in position order.  The per-(position, k) terms of ddist go through LDS,
//    term[k * (64 + G) + position]: in one step the lanes (group j, filter k) write
//    k (64 + G) + j + const = k G + j (mod 64), a bijection onto the banks, and the read is
//    one position per lane, consecutive addresses.  One position per lane adds them in k
//    order and writes its edge id once per tile (the same lane adds the next tile's sum to
//    what it wrote).  One partial record of 3 K floats per wave -- gmm_records(nnz) of
//    them, a function of nnz alone -- and k_atomic_param_reduce adds them in record order.
//    Each of the four outputs is optional; a NULL output is not computed.
//  * Matrix instructions do not fit: per destination the product is (T x deg) . (deg x K)
//    with deg ~ 12, segmented by rows of varying length, its right factor does not exist
//    until exp and cos have produced it, and the time is in those transcendentals (about
//    40 VALU operations per (edge, k) against T multiply-adds); an MFMA would take a tile
//    that is mostly padding and save none of it.
//  * No floating-point atomics; every sum has one fixed order: bit-reproducible.
//  * exp, cos, sin: HIP's expf, cosf, sinf (documented maximum errors 1, 1 and 1 ulp in the
//    HIP math API reference), e_k through atomic_weight in both kernels, so forward and
//    backward see the same e_k.
#include <hip/hip_runtime.h>

#include "internal.h"

namespace dglmi {
namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
static_assert(kAtomicChunk == kWave && kAtomicChunk == kGmmChunk,
              "one position per lane; gmm_chunks / gmm_records count these chunks");

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// what a lane keeps of its filter
struct Filter {
  float gamma, r, c, pic;  // pic = pi / c
};
__device__ __forceinline__ Filter load_filter(const AtomicArgs& a, int k) {
  Filter p;
  p.gamma = a.scaling[k];
  p.r = a.means[k];
  p.c = a.cutoffs[k];
  p.pic = 3.14159265358979323846f / p.c;
  return p;
}

// e_k(d); h = exp(-gamma (d - r)^2) and arg = pi d / c for the backward
__device__ __forceinline__ float atomic_weight(float d, const Filter& p, float& h, float& arg) {
  const float t = d - p.r;
  h = expf(-(p.gamma * (t * t)));
  arg = d * p.pic;
  return d <= p.c ? h * (0.5f * (cosf(arg) + 1.0f)) : 0.0f;
}

// the lane's place: group gi of G = 64 / kp, filter kk of its group's kp
struct Place {
  int lane, gi, kk, G;
};
__device__ __forceinline__ Place place_of(const AtomicArgs& a) {
  Place q;
  q.lane = threadIdx.x & (kWave - 1);
  q.gi = q.lane >> a.kp_shift;
  q.kk = q.lane & ((1 << a.kp_shift) - 1);
  q.G = kWave >> a.kp_shift;
  return q;
}

// phase 1: the lane's position (the chunk's last one for the lanes past its end) and that
// position's T source values into the wave's slot
struct Position {
  int row, col;
  int64_t eid;
  float d;
};
__device__ __forceinline__ Position stage_chunk(const AtomicArgs& a, int64_t p0, int n, int lane,
                                                float* slot, int stride) {
  const int64_t pl = p0 + (lane < n ? lane : n - 1);
  Position me;
  me.row = a.rows[pl];
  me.col = a.cols[pl];
  me.eid = a.eids[pl];
  me.d = a.dist[me.eid];
  const float* xr = a.x + (int64_t)me.col * a.T;
  for (int t = 0; t < a.T; ++t) slot[lane * stride + t] = xr[t];
  return me;
}

template <int TT>
__global__ void __launch_bounds__(kBlock) k_atomic_aggregate(AtomicArgs a) {
  extern __shared__ float lds[];
  const Place pl = place_of(a);
  const int lane = pl.lane, wave = threadIdx.x / kWave;
  const int64_t chunk = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  const int64_t nchunks = gmm_chunks(a.nnz);
  if (chunk >= nchunks) return;
  const int K = a.K, T = a.T, stride = T | 1;
  const int k = blockIdx.y * kWave + pl.kk;
  const bool kin = k < K;
  const Filter flt = load_filter(a, kin ? k : 0);
  float* slot = lds + wave * (kWave * stride);
  const int64_t rec = (int64_t)T * K;
  float acc[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) acc[t] = 0.0f;
  const int64_t p0 = chunk * kAtomicChunk;
  if (p0 < a.nnz) {
    const int64_t p1 = p0 + kAtomicChunk < a.nnz ? p0 + kAtomicChunk : a.nnz;
    const int n = static_cast<int>(p1 - p0);
    if (blockIdx.y == 0) seg_reset(a.seg_cnt, chunk, lane);
    const Position me = stage_chunk(a, p0, n, lane, slot, stride);
    wave_lds_sync();
    // phase 2: row span by row span; group gi takes every G-th position of the span
    int s = 0;
    while (s < n) {
      const int cur = __shfl(me.row, s);
      const uint64_t later = __ballot(lane > s && lane < n && me.row != cur);
      const int e = later ? __builtin_ctzll(later) : n;
      for (int q0 = s; q0 < e; q0 += pl.G) {
        const int q = q0 + pl.gi;
        const float d = __shfl(me.d, q < n ? q : n - 1);
        if (q < e && kin) {
          float h, arg;
          const float w = atomic_weight(d, flt, h, arg);
          const float* xs = slot + q * stride;
#pragma unroll
          for (int t = 0; t < TT; ++t)
            if (t < T) acc[t] += w * xs[t];
        }
      }
      // the groups' partials, one association; every group ends with the span's sum
      for (int off = kWave >> 1; off >= (1 << a.kp_shift); off >>= 1) {
#pragma unroll
        for (int t = 0; t < TT; ++t) acc[t] += __shfl_xor(acc[t], off);
      }
      const bool cont = s == 0 && p0 > 0 && a.rows[p0 - 1] == cur;
      float* o = cont ? a.carry + chunk * rec : a.out + (int64_t)cur * rec;
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        if (t < T && pl.gi == 0 && kin) o[t * K + k] = acc[t];
        acc[t] = 0.0f;
      }
      s = e;
    }
  }
  if (blockIdx.y == 0)
    fill_empty_rows(a.indptr, a.num_rows, chunk, nchunks, kWave, lane, [&](int64_t r) {
      for (int64_t j = lane; j < rec; j += kWave) a.out[r * rec + j] = 0.0f;
    });
}

// folds a cut row's carries into its head in chunk order
__global__ void __launch_bounds__(kBlock) k_atomic_fixup(AtomicArgs a) {
  fixup_float_records(a, a.indptr, (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave,
                      (int64_t)a.T * a.K, threadIdx.x & (kWave - 1));
}

// LDS floats of one wave of the edge gradient: the x slot, then the ddist terms
__host__ __device__ inline int grad_wave_floats(int T, int kp_shift) {
  return kWave * (T | 1) + (1 << kp_shift) * (kWave + (kWave >> kp_shift));
}

template <int TT>
__global__ void __launch_bounds__(kBlock) k_atomic_edge_grad(AtomicArgs a, int64_t chunks_per_rec,
                                                             int64_t num_recs) {
  extern __shared__ float lds[];
  const Place pl = place_of(a);
  const int lane = pl.lane, wave = threadIdx.x / kWave;
  const int64_t rec = (int64_t)blockIdx.x * (blockDim.x / kWave) + wave;
  if (rec >= num_recs) return;
  const int K = a.K, T = a.T, stride = T | 1, S = kWave + pl.G;
  float* slot = lds + wave * grad_wave_floats(T, a.kp_shift);
  float* term = slot + kWave * stride;
  const int64_t grow = (int64_t)T * K;
  const bool want_d = a.ddist != nullptr;
  const bool want_c = a.dcutoffs != nullptr, want_m = a.dmeans != nullptr, want_g = a.dscaling != nullptr;
  const int64_t nchunks = gmm_chunks(a.nnz);
  const int64_t c_end = (rec + 1) * chunks_per_rec < nchunks ? (rec + 1) * chunks_per_rec : nchunks;
  for (int k0 = 0; k0 < K; k0 += kWave) {
    const int k = k0 + pl.kk;
    const bool kin = k < K;
    const int kn = K - k0 < kWave ? K - k0 : kWave;
    const Filter flt = load_filter(a, kin ? k : 0);
    const float pic_c = flt.pic / flt.c;  // pi / c^2
    float sc = 0.0f, sm = 0.0f, sg = 0.0f;
    for (int64_t chunk = rec * chunks_per_rec; chunk < c_end; ++chunk) {
      const int64_t p0 = chunk * kAtomicChunk;
      const int64_t p1 = p0 + kAtomicChunk < a.nnz ? p0 + kAtomicChunk : a.nnz;
      const int n = static_cast<int>(p1 - p0);
      const Position me = stage_chunk(a, p0, n, lane, slot, stride);
      wave_lds_sync();
      // group gi: positions gi, gi + G, .. of the chunk, g of the position's row in registers
      int cur = -1;
      float g[TT];
#pragma unroll
      for (int t = 0; t < TT; ++t) g[t] = 0.0f;
      for (int q0 = 0; q0 < n; q0 += pl.G) {
        const int q = q0 + pl.gi;
        const int qc = q < n ? q : n - 1;
        const int row = __shfl(me.row, qc);
        const float d = __shfl(me.d, qc);
        if (q < n && kin) {
          if (row != cur) {
            cur = row;
            const float* gr = a.g + (int64_t)row * grow + k;
#pragma unroll
            for (int t = 0; t < TT; ++t)
              if (t < T) g[t] = gr[t * K];
          }
          const float* xs = slot + q * stride;
          float dw = 0.0f;
#pragma unroll
          for (int t = 0; t < TT; ++t)
            if (t < T) dw += xs[t] * g[t];
          float h, arg;
          const float e = atomic_weight(d, flt, h, arg);
          const float hs = d <= flt.c ? h * (0.5f * sinf(arg)) : 0.0f;  // -h f' c / pi
          const float t = d - flt.r;
          const float de = dw * e;
          const float dr = de * (2.0f * flt.gamma * t);
          const float dc = dw * hs;
          if (want_g) sg -= de * (t * t);
          if (want_m) sm += dr;
          if (want_c) sc += dc * (d * pic_c);
          if (want_d) term[pl.kk * S + q] = -dr - dc * flt.pic;
        }
      }
      if (want_d) {
        wave_lds_sync();
        if (lane < n) {
          float sum = 0.0f;
          for (int j = 0; j < kn; ++j) sum += term[j * S + lane];
          a.ddist[me.eid] = k0 == 0 ? sum : a.ddist[me.eid] + sum;
        }
      }
      wave_lds_sync();  // the slots are read before the next chunk overwrites them
    }
    for (int off = kWave >> 1; off >= (1 << a.kp_shift); off >>= 1) {
      sc += __shfl_xor(sc, off);
      sm += __shfl_xor(sm, off);
      sg += __shfl_xor(sg, off);
    }
    if (pl.gi == 0 && kin) {
      float* part = a.part + rec * 3 * K;
      part[k] = sc;
      part[K + k] = sm;
      part[2 * K + k] = sg;
    }
  }
}

// dcutoffs / dmeans / dscaling = the records added in record order (none: zeros)
__global__ void __launch_bounds__(kWave) k_atomic_param_reduce(AtomicArgs a, int64_t num_recs) {
  constexpr int UR = 8;  // loads in flight; the additions keep record order
  const int K = a.K;
  const int j = blockIdx.x * kWave + threadIdx.x;
  if (j >= 3 * K) return;
  float* dst = j < K ? a.dcutoffs : j < 2 * K ? a.dmeans : a.dscaling;
  if (dst == nullptr) return;
  float s = 0.0f;
  int64_t r = 0;
  for (; r + UR <= num_recs; r += UR) {
    float v[UR];
#pragma unroll
    for (int i = 0; i < UR; ++i) v[i] = a.part[(r + i) * 3 * K + j];
#pragma unroll
    for (int i = 0; i < UR; ++i) s += v[i];
  }
  for (; r < num_recs; ++r) s += a.part[r * 3 * K + j];
  dst[j % K] = s;
}

template <bool GRAD, int TT>
void launch_inst(const AtomicArgs& a, hipStream_t s) {
  if constexpr (GRAD) {
    // 32 or 64 filters per group: 17 to 25 KB of LDS per wave, two waves per workgroup
    const int waves = a.kp_shift >= 5 ? 2 : kBlock / kWave;
    const int64_t recs = gmm_records(a.nnz);
    const size_t lds = sizeof(float) * static_cast<size_t>(waves * grad_wave_floats(a.T, a.kp_shift));
    hipLaunchKernelGGL((k_atomic_edge_grad<TT>), dim3(static_cast<unsigned>((recs + waves - 1) / waves)),
                       dim3(waves * kWave), lds, s, a, gmm_chunks_per_record(a.nnz), recs);
  } else {
    const size_t lds = sizeof(float) * static_cast<size_t>(kBlock * (a.T | 1));
    const unsigned blocks =
        static_cast<unsigned>((gmm_chunks(a.nnz) + kBlock / kWave - 1) / (kBlock / kWave));
    hipLaunchKernelGGL((k_atomic_aggregate<TT>),
                       dim3(blocks, static_cast<unsigned>((a.K + kWave - 1) / kWave)), dim3(kBlock),
                       lds, s, a);
  }
}
template <bool GRAD>
void launch_tt(const AtomicArgs& a, hipStream_t s) {
  switch (atomic_tt(a.T)) {
    case 1: launch_inst<GRAD, 1>(a, s); break;
    case 2: launch_inst<GRAD, 2>(a, s); break;
    case 4: launch_inst<GRAD, 4>(a, s); break;
    case 8: launch_inst<GRAD, 8>(a, s); break;
    case 16: launch_inst<GRAD, 16>(a, s); break;
    default: launch_inst<GRAD, 32>(a, s); break;
  }
}

}  // namespace

void launch_atomic_aggregate(const AtomicArgs& a, hipStream_t s) {
  if (a.num_rows == 0) return;
  launch_tt<false>(a, s);
  if (a.nnz > kAtomicChunk) {
    const unsigned blocks =
        static_cast<unsigned>((gmm_chunks(a.nnz) + kBlock / kWave - 1) / (kBlock / kWave));
    hipLaunchKernelGGL(k_atomic_fixup, dim3(blocks), dim3(kBlock), 0, s, a);
  }
}

void launch_atomic_edge_grad(const AtomicArgs& a, hipStream_t s) {
  if (a.nnz > 0) launch_tt<true>(a, s);
  if (a.dcutoffs != nullptr || a.dmeans != nullptr || a.dscaling != nullptr)
    hipLaunchKernelGGL(k_atomic_param_reduce, dim3(static_cast<unsigned>((3 * a.K + kWave - 1) / kWave)),
                       dim3(kWave), 0, s, a, gmm_records(a.nnz));
}

}  // namespace dglmi
