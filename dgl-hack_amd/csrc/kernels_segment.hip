// Segment kernels: reductions, broadcasts and the softmax over the segments of a batch
// (dgl.batch: segment b = the nodes or edges of graph b, rows offsets[b] .. offsets[b + 1]
// of an (N, F) table).  The reference reads a batch out with scatter_add_ over a host-built
// segment id (float atomics, backend/pytorch/tensor.py:228-239) and pads every graph to the
// largest for max / softmax (readout.py:396-432).
//
// The walk is the chunked walk of kernels_spmm.hip without the gather: rows in position
// order, cut into fixed chunks of K whole rows (one workgroup each, so the work of a
// workgroup does not depend on segment sizes).  Inside a workgroup lane (ry, tx) owns the
// VW-float column slot tx of kSegRowsPerLane consecutive rows; TX = slots per column tile,
// TY = 256 / TX row-lanes, K = TY * kSegRowsPerLane.  A lane starts at the segment of its
// first row (binary search in offsets, narrowed to the chunk's segments) and advances.
//   - a segment inside one lane's rows is stored directly;
//   - a segment cut by a lane boundary leaves a head and / or a tail partial in LDS, which
//     the slot's first row-lane folds in row-lane order (fixed, so deterministic);
//   - a segment cut by the chunk's start leaves that fold in the chunk's carry record, one
//     cut by its end in the output row; the fixup (fixup_role_segments + seg_fold of
//     internal.h, the protocol of every chunked walk here) merges them in chunk order.
// No atomics on data, and the association order is a function of (N, F, offsets) alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "internal.h"

namespace dglmi {
namespace {

constexpr int kSegBlock = 256;
constexpr int kSegRowsPerLane = 16;
constexpr int kSegBatch = 8;  // rows loaded ahead of their use

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int VW>
__device__ __forceinline__ void ld_nt(const float* p, float (&v)[VW]) {
  if constexpr (VW == 4) {
    const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else if constexpr (VW == 2) {
    const f32x2 t = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(p));
    v[0] = t.x; v[1] = t.y;
  } else {
    v[0] = __builtin_nontemporal_load(p);
  }
}
template <int VW>
__device__ __forceinline__ void ld(const float* p, float (&v)[VW]) {
  if constexpr (VW == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else if constexpr (VW == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  } else {
    v[0] = *p;
  }
}
template <int VW>
__device__ __forceinline__ void st(float* p, const float (&v)[VW]) {
  if constexpr (VW == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else if constexpr (VW == 2) *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  else *p = v[0];
}

// the online-softmax merge of kernels_softmax.hip (merge1): one exponential, NaN kept
__device__ __forceinline__ void sm_merge1(float& m, float& l, float m2, float l2) {
  const bool ge = m >= m2;
  const float hi = ge ? m : m2, lo = ge ? m2 : m;
  const float lhi = ge ? l : l2, llo = ge ? l2 : l;
  l = lhi + llo * expf(lo - (hi == -INFINITY ? 0.0f : hi));
  m = hi;
}

// One column's running state: v the sum / max / min / running max, l the softmax's sum of
// exp(s - v), a the lowest row that attains v (-1: no row yet).
template <int RED>
__device__ __forceinline__ void seg_init(float& v, float& l, int64_t& a) {
  v = RED == SEG_SUM ? 0.0f : (RED == SEG_MIN ? INFINITY : -INFINITY);
  l = 0.0f;
  a = -1;
}
// (x, i) comes after everything in (v, a); numpy.max / argmax: a NaN wins and stays, and
// among equals the first row is kept
template <int RED>
__device__ __forceinline__ void seg_take(float& v, int64_t& a, float x, int64_t i) {
  const bool better = RED == SEG_MAX ? x > v : x < v;
  if (a < 0 || (v == v && (x != x || better))) {
    v = x;
    a = i;
  }
}
template <int RED>
__device__ __forceinline__ void seg_update(float& v, float& l, int64_t& a, float x, int64_t i) {
  if constexpr (RED == SEG_SUM) v += x;
  else if constexpr (RED == SEG_STATS)
    sm_merge1(v, l, x, x == INFINITY ? __builtin_nanf("") : (x == -INFINITY ? 0.0f : 1.0f));
  else seg_take<RED>(v, a, x, i);
}
// the partial (v2, l2, a2) covers later rows than (v, l, a)
template <int RED>
__device__ __forceinline__ void seg_merge(float& v, float& l, int64_t& a, float v2, float l2,
                                          int64_t a2) {
  if constexpr (RED == SEG_SUM) v += v2;
  else if constexpr (RED == SEG_STATS) sm_merge1(v, l, v2, l2);
  else if (a2 >= 0) seg_take<RED>(v, a, v2, a2);
}

template <int RED> constexpr bool kHasArg = RED == SEG_MAX || RED == SEG_MIN;
template <int RED> constexpr bool kHasL = RED == SEG_STATS;

// where the parts of chunk c's carry record lie (values, then sums, then args)
__device__ __forceinline__ float* carry_v(const SegArgs& a, int64_t c) { return a.carry + c * a.F; }
__device__ __forceinline__ float* carry_l(const SegArgs& a, int64_t c) {
  return a.carry + (a.chunks + c) * a.F;
}
__device__ __forceinline__ int64_t* carry_a(const SegArgs& a, int64_t c) {
  return reinterpret_cast<int64_t*>(a.carry + ((a.chunks * a.F + 1) & ~int64_t(1))) + c * a.F;
}

template <int RED, int VW, int MUL>
__global__ void __launch_bounds__(kSegBlock) k_seg_reduce(SegArgs a, int TX, int TY, int tiles) {
  constexpr bool kA = kHasArg<RED>, kL = kHasL<RED>;
  __shared__ float sh_v[2][kSegBlock * VW];
  __shared__ float sh_l[2][kL ? kSegBlock * VW : 1];
  __shared__ int64_t sh_a[2][kA ? kSegBlock * VW : 1];
  __shared__ int sh_flag[kSegBlock];
  __shared__ int64_t sh_seg[2][kSegBlock];
  __shared__ int64_t sh_range[2];
  const int tid = threadIdx.x;
  const int ry = tid / TX, tx = tid - ry * TX;
  const bool active = ry < TY;
  const int64_t B = a.num_segments, F = a.F, S = F / VW;
  const int64_t chunk = blockIdx.x;
  const int64_t c0 = chunk * a.chunk;
  const int64_t c1 = c0 + a.chunk < a.num_rows ? c0 + a.chunk : a.num_rows;
  // the segments of the chunk's first and last row: two searches of the whole of offsets,
  // side by side in two wavefronts; every row-lane then searches between them only
  if ((tid == 0 || tid == 64) && c0 < c1)
    sh_range[tid >> 6] = seg_of_row(a.offsets, 0, B - 1, tid == 0 ? c0 : c1 - 1);
  __syncthreads();
  const int64_t ra = c0 + (int64_t)ry * kSegRowsPerLane;
  const int64_t rb = ra + kSegRowsPerLane < c1 ? ra + kSegRowsPerLane : c1;
  const bool has_rows = active && ra < rb;
  const int64_t s0 = has_rows ? seg_of_row(a.offsets, sh_range[0], sh_range[1], ra) : 0;
  const bool fresh0 = has_rows && a.offsets[s0] == ra;

  for (int tile = 0; tile < tiles; ++tile) {
    const int64_t sx = (int64_t)tile * TX + tx;
    const bool col = sx < S;
    const int li = tid * VW;
    int flags = 0;  // 1: head partial, 2: its segment ends here, 4: tail partial
    int64_t seg_tail = 0;
    if (has_rows && col) {
      float v[VW], l[VW];
      int64_t g[VW];
#pragma unroll
      for (int k = 0; k < VW; ++k) seg_init<RED>(v[k], l[k], g[k]);
      int64_t s = s0, end = a.offsets[s0 + 1];
      bool fresh = fresh0, dirty = false;
      const int64_t col0 = sx * VW;
      for (int64_t i = ra; i < rb; i += kSegBatch) {
        float xv[kSegBatch][VW], yv[kSegBatch][VW], wv[kSegBatch];
#pragma unroll
        for (int j = 0; j < kSegBatch; ++j) {
          if (i + j < rb) {
            ld_nt<VW>(a.x + (i + j) * F + col0, xv[j]);
            if constexpr (MUL == 2) ld_nt<VW>(a.y + (i + j) * F + col0, yv[j]);
            if constexpr (MUL == 1) wv[j] = a.w[i + j];
          }
        }
#pragma unroll
        for (int j = 0; j < kSegBatch; ++j) {
          if (i + j < rb) {
#pragma unroll
            for (int k = 0; k < VW; ++k) {
              float t = xv[j][k];
              if constexpr (MUL == 1) t = t * wv[j];
              if constexpr (MUL == 2) t = t * yv[j][k];
              seg_update<RED>(v[k], l[k], g[k], t, i + j);
            }
            dirty = true;
            if (i + j + 1 == end) {
              if (fresh) {
                st<VW>(a.out + s * F + col0, v);
                if constexpr (kL) st<VW>(a.out2 + s * F + col0, l);
                if constexpr (kA) {
#pragma unroll
                  for (int k = 0; k < VW; ++k) a.arg[s * F + col0 + k] = g[k];
                }
              } else {
#pragma unroll
                for (int k = 0; k < VW; ++k) {
                  sh_v[0][li + k] = v[k];
                  if constexpr (kL) sh_l[0][li + k] = l[k];
                  if constexpr (kA) sh_a[0][li + k] = g[k];
                }
                flags |= 3;
              }
              do {
                ++s;
              } while (s < B && a.offsets[s + 1] == i + j + 1);
              end = s < B ? a.offsets[s + 1] : INT64_MAX;
              fresh = true;
              dirty = false;
#pragma unroll
              for (int k = 0; k < VW; ++k) seg_init<RED>(v[k], l[k], g[k]);
            }
          }
        }
      }
      if (dirty) {
        const int rec = fresh ? 1 : 0;
#pragma unroll
        for (int k = 0; k < VW; ++k) {
          sh_v[rec][li + k] = v[k];
          if constexpr (kL) sh_l[rec][li + k] = l[k];
          if constexpr (kA) sh_a[rec][li + k] = g[k];
        }
        flags |= fresh ? 4 : 1;
        seg_tail = s;
      }
    }
    if (active && tx == 0) {
      sh_flag[ry] = flags;
      sh_seg[0][ry] = s0;
      sh_seg[1][ry] = seg_tail;
    }
    __syncthreads();
    if (ry == 0 && col) {
      // the slot's partials in row-lane order; `cont`: the open segment began before c0
      float v[VW], l[VW];
      int64_t g[VW];
#pragma unroll
      for (int k = 0; k < VW; ++k) seg_init<RED>(v[k], l[k], g[k]);
      bool open = false, cont = false;
      int64_t oseg = 0;
      const int64_t col0 = sx * VW;
      auto emit = [&]() {
        float* pv = cont ? carry_v(a, chunk) + col0 : a.out + oseg * F + col0;
#pragma unroll
        for (int k = 0; k < VW; ++k) pv[k] = v[k];
        if constexpr (kL) {
          float* pl = cont ? carry_l(a, chunk) + col0 : a.out2 + oseg * F + col0;
#pragma unroll
          for (int k = 0; k < VW; ++k) pl[k] = l[k];
        }
        if constexpr (kA) {
          int64_t* pa = cont ? carry_a(a, chunk) + col0 : a.arg + oseg * F + col0;
#pragma unroll
          for (int k = 0; k < VW; ++k) pa[k] = g[k];
        }
      };
      for (int q = 0; q < TY; ++q) {
        const int fl = sh_flag[q];
        const int qi = (q * TX + tx) * VW;
        if (fl & 1) {
          if (!open) {
            open = true;
            cont = true;
            oseg = sh_seg[0][q];
          }
#pragma unroll
          for (int k = 0; k < VW; ++k)
            seg_merge<RED>(v[k], l[k], g[k], sh_v[0][qi + k], kL ? sh_l[0][kL ? qi + k : 0] : 0.0f,
                           kA ? sh_a[0][kA ? qi + k : 0] : int64_t(-1));
          if (fl & 2) {
            emit();
            open = false;
#pragma unroll
            for (int k = 0; k < VW; ++k) seg_init<RED>(v[k], l[k], g[k]);
          }
        }
        if (fl & 4) {
#pragma unroll
          for (int k = 0; k < VW; ++k) {
            v[k] = sh_v[1][qi + k];
            if constexpr (kL) l[k] = sh_l[1][qi + k];
            if constexpr (kA) g[k] = sh_a[1][qi + k];
          }
          open = true;
          cont = false;
          oseg = sh_seg[1][q];
        }
      }
      if (open) emit();
    }
    __syncthreads();
  }

  seg_reset(a.seg_cnt, chunk, tid);
  // empty segments take the identity; every workgroup checks its share of the segments
  const int64_t share = (B + gridDim.x - 1) / gridDim.x;
  const int64_t e0 = chunk * share;
  const int64_t e1 = e0 + share < B ? e0 + share : B;
  for (int64_t idx = tid; idx < (e1 - e0) * F; idx += kSegBlock) {
    const int64_t s = e0 + idx / F;
    if (a.offsets[s] != a.offsets[s + 1]) continue;
    const int64_t o = s * F + idx % F;
    float v, l;
    int64_t g;
    seg_init<RED>(v, l, g);
    a.out[o] = v;
    if constexpr (kL) a.out2[o] = l;
    if constexpr (kA) a.arg[o] = g;
  }
}

// L lanes per chunk (a power of two <= 64, inside one wavefront); lane t folds columns
// t, t + L, ...
template <int RED>
__global__ void __launch_bounds__(kSegBlock) k_seg_fixup(SegArgs a, int L) {
  constexpr bool kA = kHasArg<RED>, kL = kHasL<RED>;
  const int64_t c = ((int64_t)blockIdx.x * kSegBlock + threadIdx.x) / L;
  const int lane = threadIdx.x & (L - 1);
  if (c >= a.chunks) return;
  const FixupRole w = fixup_role_segments(a, c);
  if (!w.work) return;
  const int64_t F = a.F;
  seg_fold(w, a.seg_cnt, L, lane, [&](bool head, int64_t c0, int64_t c1, int64_t step) {
    float* dv = head ? a.out + w.r * F : carry_v(a, c0);
    float* dl = !kL ? nullptr : (head ? a.out2 + w.r * F : carry_l(a, c0));
    int64_t* da = !kA ? nullptr : (head ? a.arg + w.r * F : carry_a(a, c0));
    for (int64_t f = lane; f < F; f += L) {
      float v = dv[f], l = 0.0f;
      int64_t g = -1;
      if constexpr (kL) l = dl[f];
      if constexpr (kA) g = da[f];
      for (int64_t cc = head ? c0 : c0 + 1; cc <= c1; cc += step) {
        float l2 = 0.0f;
        int64_t g2 = -1;
        if constexpr (kL) l2 = carry_l(a, cc)[f];
        if constexpr (kA) g2 = carry_a(a, cc)[f];
        seg_merge<RED>(v, l, g, carry_v(a, cc)[f], l2, g2);
      }
      dv[f] = v;
      if constexpr (kL) dl[f] = l;
      if constexpr (kA) da[f] = g;
    }
  });
}

// Per-row kernels on the same lane layout (no LDS: a lane needs only its row's segment).
enum { ROWS_BCAST = 0, ROWS_NORM = 1, ROWS_SMBWD = 2 };
template <int MODE, int VW>
__global__ void __launch_bounds__(kSegBlock) k_seg_rows(SegRowArgs a, int TX, int TY, int tiles) {
  const int tid = threadIdx.x;
  const int ry = tid / TX, tx = tid - ry * TX;
  const int64_t B = a.num_segments, F = a.F, S = F / VW;
  const int64_t ra = ((int64_t)blockIdx.x * TY + ry) * kSegRowsPerLane;
  const int64_t rb = ra + kSegRowsPerLane < a.num_rows ? ra + kSegRowsPerLane : a.num_rows;
  if (ry >= TY || ra >= rb) return;
  const int64_t s0 = seg_of_row(a.offsets, 0, B - 1, ra);
  for (int tile = 0; tile < tiles; ++tile) {
    const int64_t sx = (int64_t)tile * TX + tx;
    if (sx >= S) continue;
    const int64_t col0 = sx * VW;
    int64_t s = s0, end = a.offsets[s0 + 1];
    float sv[VW], sv2[VW];
    auto load_seg = [&]() {
      ld<VW>(a.v + s * F + col0, sv);
      if constexpr (MODE == ROWS_NORM) ld<VW>(a.v2 + s * F + col0, sv2);
      if constexpr (MODE == ROWS_BCAST) {
        if (a.divide) {
          const int64_t n = end - a.offsets[s];
          const float d = static_cast<float>(n > 1 ? n : 1);
#pragma unroll
          for (int k = 0; k < VW; ++k) sv[k] = sv[k] / d;
        }
      }
    };
    load_seg();
    for (int64_t i = ra; i < rb; i += kSegBatch) {
      float xv[kSegBatch][VW], yv[kSegBatch][VW], wv[kSegBatch];
#pragma unroll
      for (int j = 0; j < kSegBatch; ++j) {
        if (i + j < rb) {
          if constexpr (MODE != ROWS_BCAST) ld_nt<VW>(a.x + (i + j) * F + col0, xv[j]);
          if constexpr (MODE == ROWS_SMBWD) ld_nt<VW>(a.y + (i + j) * F + col0, yv[j]);
          if constexpr (MODE == ROWS_BCAST) wv[j] = a.w != nullptr ? a.w[i + j] : 1.0f;
        }
      }
#pragma unroll
      for (int j = 0; j < kSegBatch; ++j) {
        if (i + j < rb) {
          if (i + j == end) {
            do {
              ++s;
            } while (s + 1 < B && a.offsets[s + 1] <= i + j);
            end = a.offsets[s + 1];
            load_seg();
          }
          float o[VW];
#pragma unroll
          for (int k = 0; k < VW; ++k) {
            if constexpr (MODE == ROWS_BCAST) o[k] = a.w != nullptr ? sv[k] * wv[j] : sv[k];
            else if constexpr (MODE == ROWS_NORM) o[k] = expf(xv[j][k] - sv[k]) / sv2[k];
            else o[k] = xv[j][k] * yv[j][k] - xv[j][k] * sv[k];
          }
          st<VW>(a.out + (i + j) * F + col0, o);
        }
      }
    }
  }
}

// out[i] = sum_f x[i, f] v[seg(i), f].  L lanes per row (a power of two <= 64); lane t adds
// the products of slots t, t + L, ... in ascending column order into one accumulator
// (product rounded, then the add), and the L partials are combined by an xor butterfly at
// distances 1, 2, 4, ... (both partners add the same two values, so every lane holds the
// same bits).  A group of L lanes takes kSegRowsPerLane consecutive rows.
template <int VW>
__global__ void __launch_bounds__(kSegBlock) k_seg_rowdot(SegRowArgs a, int L) {
  const int64_t grp = ((int64_t)blockIdx.x * kSegBlock + threadIdx.x) / L;
  const int lane = threadIdx.x & (L - 1);
  const int64_t B = a.num_segments, F = a.F, S = F / VW;
  const int64_t ra = grp * kSegRowsPerLane;
  const int64_t rb = ra + kSegRowsPerLane < a.num_rows ? ra + kSegRowsPerLane : a.num_rows;
  if (ra >= rb) return;
  int64_t s = seg_of_row(a.offsets, 0, B - 1, ra), end = a.offsets[s + 1];
  for (int64_t i = ra; i < rb; ++i) {
    if (i == end) {
      do {
        ++s;
      } while (s + 1 < B && a.offsets[s + 1] <= i);
      end = a.offsets[s + 1];
    }
    float acc = 0.0f;
    for (int64_t sx = lane; sx < S; sx += L) {
      float xv[VW], vv[VW];
      ld_nt<VW>(a.x + i * F + sx * VW, xv);
      ld<VW>(a.v + s * F + sx * VW, vv);
#pragma unroll
      for (int k = 0; k < VW; ++k) acc += xv[k] * vv[k];
    }
    for (int d = 1; d < L; d <<= 1) acc += __shfl_xor(acc, d, L);
    if (lane == 0) a.out[i] = acc;
  }
}

__global__ void __launch_bounds__(kSegBlock) k_seg_scatter_arg(const int64_t* __restrict__ arg,
                                                              const float* __restrict__ gy,
                                                              int64_t n, int64_t F,
                                                              int64_t num_rows,
                                                              float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kSegBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t r = arg[i];
  if (r >= 0 && r < num_rows) out[r * F + i % F] = gy[i];
}

struct SegPlan {
  int vw, tx, ty, tiles;
};
SegPlan seg_plan(int64_t F) {
  SegPlan p;
  p.vw = F % 4 == 0 ? 4 : (F % 2 == 0 ? 2 : 1);
  const int64_t S = F / p.vw;
  p.tiles = static_cast<int>((S + kSegBlock - 1) / kSegBlock);
  p.tx = static_cast<int>((S + p.tiles - 1) / p.tiles);
  p.ty = kSegBlock / p.tx;
  return p;
}
int pow2_lanes(int64_t n) {
  int L = 1;
  while (L < 64 && L < n) L <<= 1;
  return L;
}

template <int RED, int VW>
void reduce_mul(int mul, const SegArgs& a, const SegPlan& p, hipStream_t s) {
  const dim3 grid(static_cast<unsigned>(a.chunks)), block(kSegBlock);
  if (mul == 0) hipLaunchKernelGGL((k_seg_reduce<RED, VW, 0>), grid, block, 0, s, a, p.tx, p.ty, p.tiles);
  else if (mul == 1) hipLaunchKernelGGL((k_seg_reduce<RED, VW, 1>), grid, block, 0, s, a, p.tx, p.ty, p.tiles);
  else hipLaunchKernelGGL((k_seg_reduce<RED, VW, 2>), grid, block, 0, s, a, p.tx, p.ty, p.tiles);
}
template <int RED>
void reduce_red(int mul, const SegArgs& a, hipStream_t s) {
  const SegPlan p = seg_plan(a.F);
  if (p.vw == 4) reduce_mul<RED, 4>(mul, a, p, s);
  else if (p.vw == 2) reduce_mul<RED, 2>(mul, a, p, s);
  else reduce_mul<RED, 1>(mul, a, p, s);
  if (a.chunks > 1) {
    const int L = pow2_lanes(a.F);
    const int64_t blocks = (a.chunks * L + kSegBlock - 1) / kSegBlock;
    hipLaunchKernelGGL((k_seg_fixup<RED>), dim3(static_cast<unsigned>(blocks)), dim3(kSegBlock), 0,
                       s, a, L);
  }
}

template <int MODE>
void rows_mode(const SegRowArgs& a, hipStream_t s) {
  const SegPlan p = seg_plan(a.F);
  const int64_t K = (int64_t)p.ty * kSegRowsPerLane;
  const dim3 grid(static_cast<unsigned>((a.num_rows + K - 1) / K)), block(kSegBlock);
  if (p.vw == 4) hipLaunchKernelGGL((k_seg_rows<MODE, 4>), grid, block, 0, s, a, p.tx, p.ty, p.tiles);
  else if (p.vw == 2) hipLaunchKernelGGL((k_seg_rows<MODE, 2>), grid, block, 0, s, a, p.tx, p.ty, p.tiles);
  else hipLaunchKernelGGL((k_seg_rows<MODE, 1>), grid, block, 0, s, a, p.tx, p.ty, p.tiles);
}

}  // namespace

int64_t seg_chunk_rows(int64_t F) { return (int64_t)seg_plan(F).ty * kSegRowsPerLane; }

// sum: F values; softmax statistics: F maxima + F sums; max / min: F values + F int64 rows
// (8-byte aligned behind all the values: one spare float)
int64_t seg_rec_floats(int red, int64_t F) {
  return red == SEG_SUM ? F : (red == SEG_STATS ? 2 * F : 3 * F + 1);
}

int64_t seg_workspace_bytes(int64_t num_rows, int64_t F) {
  if (F <= 0) return 0;
  const int64_t K = seg_chunk_rows(F);
  const int64_t chunks = num_rows > 0 ? (num_rows + K - 1) / K : 1;
  return CarryLayout(chunks, seg_rec_floats(SEG_MAX, F)).bytes;
}

void launch_seg_reduce(int red, int mul, const SegArgs& a, hipStream_t s) {
  if (red == SEG_SUM) reduce_red<SEG_SUM>(mul, a, s);
  else if (red == SEG_MAX) reduce_red<SEG_MAX>(mul, a, s);
  else if (red == SEG_MIN) reduce_red<SEG_MIN>(mul, a, s);
  else reduce_red<SEG_STATS>(0, a, s);
}

void launch_seg_rows(int mode, const SegRowArgs& a, hipStream_t s) {
  if (a.num_rows == 0) return;
  if (mode == ROWS_BCAST) rows_mode<ROWS_BCAST>(a, s);
  else if (mode == ROWS_NORM) rows_mode<ROWS_NORM>(a, s);
  else rows_mode<ROWS_SMBWD>(a, s);
}

void launch_seg_rowdot(const SegRowArgs& a, hipStream_t s) {
  if (a.num_rows == 0) return;
  const int vw = a.F % 4 == 0 ? 4 : (a.F % 2 == 0 ? 2 : 1);
  const int L = pow2_lanes(a.F / vw);
  const int64_t groups = (a.num_rows + kSegRowsPerLane - 1) / kSegRowsPerLane;
  const dim3 grid(static_cast<unsigned>((groups * L + kSegBlock - 1) / kSegBlock)), block(kSegBlock);
  if (vw == 4) hipLaunchKernelGGL((k_seg_rowdot<4>), grid, block, 0, s, a, L);
  else if (vw == 2) hipLaunchKernelGGL((k_seg_rowdot<2>), grid, block, 0, s, a, L);
  else hipLaunchKernelGGL((k_seg_rowdot<1>), grid, block, 0, s, a, L);
}

void launch_seg_scatter_arg(const int64_t* arg, const float* gy, int64_t B, int64_t F,
                            int64_t num_rows, float* out, hipStream_t s) {
  const int64_t n = B * F;
  if (n == 0) return;
  hipLaunchKernelGGL(k_seg_scatter_arg, dim3(static_cast<unsigned>((n + kSegBlock - 1) / kSegBlock)),
                     dim3(kSegBlock), 0, s, arg, gy, n, F, num_rows, out);
}

}  // namespace dglmi
