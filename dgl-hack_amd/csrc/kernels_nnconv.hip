// NNConv (MPNN): edge-conditioned convolution, one in x out weight matrix per edge.
//
//   out[v, :] = scale[v] sum_{e = (u -> v)} x[u, :] . W[eid(e)]          W (E, in, out)
//
// The reference multiplies (N, in, 1) by (E, in, out), reduces that to (N, in, out) and
// sums over `in` afterwards; sum and mean are linear, so the sum over `in` is taken inside
// the walk and neither the (N, in, out) table nor, backwards, a second (E, in, out) pass
// exists.  The work is one mat-vec per edge, 2 flops per 4 bytes of W, and every W[e] is
// used exactly once: the kernels are bound by streaming W once.  Matrix instructions do
// not fit: an MFMA needs an operand that several rows or columns share, and here each
// W[e] meets one vector; there is no reuse to feed one with.
//
//  * Lane layout (vector instance: out % 4 == 0, LR = out / 4 a power of two <= 64):
//    LR lanes cover one row of W[e] with one 16-byte load each, RS = 64 / LR rows per
//    wave-wide load, so every load instruction of a wave fetches 1 KB contiguous
//    (lane l reads floats 256 j + 4 l of W[e] at step j).  Lane l = rg LR + cg keeps 4
//    accumulators, columns 4 cg .. 4 cg + 3, for the rows i = rg (mod RS).  Scalar instance
//    (any other out): LR = 64, RS = 1, lane l owns columns l, l + 64, .. (NC of them) and
//    walks W[e] row by row with 4-byte loads.
//  * k_nnconv_aggregate (in-CSR): one wave owns `chunk` consecutive positions (a launch
//    parameter, nnconv_chunk: a position is in * out * 4 bytes here).  Per position the
//    source row x[u, :] is staged once in the wave's LDS slot and read as broadcasts; U
//    loads of W are in flight per lane.  The RS partial row groups are NOT reduced per
//    edge: accumulation over a row's edges is linear, so the cross-lane reduce (log2 RS
//    shuffles per accumulator) runs once where a row, or a chunk's piece of one, is flushed.
//  * k_nnconv_backward (out-CSR, rows are sources), templated on the gradients wanted.
//    Per position it gathers gs = scale[v] g[v, lane's columns].  dW[eid] = x[u] (x) gs is
//    written with the forward's addresses (16-byte stores, 1 KB per wave instruction, every
//    edge id once, no reduction).  dx[u, i] = sum_e <W[eid, i, :], gs>: a lane adds its
//    columns' part of the dot product of row step j into accumulator j (kNnAccTile = 32
//    per lane, i.e. 32 RS rows of W; more rows are tiles over gridDim.y, and a tile reads
//    only its own rows of W) across all of a source's edges; the reduce over the LR lanes
//    of a row happens once per flush, by a transposing butterfly (values halve as lanes
//    pair up: 31 shuffles for 32 values, not 32 log2 LR).  Without dx, W is not read;
//    without dW nothing of size E in out is written.
//  * Rows cut by a chunk boundary: internal.h's segmented fixup protocol (seg_reset,
//    fixup_role, seg_fold, CarryLayout) with records of `out` (forward) or `in` (dx) floats.
//    The row scale (1 / in-degree for "mean") is applied where a row is finished; rows
//    without positions are written as zeros.
//  * No floating-point atomics; every sum has one fixed order: bit-reproducible.
#include <hip/hip_runtime.h>

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

// the lane's k-th column
template <bool VEC, int LR>
__device__ __forceinline__ int col_of(int lane, int k) {
  return VEC ? 4 * (lane & (LR - 1)) + k : lane + kWave * k;
}

// the lane's float offset inside a wave-wide step of W[e]: the vector instance's step is RS
// rows = 256 floats, 4 per lane; the scalar instance's is one row, column `lane` first
template <bool VEC>
__device__ __forceinline__ unsigned lane_offset(int lane) {
  return VEC ? 4u * lane : static_cast<unsigned>(lane);
}

// the lane's columns of the step of W (or dW) that starts at `step` (wave-uniform, so the
// address is one scalar base and one 32-bit lane offset); !ok: zeros / nothing
template <bool VEC, int NC>
__device__ __forceinline__ void load_cols(const float* step, unsigned off, int lane, int fout,
                                          bool ok, float (&v)[NC]) {
  if constexpr (VEC) {
    float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (ok) t = *reinterpret_cast<const float4*>(step + off);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < NC; ++k) v[k] = ok && lane + kWave * k < fout ? step[off + kWave * k] : 0.0f;
  }
}
template <bool VEC, int NC>
__device__ __forceinline__ void store_cols(float* step, unsigned off, int lane, int fout, bool ok,
                                           const float (&v)[NC]) {
  if constexpr (VEC) {
    if (ok) *reinterpret_cast<float4*>(step + off) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (ok && lane + kWave * k < fout) step[off + kWave * k] = v[k];
  }
}

template <bool VEC, int LR, int NC>
__global__ void __launch_bounds__(kBlock) k_nnconv_aggregate(NnconvArgs a) {
  constexpr int RS = kWave / LR;
  constexpr int U = VEC ? 8 : (NC >= 4 ? 2 : NC == 2 ? 4 : 8);  // loads of W in flight per lane
  extern __shared__ float lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int fin = a.fin, fout = a.fout;
  const int64_t CH = a.chunk;
  const int64_t chunk = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  const int64_t nchunks = nnconv_chunks(a.nnz, CH);
  if (chunk >= nchunks) return;
  float* slot = lds + wave * fin;
  const int rg = lane / LR;
  const unsigned loff = lane_offset<VEC>(lane);
  float acc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) acc[k] = 0.0f;
  const int64_t p0 = chunk * CH;
  if (p0 < a.nnz) {
    const int64_t p1 = p0 + CH < a.nnz ? p0 + CH : a.nnz;
    const int n = static_cast<int>(p1 - p0);
    seg_reset(a.seg_cnt, chunk, lane);
    const int64_t pl = p0 + (lane < n ? lane : n - 1);
    const int my_row = a.rows[pl], my_col = a.cols[pl], my_eid = a.eids[pl];
    int64_t cur = __builtin_amdgcn_readlane(my_row, 0);
    bool cont = p0 > 0 && a.rows[p0 - 1] == cur;
    auto flush = [&]() {
      const bool done = !cont && a.indptr[cur + 1] <= p1;
      float* o = cont ? a.carry + chunk * fout : a.out + cur * fout;
      const float scale = done && a.row_scale ? a.row_scale[cur] : 1.0f;
#pragma unroll
      for (int off = kWave / 2; off >= LR; off >>= 1)
#pragma unroll
        for (int k = 0; k < NC; ++k) acc[k] += __shfl_xor(acc[k], off);
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int c = col_of<VEC, LR>(lane, k);
        if (lane < LR && c < fout) o[c] = acc[k] * scale;
        acc[k] = 0.0f;
      }
    };
    const int steps = (fin + RS - 1) / RS;
    for (int t = 0; t < n; ++t) {
      const int r = __builtin_amdgcn_readlane(my_row, t);
      const int64_t u = __builtin_amdgcn_readlane(my_col, t), e = __builtin_amdgcn_readlane(my_eid, t);
      if (r != cur) {
        flush();
        cur = r;
        cont = false;
      }
      wave_lds_sync();  // the last position's reads are done
      for (int i = lane; i < fin; i += kWave) slot[i] = a.x[u * fin + i];
      wave_lds_sync();
      const float* wp = a.w + e * fin * fout;
      for (int j0 = 0; j0 < steps; j0 += U) {
        float wv[U][NC], xv[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {
          const int row = (j0 + q) * RS + rg;
          const bool ok = row < fin;
          load_cols<VEC, NC>(wp + (j0 + q) * RS * fout, loff, lane, fout, ok, wv[q]);
          xv[q] = ok ? slot[row] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < U; ++q)
#pragma unroll
          for (int k = 0; k < NC; ++k) acc[k] += xv[q] * wv[q][k];
      }
    }
    flush();
  }
  fill_empty_rows(a.indptr, a.num_rows, chunk, nchunks, kWave, lane, [&](int64_t r) {
    for (int c = lane; c < fout; c += kWave) a.out[r * fout + c] = 0.0f;
  });
}

// folds a cut row's carries into its head in chunk order, then the row scale
__global__ void __launch_bounds__(kBlock) k_nnconv_fixup(NnconvArgs a) {
  fixup_float_records(a, a.indptr, (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave, a.rec,
                      threadIdx.x & (kWave - 1));
}

// v[0..N) per lane, summed over the lanes that differ in the bits OFF, OFF / 2, .. 1: while
// a lane keeps more than one value each step pairs lanes and halves what they keep (the
// lane with the bit set keeps the upper half; `base` follows the first kept index), then
// plain xor steps.  Afterwards v[0 .. max(N / lanes, 1)) are the sums of base, base + 1, ..
template <int N, int OFF>
__device__ __forceinline__ void group_sum_transposed(float (&v)[kNnAccTile], int lane, int& base) {
  if constexpr (OFF >= 1) {
    if constexpr (N > 1) {
      const bool hi = (lane & OFF) != 0;
#pragma unroll
      for (int i = 0; i < N / 2; ++i) {
        const float send = hi ? v[i] : v[i + N / 2];
        const float keep = hi ? v[i + N / 2] : v[i];
        v[i] = keep + __shfl_xor(send, OFF);
      }
      if (hi) base += N / 2;
      group_sum_transposed<N / 2, OFF / 2>(v, lane, base);
    } else {
      v[0] += __shfl_xor(v[0], OFF);
      group_sum_transposed<1, OFF / 2>(v, lane, base);
    }
  }
}

template <bool VEC, int LR, int NC, bool DX, bool DW>
__global__ void __launch_bounds__(kBlock) k_nnconv_backward(NnconvArgs a) {
  constexpr int RS = kWave / LR;
  constexpr int AJ = kNnAccTile;
  constexpr int U = VEC ? 4 : (NC >= 4 ? 2 : 4);
  constexpr int CNT = AJ >= LR ? AJ / LR : 1;           // sums a lane holds after the butterfly
  constexpr int WMASK = LR > AJ ? LR / AJ - 1 : 0;      // lanes that hold them: (lane & WMASK) == 0
  extern __shared__ float lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int fin = a.fin, fout = a.fout;
  const int64_t CH = a.chunk;
  const int64_t chunk = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  const int64_t nchunks = nnconv_chunks(a.nnz, CH);
  if (chunk >= nchunks) return;
  float* slot = lds + wave * fin;  // x[u, :] of the current row (DW)
  const int rg = lane / LR;
  const unsigned loff = lane_offset<VEC>(lane);
  const int i0 = blockIdx.y * (AJ * RS);  // this tile's rows of W: i0 .. i0 + AJ RS
  const int left = (fin - i0 + RS - 1) / RS;
  const int nst = left < AJ ? left : AJ;
  float acc[AJ];
#pragma unroll
  for (int j = 0; j < AJ; ++j) acc[j] = 0.0f;
  const int64_t p0 = chunk * CH;
  if (p0 < a.nnz) {
    const int64_t p1 = p0 + CH < a.nnz ? p0 + CH : a.nnz;
    const int n = static_cast<int>(p1 - p0);
    if (DX && blockIdx.y == 0) seg_reset(a.seg_cnt, chunk, lane);
    const int64_t pl = p0 + (lane < n ? lane : n - 1);
    const int my_row = a.rows[pl], my_col = a.cols[pl], my_eid = a.eids[pl];
    int64_t cur = __builtin_amdgcn_readlane(my_row, 0);
    bool cont = p0 > 0 && a.rows[p0 - 1] == cur;
    auto flush = [&]() {
      if constexpr (DX) {
        float* o = cont ? a.carry + chunk * fin : a.out + cur * fin;
        int base = 0;
        group_sum_transposed<AJ, LR / 2>(acc, lane, base);
#pragma unroll
        for (int i = 0; i < CNT; ++i) {
          const int row = i0 + (base + i) * RS + rg;
          if ((lane & WMASK) == 0 && row < fin) o[row] = acc[i];
        }
#pragma unroll
        for (int j = 0; j < AJ; ++j) acc[j] = 0.0f;
      }
    };
    auto stage = [&]() {
      if constexpr (DW) {
        wave_lds_sync();
        for (int i = lane; i < fin; i += kWave) slot[i] = a.x[cur * fin + i];
        wave_lds_sync();
      }
    };
    stage();
    for (int t = 0; t < n; ++t) {
      const int r = __builtin_amdgcn_readlane(my_row, t);
      const int64_t v = __builtin_amdgcn_readlane(my_col, t), e = __builtin_amdgcn_readlane(my_eid, t);
      if (r != cur) {
        flush();
        cur = r;
        cont = false;
        stage();
      }
      const float sc = a.row_scale ? a.row_scale[v] : 1.0f;
      float gs[NC];
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int c = col_of<VEC, LR>(lane, k);
        gs[k] = c < fout ? a.g[v * fout + c] * sc : 0.0f;
      }
      // the tile's first row of W[e] and dW[e]
      const float* wp = DX ? a.w + (e * fin + i0) * fout : nullptr;
      float* dwp = DW ? a.dw + (e * fin + i0) * fout : nullptr;
#pragma unroll
      for (int jb = 0; jb < AJ; jb += U) {
        if (jb < nst) {  // wave-uniform
          float wv[U][NC];
          if constexpr (DX) {
#pragma unroll
            for (int q = 0; q < U; ++q) {
              const int row = i0 + (jb + q) * RS + rg;
              load_cols<VEC, NC>(wp + (jb + q) * RS * fout, loff, lane, fout,
                                 jb + q < nst && row < fin, wv[q]);
            }
          }
#pragma unroll
          for (int q = 0; q < U; ++q) {
            const int row = i0 + (jb + q) * RS + rg;
            const bool ok = jb + q < nst && row < fin;
            if constexpr (DX) {
              float d = wv[q][0] * gs[0];
#pragma unroll
              for (int k = 1; k < NC; ++k) d += wv[q][k] * gs[k];
              acc[jb + q] += d;
            }
            if constexpr (DW) {
              const float xr = ok ? slot[row] : 0.0f;
              float o[NC];
#pragma unroll
              for (int k = 0; k < NC; ++k) o[k] = xr * gs[k];
              store_cols<VEC, NC>(dwp + (jb + q) * RS * fout, loff, lane, fout, ok, o);
            }
          }
        }
      }
    }
    flush();
  }
  if (DX && blockIdx.y == 0)
    fill_empty_rows(a.indptr, a.num_rows, chunk, nchunks, kWave, lane, [&](int64_t r) {
      for (int c = lane; c < fin; c += kWave) a.out[r * fin + c] = 0.0f;
    });
}

unsigned blocks_of(const NnconvArgs& a) {
  return static_cast<unsigned>((nnconv_chunks(a.nnz, a.chunk) + kWavesPerBlock - 1) / kWavesPerBlock);
}

template <bool VEC, int LR, int NC>
void launch_inst(bool backward, const NnconvArgs& a, hipStream_t s) {
  const size_t lds = sizeof(float) * static_cast<size_t>(kWavesPerBlock * a.fin);
  if (!backward) {
    hipLaunchKernelGGL((k_nnconv_aggregate<VEC, LR, NC>), dim3(blocks_of(a)), dim3(kBlock), lds, s, a);
    return;
  }
  const int tile = kNnAccTile * (kWave / LR);
  const dim3 grid(blocks_of(a), static_cast<unsigned>((a.fin + tile - 1) / tile));
  if (a.out != nullptr && a.dw != nullptr)
    hipLaunchKernelGGL((k_nnconv_backward<VEC, LR, NC, true, true>), grid, dim3(kBlock), lds, s, a);
  else if (a.out != nullptr)
    hipLaunchKernelGGL((k_nnconv_backward<VEC, LR, NC, true, false>), grid, dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL((k_nnconv_backward<VEC, LR, NC, false, true>), grid, dim3(kBlock), lds, s, a);
}

void launch_shape(bool backward, const NnconvArgs& a, hipStream_t s) {
  if (a.vec) {
    switch (nnconv_row_lanes(a.fout)) {
      case 1: launch_inst<true, 1, 4>(backward, a, s); break;
      case 2: launch_inst<true, 2, 4>(backward, a, s); break;
      case 4: launch_inst<true, 4, 4>(backward, a, s); break;
      case 8: launch_inst<true, 8, 4>(backward, a, s); break;
      case 16: launch_inst<true, 16, 4>(backward, a, s); break;
      case 32: launch_inst<true, 32, 4>(backward, a, s); break;
      default: launch_inst<true, 64, 4>(backward, a, s); break;
    }
  } else if (a.fout <= kWave) {
    launch_inst<false, 64, 1>(backward, a, s);
  } else if (a.fout <= 2 * kWave) {
    launch_inst<false, 64, 2>(backward, a, s);
  } else {
    launch_inst<false, 64, 4>(backward, a, s);
  }
}

void launch_fixup(const NnconvArgs& a, hipStream_t s) {
  if (a.nnz > a.chunk) hipLaunchKernelGGL(k_nnconv_fixup, dim3(blocks_of(a)), dim3(kBlock), 0, s, a);
}

}  // namespace

void launch_nnconv_aggregate(const NnconvArgs& a, hipStream_t s) {
  if (a.num_rows == 0) return;
  launch_shape(false, a, s);
  launch_fixup(a, s);
}

// a.out = dx or NULL, a.dw = dW or NULL, a.row_scale per destination (the walk's columns)
void launch_nnconv_backward(const NnconvArgs& a, hipStream_t s) {
  if (a.out == nullptr && (a.dw == nullptr || a.nnz == 0)) return;
  if (a.out != nullptr && a.num_rows == 0) return;
  launch_shape(true, a, s);
  if (a.out != nullptr) {
    NnconvArgs f = a;
    f.row_scale = nullptr;  // already in gs
    launch_fixup(f, s);
  }
}

}  // namespace dglmi
