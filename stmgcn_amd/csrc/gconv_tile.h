// Tile primitives shared by the fused graph-convolution kernels
// (cheb_gconv.hip, dual_gconv.hip) — CDNA4 (gfx950). Included by .hip files
// only: the device primitives, and the launchers' slot-size / dispatch helpers.
//
// A workgroup of 256 threads owns GC_ST graph-node rows of one batch element.
// A tile of up to 64 channels lives in one LDS slot, either as bf16/f16 in the
// lds_swz layout feeding v_mfma_f32_16x16x32 fragments (MF) or as fp32 with a
// 64-float row stride for the scalar path (!MF: fp32 parity and channel counts
// that are not MFMA-tileable). The .hip files hold only their kernels' control
// flow and launchers; everything a second support kind would share is here.
#pragma once
#include <type_traits>

#include "common.h"

constexpr int GC_ST = 32;  // graph-node rows per workgroup tile

// (Frag8, f32x4 and mfma16x16x32 come from common.h.)

// ---- host side: one definition of slot sizes and MFMA eligibility ---------
// Each launcher uses these for both its dispatch and its LDS byte count.
constexpr int gc_slot_bytes(bool mf) { return mf ? GC_ST * 128 : GC_ST * 64 * 4; }
constexpr int GC_F32_TILE_BYTES = gc_slot_bytes(false);  // fp32 U tile (bwd)

// forward mix: K = C in 32-chunks, 16 output columns per wave
template <typename T> inline bool gc_fwd_mfma(int C, int Cout) {
  return !std::is_same<T, float>::value && C % 32 == 0 && Cout % 16 == 0;
}
// backward U = dz @ W^T: K = Cout in 32-chunks, 16 U columns per wave (4 waves)
template <typename T> inline bool gc_bwd_mfma(int C, int Cout) {
  return !std::is_same<T, float>::value && Cout % 32 == 0 && C % 16 == 0 && C <= 64;
}

inline dim3 gc_grid(int N, int B) { return dim3((N + GC_ST - 1) / GC_ST, B); }

// f(std::true_type) when the MFMA variant serves, f(std::false_type) otherwise;
// fp32 never instantiates the MFMA variant.
template <typename T, typename F> void gc_dispatch_mf(bool mf, F&& f) {
  if constexpr (!std::is_same<T, float>::value) {
    if (mf) { f(std::true_type{}); return; }
  }
  f(std::false_type{});
}

// ---- device side ----------------------------------------------------------

// (G @ xb)[row, c] over row-major xb with row_stride elements between rows.
// An empty row (rowptr[row] == rowptr[row + 1], e.g. a node without in-edges)
// runs neither loop -> 0. 4-wide unroll: the col/val loads and the x gathers
// of a chunk issue together instead of forming one serial load-latency chain
// per nnz; the scalar tail is mul+add (not fmaf) — kept for bit parity.
template <typename T>
__device__ __forceinline__ float gc_gather(const StmCsr g, const T* xb, int row,
                                           long row_stride, int c) {
  float acc = 0.f;
  const int s = g.rowptr[row], e = g.rowptr[row + 1];
  int j = s;
  for (; j + 4 <= e; j += 4) {
    int cc[4];
    float vv[4];
    #pragma unroll
    for (int k = 0; k < 4; ++k) { cc[k] = g.colidx[j + k]; vv[k] = g.vals[j + k]; }
    float xv[4];
    #pragma unroll
    for (int k = 0; k < 4; ++k) xv[k] = toF<T>(xb[(long)cc[k] * row_stride + c]);
    #pragma unroll
    for (int k = 0; k < 4; ++k) acc = fmaf(vv[k], xv[k], acc);
  }
  for (; j < e; ++j) acc += g.vals[j] * toF<T>(xb[(long)g.colidx[j] * row_stride + c]);
  return acc;
}

// fp32 view of a !MF slot (and of the fp32 U tiles): element (rl, c)
__device__ __forceinline__ float& gc_f32(void* slot, int rl, int c) {
  return ((float*)slot)[rl * 64 + c];
}
__device__ __forceinline__ float gc_f32(const void* slot, int rl, int c) {
  return ((const float*)slot)[rl * 64 + c];
}

// store tile element (rl, c) into an LDS slot
template <typename T, bool MF>
__device__ __forceinline__ void gc_tile_store(char* slot, int rl, int c, float v) {
  if constexpr (MF) *(T*)&slot[lds_swz(rl, c * 2)] = fromF<T>(v);
  else gc_f32(slot, rl, c) = v;
}

// lane coordinates of the 16x16x32 fragments: wave wv owns 16 output columns
struct GcLane {
  int wv, l16, lgrp;
  __device__ __forceinline__ GcLane()
      : wv(threadIdx.x >> 6), l16(threadIdx.x & 15), lgrp((threadIdx.x & 63) >> 4) {}
};

// MFMA mix pass: acc (2 x 16 rows) += slot-tile @ W[kofs:kofs+C, 16wv:16wv+16].
// slot (LDS) and W (global) never alias and neither is written here; without
// the __restrict__ the two-pass ChebConv forward allocates 47 VGPRs, not 41.
template <typename T>
__device__ __forceinline__ void gc_mix_mfma(const char* __restrict__ slot,
                                            const T* __restrict__ W, int kofs, int C,
                                            int Cout, GcLane l, f32x4* acc) {
  using frag = typename Frag8<T>::type;
  using elem = typename Frag8<T>::elem;
  for (int kk = 0; kk < (C >> 5); ++kk) {
    frag bfr;
    #pragma unroll
    for (int j = 0; j < 8; ++j)
      ((elem*)&bfr)[j] =
          *(const elem*)&W[(kofs + kk * 32 + l.lgrp * 8 + j) * Cout + 16 * l.wv + l.l16];
    frag a0 = *(const frag*)&slot[lds_swz(l.l16, (kk * 32 + l.lgrp * 8) * 2)];
    frag a1 = *(const frag*)&slot[lds_swz(16 + l.l16, (kk * 32 + l.lgrp * 8) * 2)];
    acc[0] = mfma16x16x32(a0, bfr, acc[0]);
    acc[1] = mfma16x16x32(a1, bfr, acc[1]);
  }
}

// scalar mix pass: v += slot-tile[rl, :] @ W[kofs:kofs+C, co]
template <typename T>
__device__ __forceinline__ float gc_mix_scalar(const char* slot, const T* W, int kofs,
                                               int C, int Cout, int rl, int co, float v) {
  for (int c = 0; c < C; ++c)
    v = fmaf(gc_f32(slot, rl, c), toF<T>(W[(kofs + c) * Cout + co]), v);
  return v;
}

// y epilogue of one element: v (+= yacc unless first); the last step writes
// yout = act(v + bias), every other step parks v in the fp32 yacc.
template <typename T>
__device__ __forceinline__ void gc_y_store(float v, long idx, int col, const T* bias,
                                           float* yacc, T* yout, int first, int act) {
  if (!first) v += yacc[idx];
  if (yout != nullptr) {
    if (bias != nullptr) v += toF<T>(bias[col]);
    if (act == 1 && v < 0.f) v = 0.f;
    yout[idx] = fromF<T>(v);
  } else {
    yacc[idx] = v;
  }
}

// y epilogue of a wave's MFMA accumulator pair (D-fragment row ownership)
template <typename T>
__device__ __forceinline__ void gc_y_store_frag(const f32x4* acc, int b, int n0,
                                                int N, int Cout, GcLane l,
                                                const T* bias, float* yacc, T* yout,
                                                int first, int act) {
  #pragma unroll
  for (int m = 0; m < 2; ++m)
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = n0 + 16 * m + 4 * l.lgrp + r;
      if (row < N)
        gc_y_store<T>(acc[m][r], ((long)b * N + row) * Cout + 16 * l.wv + l.l16,
                      16 * l.wv + l.l16, bias, yacc, yout, first, act);
    }
}

// stage rows [n0, n0 + GC_ST) of dzb (N, Cout) into an LDS slot, zero-padded
template <typename T, bool MF>
__device__ __forceinline__ void gc_stage_dz(char* dzt, const T* dzb, int n0, int N,
                                            int Cout) {
  for (int i = threadIdx.x; i < GC_ST * Cout; i += 256) {
    const int co = i % Cout, rl = i / Cout;
    const int row = n0 + rl;
    const float v = (row < N) ? toF<T>(dzb[(long)row * Cout + co]) : 0.f;
    gc_tile_store<T, MF>(dzt, rl, co, v);
  }
}

// U-tile[row][c] = sum_co dz[row][co] * W[kofs + c][co], fp32 into ut (stride 64)
template <typename T, bool MF>
__device__ __forceinline__ void gc_u_pass(const char* dzt, const T* W, int kofs, int C,
                                          int Cout, float* ut) {
  if constexpr (MF) {
    using frag = typename Frag8<T>::type;
    const GcLane l;
    if (l.wv < (C >> 4)) {             // wave wv owns U cols [16wv, 16wv+16)
      f32x4 acc[2];
      acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kk = 0; kk < (Cout >> 5); ++kk) {
        // W_j^T[co][c] = W[kofs + c][co] -> 8 consecutive co per lane: one load
        frag bfr =
            *(const frag*)&W[(kofs + 16 * l.wv + l.l16) * Cout + kk * 32 + l.lgrp * 8];
        frag a0 = *(const frag*)&dzt[lds_swz(l.l16, (kk * 32 + l.lgrp * 8) * 2)];
        frag a1 = *(const frag*)&dzt[lds_swz(16 + l.l16, (kk * 32 + l.lgrp * 8) * 2)];
        acc[0] = mfma16x16x32(a0, bfr, acc[0]);
        acc[1] = mfma16x16x32(a1, bfr, acc[1]);
      }
      #pragma unroll
      for (int m = 0; m < 2; ++m)
        #pragma unroll
        for (int r = 0; r < 4; ++r)
          gc_f32(ut, 16 * m + 4 * l.lgrp + r, 16 * l.wv + l.l16) = acc[m][r];
    }
  } else {
    for (int i = threadIdx.x; i < GC_ST * C; i += 256) {
      const int c = i % C, rl = i / C;
      float v = 0.f;
      for (int co = 0; co < Cout; ++co)
        v = fmaf(gc_f32(dzt, rl, co), toF<T>(W[(kofs + c) * Cout + co]), v);
      gc_f32(ut, rl, c) = v;
    }
  }
}
