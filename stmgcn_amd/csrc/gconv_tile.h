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
//
// Thread mapping of the gather phases (forward phase 1, backward phase C):
// when C is a multiple of 8 from 16 up (gc_vec8) a thread owns one (row,
// 8-channel group) unit, so at C = 64 the 32-row tile is one unit per thread
// (the backward issues its gather before the dz staging and holds the result
// in registers, the forward fetches its W fragments and yacc first): x, p1, x0 and the
// outputs move as 16-byte vectors (two for fp32), a row's colidx/vals are read
// once per 8-lane group (the 8 lanes name the same words) in blocks of 6 nnz
// with the next block's indices already in flight, and the tile goes into the
// LDS slot with one 16-byte store. Any other C keeps one (row, channel)
// element per thread (gc_gather). Both mappings run the same per-element
// arithmetic in the same order, so they give the same bits.
#pragma once
#include <cstdint>
#include <initializer_list>
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

// The 8-channel vector mapping serves a channel count that is a multiple of 8
// when every (B, N, C) tensor the gather phase touches is 16-byte aligned (null
// pointers pass); anything else takes the element-wise mapping. So does C = 8:
// its tile is one element per thread, a single pass already, and with one
// unit per row only 32 of the 256 threads would work. The temporal gconv
// (7.2 - 8.0 us) measured no faster with the vector mapping.
// N * C < 2^31: gc_gather8 indexes a batch slice with 32-bit element offsets.
inline bool gc_vec8(int N, int C, std::initializer_list<const void*> ptrs) {
  if (C % 8 != 0 || C < 16 || (long)N * C >= (1L << 31)) return false;
  for (const void* p : ptrs)
    if (((uintptr_t)p & 15) != 0) return false;
  return true;
}

// f(std::true_type) when the MFMA variant serves, f(std::false_type) otherwise;
// fp32 never instantiates the MFMA variant.
template <typename T, typename F> const char* gc_dispatch_mf(bool mf, F&& f) {
  if constexpr (!std::is_same<T, float>::value) {
    if (mf) return f(std::true_type{});
  }
  return f(std::false_type{});
}

// ---- device side ----------------------------------------------------------

// (G @ xb)[row, c] over row-major xb with row_stride elements between rows.
// An empty row (rowptr[row] == rowptr[row + 1], e.g. a node without in-edges)
// runs neither loop -> 0. 4-wide unroll: the col/val loads and the x gathers
// of a chunk issue together instead of forming one serial load-latency chain
// per nnz. Every nnz is one fmaf in CSR order, the tail included (written
// `acc += v * x` it was always contracted to that), so gc_gather8 below, which
// blocks the same chain differently, gives the same bits.
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
  for (; j < e; ++j)
    acc = fmaf(g.vals[j], toF<T>(xb[(long)g.colidx[j] * row_stride + c]), acc);
  return acc;
}

// ---- 8-channel vector forms (C % 8 == 0, 16-byte aligned tensors) ----------
// 8 consecutive channels as they lie in memory: one 16-byte word of bf16/f16,
// two of fp32. Kept raw while the load is in flight, turned to fp32 at the use.
template <typename T> struct GcRaw8 { uint4 q[sizeof(T) / 2]; };

template <typename T>
__device__ __forceinline__ GcRaw8<T> gc_load8(const T* p) {
  GcRaw8<T> r;
  #pragma unroll
  for (int i = 0; i < (int)sizeof(T) / 2; ++i) r.q[i] = ((const uint4*)p)[i];
  return r;
}
template <typename T>
__device__ __forceinline__ void gc_unpack8(const GcRaw8<T>& r, float (&v)[8]) {
  union { GcRaw8<T> r; T t[8]; } u;
  u.r = r;
  #pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = toF<T>(u.t[j]);
}
template <typename T>
__device__ __forceinline__ GcRaw8<T> gc_pack8(const float (&v)[8]) {
  union { GcRaw8<T> r; T t[8]; } u;
  #pragma unroll
  for (int j = 0; j < 8; ++j) u.t[j] = fromF<T>(v[j]);
  return u.r;
}
template <typename T>
__device__ __forceinline__ void gc_store8(T* p, const float (&v)[8]) {
  const GcRaw8<T> r = gc_pack8<T>(v);
  #pragma unroll
  for (int i = 0; i < (int)sizeof(T) / 2; ++i) ((uint4*)p)[i] = r.q[i];
}

// acc[0..8) = (G @ xb)[row, c .. c + 8) over row-major xb with C channels per
// row: gc_gather's fmaf chain for each of the 8 channels, nnz in CSR order.
// Blocks of NB nnz: the NB x rows of a block are loaded together, and the next
// block's colidx/vals are requested before the block's arithmetic, so a row of
// d nnz costs 2 + ceil(d / NB) dependent round trips (rowptr, first indices,
// then one per block) instead of two per 4 nnz plus two per tail nnz. Slots
// past the row's end re-read its last entry (a valid address) and are masked
// out of the arithmetic. NB = 6 for bf16/f16 (4 for fp32, whose rows are
// twice as wide) is what keeps every kernel that calls this inside 128 VGPRs
// without scratch, i.e. at four workgroups per CU, which is the whole
// (N = 1024, B = 32) grid in one round; 8 spilled in the MFMA forward.
// xb is the workgroup's batch slice (a uniform base); element offsets inside
// it fit 32 bits (gc_vec8 admits N * C < 2^31 only).
template <typename T, int NB = (sizeof(T) == 4 ? 4 : 6)>
__device__ __forceinline__ void gc_gather8(const StmCsr g, const T* xb, int row, int C,
                                           int c, float (&acc)[8]) {
  #pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = 0.f;
  const int s = g.rowptr[row], e = g.rowptr[row + 1];
  if (s >= e) return;
  unsigned xo[NB];   // element offset of the x row's 8 channels
  float vv[NB];
  #pragma unroll
  for (int k = 0; k < NB; ++k) {
    const int jj = min(s + k, e - 1);
    xo[k] = (unsigned)g.colidx[jj] * (unsigned)C + (unsigned)c;
    vv[k] = g.vals[jj];
  }
  for (int j = s; j < e; j += NB) {
    GcRaw8<T> xr[NB];
    #pragma unroll
    for (int k = 0; k < NB; ++k) xr[k] = gc_load8<T>(xb + xo[k]);
    const int rem = e - j;
    float vc[NB];
    #pragma unroll
    for (int k = 0; k < NB; ++k) vc[k] = vv[k];
    if (rem > NB) {
      #pragma unroll
      for (int k = 0; k < NB; ++k) {
        const int jj = min(j + NB + k, e - 1);
        xo[k] = (unsigned)g.colidx[jj] * (unsigned)C + (unsigned)c;
        vv[k] = g.vals[jj];
      }
    }
    #pragma unroll
    for (int k = 0; k < NB; ++k) {
      if (k < rem) {
        float xv[8];
        gc_unpack8<T>(xr[k], xv);
        #pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = fmaf(vc[k], xv[q], acc[q]);
      }
    }
  }
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

// store 8 consecutive channels (rl, c .. c + 8), c % 8 == 0: one 16-byte store
// into the lds_swz image (the XOR moves whole 16-byte windows), two into fp32
template <typename T, bool MF>
__device__ __forceinline__ void gc_tile_store8(char* slot, int rl, int c,
                                               const float (&v)[8]) {
  if constexpr (MF) {
    *(uint4*)&slot[lds_swz(rl, c * 2)] = gc_pack8<T>(v).q[0];
  } else {
    float4* d = (float4*)&gc_f32(slot, rl, c);
    d[0] = float4{v[0], v[1], v[2], v[3]};
    d[1] = float4{v[4], v[5], v[6], v[7]};
  }
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
//
// The W B-fragments of a pass (GcMixB: C <= 64, so two K-chunks) are fetched
// by gc_mix_load before the gather phase, so their L2 round trip runs under
// the gather instead of after the barrier. A lane's 8 k-values of one output
// column are Cout elements apart in the row-major W, so they stay 8 two-byte
// loads: no wider load holds two of them.
template <typename T> struct GcMixB { typename Frag8<T>::type b[2]; };

template <typename T>
__device__ __forceinline__ GcMixB<T> gc_mix_load(const T* __restrict__ W, int kofs,
                                                 int C, int Cout, GcLane l) {
  using elem = typename Frag8<T>::elem;
  GcMixB<T> m = {};
  #pragma unroll
  for (int kk = 0; kk < 2; ++kk)
    if (kk < (C >> 5)) {
      #pragma unroll
      for (int j = 0; j < 8; ++j)
        ((elem*)&m.b[kk])[j] =
            *(const elem*)&W[(kofs + kk * 32 + l.lgrp * 8 + j) * Cout + 16 * l.wv + l.l16];
    }
  return m;
}

template <typename T>
__device__ __forceinline__ void gc_mix_mfma(const char* __restrict__ slot,
                                            const GcMixB<T>& m, int C, GcLane l,
                                            f32x4* acc) {
  using frag = typename Frag8<T>::type;
  #pragma unroll
  for (int kk = 0; kk < 2; ++kk)
    if (kk < (C >> 5)) {
      frag a0 = *(const frag*)&slot[lds_swz(l.l16, (kk * 32 + l.lgrp * 8) * 2)];
      frag a1 = *(const frag*)&slot[lds_swz(16 + l.l16, (kk * 32 + l.lgrp * 8) * 2)];
      acc[0] = mfma16x16x32(a0, m.b[kk], acc[0]);
      acc[1] = mfma16x16x32(a1, m.b[kk], acc[1]);
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

// What the y epilogue of a wave's accumulator pair reads back: the parked yacc
// values of its 8 elements (unless first) and its column's bias (last step).
// Fetched with the W fragments, before the gather phase.
struct GcYPrev { f32x4 y[2]; float bias; };

template <typename T>
__device__ __forceinline__ GcYPrev gc_y_prefetch(int b, int n0, int N, int Cout,
                                                 GcLane l, const T* bias,
                                                 const float* yacc, const T* yout,
                                                 int first) {
  GcYPrev p;
  p.y[0] = f32x4{0.f, 0.f, 0.f, 0.f};
  p.y[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  p.bias = (yout != nullptr && bias != nullptr) ? toF<T>(bias[16 * l.wv + l.l16]) : 0.f;
  if (!first) {
    #pragma unroll
    for (int m = 0; m < 2; ++m)
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n0 + 16 * m + 4 * l.lgrp + r;
        if (row < N) p.y[m][r] = yacc[((long)b * N + row) * Cout + 16 * l.wv + l.l16];
      }
  }
  return p;
}

// y epilogue of a wave's MFMA accumulator pair (D-fragment row ownership):
// gc_y_store's arithmetic on the prefetched values
template <typename T>
__device__ __forceinline__ void gc_y_store_frag(const f32x4* acc, const GcYPrev& p,
                                                int b, int n0, int N, int Cout,
                                                GcLane l, const T* bias, float* yacc,
                                                T* yout, int first, int act) {
  #pragma unroll
  for (int m = 0; m < 2; ++m)
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = n0 + 16 * m + 4 * l.lgrp + r;
      if (row >= N) continue;
      const long idx = ((long)b * N + row) * Cout + 16 * l.wv + l.l16;
      float v = acc[m][r];
      if (!first) v += p.y[m][r];
      if (yout != nullptr) {
        if (bias != nullptr) v += p.bias;
        if (act == 1 && v < 0.f) v = 0.f;
        yout[idx] = fromF<T>(v);
      } else {
        yacc[idx] = v;
      }
    }
}

// stage rows [n0, n0 + GC_ST) of dzb (N, Cout) into an LDS slot, zero-padded;
// vec (Cout % 8 == 0, dzb 16-byte aligned): one 8-channel unit per thread
template <typename T, bool MF>
__device__ __forceinline__ void gc_stage_dz(char* dzt, const T* dzb, int n0, int N,
                                            int Cout, bool vec) {
  if (vec) {
    const int G = Cout >> 3;
    for (int u = threadIdx.x; u < GC_ST * G; u += 256) {
      const int rl = u / G, co = (u % G) * 8;
      const int row = n0 + rl;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (row < N) gc_unpack8<T>(gc_load8<T>(&dzb[(long)row * Cout + co]), v);
      gc_tile_store8<T, MF>(dzt, rl, co, v);
    }
    return;
  }
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
