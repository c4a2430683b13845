// Dual random-walk diffusion graph convolution on CSR — CDNA4 (gfx950).
//
// The bidirectional diffusion convolution (Li et al., ICLR'18) mixes 2K+1
// supports: I, T_1..T_K of the forward generator G_f = (D_out^-1 A)^T and
// T_1..T_K of the backward generator G_b = (D_in^-1 A^T)^T. Weight rows:
// [0,C) -> T_0, [kC,(k+1)C) -> T_k(G_f), [(K+k)C,(K+k+1)C) -> T_k(G_b).
//
// These step kernels are the two-generator siblings of cheb_fused_fwd_kernel /
// cheb_fused_bwd_kernel (cheb_gconv.hip): same 32-row tile, 256-thread
// workgroups, lds_swz staging and v_mfma_f32_16x16x32 fragments, but one
// launch advances BOTH recurrences and folds both mixes into one accumulator
// pair, so K launches serve 2K+1 supports with K-1 passes over the fp32 yacc
// (K == 1 needs no yacc at all). The backward runs both Clenshaw chains per
// launch from a single staged dz tile: K+1 launches instead of 2(K+1).

#include <type_traits>

#include "common.h"

#define DG_ST 32  // graph-node rows per workgroup tile

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 dg_bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 dg_f16x8;
typedef __attribute__((ext_vector_type(4))) float dg_f32x4;

template <typename T> struct DFrag8 { using type = float; using elem = float; };
template <> struct DFrag8<__hip_bfloat16> { using type = dg_bf16x8; using elem = __bf16; };
template <> struct DFrag8<__half> { using type = dg_f16x8; using elem = _Float16; };

__device__ __forceinline__ dg_f32x4 dg_mfma(dg_bf16x8 a, dg_bf16x8 b, dg_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ dg_f32x4 dg_mfma(dg_f16x8 a, dg_f16x8 b, dg_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// CSR generator (or its transpose)
struct DgCsr {
  const int* rowptr;
  const int* colidx;
  const float* vals;
};

// (G @ xb)[row, c] over (N, C) row-major xb. An empty row (rowptr[row] ==
// rowptr[row + 1], e.g. a node without in-edges) runs neither loop -> 0; the
// two generators are walked independently, so a row may be empty in one
// direction only. 4-wide unroll + scalar tail as in cheb_gconv.hip.
template <typename T>
__device__ __forceinline__ float dg_gather(const DgCsr g, const T* xb, int row,
                                           int C, int c) {
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
    for (int k = 0; k < 4; ++k) xv[k] = toF<T>(xb[(long)cc[k] * C + c]);
    #pragma unroll
    for (int k = 0; k < 4; ++k) acc = fmaf(vv[k], xv[k], acc);
  }
  for (; j < e; ++j) acc += g.vals[j] * toF<T>(xb[(long)g.colidx[j] * C + c]);
  return acc;
}

// y-tile += A-tile (LDS slot, lds_swz layout) @ W[kofs:kofs+C, 16wv:16wv+16]
template <typename T>
__device__ __forceinline__ void dg_mix_pass(const char* slot, const T* W,
                                            int kofs, int C, int Cout, int wv,
                                            int l16, int lgrp, dg_f32x4* acc) {
  using frag = typename DFrag8<T>::type;
  using elem = typename DFrag8<T>::elem;
  for (int kk = 0; kk < (C >> 5); ++kk) {
    frag bfr;
    #pragma unroll
    for (int j = 0; j < 8; ++j)
      ((elem*)&bfr)[j] =
          *(const elem*)&W[(kofs + kk * 32 + lgrp * 8 + j) * Cout + 16 * wv + l16];
    frag a0 = *(const frag*)&slot[lds_swz(l16, (kk * 32 + lgrp * 8) * 2)];
    frag a1 = *(const frag*)&slot[lds_swz(16 + l16, (kk * 32 + lgrp * 8) * 2)];
    acc[0] = dg_mfma(a0, bfr, acc[0]);
    acc[1] = dg_mfma(a1, bfr, acc[1]);
  }
}

// One fused forward step k over (B, N, C) states, both directions:
//   pf_k = alpha * (G_f @ xf)[rows] + beta * pf1[rows]    (pf1 optional)
//   pb_k = alpha * (G_b @ xb)[rows] + beta * pb1[rows]
//   acc  = pf_k @ W[kofs_f:+C] + pb_k @ W[kofs_b:+C]  (+ x0 @ W[0:C] at k = 1)
//   yacc (+)= acc, or on the last step yout = act(yacc + acc + bias)
// pf1/pb1 are read only at the thread's own (row, c) element before that
// element of pfout/pbout is written, so pf1 == pfout (pb1 == pbout) aliasing
// is safe per direction; the gather operands must be distinct buffers.
template <typename T, bool MF>
__global__ void __launch_bounds__(256)
dual_fused_fwd_kernel(const DgCsr gf, const DgCsr gb,
                      const T* __restrict__ xf, const T* pf1,
                      const T* __restrict__ xb, const T* pb1,
                      const T* __restrict__ x0,
                      const T* __restrict__ W, const T* __restrict__ bias,
                      T* pfout, T* pbout, float* __restrict__ yacc,
                      T* __restrict__ yout, int N, int C, int Cout,
                      int kofs_f, int kofs_b, float alpha, float beta,
                      int first, int act) {
  const int b = blockIdx.y;
  const int n0 = blockIdx.x * DG_ST;
  extern __shared__ char lds[];
  constexpr int kSlot = MF ? DG_ST * 128 : DG_ST * 64 * 4;
  char* lf = lds;                 // pf_k tile
  char* lb = lds + kSlot;         // pb_k tile
  char* l0 = lds + 2 * kSlot;     // x tile (k = 1 only)
  const long boff = (long)b * N * C;
  const T* xfb = xf + boff;
  const T* xbb = xb + boff;

  // ---- phase 1: both recurrences (SpMM + axpby), tiles staged in LDS ----
  for (int i = threadIdx.x; i < DG_ST * C; i += 256) {
    const int c = i % C, rl = i / C;
    const int row = n0 + rl;
    float af = 0.f, ab = 0.f, v0 = 0.f;
    if (row < N) {
      const long e = boff + (long)row * C + c;
      af = alpha * dg_gather<T>(gf, xfb, row, C, c);
      ab = alpha * dg_gather<T>(gb, xbb, row, C, c);
      if (pf1 != nullptr) af = fmaf(beta, toF<T>(pf1[e]), af);
      if (pb1 != nullptr) ab = fmaf(beta, toF<T>(pb1[e]), ab);
      pfout[e] = fromF<T>(af);
      pbout[e] = fromF<T>(ab);
      if (x0 != nullptr) v0 = toF<T>(x0[e]);
    }
    if (MF) {
      *(T*)&lf[lds_swz(rl, c * 2)] = fromF<T>(af);
      *(T*)&lb[lds_swz(rl, c * 2)] = fromF<T>(ab);
      if (x0 != nullptr) *(T*)&l0[lds_swz(rl, c * 2)] = fromF<T>(v0);
    } else {
      ((float*)lf)[rl * 64 + c] = af;
      ((float*)lb)[rl * 64 + c] = ab;
      if (x0 != nullptr) ((float*)l0)[rl * 64 + c] = v0;
    }
  }
  __syncthreads();

  // ---- phase 2: mix epilogue, one accumulator for all passes ----
  if constexpr (MF) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int l16 = lane & 15, lgrp = lane >> 4;
    if (wv < (Cout >> 4)) {            // wave wv owns output cols [16wv,16wv+16)
      dg_f32x4 acc[2];
      acc[0] = dg_f32x4{0.f, 0.f, 0.f, 0.f};
      acc[1] = dg_f32x4{0.f, 0.f, 0.f, 0.f};
      dg_mix_pass<T>(lf, W, kofs_f, C, Cout, wv, l16, lgrp, acc);
      dg_mix_pass<T>(lb, W, kofs_b, C, Cout, wv, l16, lgrp, acc);
      if (x0 != nullptr) dg_mix_pass<T>(l0, W, 0, C, Cout, wv, l16, lgrp, acc);
      #pragma unroll
      for (int m = 0; m < 2; ++m)
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = n0 + 16 * m + 4 * lgrp + r;
          if (row < N) {
            const long idx = ((long)b * N + row) * Cout + 16 * wv + l16;
            float v = acc[m][r];
            if (!first) v += yacc[idx];
            if (yout != nullptr) {
              if (bias != nullptr) v += toF<T>(bias[16 * wv + l16]);
              if (act == 1 && v < 0.f) v = 0.f;
              yout[idx] = fromF<T>(v);
            } else {
              yacc[idx] = v;
            }
          }
        }
    }
  } else {
    const float* ff = (const float*)lf;
    const float* fb = (const float*)lb;
    const float* f0 = (const float*)l0;
    for (int i = threadIdx.x; i < DG_ST * Cout; i += 256) {
      const int co = i % Cout, rl = i / Cout;
      const int row = n0 + rl;
      if (row >= N) continue;
      float v = 0.f;
      for (int c = 0; c < C; ++c)
        v = fmaf(ff[rl * 64 + c], toF<T>(W[(kofs_f + c) * Cout + co]), v);
      for (int c = 0; c < C; ++c)
        v = fmaf(fb[rl * 64 + c], toF<T>(W[(kofs_b + c) * Cout + co]), v);
      if (x0 != nullptr)
        for (int c = 0; c < C; ++c)
          v = fmaf(f0[rl * 64 + c], toF<T>(W[c * Cout + co]), v);
      const long idx = ((long)b * N + row) * Cout + co;
      if (!first) v += yacc[idx];
      if (yout != nullptr) {
        if (bias != nullptr) v += toF<T>(bias[co]);
        if (act == 1 && v < 0.f) v = 0.f;
        yout[idx] = fromF<T>(v);
      } else {
        yacc[idx] = v;
      }
    }
  }
}

// U-tile[row][c] = sum_co dz[row][co] * W[kofs + c][co], fp32 into ut (stride 64)
template <typename T, bool MF>
__device__ __forceinline__ void dg_u_pass(const char* dzt, const T* W, int kofs,
                                          int C, int Cout, float* ut) {
  if constexpr (MF) {
    using frag = typename DFrag8<T>::type;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int l16 = lane & 15, lgrp = lane >> 4;
    if (wv < (C >> 4)) {               // wave wv owns U cols [16wv, 16wv+16)
      dg_f32x4 acc[2];
      acc[0] = dg_f32x4{0.f, 0.f, 0.f, 0.f};
      acc[1] = dg_f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kk = 0; kk < (Cout >> 5); ++kk) {
        // W_j^T[co][c] = W[kofs + c][co] -> 8 consecutive co per lane: one load
        frag bfr = *(const frag*)&W[(kofs + 16 * wv + l16) * Cout + kk * 32 + lgrp * 8];
        frag a0 = *(const frag*)&dzt[lds_swz(l16, (kk * 32 + lgrp * 8) * 2)];
        frag a1 = *(const frag*)&dzt[lds_swz(16 + l16, (kk * 32 + lgrp * 8) * 2)];
        acc[0] = dg_mfma(a0, bfr, acc[0]);
        acc[1] = dg_mfma(a1, bfr, acc[1]);
      }
      #pragma unroll
      for (int m = 0; m < 2; ++m)
        #pragma unroll
        for (int r = 0; r < 4; ++r)
          ut[(16 * m + 4 * lgrp + r) * 64 + 16 * wv + l16] = acc[m][r];
    }
  } else {
    const float* fdz = (const float*)dzt;
    for (int i = threadIdx.x; i < DG_ST * C; i += 256) {
      const int c = i % C, rl = i / C;
      float v = 0.f;
      for (int co = 0; co < Cout; ++co)
        v = fmaf(fdz[rl * 64 + co], toF<T>(W[(kofs + c) * Cout + co]), v);
      ut[rl * 64 + c] = v;
    }
  }
}

// One fused backward (Clenshaw) step over the transposed generators.
// final == 0 (step j):
//   outf[rows] = alpha * (G_f^T @ xf)[rows] + beta * pf1[rows] + (dz @ W_j^T)[rows]
//   outb[rows] = alpha * (G_b^T @ xb)[rows] + beta * pb1[rows] + (dz @ W_{K+j}^T)[rows]
// with kofs_f = j*C, kofs_b = (K+j)*C; xf/xb null -> the chain start b_K = U_K.
// final == 1:
//   outf[rows] = (dz @ W_0^T) + alpha*(G_f^T @ xf) + beta*pf1
//                             + alpha*(G_b^T @ xb) + beta*pb1      (= dX)
// The dz tile is staged once for both U GEMMs. pf1 == outf / pb1 == outb
// aliasing is element-safe as in the forward kernel.
template <typename T, bool MF>
__global__ void __launch_bounds__(256)
dual_fused_bwd_kernel(const DgCsr gft, const DgCsr gbt,
                      const T* __restrict__ xf, const T* pf1,
                      const T* __restrict__ xb, const T* pb1,
                      const T* __restrict__ dz, const T* __restrict__ W,
                      T* outf, T* outb, int N, int C, int Cout, int kofs_f,
                      int kofs_b, float alpha, float beta, int final_step) {
  const int b = blockIdx.y;
  const int n0 = blockIdx.x * DG_ST;
  extern __shared__ char lds[];
  char* dzt = lds;
  float* utf = (float*)(lds + (MF ? DG_ST * 128 : DG_ST * 64 * 4));
  float* utb = utf + DG_ST * 64;

  // ---- phase A: stage the dz tile (once for both chains) ----
  const T* dzb = dz + (long)b * N * Cout;
  for (int i = threadIdx.x; i < DG_ST * Cout; i += 256) {
    const int co = i % Cout, rl = i / Cout;
    const int row = n0 + rl;
    const float v = (row < N) ? toF<T>(dzb[(long)row * Cout + co]) : 0.f;
    if (MF) *(T*)&dzt[lds_swz(rl, co * 2)] = fromF<T>(v);
    else ((float*)dzt)[rl * 64 + co] = v;
  }
  __syncthreads();

  // ---- phase B: U_f (and U_b) = dz @ W_j^T ----
  dg_u_pass<T, MF>(dzt, W, kofs_f, C, Cout, utf);
  if (!final_step) dg_u_pass<T, MF>(dzt, W, kofs_b, C, Cout, utb);
  __syncthreads();

  // ---- phase C: the two SpMM/axpby updates ----
  const long boff = (long)b * N * C;
  for (int i = threadIdx.x; i < DG_ST * C; i += 256) {
    const int c = i % C, rl = i / C;
    const int row = n0 + rl;
    if (row >= N) continue;
    const long e = boff + (long)row * C + c;
    float af = utf[rl * 64 + c];
    float ab = final_step ? 0.f : utb[rl * 64 + c];
    if (xf != nullptr) af = fmaf(alpha, dg_gather<T>(gft, xf + boff, row, C, c), af);
    if (xb != nullptr) ab = fmaf(alpha, dg_gather<T>(gbt, xb + boff, row, C, c), ab);
    if (pf1 != nullptr) af = fmaf(beta, toF<T>(pf1[e]), af);
    if (pb1 != nullptr) ab = fmaf(beta, toF<T>(pb1[e]), ab);
    if (final_step) {
      outf[e] = fromF<T>(af + ab);
    } else {
      outf[e] = fromF<T>(af);
      outb[e] = fromF<T>(ab);
    }
  }
}

struct DualFwdArgs {
  DgCsr gf, gb;
  const void *xf, *pf1, *xb, *pb1, *x0, *W, *bias;
  void *pfout, *pbout;
  float* yacc;
  void* yout;
  int B, N, C, Cout, kofs_f, kofs_b;
  float alpha, beta;
  int first, act;
};

// MFMA epilogue when C % 32 == 0 and Cout % 16 == 0 (as launch_fused_fwd),
// scalar epilogue otherwise. Three LDS slots: pf tile, pb tile, x tile.
template <typename T>
void launch_dual_fwd(hipStream_t st, const DualFwdArgs& a) {
  dim3 grid((a.N + DG_ST - 1) / DG_ST, a.B);
  const size_t nslot = a.x0 ? 3 : 2;
  if constexpr (!std::is_same<T, float>::value) {
    if ((a.C % 32 == 0) && (a.Cout % 16 == 0)) {
      hipLaunchKernelGGL((dual_fused_fwd_kernel<T, true>), grid, dim3(256),
                         nslot * DG_ST * 128, st, a.gf, a.gb, (const T*)a.xf,
                         (const T*)a.pf1, (const T*)a.xb, (const T*)a.pb1,
                         (const T*)a.x0, (const T*)a.W, (const T*)a.bias,
                         (T*)a.pfout, (T*)a.pbout, a.yacc, (T*)a.yout, a.N,
                         a.C, a.Cout, a.kofs_f, a.kofs_b, a.alpha, a.beta,
                         a.first, a.act);
      return;
    }
  }
  hipLaunchKernelGGL((dual_fused_fwd_kernel<T, false>), grid, dim3(256),
                     nslot * DG_ST * 64 * 4, st, a.gf, a.gb, (const T*)a.xf,
                     (const T*)a.pf1, (const T*)a.xb, (const T*)a.pb1,
                     (const T*)a.x0, (const T*)a.W, (const T*)a.bias,
                     (T*)a.pfout, (T*)a.pbout, a.yacc, (T*)a.yout, a.N, a.C,
                     a.Cout, a.kofs_f, a.kofs_b, a.alpha, a.beta, a.first,
                     a.act);
}

struct DualBwdArgs {
  DgCsr gft, gbt;
  const void *xf, *pf1, *xb, *pb1, *dz, *W;
  void *outf, *outb;
  int B, N, C, Cout, kofs_f, kofs_b;
  float alpha, beta;
  int final_step;
};

// MFMA U GEMMs when Cout % 32 == 0 and C % 16 == 0 (as launch_fused_bwd),
// scalar loop otherwise. LDS: dz tile + two fp32 U tiles.
template <typename T>
void launch_dual_bwd(hipStream_t st, const DualBwdArgs& a) {
  dim3 grid((a.N + DG_ST - 1) / DG_ST, a.B);
  if constexpr (!std::is_same<T, float>::value) {
    if ((a.Cout % 32 == 0) && (a.C % 16 == 0) && (a.C <= 64)) {
      hipLaunchKernelGGL((dual_fused_bwd_kernel<T, true>), grid, dim3(256),
                         DG_ST * 128 + 2 * DG_ST * 64 * 4, st, a.gft, a.gbt,
                         (const T*)a.xf, (const T*)a.pf1, (const T*)a.xb,
                         (const T*)a.pb1, (const T*)a.dz, (const T*)a.W,
                         (T*)a.outf, (T*)a.outb, a.N, a.C, a.Cout, a.kofs_f,
                         a.kofs_b, a.alpha, a.beta, a.final_step);
      return;
    }
  }
  hipLaunchKernelGGL((dual_fused_bwd_kernel<T, false>), grid, dim3(256),
                     3 * DG_ST * 64 * 4, st, a.gft, a.gbt, (const T*)a.xf,
                     (const T*)a.pf1, (const T*)a.xb, (const T*)a.pb1,
                     (const T*)a.dz, (const T*)a.W, (T*)a.outf, (T*)a.outb,
                     a.N, a.C, a.Cout, a.kofs_f, a.kofs_b, a.alpha, a.beta,
                     a.final_step);
}

}  // namespace

// Host contract (checked in bindings.cpp): bf16/f16 only, C <= 64, Cout <= 64.
extern "C" void stmgcn_dual_fused_fwd_step(
    void* stream_v, int dtype, const int* rpf, const int* cif, const float* vf,
    const int* rpb, const int* cib, const float* vb, const void* xf,
    const void* pf1, const void* xb, const void* pb1, const void* x0,
    const void* W, const void* bias, void* pfout, void* pbout, float* yacc,
    void* yout, int B, int N, int C, int Cout, int kofs_f, int kofs_b,
    float alpha, float beta, int first, int act) {
  const DualFwdArgs a{{rpf, cif, vf}, {rpb, cib, vb}, xf, pf1, xb, pb1, x0, W,
                      bias, pfout, pbout, yacc, yout, B, N, C, Cout, kofs_f,
                      kofs_b, alpha, beta, first, act};
  hipStream_t st = (hipStream_t)stream_v;
  if (dtype == STM_BF16) launch_dual_fwd<__hip_bfloat16>(st, a);
  else if (dtype == STM_F16) launch_dual_fwd<__half>(st, a);
}

extern "C" void stmgcn_dual_fused_bwd_step(
    void* stream_v, int dtype, const int* rpf, const int* cif, const float* vf,
    const int* rpb, const int* cib, const float* vb, const void* xf,
    const void* pf1, const void* xb, const void* pb1, const void* dz,
    const void* W, void* outf, void* outb, int B, int N, int C, int Cout,
    int kofs_f, int kofs_b, float alpha, float beta, int final_step) {
  const DualBwdArgs a{{rpf, cif, vf}, {rpb, cib, vb}, xf, pf1, xb, pb1, dz, W,
                      outf, outb, B, N, C, Cout, kofs_f, kofs_b, alpha, beta,
                      final_step};
  hipStream_t st = (hipStream_t)stream_v;
  if (dtype == STM_BF16) launch_dual_bwd<__hip_bfloat16>(st, a);
  else if (dtype == STM_F16) launch_dual_bwd<__half>(st, a);
}
