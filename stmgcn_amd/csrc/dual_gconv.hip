// Dual random-walk diffusion graph convolution on CSR — CDNA4 (gfx950).
//
// The bidirectional diffusion convolution (Li et al., ICLR'18) mixes 2K+1
// supports: I, T_1..T_K of the forward generator G_f = (D_out^-1 A)^T and
// T_1..T_K of the backward generator G_b = (D_in^-1 A^T)^T. Weight rows:
// [0,C) -> T_0, [kC,(k+1)C) -> T_k(G_f), [(K+k)C,(K+k+1)C) -> T_k(G_b).
//
// These step kernels are the two-generator siblings of cheb_fused_fwd_kernel /
// cheb_fused_bwd_kernel (cheb_gconv.hip), built from the same gconv_tile.h
// primitives (32-row tile, 256-thread workgroups, lds_swz staging,
// v_mfma_f32_16x16x32 fragments), but one launch advances BOTH recurrences
// and folds both mixes into one accumulator pair, so K launches serve 2K+1
// supports with K-1 passes over the fp32 yacc (K == 1 needs no yacc at all).
// The backward runs both Clenshaw chains per launch from a single staged dz
// tile: K+1 launches instead of 2(K+1).

#include "gconv_tile.h"

namespace {

// One fused forward step k over (B, N, C) states, both directions:
//   pf_k = alpha * (G_f @ xf)[rows] + beta * pf1[rows]    (pf1 optional)
//   pb_k = alpha * (G_b @ xb)[rows] + beta * pb1[rows]
//   acc  = pf_k @ W[kofs_f:+C] + pb_k @ W[kofs_b:+C]  (+ x0 @ W[0:C] at k = 1)
//   yacc (+)= acc, or on the last step yout = act(yacc + acc + bias)
// The two generators are walked independently, so a row may be empty in one
// direction only. pf1/pb1 are read only at the thread's own (row, c) element
// before that element of pfout/pbout is written, so pf1 == pfout (pb1 ==
// pbout) aliasing is safe per direction; the gather operands must be distinct
// buffers.
template <typename T, bool MF>
__global__ void __launch_bounds__(256, 4)
dual_fused_fwd_kernel(const StmCsr gf, const StmCsr gb,
                      const T* __restrict__ xf, const T* pf1,
                      const T* __restrict__ xb, const T* pb1,
                      const T* __restrict__ x0,
                      const T* __restrict__ W, const T* __restrict__ bias,
                      T* pfout, T* pbout, float* __restrict__ yacc,
                      T* __restrict__ yout, int N, int C, int Cout,
                      int kofs_f, int kofs_b, float alpha, float beta,
                      int first, int act, int vec) {
  const int b = blockIdx.y;
  const int n0 = blockIdx.x * GC_ST;
  extern __shared__ char lds[];
  constexpr int kSlot = gc_slot_bytes(MF);
  char* lf = lds;                 // pf_k tile
  char* lb = lds + kSlot;         // pb_k tile
  char* l0 = lds + 2 * kSlot;     // x tile (k = 1 only)
  const long boff = (long)b * N * C;
  const T* xfb = xf + boff;
  const T* xbb = xb + boff;

  // ---- phase 0 (MFMA mix): the yacc / bias reads of phase 2, requested
  // ahead. The W fragments (three passes: 24 VGPRs) are fetched after the
  // barrier here: held across two gathers they spill. ----
  const GcLane l;
  GcYPrev yp = {};
  if constexpr (MF) {
    if (l.wv < (Cout >> 4))
      yp = gc_y_prefetch<T>(b, n0, N, Cout, l, bias, yacc, yout, first);
  }

  // ---- phase 1: both recurrences (SpMM + axpby), tiles staged in LDS ----
  const int G = C >> 3;
  for (int u = threadIdx.x; vec && u < GC_ST * G; u += 256) {
    // one (row, 8-channel group) unit per thread, both directions
    const int rl = u / G, c = (u % G) * 8;
    const int row = n0 + rl;
    float af[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float ab[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float v0[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (row < N) {
      const long e = boff + (long)row * C + c;
      GcRaw8<T> r0 = {}, rf = {}, rb = {};
      if (x0 != nullptr) r0 = gc_load8<T>(&x0[e]);
      if (pf1 != nullptr) rf = gc_load8<T>(&pf1[e]);
      if (pb1 != nullptr) rb = gc_load8<T>(&pb1[e]);
      gc_gather8<T>(gf, xfb, row, C, c, af);
      gc_gather8<T>(gb, xbb, row, C, c, ab);
      float pv[8];
      #pragma unroll
      for (int q = 0; q < 8; ++q) af[q] = stm_fmul(alpha, af[q]);
      #pragma unroll
      for (int q = 0; q < 8; ++q) ab[q] = stm_fmul(alpha, ab[q]);
      if (pf1 != nullptr) {
        gc_unpack8<T>(rf, pv);
        #pragma unroll
        for (int q = 0; q < 8; ++q) af[q] = fmaf(beta, pv[q], af[q]);
      }
      if (pb1 != nullptr) {
        gc_unpack8<T>(rb, pv);
        #pragma unroll
        for (int q = 0; q < 8; ++q) ab[q] = fmaf(beta, pv[q], ab[q]);
      }
      gc_store8<T>(&pfout[e], af);
      gc_store8<T>(&pbout[e], ab);
      if (x0 != nullptr) gc_unpack8<T>(r0, v0);
    }
    gc_tile_store8<T, MF>(lf, rl, c, af);
    gc_tile_store8<T, MF>(lb, rl, c, ab);
    if (x0 != nullptr) gc_tile_store8<T, MF>(l0, rl, c, v0);
  }
  for (int i = threadIdx.x; !vec && i < GC_ST * C; i += 256) {
    const int c = i % C, rl = i / C;
    const int row = n0 + rl;
    float af = 0.f, ab = 0.f, v0 = 0.f;
    if (row < N) {
      const long e = boff + (long)row * C + c;
      af = alpha * gc_gather<T>(gf, xfb, row, C, c);
      ab = alpha * gc_gather<T>(gb, xbb, row, C, c);
      if (pf1 != nullptr) af = fmaf(beta, toF<T>(pf1[e]), af);
      if (pb1 != nullptr) ab = fmaf(beta, toF<T>(pb1[e]), ab);
      pfout[e] = fromF<T>(af);
      pbout[e] = fromF<T>(ab);
      if (x0 != nullptr) v0 = toF<T>(x0[e]);
    }
    gc_tile_store<T, MF>(lf, rl, c, af);
    gc_tile_store<T, MF>(lb, rl, c, ab);
    if (x0 != nullptr) gc_tile_store<T, MF>(l0, rl, c, v0);
  }
  __syncthreads();

  // ---- phase 2: mix epilogue, one accumulator for all passes ----
  if constexpr (MF) {
    if (l.wv < (Cout >> 4)) {          // wave wv owns output cols [16wv,16wv+16)
      f32x4 acc[2];
      acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
      const GcMixB<T> wf = gc_mix_load<T>(W, kofs_f, C, Cout, l);
      const GcMixB<T> wb = gc_mix_load<T>(W, kofs_b, C, Cout, l);
      GcMixB<T> w0 = {};
      if (x0 != nullptr) w0 = gc_mix_load<T>(W, 0, C, Cout, l);
      gc_mix_mfma<T>(lf, wf, C, l, acc);
      gc_mix_mfma<T>(lb, wb, C, l, acc);
      if (x0 != nullptr) gc_mix_mfma<T>(l0, w0, C, l, acc);
      gc_y_store_frag<T>(acc, yp, b, n0, N, Cout, l, bias, yacc, yout, first, act);
    }
  } else {
    for (int i = threadIdx.x; i < GC_ST * Cout; i += 256) {
      const int co = i % Cout, rl = i / Cout;
      const int row = n0 + rl;
      if (row >= N) continue;
      float v = gc_mix_scalar<T>(lf, W, kofs_f, C, Cout, rl, co, 0.f);
      v = gc_mix_scalar<T>(lb, W, kofs_b, C, Cout, rl, co, v);
      if (x0 != nullptr) v = gc_mix_scalar<T>(l0, W, 0, C, Cout, rl, co, v);
      gc_y_store<T>(v, ((long)b * N + row) * Cout + co, co, bias, yacc, yout, first, act);
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
__global__ void __launch_bounds__(256, 4)
dual_fused_bwd_kernel(const StmCsr gft, const StmCsr gbt,
                      const T* __restrict__ xf, const T* pf1,
                      const T* __restrict__ xb, const T* pb1,
                      const T* __restrict__ dz, const T* __restrict__ W,
                      T* outf, T* outb, int N, int C, int Cout, int kofs_f,
                      int kofs_b, float alpha, float beta, int final_step,
                      int vec, int vec_dz) {
  const int b = blockIdx.y;
  const int n0 = blockIdx.x * GC_ST;
  extern __shared__ char lds[];
  float* utf = (float*)(lds + gc_slot_bytes(MF));
  float* utb = utf + GC_ST * 64;
  const long boff = (long)b * N * C;

  // ---- phase C's loads, first: the two gathers depend on neither dz, W nor
  // U; one (row, 8-channel group) unit per thread, held in registers ----
  const int G = C >> 3;
  const int rl = threadIdx.x / (G > 0 ? G : 1), c = (threadIdx.x % (G > 0 ? G : 1)) * 8;
  const int row = n0 + rl;
  const bool live = vec && rl < GC_ST && row < N;
  const long e8 = boff + (long)row * C + c;
  float gf8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float gb8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  GcRaw8<T> rf = {}, rb = {};
  if (live) {
    if (pf1 != nullptr) rf = gc_load8<T>(&pf1[e8]);
    if (pb1 != nullptr) rb = gc_load8<T>(&pb1[e8]);
    if (xf != nullptr) gc_gather8<T>(gft, xf + boff, row, C, c, gf8);
    if (xb != nullptr) gc_gather8<T>(gbt, xb + boff, row, C, c, gb8);
  }

  // ---- phase A: stage the dz tile (once for both chains) ----
  gc_stage_dz<T, MF>(lds, dz + (long)b * N * Cout, n0, N, Cout, vec_dz);
  __syncthreads();

  // ---- phase B: U_f (and U_b) = dz @ W_j^T ----
  gc_u_pass<T, MF>(lds, W, kofs_f, C, Cout, utf);
  if (!final_step) gc_u_pass<T, MF>(lds, W, kofs_b, C, Cout, utb);
  __syncthreads();

  // ---- phase C: the two SpMM/axpby updates ----
  if (vec) {
    if (!live) return;
    const float4* uf = (const float4*)&utf[rl * 64 + c];
    const float4 f0 = uf[0], f1 = uf[1];
    float af[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
    float ab[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (!final_step) {
      const float4* ub = (const float4*)&utb[rl * 64 + c];
      const float4 b0 = ub[0], b1 = ub[1];
      ab[0] = b0.x; ab[1] = b0.y; ab[2] = b0.z; ab[3] = b0.w;
      ab[4] = b1.x; ab[5] = b1.y; ab[6] = b1.z; ab[7] = b1.w;
    }
    float pv[8];
    #pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (xf != nullptr) af[q] = fmaf(alpha, gf8[q], af[q]);
      if (xb != nullptr) ab[q] = fmaf(alpha, gb8[q], ab[q]);
    }
    if (pf1 != nullptr) {
      gc_unpack8<T>(rf, pv);
      #pragma unroll
      for (int q = 0; q < 8; ++q) af[q] = fmaf(beta, pv[q], af[q]);
    }
    if (pb1 != nullptr) {
      gc_unpack8<T>(rb, pv);
      #pragma unroll
      for (int q = 0; q < 8; ++q) ab[q] = fmaf(beta, pv[q], ab[q]);
    }
    if (final_step) {
      #pragma unroll
      for (int q = 0; q < 8; ++q) af[q] = stm_fadd(af[q], ab[q]);
      gc_store8<T>(&outf[e8], af);
    } else {
      gc_store8<T>(&outf[e8], af);
      gc_store8<T>(&outb[e8], ab);
    }
    return;
  }
  for (int i = threadIdx.x; i < GC_ST * C; i += 256) {
    const int c = i % C, rl = i / C;
    const int row = n0 + rl;
    if (row >= N) continue;
    const long e = boff + (long)row * C + c;
    float af = gc_f32(utf, rl, c);
    float ab = final_step ? 0.f : gc_f32(utb, rl, c);
    if (xf != nullptr) af = fmaf(alpha, gc_gather<T>(gft, xf + boff, row, C, c), af);
    if (xb != nullptr) ab = fmaf(alpha, gc_gather<T>(gbt, xb + boff, row, C, c), ab);
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

// MFMA epilogue when gc_fwd_mfma serves the widths, scalar epilogue
// otherwise. LDS slots: pf tile, pb tile (+ the x tile at k = 1).
template <typename T>
const char* launch_dual_fwd(hipStream_t st, const DualFwdArgs& a) {
  return gc_dispatch_mf<T>(gc_fwd_mfma<T>(a.C, a.Cout), [&](auto mf) {
    constexpr bool MF = decltype(mf)::value;
    hipLaunchKernelGGL((dual_fused_fwd_kernel<T, MF>), gc_grid(a.N, a.B), dim3(256),
                       (a.x0 ? 3 : 2) * gc_slot_bytes(MF), st, a.gf, a.gb,
                       (const T*)a.xf, (const T*)a.pf1, (const T*)a.xb,
                       (const T*)a.pb1, (const T*)a.x0, (const T*)a.W,
                       (const T*)a.bias, (T*)a.pfout, (T*)a.pbout, a.yacc,
                       (T*)a.yout, a.N, a.C, a.Cout, a.kofs_f, a.kofs_b, a.alpha,
                       a.beta, a.first, a.act,
                       (int)gc_vec8(a.N, a.C, {a.xf, a.pf1, a.xb, a.pb1, a.x0, a.pfout,
                                          a.pbout}));
    return stm_launched();
  });
}

// MFMA U GEMMs when gc_bwd_mfma serves the widths, scalar loop otherwise.
// LDS: dz slot + two fp32 U tiles.
template <typename T>
const char* launch_dual_bwd(hipStream_t st, const DualBwdArgs& a) {
  return gc_dispatch_mf<T>(gc_bwd_mfma<T>(a.C, a.Cout), [&](auto mf) {
    constexpr bool MF = decltype(mf)::value;
    hipLaunchKernelGGL((dual_fused_bwd_kernel<T, MF>), gc_grid(a.N, a.B), dim3(256),
                       gc_slot_bytes(MF) + 2 * GC_F32_TILE_BYTES, st, a.gft, a.gbt,
                       (const T*)a.xf, (const T*)a.pf1, (const T*)a.xb,
                       (const T*)a.pb1, (const T*)a.dz, (const T*)a.W, (T*)a.outf,
                       (T*)a.outb, a.N, a.C, a.Cout, a.kofs_f, a.kofs_b, a.alpha,
                       a.beta, a.final_step,
                       (int)gc_vec8(a.N, a.C, {a.xf, a.pf1, a.xb, a.pb1, a.outf, a.outb}),
                       (int)gc_vec8(a.N, a.Cout, {a.dz}));
    return stm_launched();
  });
}

}  // namespace

// bf16/f16 only (no fp32 kernels are instantiated); C <= 64, Cout <= 64 is
// checked in bindings.cpp.
extern "C" const char* stmgcn_dual_fused_fwd_step(void* stream_v, int dtype,
                                                  const DualFwdArgs& a) {
  return stm_dispatch_lowp("stmgcn_dual_fused_fwd_step: dtype code is not bf16/f16",
                           dtype, [&](auto t) {
    return launch_dual_fwd<decltype(t)>((hipStream_t)stream_v, a);
  });
}

extern "C" const char* stmgcn_dual_fused_bwd_step(void* stream_v, int dtype,
                                                  const DualBwdArgs& a) {
  return stm_dispatch_lowp("stmgcn_dual_fused_bwd_step: dtype code is not bf16/f16",
                           dtype, [&](auto t) {
    return launch_dual_bwd<decltype(t)>((hipStream_t)stream_v, a);
  });
}
