// Chebyshev graph-convolution support recurrence on CSR — CDNA4 (gfx950).
//
// Replaces the reference's dense einsum('ij,bjp->bip') per materialized
// support (GCN.py:34-36): the (K_s, N, N) T_k stacks are never built; only
// the sparse generator G is stored and the first-kind recurrence
// T_k x = 2 G (T_{k-1} x) - T_{k-2} x runs on-device.
//
// This file holds the single-generator kernels' control flow and launchers;
// the CSR gather, LDS tile layout, MFMA/scalar passes and the y epilogue are
// the shared primitives of gconv_tile.h (also used by dual_gconv.hip).
//
// spmm_step computes one recurrence step as a fused SpMM + axpby:
//     out = alpha * (G @ xin) + beta * p1 + gamma * p2
// over (B, N, C) slices embedded in a (B, N, K, C) stack (per-tensor row
// strides). Thread mapping of spmm_step: 256-thread blocks; each thread owns
// one (row, channel) pair, so a row's C channels sit in consecutive lanes and
// every gather xin[col, c] is a coalesced C-wide segment. Host-side sequencing
// of the K steps lives in bindings.cpp (cheb_apply / cheb_combine via
// Clenshaw). The fused kernels below map a thread to one (row, 8-channel
// group) unit when the channel count allows (gconv_tile.h, gc_vec8): one pass
// per 32-row tile, 16-byte accesses, the gather's loads in flight together,
// and in the backward the gather issued before the dz staging and the U GEMM.

#include "gconv_tile.h"

namespace {

template <typename T>
__global__ void spmm_step_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ colidx,
    const float* __restrict__ vals,
    const T* __restrict__ xin, const T* __restrict__ p1, const T* __restrict__ p2,
    T* __restrict__ out,
    int N, int C, int rows_per_block,
    long sx, long s1, long s2, long so,          // element stride between rows
    long bx, long b1, long b2, long bo,          // element stride between batches
    float alpha, float beta, float gamma) {
  const int b = blockIdx.y;
  const int local = (C <= 256) ? (threadIdx.x / C) : 0;
  const int row = blockIdx.x * rows_per_block + local;
  if (row >= N || (C <= 256 && threadIdx.x >= rows_per_block * C)) return;

  const int c0 = (C <= 256) ? (threadIdx.x % C) : threadIdx.x;
  const int cstep = (C <= 256) ? C : 256;

  const StmCsr g{rowptr, colidx, vals};
  const T* xb = xin ? xin + (long)b * bx : nullptr;
  for (int c = c0; c < C; c += cstep) {
    float acc = 0.0f;
    if (alpha != 0.0f && xb) {
      acc = gc_gather<T>(g, xb, row, sx, c);
      acc *= alpha;
    }
    const long ro = (long)b * bo + (long)row * so + c;
    if (p1) acc += beta * toF<T>(p1[(long)b * b1 + (long)row * s1 + c]);
    if (p2) acc += gamma * toF<T>(p2[(long)b * b2 + (long)row * s2 + c]);
    out[ro] = fromF<T>(acc);
  }
}

// ===========================================================================
// Fully fused ChebConv (SURVEY K1+K2): support recurrence + mix GEMM + bias
// + activation in-kernel. The reference materializes a dense (K,N,N) support
// stack offline and a (B,N,K_s,C) feature concat per forward
// (GCN.py:34-42); here NEITHER exists: each recurrence step k computes its
// (B,N,C) state p_k = alpha*(G @ p_gather) + beta*p_prev, stages the 32-row
// tile in LDS (lds_swz layout), and folds p_k @ W_k straight into an fp32
// accumulator of y with v_mfma_f32_16x16x32 matrix cores. The final step
// adds the bias and applies the activation. A scalar epilogue serves fp32
// parity and channel counts that are not MFMA-tileable. The backward
// (Clenshaw) variant fuses U_j = dz @ W_j^T into each combine step the same
// way, so the dgrad U stack is never materialized either.

// One fused forward step over (B, N, C) state tensors:
//   tile = alpha * (G @ xin)[rows] + beta * p1[rows]     (either term optional)
//   pout[rows] = tile                                    (optional)
//   mix (W != null): yacc[rows] (+)= tile @ W[kofs:kofs+C, :]
//                    (+ x0 != null: also += x0[rows] @ W[0:C, :] — the T_0
//                     term folded into the T_1 launch, one launch fewer)
//   final (yout != null): yout = act(yacc_total + bias)
// p1 is read only at the thread's own (row, c) element, so p1 == pout
// aliasing is safe (the gather operand xin must be a distinct buffer).
template <typename T, bool MF>
__global__ void __launch_bounds__(256, 4)
cheb_fused_fwd_kernel(const int* __restrict__ rowptr,
                      const int* __restrict__ colidx,
                      const float* __restrict__ vals,
                      const T* __restrict__ xin, const T* __restrict__ p1,
                      const T* __restrict__ x0,
                      const T* __restrict__ W, const T* __restrict__ bias,
                      T* __restrict__ pout, float* __restrict__ yacc,
                      T* __restrict__ yout, int N, int C, int Cout, int kofs,
                      float alpha, float beta, int first, int act, int vec) {
  const int b = blockIdx.y;
  const int n0 = blockIdx.x * GC_ST;
  extern __shared__ char lds[];
  char* l0 = lds + gc_slot_bytes(MF);  // x0 tile slot
  const StmCsr g{rowptr, colidx, vals};
  const T* xb = xin ? xin + (long)b * N * C : nullptr;
  const T* pb = p1 ? p1 + (long)b * N * C : nullptr;
  const T* x0b = x0 ? x0 + (long)b * N * C : nullptr;

  // ---- phase 0 (MFMA mix): what phase 2 reads from global memory, requested
  // now so that it arrives under the gather ----
  const GcLane l;
  GcMixB<T> wk = {}, w0 = {};
  GcYPrev yp = {};
  if constexpr (MF) {
    if (l.wv < (Cout >> 4)) {
      wk = gc_mix_load<T>(W, kofs, C, Cout, l);
      if (x0 != nullptr) w0 = gc_mix_load<T>(W, 0, C, Cout, l);
      yp = gc_y_prefetch<T>(b, n0, N, Cout, l, bias, yacc, yout, first);
    }
  }

  // ---- phase 1: recurrence (SpMM + axpby), tile staged in LDS ----
  if (vec) {
    // one (row, 8-channel group) unit per thread; at C = 64 a single pass
    const int G = C >> 3;
    for (int u = threadIdx.x; u < GC_ST * G; u += 256) {
      const int rl = u / G, c = (u % G) * 8;
      const int row = n0 + rl;
      const bool live = row < N;
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      GcRaw8<T> r0 = {}, rp = {};
      if (live && x0b != nullptr) r0 = gc_load8<T>(&x0b[(long)row * C + c]);
      if (live && pb != nullptr) rp = gc_load8<T>(&pb[(long)row * C + c]);
      if (live) {
        if (xb != nullptr && alpha != 0.f) {
          gc_gather8<T>(g, xb, row, C, c, acc);
          #pragma unroll
          for (int q = 0; q < 8; ++q) acc[q] = stm_fmul(acc[q], alpha);
        }
        if (pb != nullptr) {
          float pv[8];
          gc_unpack8<T>(rp, pv);
          #pragma unroll
          for (int q = 0; q < 8; ++q) acc[q] = fmaf(beta, pv[q], acc[q]);
        }
        if (pout != nullptr) gc_store8<T>(&pout[((long)b * N + row) * C + c], acc);
      }
      if (x0b != nullptr) {
        float v0[8];
        gc_unpack8<T>(r0, v0);
        gc_tile_store8<T, MF>(l0, rl, c, v0);
      }
      if (W != nullptr) gc_tile_store8<T, MF>(lds, rl, c, acc);
    }
  } else {
    for (int i = threadIdx.x; i < GC_ST * C; i += 256) {
      const int c = i % C, rl = i / C;
      const int row = n0 + rl;
      float acc = 0.f;
      if (x0b != nullptr)
        gc_tile_store<T, MF>(l0, rl, c, (row < N) ? toF<T>(x0b[(long)row * C + c]) : 0.f);
      if (row < N) {
        if (xb != nullptr && alpha != 0.f) {
          acc = gc_gather<T>(g, xb, row, C, c);
          acc *= alpha;
        }
        if (pb != nullptr) acc = fmaf(beta, toF<T>(pb[(long)row * C + c]), acc);
        if (pout != nullptr) pout[((long)b * N + row) * C + c] = fromF<T>(acc);
      }
      if (W != nullptr) gc_tile_store<T, MF>(lds, rl, c, acc);
    }
  }
  if (W == nullptr) return;
  __syncthreads();

  // ---- phase 2: mix epilogue y += tile @ W_k (+ x0 @ W_0) ----
  if constexpr (MF) {
    if (l.wv < (Cout >> 4)) {          // wave wv owns output cols [16wv,16wv+16)
      f32x4 acc[2];
      acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
      gc_mix_mfma<T>(lds, wk, C, l, acc);
      if (x0 != nullptr) gc_mix_mfma<T>(l0, w0, C, l, acc);
      gc_y_store_frag<T>(acc, yp, b, n0, N, Cout, l, bias, yacc, yout, first, act);
    }
  } else {
    for (int i = threadIdx.x; i < GC_ST * Cout; i += 256) {
      const int co = i % Cout, rl = i / Cout;
      const int row = n0 + rl;
      if (row >= N) continue;
      float v = gc_mix_scalar<T>(lds, W, kofs, C, Cout, rl, co, 0.f);
      if (x0 != nullptr) v = gc_mix_scalar<T>(l0, W, 0, C, Cout, rl, co, v);
      gc_y_store<T>(v, ((long)b * N + row) * Cout + co, co, bias, yacc, yout, first, act);
    }
  }
}

// One fused backward (Clenshaw) step over the G^T CSR:
//   out[rows] = alpha * (G^T @ xin)[rows] + beta * p1[rows] + (dz @ W_j^T)[rows]
// The U_j = dz W_j^T term is computed in-kernel from an LDS-staged dz tile —
// the dgrad U stack (B,N,K_s,C) of the unfused design never exists.
template <typename T, bool MF>
__global__ void __launch_bounds__(256, 4)
cheb_fused_bwd_kernel(const int* __restrict__ rowptr,
                      const int* __restrict__ colidx,
                      const float* __restrict__ vals,
                      const T* __restrict__ xin, const T* __restrict__ p1,
                      const T* __restrict__ dz, const T* __restrict__ W,
                      T* __restrict__ out, int N, int C, int Cout, int kofs,
                      float alpha, float beta, int vec, int vec_dz) {
  const int b = blockIdx.y;
  const int n0 = blockIdx.x * GC_ST;
  extern __shared__ char lds[];
  float* ut = (float*)(lds + gc_slot_bytes(MF));
  const StmCsr g{rowptr, colidx, vals};
  const T* xb = xin ? xin + (long)b * N * C : nullptr;
  const T* pb = p1 ? p1 + (long)b * N * C : nullptr;

  // ---- phase C's loads, first: the gather depends on neither dz, W nor U, so
  // its round trips run under phases A and B. One (row, 8-channel group) unit
  // per thread (C <= 64: the U tile's row stride), held in registers. ----
  const int G = C >> 3;
  const int rl = threadIdx.x / (G > 0 ? G : 1), c = (threadIdx.x % (G > 0 ? G : 1)) * 8;
  const int row = n0 + rl;
  const bool live = vec && rl < GC_ST && row < N;
  float gth[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  GcRaw8<T> rp = {};
  if (live) {
    if (pb != nullptr) rp = gc_load8<T>(&pb[(long)row * C + c]);
    if (xb != nullptr && alpha != 0.f) gc_gather8<T>(g, xb, row, C, c, gth);
  }

  // ---- phase A: stage the dz tile;  phase B: U = dz @ W_j^T ----
  gc_stage_dz<T, MF>(lds, dz + (long)b * N * Cout, n0, N, Cout, vec_dz);
  __syncthreads();
  gc_u_pass<T, MF>(lds, W, kofs, C, Cout, ut);
  __syncthreads();

  // ---- phase C: out = alpha*(G^T @ xin) + beta*p1 + U ----
  if (vec) {
    if (!live) return;
    const float4* up = (const float4*)&ut[rl * 64 + c];
    const float4 u0 = up[0], u1 = up[1];
    float acc[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
    if (xb != nullptr && alpha != 0.f) {
      #pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = fmaf(alpha, gth[q], acc[q]);
    }
    if (pb != nullptr) {
      float pv[8];
      gc_unpack8<T>(rp, pv);
      #pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = fmaf(beta, pv[q], acc[q]);
    }
    gc_store8<T>(&out[((long)b * N + row) * C + c], acc);
    return;
  }
  for (int i = threadIdx.x; i < GC_ST * C; i += 256) {
    const int c = i % C, rl = i / C;
    const int row = n0 + rl;
    if (row >= N) continue;
    float acc = gc_f32(ut, rl, c);
    if (xb != nullptr && alpha != 0.f)
      acc = fmaf(alpha, gc_gather<T>(g, xb, row, C, c), acc);
    if (pb != nullptr) acc = fmaf(beta, toF<T>(pb[(long)row * C + c]), acc);
    out[((long)b * N + row) * C + c] = fromF<T>(acc);
  }
}

// MFMA epilogue when the mix runs (W != null) and gc_fwd_mfma serves the
// widths, scalar kernel otherwise. LDS: the tile slot (+ the x0 slot).
template <typename T>
const char* launch_fused_fwd(hipStream_t st, const ChebFwdArgs& a) {
  return gc_dispatch_mf<T>(a.W != nullptr && gc_fwd_mfma<T>(a.C, a.Cout), [&](auto mf) {
    constexpr bool MF = decltype(mf)::value;
    hipLaunchKernelGGL((cheb_fused_fwd_kernel<T, MF>), gc_grid(a.N, a.B), dim3(256),
                       (a.x0 ? 2 : 1) * gc_slot_bytes(MF), st, a.g.rowptr,
                       a.g.colidx, a.g.vals, (const T*)a.xin, (const T*)a.p1,
                       (const T*)a.x0, (const T*)a.W, (const T*)a.bias, (T*)a.pout,
                       a.yacc, (T*)a.yout, a.N, a.C, a.Cout, a.kofs, a.alpha, a.beta,
                       a.first, a.act, (int)gc_vec8(a.N, a.C, {a.xin, a.p1, a.x0, a.pout}));
    return stm_launched();
  });
}

// MFMA U GEMM when gc_bwd_mfma serves the widths. LDS: dz slot + one fp32 U tile.
template <typename T>
const char* launch_fused_bwd(hipStream_t st, const ChebBwdArgs& a) {
  return gc_dispatch_mf<T>(gc_bwd_mfma<T>(a.C, a.Cout), [&](auto mf) {
    constexpr bool MF = decltype(mf)::value;
    hipLaunchKernelGGL((cheb_fused_bwd_kernel<T, MF>), gc_grid(a.N, a.B), dim3(256),
                       gc_slot_bytes(MF) + GC_F32_TILE_BYTES, st, a.g.rowptr,
                       a.g.colidx, a.g.vals, (const T*)a.xin, (const T*)a.p1,
                       (const T*)a.dz, (const T*)a.W, (T*)a.out, a.N, a.C, a.Cout,
                       a.kofs, a.alpha, a.beta,
                       (int)gc_vec8(a.N, a.C, {a.xin, a.p1, a.out}),
                       (int)gc_vec8(a.N, a.Cout, {a.dz}));
    return stm_launched();
  });
}

}  // namespace

extern "C" const char* stmgcn_spmm_step(void* stream_v, int dtype, const SpmmArgs& a) {
  const int C = a.C;
  const int rows_per_block = (C <= 256) ? (256 / C > 0 ? 256 / C : 1) : 1;
  const dim3 grid((a.N + rows_per_block - 1) / rows_per_block, a.B);
  return stm_dispatch_dtype("stmgcn_spmm_step: unsupported dtype code", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((spmm_step_kernel<T>), grid, dim3(256), 0,
                       (hipStream_t)stream_v, a.g.rowptr, a.g.colidx, a.g.vals,
                       (const T*)a.xin.ptr, (const T*)a.p1.ptr, (const T*)a.p2.ptr,
                       (T*)const_cast<void*>(a.out.ptr), a.N, C, rows_per_block,
                       a.xin.srow, a.p1.srow, a.p2.srow, a.out.srow, a.xin.sbatch,
                       a.p1.sbatch, a.p2.sbatch, a.out.sbatch, a.alpha, a.beta, a.gamma);
    return stm_launched();
  });
}

extern "C" const char* stmgcn_cheb_fused_fwd_step(void* stream_v, int dtype,
                                                  const ChebFwdArgs& a) {
  return stm_dispatch_dtype("stmgcn_cheb_fused_fwd_step: unsupported dtype code", dtype,
                            [&](auto t) {
    return launch_fused_fwd<decltype(t)>((hipStream_t)stream_v, a);
  });
}

extern "C" const char* stmgcn_cheb_fused_bwd_step(void* stream_v, int dtype,
                                                  const ChebBwdArgs& a) {
  return stm_dispatch_dtype("stmgcn_cheb_fused_bwd_step: unsupported dtype code", dtype,
                            [&](auto t) {
    return launch_fused_bwd<decltype(t)>((hipStream_t)stream_v, a);
  });
}
