// Common device helpers for the stmgcn_amd CDNA4 (gfx950) kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <type_traits>

#include "kernels.h"  // entry-point prototypes, argument structs, SEQ_TILE

#define STM_WAVE 64  // CDNA wavefront width (never 32)

// dtype codes shared with the python side
enum StmDtype : int { STM_F32 = 0, STM_BF16 = 1, STM_F16 = 2 };

template <typename T> __device__ __forceinline__ float toF(T v);
template <> __device__ __forceinline__ float toF<float>(float v) { return v; }
template <> __device__ __forceinline__ float toF<__hip_bfloat16>(__hip_bfloat16 v) {
  return __bfloat162float(v);
}
template <> __device__ __forceinline__ float toF<__half>(__half v) { return __half2float(v); }

template <typename T> __device__ __forceinline__ T fromF(float v);
template <> __device__ __forceinline__ float fromF<float>(float v) { return v; }
template <> __device__ __forceinline__ __hip_bfloat16 fromF<__hip_bfloat16>(float v) {
  return __float2bfloat16(v);
}
template <> __device__ __forceinline__ __half fromF<__half>(float v) { return __float2half(v); }

// ---------------------------------------------------------------------------
// Launcher status (kernels.h): null, or a static message. stm_launched() is
// taken directly after each hipLaunchKernelGGL; hipGetLastError neither
// synchronises nor queries the stream, so it is safe under stream capture.
inline const char* stm_status(hipError_t e) {
  return e == hipSuccess ? nullptr : hipGetErrorString(e);
}
inline const char* stm_launched() { return stm_status(hipGetLastError()); }

// Host-side dtype dispatch: f(T{}) for the element type of a StmDtype code, so
// a launcher writes each launch once inside a generic lambda
// ([&](auto t) { using T = decltype(t); ... return stm_launched(); }). f's
// status is returned; a code outside the enum launches nothing and returns
// `bad`, the entry point's message for it.
template <typename F> const char* stm_dispatch_dtype(const char* bad, int dtype, F&& f) {
  switch (dtype) {
    case STM_F32: return f(float{});
    case STM_BF16: return f(__hip_bfloat16{});
    case STM_F16: return f(__half{});
    default: return bad;
  }
}
// The same for kernels that have no fp32 form (MFMA fragments, packed 16 B
// moves).
template <typename F> const char* stm_dispatch_lowp(const char* bad, int dtype, F&& f) {
  switch (dtype) {
    case STM_BF16: return f(__hip_bfloat16{});
    case STM_F16: return f(__half{});
    default: return bad;
  }
}
// A runtime flag as a template argument: f(std::true_type{}) or
// f(std::false_type{}); the kernel takes decltype(flag)::value.
template <typename F> const char* stm_dispatch_bool(bool flag, F&& f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}

// ---------------------------------------------------------------------------
// MFMA fragment vocabulary of v_mfma_f32_16x16x32_{bf16,f16}: a lane's 8-wide
// A/B operand and 4-wide fp32 C/D accumulator (lane maps: mfma_probe_kernel,
// fused_rnn.hip). Frag8<float> exists only so that templates which also serve
// the gconv scalar (fp32) path can name the types; it feeds no MFMA.
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

template <typename T> struct Frag8 { using type = float; using elem = float; };
template <> struct Frag8<__hip_bfloat16> { using type = bf16x8; using elem = __bf16; };
template <> struct Frag8<__half> { using type = f16x8; using elem = _Float16; };

__device__ __forceinline__ float elemF(__bf16 v) { return (float)v; }
__device__ __forceinline__ float elemF(_Float16 v) { return (float)v; }

__device__ __forceinline__ f32x4 mfma16x16x32(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16x16x32(f16x8 a, f16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// Fast device transcendentals: v_exp_f32 + v_rcp_f32 (~1 ulp each) instead
// of libm tanhf (~30 VALU instr) / IEEE divide — the RNN pointwise phase is
// VALU-bound on these (up to 40 per thread per (layer,t) stage) and the
// results are rounded to bf16/f16 anyway.
__device__ __forceinline__ float stm_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}
__device__ __forceinline__ float stm_tanh(float x) {
  // tanh(x) = 2*sigmoid(2x) - 1, the 2 of 2x folded into the exponent's
  // constant (a power of two: the product keeps its bits). No clamp: where
  // exp2 underflows to 0 or overflows to inf, rcp gives 1 or 0 and the fma
  // exactly +-1, which is what every |x| > 9.1 rounds to anyway; NaN stays NaN.
  const float e = __builtin_amdgcn_exp2f(x * (-2.0f * 0x1.715476p+0f));
  return fmaf(2.0f, __builtin_amdgcn_rcpf(1.0f + e), -1.0f);
}

// One separately rounded fp32 product / sum: never contracted into an FMA with
// a neighbour, whatever the surrounding code looks like (HIP contracts a * b + c
// by default, and which of two products it fuses depends on the context).
// Where a kernel's results are pinned bit for bit, its pointwise arithmetic is
// written with these and fmaf.
__device__ __forceinline__ float stm_fmul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float stm_fadd(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// LDS swizzle for 128-byte tile rows (64 bf16/f16 channels): element (row s,
// channel byte cbyte) of one tile slot. XOR'd so the 16 lanes of a
// ds_read_b128 fragment group (consecutive rows, same channel window) hit 64
// distinct banks: row parity gives the 32-bank half, ((s>>1)&7) permutes the
// eight 16 B windows within it.
__device__ __forceinline__ int lds_swz(int s, int cbyte) {
  return s * 128 + (cbyte ^ ((((unsigned)s >> 1) & 7) << 4));
}

// ---------------------------------------------------------------------------
// dA stream layout (lstm_bwd -> lstm_wgrad hand-off).
//
// The gate-preactivation gradient tensor keeps its logical shape
// (L, Tst, S_pad, 4H) and size, but inside every 32-row sequence tile the
// elements are stored in the wgrad MFMA A-fragment order instead of row-major:
//
//   tile (l, t, b = s / 32) starts at element ((l*Tst + t)*S_pad + 32b) * 4H
//   and holds [gate g = 0..4H-1][k' = 0..31] (k' contiguous, 64 B per gate);
//   element (g, k') is dA[row 32b + rho(k')][g] with
//     rho(k') = 16*((k'>>2)&1) + 4*(k'>>3) + (k'&3)
//   i.e. k' = 8*lgrp + 4*m + r  <->  row = 16*m + 4*lgrp + r, which is the
//   MFMA D-fragment ownership of the pointwise phase of lstm_bwd_kernel: a
//   lane's 8 values per (gate slot, channel) are 8 consecutive k' = one 16 B
//   store, and the wgrad lane (l16, lgrp) of gate g loads its A-fragment as
//   the 16 B at k' = 8*lgrp. The permutation rho of the reduction index is
//   free as long as the B operand (h_{t-1} / layer input rows) uses it too.
// SEQ_TILE (kernels.h): sequences per RNN workgroup tile == dA tile rows
#define STM_DA_GATES 256                          // 4H, H = 64
#define STM_DA_TILE_ELEMS (SEQ_TILE * STM_DA_GATES)
static_assert(SEQ_TILE == 32, "dA tile layout (rho) is defined for 32-row tiles");

// element offset of the tile whose first flat row (t*S_pad + s) is row0
__host__ __device__ constexpr long stm_da_tile_off(long row0) {
  return row0 * STM_DA_GATES;
}
// element offset of (gate g, reduction slot k') inside a tile
__host__ __device__ constexpr int stm_da_elem(int g, int kp) {
  return g * SEQ_TILE + kp;
}
// k' -> tile row, and its inverse
__host__ __device__ constexpr int stm_da_rho(int kp) {
  return 16 * ((kp >> 2) & 1) + 4 * (kp >> 3) + (kp & 3);
}
__host__ __device__ constexpr int stm_da_rho_inv(int row) {
  return 8 * ((row >> 2) & 3) + 4 * (row >> 4) + (row & 3);
}
static_assert(stm_da_rho(0) == 0 && stm_da_rho(4) == 16 && stm_da_rho(8) == 4 &&
              stm_da_rho(31) == 31 && stm_da_rho_inv(stm_da_rho(13)) == 13 &&
              stm_da_rho_inv(stm_da_rho(22)) == 22, "rho / rho_inv mismatch");

// ---------------------------------------------------------------------------
// "Last arriver finishes": in-launch hand-off for the reduction kernels that
// accumulate fp32 partials with unsafeAtomicAdd. Every workgroup of a slice
// calls this once, after its atomics; the call returns true (workgroup-
// uniform) in exactly one of them — the one that drew the last of `expected`
// tickets — and by then every workgroup's partials are visible to plain
// vector loads of all its waves. That workgroup rounds the sums to the
// parameter dtype and writes the gradients in their final shapes, so no
// separate convert / slice / reduce launch follows the kernel.
//
// Arrival: every wave drains its atomics (vmcnt), the workgroup meets, lane 0
// releases at agent scope, drains again (the fence's own wait is not relied
// on) and only then draws its ticket with a relaxed agent-scope add. The last
// arriver acquires at agent scope once (drops this CU's stale L1 lines),
// drains, and the closing barrier holds the other waves behind that. No
// __threadfence() per thread, no workgroup-scope fence, no assumption on
// dispatch order or placement; nobody spins, so nothing can hang.
//
// `ticket` must be zero at launch: it lives in the same zero-filled fp32
// workspace as the accumulators (one fill clears both). `flag` is one int of
// the caller's existing LDS array that no wave still reads.
__device__ __forceinline__ bool stm_last_arriver(unsigned* ticket,
                                                 unsigned expected, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
    const bool last = (t + 1 == expected);
    *flag = last ? 1 : 0;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  return *flag != 0;
}

// 4 fp32 sums -> 4 values of T, one 8-byte store (dst 8-byte aligned)
template <typename T>
__device__ __forceinline__ void stm_store4(T* dst, float a, float b, float c,
                                           float d) {
  union { T t[4]; uint2 u; } pk;
  pk.t[0] = fromF<T>(a); pk.t[1] = fromF<T>(b);
  pk.t[2] = fromF<T>(c); pk.t[3] = fromF<T>(d);
  *(uint2*)dst = pk.u;
}
