// Fused pointwise/reduction kernels — CDNA4 (gfx950).
//
//  K3  seqsum_permute: (B,T,N,C) -> (B,N,T) feature-sum + transpose
//      (reference STMGCN.py:36,39)
//  K4  contextual gate: z = mean_n(gconv + x_seq); s = sigmoid(FC(relu(FC(z))))
//      with ONE weight-tied FC applied twice (STMGCN.py:43, quirk 2);
//      out = obs * s  (eqs. 6-9). Forward = one node-reduce kernel whose last
//      workgroup per batch row runs the FC stages + one broadcast-multiply;
//      backward mirrors it and also sums dw/db over the batch.
//  K7  branch-fuse + FC head: y = (sum_m feats_m) @ W^T + b (STMGCN.py:116-118)
//      head_multi_*: the same head with 2..32 output columns (multi-step
//      horizon, column o = p*C + c) on MFMA tiles
//  K8  fused MSE loss + grad  (Model_Trainer.py:38)
//      masked_loss_*: MSE / MAE / Huber over the targets that are not NaN
//  K9  multi-tensor Adam over a flat fp32 master arena with bf16/f16 working
//      params (torch.optim.Adam semantics incl. L2-style weight decay)

#include "common.h"

#define GATE_MAX_T 16

namespace {

// ---- K3 ------------------------------------------------------------------
template <typename T>
__global__ void seqsum_permute_kernel(const T* __restrict__ obs,  // (B,T,N,C)
                                      T* __restrict__ out,        // (B,N,T)
                                      int B, int Tst, int N, int C) {
  // iterate in (b,t,n) source order: consecutive threads read consecutive
  // C-runs (fully coalesced); the (B,N,T) write is a small-stride scatter
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over B*T*N
  if (i >= (long)B * Tst * N) return;
  const int n = i % N;
  const int t = (i / N) % Tst;
  const long b = i / ((long)N * Tst);
  float acc = 0.f;
  const T* src = obs + i * (long)C;
  int c = 0;
  for (; c + 4 <= C; c += 4) {
    acc += toF<T>(src[c]) + toF<T>(src[c + 1]) + toF<T>(src[c + 2]) +
           toF<T>(src[c + 3]);
  }
  for (; c < C; ++c) acc += toF<T>(src[c]);
  out[(b * N + n) * (long)Tst + t] = fromF<T>(acc);
}

template <typename T>
__global__ void seqsum_permute_bwd_kernel(const T* __restrict__ dxs,  // (B,N,T)
                                          T* __restrict__ dobs,       // (B,T,N,C)
                                          int B, int Tst, int N, int C) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over B*T*N*C
  if (i >= (long)B * Tst * N * C) return;
  const int n = (i / C) % N;
  const int t = (i / ((long)C * N)) % Tst;
  const long b = i / ((long)C * N * Tst);
  // every element written exactly once -> caller may pass uninitialized dobs
  dobs[i] = dxs[(b * N + n) * (long)Tst + t];
}

// ---- K4 forward part A: multi-block node reduce + tied double-FC ----------
// grid (nchunks, B): scales to any N (the old one-block-per-batch form was
// 3.5 ms/call at N=4096 — 16 blocks on 256 CUs). The workgroups of batch row
// b add their partial pooled sums to zsum[b] and arrive at ticket b
// (stm_last_arriver, common.h); the last one of the row turns the sums into
// z = mean, u = relu(W z + b), s = sigmoid(W u + b) — lane t of its first
// wave owns output t, so the T x T products run T-wide instead of on one
// serial thread per row in a launch of its own. z overwrites zsum in place.
template <typename T>
__global__ void gate_fwd_reduce_kernel(const T* __restrict__ g,     // (B,N,T)
                                       const T* __restrict__ xs,    // (B,N,T)
                                       float* __restrict__ zsum,    // (B,T) zeroed
                                       const T* __restrict__ fcw,   // (T,T)
                                       const T* __restrict__ fcb,   // (T,)
                                       float* __restrict__ u_out,   // (B,T)
                                       float* __restrict__ s_out,   // (B,T)
                                       unsigned* tickets,           // (B,) zeroed
                                       int N, int Tst) {
  __shared__ float red[256];
  // arrival flag: the last word of red (the reduce uses the first 4 *
  // GATE_MAX_T words, the FC stage the first 2 * GATE_MAX_T)
  int* last_flag = (int*)&red[255];
  const long b = blockIdx.y;
  const int nchunks = gridDim.x;
  const int chunk = (N + nchunks - 1) / nchunks;
  const int n0 = blockIdx.x * chunk;
  const int n1 = min(n0 + chunk, N);
  float zacc[GATE_MAX_T];
  for (int t = 0; t < Tst; ++t) zacc[t] = 0.f;
  const T* gb = g + b * (long)N * Tst;
  const T* xb = xs + b * (long)N * Tst;
  for (int n = n0 + threadIdx.x; n < n1; n += blockDim.x)
    for (int t = 0; t < Tst; ++t)
      zacc[t] += toF<T>(gb[(long)n * Tst + t]) + toF<T>(xb[(long)n * Tst + t]);
  for (int t = 0; t < Tst; ++t) {
    float v = zacc[t];
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * GATE_MAX_T + t] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      float tot = 0.f;
      for (int w = 0; w < blockDim.x / 64; ++w) tot += red[w * GATE_MAX_T + t];
      unsafeAtomicAdd(&zsum[b * Tst + t], tot);
    }
    __syncthreads();
  }

  if (!stm_last_arriver(&tickets[b], gridDim.x, last_flag)) return;
  float* zs = red;
  float* us = red + GATE_MAX_T;
  const int t = threadIdx.x;
  if (t < Tst) zs[t] = zsum[b * Tst + t] / (float)N;
  __syncthreads();
  if (t < Tst) {                                   // u = relu(W z + b)
    float a = toF<T>(fcb[t]);
    for (int j = 0; j < Tst; ++j) a += toF<T>(fcw[t * Tst + j]) * zs[j];
    us[t] = a > 0.f ? a : 0.f;
  }
  __syncthreads();
  if (t < Tst) {                                   // s = sigmoid(W u + b)
    float a = toF<T>(fcb[t]);
    for (int j = 0; j < Tst; ++j) a += toF<T>(fcw[t * Tst + j]) * us[j];
    zsum[b * Tst + t] = zs[t];
    u_out[b * Tst + t] = us[t];
    s_out[b * Tst + t] = stm_sigmoid(a);
  }
}

// ---- K4 forward part B: out = obs * s[b,t] --------------------------------
// NM (node-major): out is (B,N,T,C), the sequence layout the RNN reads, so no
// permute copy follows; thread i owns output element i either way.
template <typename T, bool NM>
__global__ void gate_scale_kernel(const T* __restrict__ obs,   // (B,T,N,C)
                                  const float* __restrict__ s, // (B,T)
                                  T* __restrict__ out, int Tst, int N, int C,
                                  long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if (!NM) {
    out[i] = fromF<T>(toF<T>(obs[i]) * s[i / ((long)N * C)]);
  } else {
    const int c = i % C;
    const int t = (i / C) % Tst;
    const long bn = i / ((long)C * Tst);
    const long b = bn / N;
    const int n = bn % N;
    const long bt = b * Tst + t;
    out[i] = fromF<T>(toF<T>(obs[(bt * N + n) * C + c]) * s[bt]);
  }
}

// ---- K4 backward part A: ds reduce + tied-FC backward + dw/db -------------
// ds[b,t] = sum_{n,c} dout*obs over grid (nchunks, B) with atomics; the last
// workgroup to arrive for row b (ticket b) runs the FC backward of that row
// (lanes own columns, as in the forward), leaving dz over ds and the row's
// dW/db partials; it then arrives at ticket B, and the last row to finish sums
// the partials over the batch and writes dw / db in fp32 and in the parameter
// dtype. NM: dout is (B,N,T,C).
template <typename T, bool NM>
__global__ void gate_bwd_reduce_kernel(const T* __restrict__ dout, // (B,T,N,C)
                                       const T* __restrict__ obs,  // (B,T,N,C)
                                       float* __restrict__ ds_out, // (B,T) zeroed
                                       const T* __restrict__ fcw,  // (T,T)
                                       const float* __restrict__ z,
                                       const float* __restrict__ u,
                                       const float* __restrict__ s,
                                       float* __restrict__ dw_part,   // (B,T,T)
                                       float* __restrict__ db_part,   // (B,T)
                                       unsigned* tickets,             // (B+1,) zeroed
                                       float* __restrict__ dw_f,      // (T,T)
                                       float* __restrict__ db_f,      // (T,)
                                       T* __restrict__ dw_out, T* __restrict__ db_out,
                                       int N, int C, int Tst) {
  __shared__ float red[256];
  // arrival flag: the last word of red (the reduce uses the first 4 *
  // GATE_MAX_T words, the FC stage the first 2 * GATE_MAX_T)
  int* last_flag = (int*)&red[255];
  const long b = blockIdx.y;
  const int B = gridDim.y;
  const long NC = (long)N * C;
  const int nchunks = gridDim.x;
  const long chunk = (NC + nchunks - 1) / nchunks;
  const long i0 = blockIdx.x * chunk;
  const long i1 = min(i0 + chunk, NC);
  float dsacc[GATE_MAX_T];
  for (int t = 0; t < Tst; ++t) dsacc[t] = 0.f;
  const T* db_ = dout + b * Tst * NC;
  const T* ob = obs + b * Tst * NC;
  if (!NM) {
    for (int t = 0; t < Tst; ++t)
      for (long i = i0 + threadIdx.x; i < i1; i += blockDim.x)
        dsacc[t] += toF<T>(db_[t * NC + i]) * toF<T>(ob[t * NC + i]);
  } else {
    // same thread -> (i, t) assignment and the same order per (thread, t),
    // with t innermost: a node's T values of dout share one cache line
    for (long i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
      const T* dp = db_ + (i / C) * Tst * C + i % C;
      #pragma unroll
      for (int t = 0; t < GATE_MAX_T; ++t)
        if (t < Tst) dsacc[t] += toF<T>(dp[t * C]) * toF<T>(ob[t * NC + i]);
    }
  }
  for (int t = 0; t < Tst; ++t) {
    float v = dsacc[t];
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * GATE_MAX_T + t] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      float tot = 0.f;
      for (int w = 0; w < blockDim.x / 64; ++w) tot += red[w * GATE_MAX_T + t];
      unsafeAtomicAdd(&ds_out[b * Tst + t], tot);
    }
    __syncthreads();
  }

  if (!stm_last_arriver(&tickets[b], gridDim.x, last_flag)) return;
  // tied double-FC backward of row b: s = sig(W u + b), u = relu(W z + b)
  float* dv2 = red;
  float* dv1 = red + GATE_MAX_T;
  const int q = threadIdx.x;
  if (q < Tst) {
    const float sv = s[b * Tst + q];
    dv2[q] = ds_out[b * Tst + q] * sv * (1.f - sv);
  }
  __syncthreads();
  if (q < Tst) {                                    // du = W^T dv2
    float a = 0.f;
    for (int t = 0; t < Tst; ++t) a += toF<T>(fcw[t * Tst + q]) * dv2[t];
    dv1[q] = u[b * Tst + q] > 0.f ? a : 0.f;
  }
  __syncthreads();
  if (q < Tst) {                                    // dz = W^T dv1
    float a = 0.f;
    for (int t = 0; t < Tst; ++t) a += toF<T>(fcw[t * Tst + q]) * dv1[t];
    ds_out[b * Tst + q] = a;
    db_part[b * Tst + q] = dv2[q] + dv1[q];
  }
  // dW partial = dv2 (x) u + dv1 (x) z
  if (q < Tst * Tst) {
    const int t = q / Tst, j = q % Tst;
    dw_part[(b * Tst + t) * Tst + j] =
        dv2[t] * u[b * Tst + j] + dv1[t] * z[b * Tst + j];
  }

  if (!stm_last_arriver(&tickets[B], B, last_flag)) return;
  if (q < Tst * Tst) {
    float a = 0.f;
    for (int bb = 0; bb < B; ++bb) a += dw_part[(long)bb * Tst * Tst + q];
    dw_f[q] = a;
    dw_out[q] = fromF<T>(a);
  }
  if (q < Tst) {
    float a = 0.f;
    for (int bb = 0; bb < B; ++bb) a += db_part[(long)bb * Tst + q];
    db_f[q] = a;
    db_out[q] = fromF<T>(a);
  }
}

// ---- K4 backward part B: dobs = dout*s + dz/N ; dg = dz/N -----------------
// NM: dout is (B,N,T,C). dobs == null (obs needs no gradient): only dg.
template <typename T, bool NM>
__global__ void gate_bwd_scatter_kernel(const T* __restrict__ dout,
                                        const float* __restrict__ s,
                                        const float* __restrict__ dz, // (B,T)
                                        T* __restrict__ dobs,         // (B,T,N,C)
                                        T* __restrict__ dg,           // (B,N,T)
                                        int Tst, int N, int C, float invN,
                                        long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long NC = (long)N * C;
  const long bt = i / NC;
  const long b = bt / Tst;
  const int t = bt % Tst;
  const int n = (i % NC) / C, c = (i % NC) % C;
  const float dzv = dz[bt] * invN;
  if (dobs != nullptr) {
    const long di = NM ? ((b * N + n) * (long)Tst + t) * C + c : i;
    dobs[i] = fromF<T>(toF<T>(dout[di]) * s[bt] + dzv);
  }
  if (c == 0) dg[(b * N + n) * (long)Tst + t] = fromF<T>(dzv);
}

// ---- K7: head y[b,n] = sum_m feats_m[b,n,:] . w + bias --------------------
template <typename T>
__global__ void head_fwd_kernel(const T* __restrict__ f0, const T* __restrict__ f1,
                                const T* __restrict__ f2, const T* __restrict__ w,
                                const T* __restrict__ bias_p, T* __restrict__ y,
                                T* __restrict__ fsum,  // saved (B*N, G)
                                int G, long BN) {
  // one wave per row; lane g covers channel g (G <= 64)
  const long row = ((long)blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int lane = threadIdx.x & 63;
  if (row >= BN) return;
  float v = 0.f;
  if (lane < G) {
    v = toF<T>(f0[row * G + lane]);
    if (f1) v += toF<T>(f1[row * G + lane]);
    if (f2) v += toF<T>(f2[row * G + lane]);
    fsum[row * G + lane] = fromF<T>(v);
    v *= toF<T>(w[lane]);
  }
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if (lane == 0) y[row] = fromF<T>(v + toF<T>(bias_p[0]));
}

// dfeat_m[b,n,g] = dy[b,n] * w[g]  (same for every branch)
template <typename T>
__global__ void head_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ w,
                                T* __restrict__ dfeat, int G, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  dfeat[i] = fromF<T>(toF<T>(dy[i / G]) * toF<T>(w[i % G]));
}

// head wgrad: dw[g] = sum_r dy[r] * fsum[r,g]; db = sum_r dy[r] — a pure
// bandwidth reduction (replaces the last library GEMM on the step: a
// hipBLASLt MT64x16x512 tall-skinny at ~85 us for 1x64 output).
// FIN: the last workgroup to arrive (stm_last_arriver, common.h; the ticket
// sits in the same zeroed workspace as dw / db) writes both in the parameter
// dtype, so no convert launches follow.
template <typename T, bool FIN>
__global__ void head_wgrad_kernel(const T* __restrict__ dy,
                                  const T* __restrict__ fsum,
                                  float* __restrict__ dw,   // (G,) zeroed
                                  float* __restrict__ db,   // (1,) zeroed
                                  int G, long BN, unsigned* ticket,
                                  T* __restrict__ dw_out, T* __restrict__ db_out) {
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const long chunk = (BN + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * chunk;
  const long r1 = (r0 + chunk < BN) ? r0 + chunk : BN;
  // two independent accumulator chains keep 2+ row loads in flight
  float acc = 0.f, acc2 = 0.f, accb = 0.f, accb2 = 0.f;
  long r = r0 + wv;
  for (; r + 4 < r1; r += 8) {
    const float d = toF<T>(dy[r]);        // wave-uniform scalar loads
    const float d2 = toF<T>(dy[r + 4]);
    if (lane < G) {
      acc += d * toF<T>(fsum[r * G + lane]);
      acc2 += d2 * toF<T>(fsum[(r + 4) * G + lane]);
    }
    accb += d;
    accb2 += d2;
  }
  for (; r < r1; r += 4) {
    const float d = toF<T>(dy[r]);
    if (lane < G) acc += d * toF<T>(fsum[r * G + lane]);
    accb += d;
  }
  acc += acc2;
  accb += accb2;
  __shared__ float red[4][64];
  __shared__ float redb[4];
  red[wv][lane] = acc;
  if (lane == 0) redb[wv] = accb;
  __syncthreads();
  if (wv == 0) {
    const float v = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
    if (lane < G) unsafeAtomicAdd(&dw[lane], v);
    if (lane == 0)
      unsafeAtomicAdd(db, redb[0] + redb[1] + redb[2] + redb[3]);
  }
  if constexpr (FIN) {
    // the flag reuses red: wave 0 has consumed it before the helper's barrier
    if (!stm_last_arriver(ticket, gridDim.x, (int*)&red[0][0])) return;
    if (threadIdx.x < G) dw_out[threadIdx.x] = fromF<T>(dw[threadIdx.x]);
    if (threadIdx.x == 64) db_out[0] = fromF<T>(db[0]);
  }
}

// ---- K7 wide: head with O = P*C output columns, 2 <= O <= 32 --------------
// (multi-step horizon; column o = p*C + c). G <= 64 with G % 8 == 0, so a
// lane's 8 channels are all inside or all outside a row and every 16-byte
// access is aligned. The MFMA lane maps are those of mfma_probe_kernel.
#define HEADM_MAX_O 32

// 8 elements of T as one MFMA operand and as one 16-byte word
template <typename T> union HeadFrag {
  uint4 u;
  T t[8];
  typename Frag8<T>::type v;
  __device__ HeadFrag() : u(make_uint4(0u, 0u, 0u, 0u)) {}
};

// y (BN, O) = fsum (BN, G) . W^T + b with fsum = sum_m f_m rounded once to T
// and stored for the backward. One wave per 16 rows, four waves a workgroup.
// A = fsum tile, built in registers from the branch loads (lane: row l % 16,
// channels 32 s + 8 (l / 16) .. + 8 of K-step s; zero for row >= BN or
// channel >= G); B[k][n] = W[n][k], held for the whole kernel (NCT column
// tiles x 2 K-steps, zero for column >= O or channel >= G).
template <typename T, int NCT>
__global__ void head_multi_fwd_kernel(const T* __restrict__ f0,
                                      const T* __restrict__ f1,
                                      const T* __restrict__ f2,
                                      const T* __restrict__ w,      // (O, G)
                                      const T* __restrict__ bias_p, // (O,)
                                      T* __restrict__ y,            // (BN, O)
                                      T* __restrict__ fsum,         // (BN, G)
                                      int G, int O, long BN) {
  const int lane = threadIdx.x & 63;
  const int l16 = lane & 15, lgrp = lane >> 4;
  const long row0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  if (row0 >= BN) return;          // wave-uniform; the kernel has no barrier
  HeadFrag<T> bw[NCT][2];
  #pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
    #pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int o = ct * 16 + l16, k0 = s * 32 + lgrp * 8;
      if (o < O && k0 < G) bw[ct][s].u = *(const uint4*)&w[(long)o * G + k0];
    }
  const long row = row0 + l16;
  f32x4 acc[NCT];
  #pragma unroll
  for (int ct = 0; ct < NCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  #pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int k0 = s * 32 + lgrp * 8;
    HeadFrag<T> a;
    if (row < BN && k0 < G) {
      const long at = row * G + k0;
      HeadFrag<T> x0, x1, x2;
      x0.u = *(const uint4*)&f0[at];
      if (f1) x1.u = *(const uint4*)&f1[at];
      if (f2) x2.u = *(const uint4*)&f2[at];
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = toF<T>(x0.t[j]);
        if (f1) v += toF<T>(x1.t[j]);
        if (f2) v += toF<T>(x2.t[j]);
        a.t[j] = fromF<T>(v);
      }
      *(uint4*)&fsum[at] = a.u;
    }
    #pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
      acc[ct] = mfma16x16x32(a.v, bw[ct][s].v, acc[ct]);
  }
  // D: lane holds rows 4 (l / 16) + r of column l % 16 of each column tile
  #pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int o = ct * 16 + l16;
    if (o >= O) continue;
    const float bv = toF<T>(bias_p[o]);
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long rr = row0 + lgrp * 4 + r;
      if (rr < BN) y[rr * O + o] = fromF<T>(acc[ct][r] + bv);
    }
  }
}

// dfeat (BN, G) = dY (BN, O) . W (O, G), the same for every branch. Computed
// transposed, D'[g][row] = sum_o W[o][g] dY[row][o], so that a lane's four
// accumulators are four consecutive channels of one row: one 8-byte store.
// The reduction index o is padded with zeros to the one K-step of 32. A row
// of dY is O contiguous elements and O need not be a multiple of 8, so both
// operands are guarded element loads: nothing past a row's end is read.
template <typename T>
__global__ void head_multi_bwd_kernel(const T* __restrict__ dy,  // (BN, O)
                                      const T* __restrict__ w,   // (O, G)
                                      T* __restrict__ dfeat,     // (BN, G)
                                      int G, int O, long BN) {
  const int lane = threadIdx.x & 63;
  const int l16 = lane & 15, lgrp = lane >> 4;
  const long row0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  if (row0 >= BN) return;          // wave-uniform; the kernel has no barrier
  const long row = row0 + l16;
  HeadFrag<T> b;                   // B'[k = o][n = row] = dY[row][o]
  if (row < BN) {
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int o = lgrp * 8 + j;
      if (o < O) b.t[j] = dy[row * O + o];
    }
  }
  for (int gt = 0; gt * 16 < G; ++gt) {
    HeadFrag<T> a;                 // A'[m = g][k = o] = W[o][g]
    const int g = gt * 16 + l16;
    if (g < G) {
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int o = lgrp * 8 + j;
        if (o < O) a.t[j] = w[(long)o * G + g];
      }
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = mfma16x16x32(a.v, b.v, acc);
    // D': lane holds channels gt*16 + 4 (l / 16) + r of row l % 16
    const int g0 = gt * 16 + lgrp * 4;
    if (row < BN && g0 < G)
      stm_store4<T>(&dfeat[row * G + g0], acc[0], acc[1], acc[2], acc[3]);
  }
}

// dW (O, G) = dY^T . fsum, db (O,) = colsum(dY): head_wgrad_kernel with up to
// 8 output columns per thread. Wave wv serves column group og = wv % NG (NG =
// ceil(O / 8) groups of 8 columns) and, where NG < 4, every (4 / NG)-th row of
// the workgroup's chunk; lane g owns channel g. The dY values are wave-uniform
// scalar loads; two row chains are in flight. The waves of a column group meet
// in LDS, and one atomic per (o, g) and workgroup goes to the fp32 sums.
// FIN: as in head_wgrad_kernel, the last workgroup to arrive writes dW / db in
// the parameter dtype (the ticket sits in the same zeroed workspace).
template <typename T, bool FIN>
__global__ void head_multi_wgrad_kernel(const T* __restrict__ dy,    // (BN, O)
                                        const T* __restrict__ fsum,  // (BN, G)
                                        float* __restrict__ dw,  // (O*G) zeroed
                                        float* __restrict__ db,  // (O,) zeroed
                                        int G, int O, long BN, unsigned* ticket,
                                        T* __restrict__ dw_out,
                                        T* __restrict__ db_out) {
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int NG = (O + 7) >> 3;            // 1..4
  const int WPG = 4 / NG;                 // waves per column group: 4, 2, 1, 1
  const int og = wv % NG, sub = wv / NG;
  const bool active = sub < WPG;          // NG == 3 leaves wave 3 idle
  const int o0 = og * 8;
  const int no = min(8, O - o0);
  const long chunk = (BN + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * chunk;
  const long r1 = (r0 + chunk < BN) ? r0 + chunk : BN;
  float acc[8], acc2[8], accb[8];
  #pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = acc2[j] = accb[j] = 0.f;
  if (active) {
    const bool in = lane < G;
    long r = r0 + sub;
    for (; r + WPG < r1; r += 2 * WPG) {
      const float f = in ? toF<T>(fsum[r * G + lane]) : 0.f;
      const float f2 = in ? toF<T>(fsum[(r + WPG) * G + lane]) : 0.f;
      #pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < no) {
          const float d = toF<T>(dy[r * O + o0 + j]);
          const float d2 = toF<T>(dy[(r + WPG) * O + o0 + j]);
          acc[j] += d * f;
          acc2[j] += d2 * f2;
          accb[j] += d + d2;
        }
    }
    for (; r < r1; r += WPG) {
      const float f = in ? toF<T>(fsum[r * G + lane]) : 0.f;
      #pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < no) {
          const float d = toF<T>(dy[r * O + o0 + j]);
          acc[j] += d * f;
          accb[j] += d;
        }
    }
  }
  __shared__ float red[4][9][64];         // [wave][8 columns + db][lane]
  #pragma unroll
  for (int j = 0; j < 8; ++j) red[wv][j][lane] = acc[j] + acc2[j];
  // db: lane j of the wave carries column j's sum (every lane has them all)
  {
    float bsel = 0.f;
    #pragma unroll
    for (int j = 0; j < 8; ++j) bsel = (lane == j) ? accb[j] : bsel;
    red[wv][8][lane] = bsel;
  }
  __syncthreads();
  if (wv < NG) {                          // wave og gathers its group's waves
    #pragma unroll
    for (int j = 0; j < 9; ++j) {
      float v = 0.f;
      for (int s = 0; s < WPG; ++s) v += red[wv + s * NG][j][lane];
      if (j < 8) {
        if (j < no && lane < G) unsafeAtomicAdd(&dw[(long)(o0 + j) * G + lane], v);
      } else if (lane < no) {
        unsafeAtomicAdd(&db[o0 + lane], v);
      }
    }
  }
  if constexpr (FIN) {
    // the flag reuses red: its readers are behind the helper's first barrier
    if (!stm_last_arriver(ticket, gridDim.x, (int*)&red[0][0][0])) return;
    // O*G is a multiple of 8: four sums per thread, one 8-byte store each
    for (int i = threadIdx.x * 4; i < O * G; i += 4 * blockDim.x)
      stm_store4<T>(&dw_out[i], dw[i], dw[i + 1], dw[i + 2], dw[i + 3]);
    if (threadIdx.x < O) db_out[threadIdx.x] = fromF<T>(db[threadIdx.x]);
  }
}

// dz = dy * (y > 0): the ReLU mask of the graph-conv backward in one pass.
// The product is formed in fp32 (dy * 1 and dy * 0 are exact), so the result,
// the sign of a zero included, is what dy * (y > 0).to(dtype) gives.
template <typename T>
__global__ void relu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y,
                                T* __restrict__ dz, long n, int vec) {
  const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i0 >= n) return;
  auto one = [&](long i) {
    dz[i] = fromF<T>(toF<T>(dy[i]) * (toF<T>(y[i]) > 0.f ? 1.f : 0.f));
  };
  if (vec && i0 + 8 <= n) {   // 16-byte path (vec: all three bases aligned)
    union { T t[8]; uint4 u; } a, b, o;
    a.u = *(const uint4*)&dy[i0];
    b.u = *(const uint4*)&y[i0];
    #pragma unroll
    for (int j = 0; j < 8; ++j)
      o.t[j] = fromF<T>(toF<T>(a.t[j]) * (toF<T>(b.t[j]) > 0.f ? 1.f : 0.f));
    *(uint4*)&dz[i0] = o.u;
  } else {   // this thread's own 8 elements (fewer at the end), one by one
    const long e = i0 + 8 < n ? i0 + 8 : n;
    for (long i = i0; i < e; ++i) one(i);
  }
}

// ---- K8: fused MSE loss + grad -------------------------------------------
template <typename T>
__global__ void mse_fwd_kernel(const T* __restrict__ pred, const T* __restrict__ tgt,
                               float* __restrict__ loss_out,  // (1,) pre-zeroed
                               T* __restrict__ diff, long n) {
  __shared__ float red[4];
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float v = 0.f;
  if (i < n) {
    const float d = toF<T>(pred[i]) - toF<T>(tgt[i]);
    diff[i] = fromF<T>(d);
    v = d * d;
  }
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicAdd(loss_out, (red[0] + red[1] + red[2] + red[3]) / (float)n);
}

template <typename T>
__global__ void mse_bwd_kernel(const T* __restrict__ diff,
                               const float* __restrict__ gscale,  // d(loss) scalar
                               T* __restrict__ dpred, float two_over_n, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dpred[i] = fromF<T>(toF<T>(diff[i]) * two_over_n * gscale[0]);
}

// ---- K8 masked: MSE / MAE / Huber over the valid targets -------------------
// A missing target is NaN (valid = target == target). loss = sum_valid l(d) /
// max(count_valid, 1), d = pred - target; kind 0: d^2, 1: |d|, 2: Huber with
// delta = 1 (SmoothL1Loss). One pass stores diff (0 on masked elements) and
// reduces sum l(d) and count_valid; the last workgroup to arrive writes the
// loss and 1 / max(count, 1) to device memory, so the host reads nothing and
// the step stays capturable. The sum is fp32 (an f16 sum of 70001 terms would
// overflow); count_valid is summed as a 32-bit unsigned integer, exact for
// every numel below 2^32 (the binding checks that).
#define MLOSS_PER_BLOCK 2048   // 8 elements per thread, 256 apart

template <int KIND> __device__ __forceinline__ float mloss_value(float d) {
  const float a = fabsf(d);
  if (KIND == 0) return d * d;
  if (KIND == 1) return a;
  return a < 1.f ? 0.5f * d * d : a - 0.5f;
}
// l'(d), with sign(0) = 0 for MAE
template <int KIND> __device__ __forceinline__ float mloss_grad(float d) {
  const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  if (KIND == 0) return 2.f * d;
  if (KIND == 1) return sg;
  return fabsf(d) < 1.f ? d : sg;
}

template <typename T, int KIND>
__global__ void masked_loss_fwd_kernel(const T* __restrict__ pred,
                                       const T* __restrict__ tgt,
                                       float* sum,                  // zeroed
                                       unsigned* count,             // zeroed
                                       unsigned* ticket,            // zeroed
                                       float* __restrict__ res,  // loss, 1/count
                                       T* __restrict__ diff, long n) {
  __shared__ float red[4];
  __shared__ unsigned redc[4];
  __shared__ int flag;
  const long base = (long)blockIdx.x * MLOSS_PER_BLOCK + threadIdx.x;
  float v = 0.f;
  unsigned c = 0;
  #pragma unroll
  for (int k = 0; k < MLOSS_PER_BLOCK / 256; ++k) {
    const long i = base + k * 256;
    if (i < n) {
      const float t = toF<T>(tgt[i]);
      const bool valid = t == t;
      const float d = valid ? toF<T>(pred[i]) - t : 0.f;
      diff[i] = fromF<T>(d);
      v += mloss_value<KIND>(d);
      c += valid ? 1u : 0u;
    }
  }
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v += __shfl_down(v, off, 64);
    c += __shfl_down(c, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = v;
    redc[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsafeAtomicAdd(sum, red[0] + red[1] + red[2] + red[3]);
    atomicAdd(count, redc[0] + redc[1] + redc[2] + redc[3]);
  }
  if (!stm_last_arriver(ticket, gridDim.x, &flag)) return;
  if (threadIdx.x == 0) {
    const unsigned cv = *count;
    const float inv = 1.f / (float)(cv > 0u ? cv : 1u);
    res[0] = *sum * inv;
    res[1] = inv;
  }
}

// dpred = l'(diff) * inv_count * gscale. The mask is not saved and the target
// is not read again: a masked element's stored diff is 0, and l'(0) = 0 for
// all three kinds (sign(0) = 0), so its gradient is exactly 0.
template <typename T, int KIND>
__global__ void masked_loss_bwd_kernel(const T* __restrict__ diff,
                                       const float* __restrict__ res,
                                       const float* __restrict__ gscale,
                                       T* __restrict__ dpred, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    dpred[i] = fromF<T>(mloss_grad<KIND>(toF<T>(diff[i])) * (res[1] * gscale[0]));
}

// f(std::integral_constant<int, kind>{}) for kind 0 (mse), 1 (mae), 2 (huber)
template <typename F> const char* mloss_dispatch_kind(int kind, F&& f) {
  switch (kind) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return "stmgcn_masked_loss: kind is not 0 (mse), 1 (mae) or 2 (huber)";
  }
}

// ---- K9: multi-tensor Adam over a flat arena ------------------------------
// torch.optim.Adam semantics: g' = g + wd*p ; m,v updates; p -= lr * mhat /
// (sqrt(vhat) + eps). fp32 master params; T-typed working copy rewritten.
template <typename T>
__global__ void adam_kernel(float* __restrict__ master, T* __restrict__ param,
                            const T* __restrict__ grad, float* __restrict__ m,
                            float* __restrict__ v, const float* __restrict__ hyper,
                            // hyper: lr, beta1, beta2, eps, wd, bc1, bc2
                            long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3],
              wd = hyper[4], bc1 = hyper[5], bc2 = hyper[6];
  const float p = master[i];
  float g = toF<T>(grad[i]) + wd * p;
  const float mn = b1 * m[i] + (1.f - b1) * g;
  const float vn = b2 * v[i] + (1.f - b2) * g * g;
  m[i] = mn; v[i] = vn;
  const float pn = p - lr * (mn / bc1) / (sqrtf(vn / bc2) + eps);
  master[i] = pn;
  param[i] = fromF<T>(pn);
}

// device-side Adam hyper-state advance: keeps the whole optimizer step
// inside a hipGraph (no host-computed bias correction per step).
// hyper: [lr, b1, b2, eps, wd, bc1, bc2, b1pow, b2pow]
__global__ void adam_prep_kernel(float* hyper) {
  if (threadIdx.x == 0) {
    hyper[7] *= hyper[1];
    hyper[8] *= hyper[2];
    hyper[5] = 1.f - hyper[7];
    hyper[6] = 1.f - hyper[8];
  }
}

// chunks so the node reduction fills the chip regardless of B
static int gate_chunks(int B, long work_per_b) {
  long per_chunk = 2048;
  long nch = (work_per_b + per_chunk - 1) / per_chunk;
  long cap = (B > 0) ? (2048 / B > 0 ? 2048 / B : 1) : 1;
  if (nch > cap) nch = cap;
  if (nch < 1) nch = 1;
  return (int)nch;
}

}  // namespace

// ---- K9b: multi-segment gradient gather into the flat Adam arena ----------
// FusedAdam runs autograd with .grad = None (no per-param accumulate-add
// kernels); the fresh grads are packed into the contiguous arena by ONE
// launch per <=64 segments. Null src -> zero-fill (param got no grad).
namespace {
struct GatherSeg {
  const void* src[64];
  long ofs[64];
  int len[64];
};

template <typename T>
__global__ void gather_grads_kernel(GatherSeg a, T* __restrict__ arena,
                                    int nseg) {
  const int seg = blockIdx.x;
  if (seg >= nseg) return;
  T* dst = arena + a.ofs[seg];
  const T* s = (const T*)a.src[seg];
  const int len = a.len[seg];
  const int step = blockDim.x * gridDim.y;
  for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < len; i += step)
    dst[i] = s ? s[i] : fromF<T>(0.f);
}

// one thread per element, 256 per workgroup
inline dim3 grid1d(long total) { return dim3((unsigned)((total + 255) / 256)); }
}  // namespace

// ---- entry points: T comes from the dtype code (stm_dispatch_dtype) --------
extern "C" {

const char* stmgcn_seqsum_permute(void* stream, int dtype, const void* obs, void* out,
                                  int B, int Tst, int N, int C) {
  return stm_dispatch_dtype("stmgcn_seqsum_permute: unsupported dtype code", dtype,
                            [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(seqsum_permute_kernel<T>, grid1d((long)B * N * Tst),
                       dim3(256), 0, (hipStream_t)stream, (const T*)obs, (T*)out,
                       B, Tst, N, C);
    return stm_launched();
  });
}

const char* stmgcn_seqsum_permute_bwd(void* stream, int dtype, const void* dxs,
                                      void* dobs, int B, int Tst, int N, int C) {
  return stm_dispatch_dtype("stmgcn_seqsum_permute_bwd: unsupported dtype code", dtype,
                            [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(seqsum_permute_bwd_kernel<T>,
                       grid1d((long)B * Tst * N * C), dim3(256), 0,
                       (hipStream_t)stream, (const T*)dxs, (T*)dobs, B, Tst, N, C);
    return stm_launched();
  });
}

// z doubles as the zsum atomic target (layout: gate_ws, kernels.h)
const char* stmgcn_gate_fwd(void* stream, int dtype, const GateFwdArgs& a) {
  hipStream_t st = (hipStream_t)stream;
  const int B = a.B, Tst = a.Tst, N = a.N, C = a.C;
  const long total = (long)B * Tst * N * C;
  const GateWs ws = gate_ws(B, Tst, false);
  float* z = a.ws + ws.z;
  unsigned* tickets = (unsigned*)(a.ws + ws.tickets);
  return stm_dispatch_dtype("stmgcn_gate_fwd: unsupported dtype code", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(gate_fwd_reduce_kernel<T>, dim3(gate_chunks(B, N), B),
                       dim3(256), 0, st, (const T*)a.g, (const T*)a.xs, z,
                       (const T*)a.fcw, (const T*)a.fcb, a.u, a.s, tickets, N, Tst);
    if (const char* e = stm_launched()) return e;
    return stm_dispatch_bool(a.node_major != 0, [&](auto nm) {
      hipLaunchKernelGGL((gate_scale_kernel<T, decltype(nm)::value>),
                         grid1d(total), dim3(256), 0, st, (const T*)a.obs, a.s,
                         (T*)a.out, Tst, N, C, total);
      return stm_launched();
    });
  });
}

// dz doubles as the ds atomic target (layout: gate_ws, kernels.h)
const char* stmgcn_gate_bwd(void* stream, int dtype, const GateBwdArgs& a) {
  hipStream_t st = (hipStream_t)stream;
  const int B = a.B, Tst = a.Tst, N = a.N, C = a.C;
  const long total = (long)B * Tst * N * C;
  const float invN = 1.f / (float)N;
  const GateWs ws = gate_ws(B, Tst, true);
  float* dz = a.ws + ws.z;
  unsigned* tickets = (unsigned*)(a.ws + ws.tickets);
  return stm_dispatch_dtype("stmgcn_gate_bwd: unsupported dtype code", dtype, [&](auto t) {
    using T = decltype(t);
    return stm_dispatch_bool(a.node_major != 0, [&](auto nm) {
      constexpr bool NM = decltype(nm)::value;
      hipLaunchKernelGGL((gate_bwd_reduce_kernel<T, NM>),
                         dim3(gate_chunks(B, (long)N * C), B), dim3(256), 0, st,
                         (const T*)a.dout, (const T*)a.obs, dz, (const T*)a.fcw, a.z,
                         a.u, a.s, a.dw_part, a.db_part, tickets, a.dw_f, a.db_f,
                         (T*)a.dw, (T*)a.db, N, C, Tst);
      if (const char* e = stm_launched()) return e;
      hipLaunchKernelGGL((gate_bwd_scatter_kernel<T, NM>), grid1d(total),
                         dim3(256), 0, st, (const T*)a.dout, a.s, dz, (T*)a.dobs,
                         (T*)a.dg, Tst, N, C, invN, total);
      return stm_launched();
    });
  });
}

const char* stmgcn_head_fwd(void* stream, int dtype, const void* f0, const void* f1,
                            const void* f2, const void* w, const void* bias, void* y,
                            void* fsum, int G, long BN) {
  return stm_dispatch_dtype("stmgcn_head_fwd: unsupported dtype code", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(head_fwd_kernel<T>, grid1d(BN * 64), dim3(256), 0,
                       (hipStream_t)stream, (const T*)f0, (const T*)f1,
                       (const T*)f2, (const T*)w, (const T*)bias, (T*)y,
                       (T*)fsum, G, BN);
    return stm_launched();
  });
}

const char* stmgcn_head_bwd(void* stream, int dtype, const void* dy, const void* w,
                            void* dfeat, int G, long BN) {
  const long total = BN * G;
  return stm_dispatch_dtype("stmgcn_head_bwd: unsupported dtype code", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(head_bwd_kernel<T>, grid1d(total), dim3(256), 0,
                       (hipStream_t)stream, (const T*)dy, (const T*)w,
                       (T*)dfeat, G, total);
    return stm_launched();
  });
}

// fill the chip: 128+ blocks at bench size
static long head_wgrad_blocks(long BN) {
  long nblk = (BN + 255) / 256;
  if (nblk > 512) nblk = 512;
  return nblk < 1 ? 1 : nblk;
}

// a.dw_out == null: the accumulate-only form (fp32 sums left in a.ws)
const char* stmgcn_head_wgrad(void* stream, int dtype, const HeadWgradArgs& a) {
  if (a.O != 1 || a.G < 1 || a.G > 64) return "stmgcn_head_wgrad: serves O == 1, G <= 64";
  const HeadWgradWs ws = head_wgrad_ws(a.G, 1);
  const bool finishing = a.dw_out != nullptr;
  unsigned* ticket = finishing ? (unsigned*)(a.ws + ws.ticket) : nullptr;
  return stm_dispatch_dtype("stmgcn_head_wgrad: unsupported dtype code", dtype, [&](auto t) {
    using T = decltype(t);
    return stm_dispatch_bool(finishing, [&](auto fin) {
      hipLaunchKernelGGL((head_wgrad_kernel<T, decltype(fin)::value>),
                         dim3((unsigned)head_wgrad_blocks(a.BN)), dim3(256), 0,
                         (hipStream_t)stream, (const T*)a.dy, (const T*)a.fsum,
                         a.ws + ws.dw, a.ws + ws.db, a.G, a.BN, ticket, (T*)a.dw_out,
                         (T*)a.db_out);
      return stm_launched();
    });
  });
}

static bool head_multi_serves(int G, int O) {
  return O >= 2 && O <= 32 && G >= 8 && G <= 64 && G % 8 == 0;
}

// wide head: one wave per 16 rows, 64 rows per workgroup
const char* stmgcn_head_multi_fwd(void* stream, int dtype, const void* f0,
                                  const void* f1, const void* f2, const void* w,
                                  const void* bias, void* y, void* fsum, int G, int O,
                                  long BN) {
  if (!head_multi_serves(G, O))
    return "stmgcn_head_multi_fwd: serves 2 <= O <= 32, G <= 64 with G % 8 == 0";
  if (BN <= 0) return nullptr;
  const dim3 grid((unsigned)((BN + 63) / 64));
  return stm_dispatch_lowp("stmgcn_head_multi_fwd: dtype code is not bf16/f16", dtype,
                           [&](auto t) {
    using T = decltype(t);
    return stm_dispatch_bool(O > 16, [&](auto two) {
      constexpr int NCT = decltype(two)::value ? 2 : 1;
      hipLaunchKernelGGL((head_multi_fwd_kernel<T, NCT>), grid, dim3(256), 0,
                         (hipStream_t)stream, (const T*)f0, (const T*)f1,
                         (const T*)f2, (const T*)w, (const T*)bias, (T*)y,
                         (T*)fsum, G, O, BN);
      return stm_launched();
    });
  });
}

const char* stmgcn_head_multi_bwd(void* stream, int dtype, const void* dy,
                                  const void* w, void* dfeat, int G, int O, long BN) {
  if (!head_multi_serves(G, O))
    return "stmgcn_head_multi_bwd: serves 2 <= O <= 32, G <= 64 with G % 8 == 0";
  if (BN <= 0) return nullptr;
  return stm_dispatch_lowp("stmgcn_head_multi_bwd: dtype code is not bf16/f16", dtype,
                           [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(head_multi_bwd_kernel<T>,
                       dim3((unsigned)((BN + 63) / 64)), dim3(256), 0,
                       (hipStream_t)stream, (const T*)dy, (const T*)w,
                       (T*)dfeat, G, O, BN);
    return stm_launched();
  });
}

// a.dw_out == null: the accumulate-only form (fp32 sums left in a.ws)
const char* stmgcn_head_multi_wgrad(void* stream, int dtype, const HeadWgradArgs& a) {
  if (!head_multi_serves(a.G, a.O))
    return "stmgcn_head_multi_wgrad: serves 2 <= O <= 32, G <= 64 with G % 8 == 0";
  const HeadWgradWs ws = head_wgrad_ws(a.G, a.O);
  const bool finishing = a.dw_out != nullptr;
  unsigned* ticket = finishing ? (unsigned*)(a.ws + ws.ticket) : nullptr;
  return stm_dispatch_lowp("stmgcn_head_multi_wgrad: dtype code is not bf16/f16", dtype,
                           [&](auto t) {
    using T = decltype(t);
    return stm_dispatch_bool(finishing, [&](auto fin) {
      hipLaunchKernelGGL((head_multi_wgrad_kernel<T, decltype(fin)::value>),
                         dim3((unsigned)head_wgrad_blocks(a.BN)), dim3(256), 0,
                         (hipStream_t)stream, (const T*)a.dy, (const T*)a.fsum,
                         a.ws + ws.dw, a.ws + ws.db, a.G, a.O, a.BN, ticket,
                         (T*)a.dw_out, (T*)a.db_out);
      return stm_launched();
    });
  });
}

// ws: the MLOSS_WS_* words of kernels.h (fp32 sum, unsigned count, ticket);
// res: loss and 1 / max(count, 1); kind 0 mse, 1 mae, 2 huber
const char* stmgcn_masked_loss_fwd(void* stream, int dtype, int kind, const void* pred,
                                   const void* tgt, float* ws, float* res, void* diff,
                                   long n) {
  const dim3 grid((unsigned)((n + MLOSS_PER_BLOCK - 1) / MLOSS_PER_BLOCK));
  return stm_dispatch_dtype("stmgcn_masked_loss_fwd: unsupported dtype code", dtype,
                            [&](auto t) {
    using T = decltype(t);
    return mloss_dispatch_kind(kind, [&](auto k) {
      hipLaunchKernelGGL((masked_loss_fwd_kernel<T, decltype(k)::value>), grid,
                         dim3(256), 0, (hipStream_t)stream, (const T*)pred,
                         (const T*)tgt, ws + MLOSS_WS_SUM,
                         (unsigned*)(ws + MLOSS_WS_COUNT),
                         (unsigned*)(ws + MLOSS_WS_TICKET), res, (T*)diff, n);
      return stm_launched();
    });
  });
}

const char* stmgcn_masked_loss_bwd(void* stream, int dtype, int kind, const void* diff,
                                   const float* res, const float* gscale, void* dpred,
                                   long n) {
  return stm_dispatch_dtype("stmgcn_masked_loss_bwd: unsupported dtype code", dtype,
                            [&](auto t) {
    using T = decltype(t);
    return mloss_dispatch_kind(kind, [&](auto k) {
      hipLaunchKernelGGL((masked_loss_bwd_kernel<T, decltype(k)::value>),
                         grid1d(n), dim3(256), 0, (hipStream_t)stream,
                         (const T*)diff, res, gscale, (T*)dpred, n);
      return stm_launched();
    });
  });
}

const char* stmgcn_relu_bwd(void* stream, int dtype, const void* dy, const void* y,
                            void* dz, long n) {
  if (n <= 0) return nullptr;
  const int vec = (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)dz) & 15) == 0;
  return stm_dispatch_lowp("stmgcn_relu_bwd: dtype code is not bf16/f16", dtype,
                           [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(relu_bwd_kernel<T>, dim3((unsigned)((n + 2047) / 2048)),
                       dim3(256), 0, (hipStream_t)stream, (const T*)dy,
                       (const T*)y, (T*)dz, n, vec);
    return stm_launched();
  });
}

const char* stmgcn_mse_fwd(void* stream, int dtype, const void* pred, const void* tgt,
                           float* loss, void* diff, long n) {
  return stm_dispatch_dtype("stmgcn_mse_fwd: unsupported dtype code", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(mse_fwd_kernel<T>, grid1d(n), dim3(256), 0,
                       (hipStream_t)stream, (const T*)pred, (const T*)tgt, loss,
                       (T*)diff, n);
    return stm_launched();
  });
}

const char* stmgcn_mse_bwd(void* stream, int dtype, const void* diff,
                           const float* gscale, void* dpred, long n) {
  return stm_dispatch_dtype("stmgcn_mse_bwd: unsupported dtype code", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(mse_bwd_kernel<T>, grid1d(n), dim3(256), 0,
                       (hipStream_t)stream, (const T*)diff, gscale, (T*)dpred,
                       2.f / (float)n, n);
    return stm_launched();
  });
}

const char* stmgcn_adam(void* stream, int dtype, float* master, void* param,
                        const void* grad, float* m, float* v, float* hyper, long n) {
  if (dtype < STM_F32 || dtype > STM_F16) return "stmgcn_adam: unsupported dtype code";
  hipLaunchKernelGGL(adam_prep_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hyper);
  if (const char* e = stm_launched()) return e;
  return stm_dispatch_dtype("stmgcn_adam: unsupported dtype code", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(adam_kernel<T>, grid1d(n), dim3(256), 0,
                       (hipStream_t)stream, master, (T*)param, (const T*)grad, m,
                       v, hyper, n);
    return stm_launched();
  });
}

const char* stmgcn_gather_grads(void* stream, int dtype, const void** srcs,
                                const long* ofs, const int* lens, int nseg,
                                void* arena) {
  if (nseg < 1 || nseg > 64) return "stmgcn_gather_grads: segment count outside 1..64";
  GatherSeg a;
  int maxlen = 1;
  for (int i = 0; i < nseg; ++i) {
    a.src[i] = srcs[i]; a.ofs[i] = ofs[i]; a.len[i] = lens[i];
    if (lens[i] > maxlen) maxlen = lens[i];
  }
  const int chunks = min(8, (maxlen + 2047) / 2048);
  return stm_dispatch_dtype("stmgcn_gather_grads: unsupported dtype code", dtype,
                            [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(gather_grads_kernel<T>, dim3(nseg, chunks), dim3(256), 0,
                       (hipStream_t)stream, a, (T*)arena, nseg);
    return stm_launched();
  });
}

}  // extern "C"
