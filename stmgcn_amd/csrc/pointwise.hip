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
//  K8  fused MSE loss + grad  (Model_Trainer.py:38)
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

void stmgcn_seqsum_permute(void* stream, int dtype, const void* obs, void* out,
                           int B, int Tst, int N, int C) {
  stm_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(seqsum_permute_kernel<T>, grid1d((long)B * N * Tst),
                       dim3(256), 0, (hipStream_t)stream, (const T*)obs, (T*)out,
                       B, Tst, N, C);
  });
}

void stmgcn_seqsum_permute_bwd(void* stream, int dtype, const void* dxs,
                               void* dobs, int B, int Tst, int N, int C) {
  stm_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(seqsum_permute_bwd_kernel<T>,
                       grid1d((long)B * Tst * N * C), dim3(256), 0,
                       (hipStream_t)stream, (const T*)dxs, (T*)dobs, B, Tst, N, C);
  });
}

// z (B*T floats) and tickets (B words) share one zero-filled allocation (z
// doubles as the zsum atomic target); node_major: out is (B,N,T,C) instead of
// (B,T,N,C)
void stmgcn_gate_fwd(void* stream, int dtype, const void* g, const void* xs,
                     const void* fcw, const void* fcb, const void* obs,
                     float* z, float* u, float* s, unsigned* tickets, void* out,
                     int B, int Tst, int N, int C, int node_major) {
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)B * Tst * N * C;
  stm_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(gate_fwd_reduce_kernel<T>, dim3(gate_chunks(B, N), B),
                       dim3(256), 0, st, (const T*)g, (const T*)xs, z,
                       (const T*)fcw, (const T*)fcb, u, s, tickets, N, Tst);
    stm_dispatch_bool(node_major != 0, [&](auto nm) {
      hipLaunchKernelGGL((gate_scale_kernel<T, decltype(nm)::value>),
                         grid1d(total), dim3(256), 0, st, (const T*)obs, s,
                         (T*)out, Tst, N, C, total);
    });
  });
}

// dz (B*T floats) and tickets (B + 1 words) share one zero-filled allocation
// (dz doubles as the ds atomic target); dw_f/db_f: fp32 sums over the batch,
// dw/db the same in `dtype`; dobs may be null (obs needs no gradient);
// node_major: dout is (B,N,T,C)
void stmgcn_gate_bwd(void* stream, int dtype, const void* dout, const void* obs,
                     const void* fcw, const float* z, const float* u,
                     const float* s, float* dz, float* dw_part, float* db_part,
                     unsigned* tickets, float* dw_f, float* db_f, void* dw,
                     void* db, void* dobs, void* dg, int B, int Tst, int N, int C,
                     int node_major) {
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)B * Tst * N * C;
  const float invN = 1.f / (float)N;
  stm_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    stm_dispatch_bool(node_major != 0, [&](auto nm) {
      constexpr bool NM = decltype(nm)::value;
      hipLaunchKernelGGL((gate_bwd_reduce_kernel<T, NM>),
                         dim3(gate_chunks(B, (long)N * C), B), dim3(256), 0, st,
                         (const T*)dout, (const T*)obs, dz, (const T*)fcw, z, u,
                         s, dw_part, db_part, tickets, dw_f, db_f, (T*)dw,
                         (T*)db, N, C, Tst);
      hipLaunchKernelGGL((gate_bwd_scatter_kernel<T, NM>), grid1d(total),
                         dim3(256), 0, st, (const T*)dout, s, dz, (T*)dobs,
                         (T*)dg, Tst, N, C, invN, total);
    });
  });
}

void stmgcn_head_fwd(void* stream, int dtype, const void* f0, const void* f1,
                     const void* f2, const void* w, const void* bias, void* y,
                     void* fsum, int G, long BN) {
  stm_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(head_fwd_kernel<T>, grid1d(BN * 64), dim3(256), 0,
                       (hipStream_t)stream, (const T*)f0, (const T*)f1,
                       (const T*)f2, (const T*)w, (const T*)bias, (T*)y,
                       (T*)fsum, G, BN);
  });
}

void stmgcn_head_bwd(void* stream, int dtype, const void* dy, const void* w,
                     void* dfeat, int G, long BN) {
  const long total = BN * G;
  stm_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(head_bwd_kernel<T>, grid1d(total), dim3(256), 0,
                       (hipStream_t)stream, (const T*)dy, (const T*)w,
                       (T*)dfeat, G, total);
  });
}

// ticket == null: the accumulate-only form (fp32 sums left in dw / db);
// otherwise the finishing form, dw_out (G,) / db_out (1,) in the dtype of dy
static void head_wgrad_launch(void* stream, int dtype, const void* dy,
                              const void* fsum, float* dw, float* db,
                              unsigned* ticket, void* dw_out, void* db_out,
                              int G, long BN) {
  long nblk = (BN + 255) / 256;   // fill the chip: 128+ blocks at bench size
  if (nblk > 512) nblk = 512;
  if (nblk < 1) nblk = 1;
  stm_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    stm_dispatch_bool(ticket != nullptr, [&](auto fin) {
      hipLaunchKernelGGL((head_wgrad_kernel<T, decltype(fin)::value>),
                         dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream,
                         (const T*)dy, (const T*)fsum, dw, db, G, BN, ticket,
                         (T*)dw_out, (T*)db_out);
    });
  });
}

void stmgcn_head_wgrad(void* stream, int dtype, const void* dy,
                       const void* fsum, float* dw, float* db, int G,
                       long BN) {
  head_wgrad_launch(stream, dtype, dy, fsum, dw, db, nullptr, nullptr, nullptr,
                    G, BN);
}

void stmgcn_head_wgrad_grads(void* stream, int dtype, const void* dy,
                             const void* fsum, float* dw, float* db,
                             unsigned* ticket, void* dw_out, void* db_out,
                             int G, long BN) {
  head_wgrad_launch(stream, dtype, dy, fsum, dw, db, ticket, dw_out, db_out, G,
                    BN);
}

void stmgcn_relu_bwd(void* stream, int dtype, const void* dy, const void* y,
                     void* dz, long n) {
  if (n <= 0) return;
  const int vec = (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)dz) & 15) == 0;
  stm_dispatch_lowp("stmgcn_relu_bwd", dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(relu_bwd_kernel<T>, dim3((unsigned)((n + 2047) / 2048)),
                       dim3(256), 0, (hipStream_t)stream, (const T*)dy,
                       (const T*)y, (T*)dz, n, vec);
  });
}

void stmgcn_mse_fwd(void* stream, int dtype, const void* pred, const void* tgt,
                    float* loss, void* diff, long n) {
  stm_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(mse_fwd_kernel<T>, grid1d(n), dim3(256), 0,
                       (hipStream_t)stream, (const T*)pred, (const T*)tgt, loss,
                       (T*)diff, n);
  });
}

void stmgcn_mse_bwd(void* stream, int dtype, const void* diff, const float* gscale,
                    void* dpred, long n) {
  stm_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(mse_bwd_kernel<T>, grid1d(n), dim3(256), 0,
                       (hipStream_t)stream, (const T*)diff, gscale, (T*)dpred,
                       2.f / (float)n, n);
  });
}

void stmgcn_adam(void* stream, int dtype, float* master, void* param,
                 const void* grad, float* m, float* v, float* hyper,
                 long n) {
  hipLaunchKernelGGL(adam_prep_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hyper);
  stm_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(adam_kernel<T>, grid1d(n), dim3(256), 0,
                       (hipStream_t)stream, master, (T*)param, (const T*)grad, m,
                       v, hyper, n);
  });
}

void stmgcn_gather_grads(void* stream, int dtype, const void** srcs,
                         const long* ofs, const int* lens, int nseg,
                         void* arena) {
  GatherSeg a;
  int maxlen = 1;
  for (int i = 0; i < nseg && i < 64; ++i) {
    a.src[i] = srcs[i]; a.ofs[i] = ofs[i]; a.len[i] = lens[i];
    if (lens[i] > maxlen) maxlen = lens[i];
  }
  const int chunks = min(8, (maxlen + 2047) / 2048);
  stm_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(gather_grads_kernel<T>, dim3(nseg, chunks), dim3(256), 0,
                       (hipStream_t)stream, a, (T*)arena, nseg);
  });
}

}  // extern "C"
