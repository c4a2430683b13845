// Persistent fused multi-layer LSTM/GRU for CDNA4 (gfx950) — SURVEY K5/K6.
//
// Replaces the reference's nn.LSTM over the flattened (B*N, T, C) sequence
// batch (STMGCN.py:21-22,47-50). One kernel runs ALL layers and ALL
// timesteps: each 256-thread workgroup owns a 32-sequence tile, keeps the
// LIVE hidden state (t-1/t ping/pong) in XOR-swizzled LDS for conflict-free
// ds_read_b128 MFMA fragment reads, computes the recurrent + input
// projections with v_mfma_f32_16x16x32_bf16 matrix cores (fp32 accumulate),
// and applies the gate nonlinearities in the MFMA accumulator fragment
// layout. The cross-LAYER sequence hand-off rides hseq_g in global memory
// (mandatory for the wgrad kernel anyway), with the input fragments
// prefetched one stage ahead.
//
// Geometry per workgroup (H = 64 fixed):
//   4 waves; wave w owns gate-channel slice [16w, 16w+16) of each of the
//   4 (LSTM) / 3 (GRU) gate types -> i/f/g/o for one (seq,channel) pair land
//   in the SAME lane's accumulators, making the cell update lane-local.
//   M = SEQ_TILE = 32 sequences = 2 MFMA row-tiles (at 64 rows the forward
//   needed 230 VGPR + 68 AGPR, one wave per SIMD; 32 rows fit two workgroups
//   per CU); K = H (+C for layers > 0) chunked by 32. Weights are loaded once
//   per layer into VGPR B-fragments (contiguous 16B per lane from the
//   (4H, H|C) row-major weight).
//
// Hand-offs between layers ride global memory, never LDS: forward writes each
// layer's hidden sequence to hseq_g (natural (S_pad, H) order, staged through
// the live LDS slot) and the next layer reads it back; backward passes the
// gradient w.r.t. that sequence through dh_g in fragment-native order.
//
// Saves for BPTT (training): per (layer, t): post-activation gates + cell
// state in fragment-native order (coalesced 16B/lane), plus hseq_g.
//
// fp32/fp64 paths are not served here: bf16/f16 in, fp32 accumulate.

#include "common.h"

// SEQ_TILE (= 32), RNN_H (= 64), MAX_LAYERS and RnnPtrs live in kernels.h;
// common.h fixes the dA tile layout on SEQ_TILE.
static_assert(4 * RNN_H == STM_DA_GATES, "dA tile layout assumes 4H = 256");
#define MAX_T 16

// (The MFMA fragment types, mfma16x16x32 and the LDS swizzle lds_swz for
// 128 B tile rows live in common.h — shared with the wgrad and gconv kernels.)

// ---------------------------------------------------------------------------
// MFMA layout probe (validated on hardware by tests/test_gpu_kernels.py):
// D[16,16] = A[16,32] @ B[32,16] with the assumed fragment maps:
//   A: lane l holds A[l%16][(l/16)*8 + j], j = 0..7
//   B: lane l holds B[(l/16)*8 + j][l%16]
//   C/D: lane l holds D[(l/16)*4 + r][l%16], r = 0..3
extern "C" __global__ void mfma_probe_kernel(const __hip_bfloat16* A,
                                             const __hip_bfloat16* B, float* D) {
  const int l = threadIdx.x;
  bf16x8 a, b;
  #pragma unroll
      for (int j = 0; j < 8; ++j) {
    a[j] = *(const __bf16*)&A[(l % 16) * 32 + (l / 16) * 8 + j];
    b[j] = *(const __bf16*)&B[((l / 16) * 8 + j) * 16 + (l % 16)];
  }
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = mfma16x16x32(a, b, c);
  #pragma unroll
      for (int r = 0; r < 4; ++r) D[((l / 16) * 4 + r) * 16 + (l % 16)] = c[r];
}

// f(std::true_type{}) or f(std::false_type{}) for a workgroup-uniform flag:
// the device-side twin of stm_dispatch_bool
template <typename F> __device__ __forceinline__ void rnn_uniform_bool(bool flag, F&& f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

// ---------------------------------------------------------------------------
// Fused LSTM/GRU forward.
//
// Template: T = element type (bf16/f16), CIN1 = first-layer input_dim == 1
// (base ST-MGCN; otherwise C_in == H, the stacked deep-variant blocks),
// GRU = cell type (the deep variant, BASELINE configs[3]).
//
// GRU rides the 4-gate MFMA structure via host-side weight packing: the
// 4 q-slots carry [r | z | n_input | n_hidden] with
//   W_ih_packed = [Wr; Wz; Wn; 0],  W_hh_packed = [Ur; Uz; 0; Un],
//   bias_packed = [bir+bhr; biz+bhz; bin; bhn]
// so acc[2] = Wn x + bin and acc[3] = Un h + bhn arrive separately and the
// pointwise phase computes n = tanh(acc2 + r*acc3), h' = (1-z) n + z h_prev.
// The c_state register carry doubles as the GRU h_prev; the cseq training
// save holds h_{t-1} (GRU) instead of c_t (LSTM). Everything else — LDS
// staging, MFMA tiling, dA streaming, the batched wgrad kernel — is shared.
//
// LDS holds only the LIVE state: two ping/pong h slots (t-1 and t of the
// CURRENT layer, parity-indexed). The cross-layer sequence hand-off goes
// through hseq_g in GLOBAL memory — in training those writes were already
// mandatory (the wgrad kernel consumes hseq_g), so the hand-off is free and
// LDS drops from (2*Tst+eps) slots (64 KB at T=8 -> 2 workgroups/CU) to
// 2 slots (~8.5 KB -> occupancy is register-bound at 4 waves/SIMD instead).
// CIN1 additionally stages the scalar input sequence ([Tst][SEQ_TILE] T).
template <typename T, bool CIN1, bool GRU>
__global__ void __launch_bounds__(256, 2)
lstm_fwd_kernel(const T* __restrict__ x,    // (S, Tst, C_in)
                T* __restrict__ out,        // (S, H) or (S, Tst, H)
                T* __restrict__ hseq_g,     // (L, Tst, S_pad, H) — ALWAYS
                                            // (layer hand-off + wgrad save)
                T* __restrict__ cseq_g,     // (L, Tst, S_pad*H) frag-native
                                            // (LSTM c_t / GRU h_{t-1})
                T* __restrict__ gates_g,    // (L, Tst, S_pad*4H) frag-native
                RnnPtrs ptrs,
                int S, int Tst, int L, int ret_seq) {
  using frag = typename Frag8<T>::type;
  using elem = typename Frag8<T>::elem;
  typedef elem elem4 __attribute__((ext_vector_type(4)));
  constexpr int MT = SEQ_TILE / 16;        // MFMA row-tiles per wave
  constexpr int SLOT = SEQ_TILE * 128;     // one timestep LDS slot, bytes
  extern __shared__ char lds[];
  const int s0 = blockIdx.x * SEQ_TILE;
  const int wv = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int l16 = lane & 15;
  const int lgrp = lane >> 4;
  const long S_pad = (long)gridDim.x * SEQ_TILE;

  // ping/pong h slots by t parity (explicit ternary: an LDS-pointer array
  // initializer is rejected by the AMDGPU backend)
  auto hslot = [&](int par) -> char* { return lds + (par & 1) * SLOT; };
  char* xbuf = lds + 2 * SLOT;                 // CIN1 scalar input stage

  // ---- stage scalar input x into LDS (CIN1 only) -------------------------
  if (CIN1) {
    for (int i = threadIdx.x; i < SEQ_TILE * Tst; i += 256) {
      const int s = i % SEQ_TILE, t = i / SEQ_TILE;
      T v = fromF<T>(0.f);
      if (s0 + s < S) v = x[(long)(s0 + s) * Tst + t];
      ((T*)xbuf)[t * SEQ_TILE + s] = v;
    }
    __syncthreads();
  }

  const int hch = 16 * wv + l16;                      // this lane's h channel
  // The lane's part of every global address, as small byte offsets; what is
  // added to them per layer and stage is workgroup-uniform (one offset
  // register serves all fragments of a stream instead of a 64-bit address each)
  const unsigned wlane = (hch * RNN_H + lgrp * 8) * sizeof(T);      // weight row hch
  const unsigned inlane = (l16 * RNN_H + lgrp * 8) * sizeof(T);     // hseq rows as A fragments
  const unsigned savelane = (wv * MT * 64 + lane) * sizeof(T);      // fragment-native saves

  // One layer: a straight-line body per combination of the workgroup-uniform
  // conditions FIRST (layer 0: the scalar-input layer of a cin = 1 model has
  // no input GEMM and adds its rank-1 input term in the pointwise phase; a
  // dense layer 0 reads x, guarded, instead of the hand-off), TRAIN (the
  // gates / cell saves exist) and TOP (the layer that writes `out`). A stage
  // then holds no code of another form: the kernel is bound by instruction
  // issue in its pointwise phase (profiles/lstm_fwd_stage.md).
  auto layer_body = [&](int layer, auto first_c, auto train_c, auto top_c) {
    constexpr bool FIRST = decltype(first_c)::value;
    constexpr bool TRAIN = decltype(train_c)::value;
    constexpr bool TOP = decltype(top_c)::value;
    constexpr bool SCALAR = CIN1 && FIRST;
    constexpr bool KEEP_H = TRAIN || !TOP;   // the top layer's sequence is dead in eval
    const char* Whh = (const char*)ptrs.w_hh[layer];
    const char* Wih = (const char*)ptrs.w_ih[layer];
    const T* bih = (const T*)ptrs.b_ih[layer];
    const T* bhh = (const T*)ptrs.b_hh[layer];

    // previous layer's output sequence (global hand-off; L2-hot: this block
    // wrote the same tile last layer), or the dense x of layer 0
    const T* hin = FIRST ? nullptr
        : hseq_g + ((long)(layer - 1) * Tst) * (S_pad * RNN_H) + (long)s0 * RNN_H;

    // input-term fragments, prefetched one stage ahead (single-buffered:
    // reloaded right after their MFMAs consume them, so the global loads
    // get a full stage of slack instead of stalling inside the MFMA loop)
    frag xfr[MT][2];
    auto load_input = [&](int t) {
      #pragma unroll
      for (int m = 0; m < MT; ++m) {
        #pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          if constexpr (FIRST) {       // dense x (S, Tst, 64): guard the tail
            const char* xt = (const char*)(x + ((long)(s0 + 16 * m) * Tst + t) * RNN_H);
            const unsigned xlane = (l16 * Tst * RNN_H + lgrp * 8) * sizeof(T);
            xfr[m][kk] = frag{};
            if (s0 + 16 * m + l16 < S)
              xfr[m][kk] = *(const frag*)(xt + (xlane + kk * 32 * sizeof(T)));
          } else {
            const char* ht = (const char*)(hin + (long)t * (S_pad * RNN_H));
            xfr[m][kk] = *(const frag*)(ht + (inlane + (m * 16 * RNN_H + kk * 32) * sizeof(T)));
          }
        }
      }
    };
    if constexpr (!SCALAR) load_input(0);

    // B-fragments for the recurrent GEMM: b_hh[q][kk]; W row g = q*64 + hch,
    // cols kk*32 + lgrp*8 .. +8 -> contiguous 16B in the (4H, H) weight.
    frag bhfrag[4][2];
    #pragma unroll
    for (int q = 0; q < 4; ++q)
      #pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        bhfrag[q][kk] = *(const frag*)(Whh + (wlane + (q * 64 * RNN_H + kk * 32) * sizeof(T)));
    // input-projection B-fragments (layers with an input GEMM)
    frag bxfrag[4][2];
    if constexpr (!SCALAR) {
      #pragma unroll
      for (int q = 0; q < 4; ++q)
        #pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          bxfrag[q][kk] = *(const frag*)(Wih + (wlane + (q * 64 * RNN_H + kk * 32) * sizeof(T)));
    }
    // scalar-input layer: W_ih[g][0]
    float wih0[4];
    float bias[4];
    #pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int g = q * 64 + hch;
      bias[q] = toF<T>(bih[g]) + toF<T>(bhh[g]);
      if constexpr (SCALAR) wih0[q] = toF<T>(((const T*)Wih)[g]);
    }

    float c_state[MT][4];  // [m][reg]
    #pragma unroll
    for (int m = 0; m < MT; ++m)
      #pragma unroll
      for (int r = 0; r < 4; ++r) c_state[m][r] = 0.f;

    #pragma clang loop unroll(disable)   // no peeled first or last stage
    for (int t = 0; t < Tst; ++t) {
      f32x4 acc[MT][4];  // [m][q]
      const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

      // recurrent term: h_{t-1} from the previous parity slot (zero at t==0);
      // the first MFMA of a chain takes the constant 0 as its accumulator
      if (t > 0) {
        char* slot = hslot(t - 1);
        #pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int row = 16 * m + l16;
          #pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            frag a = *(const frag*)&slot[lds_swz(row, (kk * 32 + lgrp * 8) * 2)];
            #pragma unroll
            for (int q = 0; q < 4; ++q)
              acc[m][q] = mfma16x16x32(a, bhfrag[q][kk], kk == 0 ? zero4 : acc[m][q]);
          }
        }
      } else {
        // (the empty asm keeps this a block of its own: without it the 32
        // zero moves are hoisted in front of the branch, into every stage.
        // Speed only, and seen in the ISA of this hipcc: the census in
        // profiles/lstm_fwd_stage.md shows 2 moves per stage when it holds)
        asm volatile("");
        #pragma unroll
        for (int m = 0; m < MT; ++m)
          #pragma unroll
          for (int q = 0; q < 4; ++q) acc[m][q] = zero4;
      }
      // input term: the fragments were prefetched last stage; reload for t+1
      // right away
      if constexpr (!SCALAR) {
        #pragma unroll
        for (int m = 0; m < MT; ++m)
          #pragma unroll
          for (int kk = 0; kk < 2; ++kk)
            #pragma unroll
            for (int q = 0; q < 4; ++q)
              acc[m][q] = mfma16x16x32(xfr[m][kk], bxfrag[q][kk], acc[m][q]);
        if (t + 1 < Tst) load_input(t + 1);
      }

      // pointwise cell update in fragment layout (+ the scalar-input term).
      // Every rounding is pinned (stm_fmul / stm_fadd / fmaf): the results are
      // those of the form this kernel had when its arithmetic was left to the
      // compiler's FMA contraction. That fused the product of the GRU's n,
      // one product of its h (z h_prev in the f16 scalar-input instantiation,
      // (1-z) n in the others) and, in the dense-input instantiations only,
      // f c of the LSTM's c; the scalar-input term was never fused.
      constexpr bool GRU_FUSED_ZH = CIN1 && std::is_same<T, __half>::value;
      T hval[MT][4];     // [m][reg] this lane's h outputs (ch = hch)
      // training saves, rounded element by element into the vectors their
      // stores send (two values per v_cvt_pk, no packing arithmetic):
      // gsave[m] = [i f | g o] (GRU: [r z | n Bn]) x [reg] post-activation
      // gates, csave[m] = [reg] LSTM c_t / GRU h_{t-1}
      frag gsave[MT][2];
      elem4 csave[MT];
      #pragma unroll
      for (int m = 0; m < MT; ++m) {
        float xv[4];
        if constexpr (SCALAR) {
          #pragma unroll
          for (int r = 0; r < 4; ++r)
            xv[r] = toF<T>(((const T*)xbuf)[t * SEQ_TILE + 16 * m + 4 * lgrp + r]);
        }
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          float pre[4];
          #pragma unroll
          for (int q = 0; q < 4; ++q) {
            pre[q] = stm_fadd(acc[m][q][r], bias[q]);
            if constexpr (SCALAR) pre[q] = stm_fadd(pre[q], stm_fmul(xv[r], wih0[q]));
          }
          const float gi = pre[0], gf = pre[1], gg = pre[2], go = pre[3];
          if constexpr (GRU) {
            // q-slots: gi = r-pre, gf = z-pre, gg = n_input, go = n_hidden
            const float r_ = stm_sigmoid(gi), z_ = stm_sigmoid(gf);
            const float n_ = stm_tanh(fmaf(r_, go, gg));
            const float hprev = c_state[m][r];
            csave[m][r] = (elem)hprev;                  // bwd needs h_{t-1}
            const float zn = stm_fmul(1.f - z_, n_);     // GRU_FUSED_ZH only
            const float h_ = GRU_FUSED_ZH ? fmaf(z_, hprev, zn)
                                          : fmaf(1.f - z_, n_, stm_fmul(z_, hprev));
            c_state[m][r] = h_;
            if constexpr (GRU_FUSED_ZH) {
              // ... and that instantiation rounded the f16 h straight from the
              // fused sum, not from its fp32 value. (GRU_FUSED_ZH and this asm
              // only keep old bits: both can go with the first change that is
              // allowed to move them.)
              unsigned hw;
              asm("v_fma_mixlo_f16 %0, %1, %2, %3"
                  : "=v"(hw) : "v"(hprev), "v"(z_), "v"(zn));
              hval[m][r] = __builtin_bit_cast(T, (unsigned short)hw);
            } else {
              hval[m][r] = fromF<T>(h_);
            }
            gsave[m][0][0 + r] = (elem)r_;
            gsave[m][0][4 + r] = (elem)z_;
            gsave[m][1][0 + r] = (elem)n_;
            gsave[m][1][4 + r] = (elem)go;   // Bn = Un h + bhn
          } else {
            const float i_ = stm_sigmoid(gi), f_ = stm_sigmoid(gf);
            const float g_ = stm_tanh(gg), o_ = stm_sigmoid(go);
            const float ig = stm_fmul(i_, g_);
            const float c_ = CIN1 ? stm_fadd(stm_fmul(f_, c_state[m][r]), ig)
                                  : fmaf(f_, c_state[m][r], ig);
            c_state[m][r] = c_;
            csave[m][r] = (elem)c_;
            const float h_ = stm_fmul(o_, stm_tanh(c_));
            hval[m][r] = fromF<T>(h_);
            gsave[m][0][0 + r] = (elem)i_;
            gsave[m][0][4 + r] = (elem)f_;
            gsave[m][1][0 + r] = (elem)g_;
            gsave[m][1][4 + r] = (elem)o_;
          }
        }
      }

      // write h_t into the parity slot: stage t-1's readers of this slot
      // (= slot (t-2)&1 == t&1) finished before the previous stage barrier
      {
        char* slot = hslot(t);
        #pragma unroll
        for (int m = 0; m < MT; ++m)
          #pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * m + 4 * lgrp + r;
            *(T*)&slot[lds_swz(row, hch * 2)] = hval[m][r];
          }
      }
      __syncthreads();

      // hand the slot off to global (next layer's input + wgrad/out source;
      // the last layer's sequence is dead in eval — only `out` is written)
      {
        static_assert(SEQ_TILE * 8 == 256, "one 16 B piece of the slot per thread");
        const int c8 = threadIdx.x & 7, sr = threadIdx.x >> 3;
        const frag v = *(const frag*)&hslot(t)[lds_swz(sr, c8 * 16)];
        if constexpr (KEEP_H) {
          char* hp = (char*)(hseq_g + ((long)layer * Tst + t) * (S_pad * RNN_H)
                             + (long)s0 * RNN_H);
          *(frag*)(hp + threadIdx.x * 16) = v;
        }
        if constexpr (TOP) {
          if (s0 + sr < S) {
            if (ret_seq)
              *(frag*)&out[((long)(s0 + sr) * Tst + t) * RNN_H + c8 * 8] = v;
            else if (t == Tst - 1)
              *(frag*)&out[(long)(s0 + sr) * RNN_H + c8 * 8] = v;
          }
        }
      }

      // training saves: gates + cell, fragment-native (16B contiguous/lane)
      if constexpr (TRAIN) {
        const long base = ((long)layer * Tst + t);
        // gates: (L,Tst, S_pad*4H) as [wave][m][lane][16] T
        char* gp = (char*)(gates_g + base * (S_pad * 4 * RNN_H)
                           + (long)blockIdx.x * (SEQ_TILE * 4 * RNN_H));
        #pragma unroll
        for (int m = 0; m < MT; ++m)
          #pragma unroll
          for (int hq = 0; hq < 2; ++hq)
            *(frag*)(gp + (savelane * 16 + (m * 64 * 16 + hq * 8) * sizeof(T))) = gsave[m][hq];
        // cell: (L,Tst, S_pad*H) model-dtype as [wave][m][lane][4]
        // (LSTM: c_t; GRU: h_{t-1}) — T-typed save halves HBM traffic vs
        // fp32; bwd tolerances cover the rounding (tests at 8% rel)
        char* cp = (char*)(cseq_g + base * (S_pad * RNN_H)
                           + (long)blockIdx.x * (SEQ_TILE * RNN_H));
        #pragma unroll
        for (int m = 0; m < MT; ++m)
          *(elem4*)(cp + (savelane * 4 + m * 64 * 4 * sizeof(T))) = csave[m];
      }
    }
  };

  for (int layer = 0; layer < L; ++layer) {
    rnn_uniform_bool(layer == 0, [&](auto first_c) {
      rnn_uniform_bool(gates_g != nullptr, [&](auto train_c) {
        rnn_uniform_bool(layer == L - 1, [&](auto top_c) {
          layer_body(layer, first_c, train_c, top_c);
        });
      });
    });
    // layer boundary: the hseq_g stores must be visible to this block's
    // next-layer input loads (workgroup-scope fence + barrier)
    __threadfence_block();
    __syncthreads();
  }
}

// f(CIN1, GRU) as std::bool_constant values: the kernel variant of a launch
template <typename F> const char* rnn_dispatch_variant(int cin, int gru, F&& f) {
  return stm_dispatch_bool(cin == 1, [&](auto cin1) {
    return stm_dispatch_bool(gru != 0, [&](auto is_gru) { return f(cin1, is_gru); });
  });
}

// the shapes both RNN kernels serve
static bool rnn_serves(int S, int Tst, int L, int cin) {
  return S >= 1 && L >= 1 && L <= MAX_LAYERS && Tst >= 1 && Tst <= MAX_T &&
         (cin == 1 || cin == RNN_H);
}

extern "C" const char* stmgcn_lstm_fwd(void* stream, int dtype, const LstmFwdArgs& a) {
  if (!rnn_serves(a.S, a.Tst, a.L, a.cin))
    return "stmgcn_lstm_fwd: serves 1..8 layers, 1..16 steps, input width 1 or 64";
  const int nblk = (a.S + SEQ_TILE - 1) / SEQ_TILE;
  return stm_dispatch_lowp("stmgcn_lstm_fwd: dtype code is not bf16/f16", dtype, [&](auto t) {
    using T = decltype(t);
    // two h slots + the CIN1 scalar input stage
    const size_t lds_bytes =
        2 * SEQ_TILE * 128 + (a.cin == 1 ? a.Tst * SEQ_TILE * sizeof(T) : 0);
    return rnn_dispatch_variant(a.cin, a.gru, [&](auto cin1, auto is_gru) {
      hipLaunchKernelGGL(
          (lstm_fwd_kernel<T, decltype(cin1)::value, decltype(is_gru)::value>),
          dim3(nblk), dim3(256), lds_bytes, (hipStream_t)stream, (const T*)a.x,
          (T*)a.out, (T*)a.hseq, (T*)a.cseq, (T*)a.gates, a.w, a.S, a.Tst, a.L,
          a.ret_seq);
      return stm_launched();
    });
  });
}

extern "C" const char* stmgcn_mfma_probe(void* stream_v, const void* A, const void* B,
                                         void* D) {
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0,
                     (hipStream_t)stream_v, (const __hip_bfloat16*)A,
                     (const __hip_bfloat16*)B, (float*)D);
  return stm_launched();
}

// ===========================================================================
// Fused LSTM backward, dgrad part (BPTT in-kernel) — SURVEY K10.
//
// Same workgroup geometry as forward. Layers walk top-down, timesteps in
// reverse. Per step the pointwise phase turns (dh, dc, saved gates, saved
// cell) into gate-preactivation grads dA — lane-local in the MFMA fragment
// layout — then two MFMA GEMMs, run from one K loop over the shared dA
// fragments, produce dh_{t-1} (recurrent carry, kept in registers) and dx_t
// (written to the global dh_g hand-off for the layer below, or to the dx
// output at layer 0). dA is also streamed to global in the tiled
// wgrad-fragment order documented in common.h (each lane's 8 values per gate
// slot are one 16 B store); lstm_wgrad_kernel (wgrad.hip) then forms all
// weight gradients dW = dA^T @ [h_prev | x] in one launch, which keeps this
// kernel lean (no long-lived dW accumulators).
//
// The kernel is latency-bound (two workgroups per CU, a serial dh chain), so
// a (layer, t) stage is laid out around what each s_waitcnt has to retire;
// vmcnt retires in issue order (profiles/lstm_bwd_stage_waits.md):
//   layer prologue     the lane's 8 W_hh^T fragments -> its LDS slots; a top
//                      layer that returns only the last step takes dout as
//                      its initial dh_rec here
//   pointwise phase    one straight-line body per layer form (layer_body), no
//                      branch and no vector-memory wait (all saves come from
//                      lane-private LDS slots; a ret_seq top layer's dout
//                      loads, waited for once, are the exception); the dA
//                      tile goes to LDS as a [gate column][row] image, 8 x
//                      ds_write_b64; the scalar-input layer 0 alone computes
//                      and reduces its dx partials (DPP)
//   issue              W_ih^T fragments (L2), THEN the next stage's saves
//                      (gates, c, upstream dh: HBM), THEN the dA stores
//   barrier            dA tile visible
//   GEMM1 + GEMM2      A fragments by ds_read_b64_tr_b16 (EXEC is all ones:
//                      every branch around a stage is workgroup-uniform);
//                      W_hh^T from LDS (lgkmcnt only); counted waits on W_ih^T
//                      that leave the saves and the stores in flight
//   dx / dh_g stores
//   stage-in           the one wait for the saves; the stores stay in flight
//   barrier            the next pointwise phase may overwrite the dA tile

// four fp32 values rounded to T, as ONE 64-bit value (not four halves that
// the compiler may keep in separate registers)
template <typename T> __device__ __forceinline__ unsigned long pack4_word(f32x4 v) {
  unsigned long w = 0;
  #pragma unroll
  for (int r = 0; r < 4; ++r)
    w |= (unsigned long)__builtin_bit_cast(unsigned short, fromF<T>(v[r])) << (16 * r);
  return w;
}

// v + (v of the lane that DPP control CTRL pairs this lane with, same row)
// (every lane of the row is read and written — full row / bank masks and
// controls that pair each lane with a lane of its row — so bound_ctrl changes
// no value; it frees the move's `old` operand, and the move folds into the add)
template <int CTRL> __device__ __forceinline__ float dpp_row_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(
                 0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// The dA tile in LDS is a [gate column c = 0..255][tile row s = 0..31] image
// with 64 B rows: the dgrad GEMMs sum over the gate column, which is the LANE
// index of the pointwise layout, so the tile is written as it falls (a lane's
// rows 4*lgrp + r of one (gate slot, m-tile) are 8 contiguous bytes: 8-byte
// slot 4*m + lgrp of row c) and read back transposed by ds_read_b64_tr_b16.
// The slot index is XORed with (c >> 1) & 7. Writes (32 banks, 16 consecutive
// lanes = 16 consecutive c per access): c & 1 picks the 64 B half of the
// 128 B bank row and (c >> 1) & 7 permutes the 8 slots of that half — 16
// distinct 8 B bank pairs. Transposed reads (64 banks, 32 lanes per access =
// image rows c0 .. c0+3 and c0+8 .. c0+11, four slots 4*m + p each): c & 3
// picks the 64 B quarter of the 256 B bank row, and bit 3 of c flips bit 2 of
// the slot, so the two row groups take the two halves of the quarter. Both
// sides are conflict-free (profiles/lstm_bwd_pointwise.md).
__device__ __forceinline__ int dA_img(int c, int slot) {
  return c * 64 + ((slot ^ ((c >> 1) & 7)) << 3);
}

// a * b rounded to T, the last product of a dA value. bf16 rounds the fp32
// product; f16 rounds the exact product once (v_fma_mixlo_f16), the form the
// compiler picks for all but a few elements when the choice is left to it.
template <typename T> __device__ __forceinline__ T stm_fmul_to(float a, float b) {
  if constexpr (std::is_same<T, __half>::value) {
    unsigned hw;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hw) : "v"(a), "v"(b));
    return __builtin_bit_cast(T, (unsigned short)hw);
  } else {
    return fromF<T>(stm_fmul(a, b));
  }
}

// GRU backward (same packed-slot scheme as forward — see lstm_fwd_kernel):
// saved gates = [r, z, n, Bn], cseq = h_{t-1}; emits packed
// dA = [dr_pre, dz_pre, dn_pre, dBn] so the dgrad GEMMs against the packed
// transposed weights and the batched wgrad kernel run unchanged. The direct
// dh_{t-1} += dh_t * z term rides the dc[][] register carry.
template <typename T, bool CIN1, bool GRU>
__global__ void __launch_bounds__(256, 2)
lstm_bwd_kernel(const T* __restrict__ dout,     // (S,H) or (S,Tst,H)
                const T* __restrict__ x,        // (S,Tst,Cin)
                const T* __restrict__ cseq_g,   // model dtype (see fwd)
                const T* __restrict__ gates_g,
                RnnPtrs w,                      // w_ih/w_hh = TRANSPOSED (C|H, 4H)
                T* __restrict__ dx,             // (S,Tst,Cin)
                T* __restrict__ dA_g,           // (L,Tst,S_pad,4H) tiled
                T* __restrict__ dh_g,           // (Tst,S_pad,H) layer hand-off
                                                // scratch (null when L == 1)
                int S, int Tst, int L, int ret_seq) {
  using frag = typename Frag8<T>::type;
  using elem = typename Frag8<T>::elem;
  constexpr int MT = SEQ_TILE / 16;
  extern __shared__ char lds[];
  const int s0 = blockIdx.x * SEQ_TILE;
  const int wv = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int l16 = lane & 15;
  const int lgrp = lane >> 4;
  const long S_pad = (long)gridDim.x * SEQ_TILE;
  const int hch = 16 * wv + l16;

  // LDS, 76.5 KB, two workgroups per CU (the register allocation allows no
  // more): ONE dA tile (the barrier at the end of a stage keeps the next
  // pointwise phase from overwriting it under a wave that still reads it),
  // the CIN1 dx reduction scratch, the lane-private parking of the saves and
  // the layer's W_hh^T. The cross-layer dh hand-off lives in GLOBAL scratch
  // dh_g.
  char* dA_lds = lds;                         // [256 gate columns][64 B] (dA_img)
  float* red = (float*)(dA_lds + SEQ_TILE * 512);   // [4][SEQ_TILE] cross-wave scratch
  // lane-PRIVATE gates staging (each lane writes exactly the 2*MT fragments
  // it alone reads next stage -> no cross-wave visibility, no barrier, and
  // the prefetched tile costs LDS instead of 32 live VGPRs)
  char* gstage = (char*)(red + 4 * SEQ_TILE);       // [256][MT*32B]
  // lane-private packed saves, parked the same way: the upstream dh words of
  // the stage ([256][MT*8B]) and the cell words by timestep parity
  // ([2][256][MT*8B]: stage t reads c_t from slot t&1 and c_{t-1} from the
  // other, and its prefetched c_{t-2} replaces the dead c_t, so nothing
  // rotates). They go from the load's registers to LDS untouched.
  char* dhstage = gstage + 256 * (MT * 32);
  char* cstage = dhstage + 256 * (MT * 8);
  // W_hh^T of the current layer in B-fragment order, [kk][256 lanes][16 B]:
  // every lane stages, once per layer, exactly the 8 fragments it reads in
  // each stage (lane-private like the slots above: no barrier), so GEMM1 —
  // the GEMM on the serial dh chain — waits on lgkmcnt only and its weights
  // are off the vector-memory queue. A wave's ds_read_b128 is 1 KiB contiguous.
  char* wstage = cstage + 2 * 256 * (MT * 8);
  char* wmine = wstage + threadIdx.x * 16;

  // the lane's part of the dA image addresses: its two 8-byte write slots of
  // row hch (the gate slot q adds q * 4096) and the four read pieces of a
  // k-step (lane 4*qq + p of a 16-lane group names row qq, slot 4*m + p of
  // the group's 4-row block; the k-step kk adds kk * 2048)
  int dA_wr[MT], dA_rd[2][MT];
  #pragma unroll
  for (int m = 0; m < MT; ++m) {
    dA_wr[m] = dA_img(hch, 4 * m + lgrp);
    #pragma unroll
    for (int hf = 0; hf < 2; ++hf)
      dA_rd[hf][m] = dA_img(8 * lgrp + 4 * hf + (l16 >> 2), 4 * m + (l16 & 3));
  }

  // One layer: a straight-line body per combination of the workgroup-uniform
  // conditions SCALAR (the scalar-input layer 0 of a cin = 1 model: no input
  // GEMM, its dx is the rank-1 term reduced in the pointwise phase) and where
  // dh comes from besides the recurrent carry — DH_UP: the layer above
  // (dh_g), DH_SEQ: dout at every stage (top layer, ret_seq), DH_LAST: dout
  // at the last timestep only (top layer, the flagship), where dh_rec is
  // still 0: it IS the initial dh_rec, loaded in the layer prologue, and the
  // t loop holds no dout code. A stage then holds no code of another form and
  // no per-element branch: the pointwise phase is bound by instruction issue
  // (profiles/lstm_bwd_pointwise.md).
  constexpr int DH_UP = 0, DH_SEQ = 1, DH_LAST = 2;
  auto layer_body = [&](int layer, auto scalar_c, auto src_c) {
    constexpr bool SCALAR = CIN1 && decltype(scalar_c)::value;
    constexpr int SRC = decltype(src_c)::value;
    const T* WhhT = (const T*)w.w_hh[layer];  // (H, 4H)
    const T* WihT = (const T*)w.w_ih[layer];  // (Cin_l, 4H)
    float dh_rec[MT][4], dc[MT][4];
    #pragma unroll
    for (int m = 0; m < MT; ++m)
      #pragma unroll
      for (int r = 0; r < 4; ++r) { dh_rec[m][r] = 0.f; dc[m][r] = 0.f; }

    // top layer: the lane's 8 dout values of one timestep, loaded back to back
    // and waited for once. Tail rows load the tile's last valid row (always in
    // bounds) and are masked by a select at their use, not by a branch around
    // the load.
    auto load_dout = [&](const T* dtile, int dstride, T (&dov)[MT][4]) {
      const int last = S - 1 - s0;
      #pragma unroll
      for (int m = 0; m < MT; ++m)
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * m + 4 * lgrp + r;
          dov[m][r] = dtile[(row < last ? row : last) * dstride + hch];
        }
    };
    // ... as fp32, all eight defined at one point: the empty asm is that one
    // wait, and it keeps the compiler from sinking a load into a branch of its
    // own around the element that uses it
    auto dout_f32 = [&](const T (&dov)[MT][4], float (&dof)[MT][4]) {
      #pragma unroll
      for (int m = 0; m < MT; ++m)
        #pragma unroll
        for (int r = 0; r < 4; ++r) dof[m][r] = toF<T>(dov[m][r]);
      static_assert(MT == 2, "eight operands");
      asm volatile("" : "+v"(dof[0][0]), "+v"(dof[0][1]), "+v"(dof[0][2]), "+v"(dof[0][3]),
                        "+v"(dof[1][0]), "+v"(dof[1][1]), "+v"(dof[1][2]), "+v"(dof[1][3]));
    };
    if constexpr (SRC == DH_LAST) {
      T dov[MT][4];
      float dof[MT][4];
      load_dout(dout + (long)s0 * RNN_H, RNN_H, dov);
      dout_f32(dov, dof);
      #pragma unroll
      for (int m = 0; m < MT; ++m)
        #pragma unroll
        for (int r = 0; r < 4; ++r)   // 0 + x: what the stage's dh_rec + dout gave
          dh_rec[m][r] = (s0 + 16 * m + 4 * lgrp + r < S) ? stm_fadd(0.f, dof[m][r]) : 0.f;
    }

    // ---- training-save prefetch pipeline: gates/cseq (and the upstream dh)
    // for step t are loaded during stage t+1 and parked in the lane's LDS
    // slots at its end; the layer prologue fills the slots for the first
    // stage ----------------------------------------------------------------
    const long lay_base = (long)layer * Tst;
    // (the *_at pointers are workgroup-uniform tile bases; the lane's place
    // in the tile is the small offset lane_frag(m), so that one offset
    // register serves every save instead of a 64-bit address each)
    auto lane_frag = [&](int m) -> unsigned { return (wv * MT + m) * 64 + lane; };
    auto g_at = [&](int t) {
      return gates_g + (lay_base + t) * (S_pad * 4 * RNN_H)
             + (long)blockIdx.x * (SEQ_TILE * 4 * RNN_H);
    };
    auto c_at = [&](int t) {
      return cseq_g + (lay_base + t) * (S_pad * RNN_H)
             + (long)blockIdx.x * (SEQ_TILE * RNN_H);
    };
    // dh hand-off is FRAG-NATIVE: the GEMM2 writer and the pointwise reader
    // use the identical lane mapping (row 16m+4lgrp+r, col hch), so each
    // lane stores/loads its 4 values as one packed 8-byte word.
    auto dh_at = [&](int t) {
      return dh_g + (long)t * (S_pad * RNN_H)
             + (long)blockIdx.x * (SEQ_TILE * RNN_H);
    };
    char* gmine = gstage + threadIdx.x * (MT * 32);
    #pragma unroll
    for (int m = 0; m < MT; ++m) {
      *(frag*)&gmine[m * 32 + 0] =
          *(((const frag*)(g_at(Tst - 1) + lane_frag(m) * 16)) + 0);
      *(frag*)&gmine[m * 32 + 16] =
          *(((const frag*)(g_at(Tst - 1) + lane_frag(m) * 16)) + 1);
    }
    // upstream dh (layer above) for step t, prefetched one stage ahead so
    // the global loads never sit at the top of the pointwise critical path
    ulong1* dhmine = (ulong1*)(dhstage + threadIdx.x * (MT * 8));
    auto cmine = [&](int t) {
      return (ulong1*)(cstage + ((t & 1) * 256 + threadIdx.x) * (MT * 8));
    };
    if constexpr (SRC == DH_UP) {
      #pragma unroll
      for (int m = 0; m < MT; ++m)
        dhmine[m] = *(const ulong1*)(dh_at(Tst - 1) + lane_frag(m) * 4);
    }
    // stage t consumes c_t and c_{t-1}; the next stage reuses c_{t-1} as ITS
    // c_t, so only ONE new (prefetched) c load per stage.
    #pragma unroll
    for (int m = 0; m < MT; ++m) {
      cmine(Tst - 1)[m] = *(const ulong1*)(c_at(Tst - 1) + lane_frag(m) * 4);
      if (!GRU && Tst >= 2)
        cmine(Tst - 2)[m] = *(const ulong1*)(c_at(Tst - 2) + lane_frag(m) * 4);
    }
    // this lane's row of W_hh^T -> its LDS slots (read back in every stage)
    {
      const unsigned wl = (hch * (4 * RNN_H) + lgrp * 8) * sizeof(T);
      #pragma unroll
      for (int kk = 0; kk < 8; ++kk)
        *(frag*)&wmine[kk * 4096] = *(const frag*)((const char*)WhhT + (wl + kk * 64));
    }
    // scalar-input layer 0: this lane's four W_ih values, once per layer
    float wih0[4];
    if constexpr (SCALAR) {
      #pragma unroll
      for (int q = 0; q < 4; ++q) wih0[q] = toF<T>(WihT[q * 64 + hch]);
    }
    // layer boundary: the dA tile's readers of the last stage must be done, and
    // this block's dh_g stores must be visible to its next-layer loads
    __threadfence_block();
    __syncthreads();

    unsigned long dh_sent[MT] = {};   // the words last stored to dh_g (see stage_rest)
    #pragma clang loop unroll(disable)   // no peeled first stage either
    for (int t = Tst - 1;; --t) {
      const long base = lay_base + t;

      float dxpart[MT][4];
      // this lane's dA values, packed in stream order: slot q, k' - 8*lgrp =
      // 4*m + r (common.h) -> one 16 B piece per gate slot
      alignas(16) T pk[4][MT * 4];

      // the stage's dout (the one vector-memory wait of a pointwise phase)
      float dof[MT][4];
      if constexpr (SRC == DH_SEQ) {
        T dov[MT][4];
        load_dout(dout + ((long)s0 * Tst + t) * RNN_H, Tst * RNN_H, dov);
        dout_f32(dov, dof);
      }

      // Every rounding below is pinned (stm_fmul / stm_fadd / fmaf /
      // stm_fmul_to), one form per cell type: the form most elements had when
      // the arithmetic was left to the compiler's FMA contraction. That fused
      // only the LSTM's dc + (dh o)(1 - tc^2) and the scalar-input term's
      // chain; 1 - v^2 is a rounded square taken from 1, every other product
      // is rounded on its own (the few elements that deviated are listed in
      // profiles/lstm_bwd_pointwise.md).
      #pragma unroll
      for (int m = 0; m < MT; ++m) {
        frag gf0 = *(const frag*)&gmine[m * 32 + 0];                 // i|f
        frag gf1 = *(const frag*)&gmine[m * 32 + 16];                // g|o
        const ulong1 cc_t = cmine(t)[m];
        // (read unconditionally, then selected: at t == 0 the other parity
        // slot holds the dead c_1, and c_{-1} = 0)
        ulong1 cc_p = ulong1{0};
        if constexpr (!GRU) {
          cc_p = cmine(t - 1)[m];
          cc_p = t > 0 ? cc_p : ulong1{0};
        }
        ulong1 dhup = ulong1{0};
        if constexpr (SRC == DH_UP) dhup = dhmine[m];
        f32x4 ct, cpv;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          ct[r] = elemF(((const elem*)&cc_t)[r]);
          cpv[r] = elemF(((const elem*)&cc_p)[r]);
        }
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * m + 4 * lgrp + r;
          float dh = dh_rec[m][r];
          if constexpr (SRC == DH_UP) {
            dh = stm_fadd(dh, elemF(((const elem*)&dhup)[r]));
          } else if constexpr (SRC == DH_SEQ) {
            dh = (s0 + row < S) ? stm_fadd(dh, dof[m][r]) : dh;
          }
          // the dA values as (a, b) of their last product a * b: rounded to T
          // for the tile and the stream, in fp32 for the scalar-input term
          float fa[4], fb[4];
          if constexpr (GRU) {
            // gf0 = [r, z], gf1 = [n, Bn]; ct = h_{t-1} (fwd csave)
            const float r_ = elemF(gf0[r]);
            const float z_ = elemF(gf0[4 + r]);
            const float n_ = elemF(gf1[r]);
            const float Bn = elemF(gf1[4 + r]);
            const float hprev = ct[r];
            dh = stm_fadd(dh, dc[m][r]);          // direct dh_t * z carry
            const float dnp = stm_fmul(dh, 1.f - z_);
            const float dnq = 1.f - stm_fmul(n_, n_);
            const float dn_pre = stm_fmul(dnp, dnq);
            fa[0] = stm_fmul(stm_fmul(dn_pre, Bn), r_); fb[0] = 1.f - r_;     // dr_pre
            fa[1] = stm_fmul(stm_fmul(dh, hprev - n_), z_); fb[1] = 1.f - z_; // dz_pre
            fa[2] = dnp; fb[2] = dnq;                                         // dn_pre
            fa[3] = dn_pre; fb[3] = r_;                                       // dBn
            dc[m][r] = stm_fmul(dh, z_);
          } else {
            const float i_ = elemF(gf0[r]);
            const float f_ = elemF(gf0[4 + r]);
            const float g_ = elemF(gf1[r]);
            const float o_ = elemF(gf1[4 + r]);
            const float tc = stm_tanh(ct[r]);
            const float dcv = fmaf(stm_fmul(dh, o_), 1.f - stm_fmul(tc, tc), dc[m][r]);
            fa[0] = stm_fmul(stm_fmul(dcv, g_), i_); fb[0] = 1.f - i_;        // dAi
            fa[1] = stm_fmul(stm_fmul(dcv, cpv[r]), f_); fb[1] = 1.f - f_;    // dAf
            fa[2] = stm_fmul(dcv, i_); fb[2] = 1.f - stm_fmul(g_, g_);        // dAg
            fa[3] = stm_fmul(stm_fmul(dh, tc), o_); fb[3] = 1.f - o_;         // dAo
            dc[m][r] = stm_fmul(dcv, f_);
          }
          #pragma unroll
          for (int q = 0; q < 4; ++q) pk[q][4 * m + r] = stm_fmul_to<T>(fa[q], fb[q]);
          if constexpr (SCALAR)   // dx partial: one fma chain, W_ih[q] the lane's four
            dxpart[m][r] = fmaf(stm_fmul(fa[3], fb[3]), wih0[3],
                           fmaf(stm_fmul(fa[2], fb[2]), wih0[2],
                           fmaf(stm_fmul(fa[0], fb[0]), wih0[0],
                                stm_fmul(stm_fmul(fa[1], fb[1]), wih0[1]))));
        }
        // the m-tile's part of the dA image: one 8-byte word per gate slot
        #pragma unroll
        for (int q = 0; q < 4; ++q)
          *(unsigned long*)&dA_lds[q * 4096 + dA_wr[m]] = *(const unsigned long*)&pk[q][4 * m];
      }
      // ---- dA stream for the wgrad kernel, tile order (common.h): the lane's
      // 4 x 16 B pieces; a wave's store per gate slot covers 1 KiB contiguous.
      // The pieces are parked in the lane-private gates slot, which is dead
      // from here until the end-of-stage stage-in (exactly 64 B per lane), and
      // stored after the GEMMs. A store issued here would be drained by GEMM1's
      // first weight-fragment wait (vmcnt retires in order) on the serial
      // dh_prev path: ~1% slower, profiles/r03_da_stream_layout.md.
      if constexpr (SCALAR) {
        // CIN1 l0: dx[s,t] = sum_g dA[s,g] W_ih[g,0], reduced here so that
        // the dA barrier below also publishes the per-wave sums. The 16 lanes of an l16
        // group are one DPP row: quad_perm pairs lanes xor 1 and xor 2, then
        // row_half_mirror / row_mirror pair lanes whose quads already hold
        // equal sums — the pairing tree of an xor butterfly, without LDS
        // permutes. The 8 values are independent chains.
        #pragma unroll
        for (int m = 0; m < MT; ++m)
          #pragma unroll
          for (int r = 0; r < 4; ++r) dxpart[m][r] = dpp_row_add<0xB1>(dxpart[m][r]);
        #pragma unroll
        for (int m = 0; m < MT; ++m)
          #pragma unroll
          for (int r = 0; r < 4; ++r) dxpart[m][r] = dpp_row_add<0x4E>(dxpart[m][r]);
        #pragma unroll
        for (int m = 0; m < MT; ++m)
          #pragma unroll
          for (int r = 0; r < 4; ++r) dxpart[m][r] = dpp_row_add<0x141>(dxpart[m][r]);
        #pragma unroll
        for (int m = 0; m < MT; ++m)
          #pragma unroll
          for (int r = 0; r < 4; ++r) dxpart[m][r] = dpp_row_add<0x140>(dxpart[m][r]);
        if (l16 == 0) {   // one predicated region: the row's 4 sums per m-tile, 16 B
          #pragma unroll
          for (int m = 0; m < MT; ++m)
            *(f32x4*)&red[wv * SEQ_TILE + 16 * m + 4 * lgrp] =
                f32x4{dxpart[m][0], dxpart[m][1], dxpart[m][2], dxpart[m][3]};
        }
      }
      T* out_dA = dA_g + stm_da_tile_off(base * S_pad + s0);
      #pragma unroll
      for (int q = 0; q < 4; ++q) *(frag*)&gmine[q * 16] = *(const frag*)pk[q];
      // ---- the rest of the stage, one straight-line body per value of REC
      // (t > 0: a recurrent GEMM and a next stage exist) inside the layer's
      // form (INP: the layer has an input GEMM, all but the scalar-input
      // layer 0; UP: a layer above hands dh down), so that every wait in it is
      // counted against loads that are certainly in flight.
      //
      // dgrad GEMMs: dh_prev = dA @ W_hh (GEMM1) and dx = dA @ W_ih (GEMM2)
      // from ONE K loop. Both read the same 16 A fragments of the dA tile, so
      // each is read once and feeds both accumulator chains (each still sums
      // kk = 0..7 in order). GEMM1's weights come from the lane's LDS slots;
      // GEMM2's eight fragments are the only weights on the vector-memory
      // queue and are requested first, before the barrier.
      //
      // The next stage's saves (gates, c, upstream dh) are prefetched from HBM
      // right behind them, also before the barrier: vmcnt retires in order, so
      // a save load in front of a weight load would make that weight's wait
      // pay the HBM latency. The words go to their lane-private LDS slots
      // untouched at the end of the stage, the one place that waits for them;
      // the dA stores are issued right behind them, the dx / dh_g stores after
      // the GEMMs, and neither is waited for.
      auto stage_rest = [&](auto rec_c) {
        constexpr bool REC = decltype(rec_c)::value;
        constexpr bool INP = !SCALAR;
        constexpr bool UP = SRC == DH_UP;
        // row hch of W_ih^T, as a 32-bit byte offset from the uniform pointer
        const unsigned wlane = (hch * (4 * RNN_H) + lgrp * 8) * sizeof(T);
        frag b2[2][4];
        f32x4 acc1[MT], acc2[MT];
        #pragma unroll
        for (int m = 0; m < MT; ++m) {
          acc1[m] = f32x4{0.f, 0.f, 0.f, 0.f};
          acc2[m] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        auto mfma_half = [&](int h) {   // k-steps 4h .. 4h+3 of both GEMMs
          frag b1[4];
          if constexpr (REC) {
            #pragma unroll
            for (int j = 0; j < 4; ++j) b1[j] = *(const frag*)&wmine[(4 * h + j) * 4096];
          }
          if constexpr (REC || INP) {
            #pragma unroll
            for (int jb = 0; jb < 4; jb += 2) {
              frag a[2][MT];
              #pragma unroll
              for (int j = 0; j < 2; ++j)
                #pragma unroll
                for (int m = 0; m < MT; ++m) {
                  // A[16m + l16][32 kk + 8 lgrp + 0..7]: two transposed reads
                  // of 4 gate columns each, the k order of a row-major fragment
                  typedef short short4v __attribute__((ext_vector_type(4)));
                  typedef short short8v __attribute__((ext_vector_type(8)));
                  typedef __attribute__((address_space(3))) short4v* lds_s4;
                  const char* p = dA_lds + (4 * h + jb + j) * 2048;
                  const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(p + dA_rd[0][m]));
                  const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(p + dA_rd[1][m]));
                  a[j][m] = __builtin_bit_cast(
                      frag, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
                }
              #pragma unroll
              for (int j = 0; j < 2; ++j)
                #pragma unroll
                for (int m = 0; m < MT; ++m) {
                  if constexpr (REC) acc1[m] = mfma16x16x32(a[j][m], b1[jb + j], acc1[m]);
                  if constexpr (INP) acc2[m] = mfma16x16x32(a[j][m], b2[h][jb + j], acc2[m]);
                }
            }
          }
        };
        // The compiler waits (vmcnt) before it overwrites the data registers
        // of a store still in flight, and the previous stage's dh_g store is
        // the youngest thing in the queue: reusing its registers at the top of
        // the pointwise phase drained the whole queue there. Naming them here
        // keeps them untouched until the store has had a pointwise phase to
        // retire.
        if constexpr (INP) {
          #pragma unroll
          for (int m = 0; m < MT; ++m) asm volatile("" :: "v"(dh_sent[m]));
        }
        if constexpr (INP) {
          #pragma unroll
          for (int kk = 0; kk < 8; ++kk)
            b2[kk / 4][kk % 4] = *(const frag*)((const char*)WihT + (wlane + kk * 64));
        }
        ulong1 dhnext[MT], cnext[MT];
        frag gld[MT][2];
        if constexpr (REC) {
          __builtin_amdgcn_sched_barrier(0);
          #pragma unroll
          for (int m = 0; m < MT; ++m) {
            gld[m][0] = *(((const frag*)(g_at(t - 1) + lane_frag(m) * 16)) + 0);
            gld[m][1] = *(((const frag*)(g_at(t - 1) + lane_frag(m) * 16)) + 1);
          }
          // LSTM rotates c_{t-1} into c_t, so only c_{t-2} is new (at t == 1
          // nothing is: the load repeats c_0 and is dropped); GRU's save is
          // h_{t-1} (no reuse), so its next stage needs c_at(t-1)
          const int tc = GRU ? t - 1 : (t >= 2 ? t - 2 : 0);
          #pragma unroll
          for (int m = 0; m < MT; ++m)
            cnext[m] = *(const ulong1*)(c_at(tc) + lane_frag(m) * 4);
          if constexpr (UP) {
            #pragma unroll
            for (int m = 0; m < MT; ++m)
              dhnext[m] = *(const ulong1*)(dh_at(t - 1) + lane_frag(m) * 4);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        // ---- stream the parked dA pieces to global (4 x ds_read_b128 of the
        // lane's own slot; no cross-lane traffic), behind every load of the
        // stage: no wait below has to retire them, and they get the rest of
        // the stage before the next pointwise phase reuses their registers ---
        #pragma unroll
        for (int q = 0; q < 4; ++q)
          *(frag*)&out_dA[(unsigned)stm_da_elem(q * RNN_H + hch, 8 * lgrp)] =
              *(const frag*)&gmine[q * 16];

        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();   // dA (and the layer-0 dx partials) visible to all waves
        mfma_half(0);
        mfma_half(1);
        if constexpr (REC) {
          #pragma unroll
          for (int m = 0; m < MT; ++m)
            #pragma unroll
            for (int r = 0; r < 4; ++r) dh_rec[m][r] = acc1[m][r];
        }

        // ---- dx -> dh_g step t (layer hand-off) / dx output ---------------
        if constexpr (INP) {
          if (layer > 0) {
            #pragma unroll
            for (int m = 0; m < MT; ++m) {
              dh_sent[m] = pack4_word<T>(acc2[m]);
              *(unsigned long*)(dh_at(t) + lane_frag(m) * 4) = dh_sent[m];
            }
          } else {
            // workgroup-uniform row pointers + one lane offset for all 8
            T* dxtile = dx + ((long)s0 * Tst + t) * RNN_H;
            const unsigned dxlane = 4 * lgrp * (Tst * RNN_H) + hch;
            #pragma unroll
            for (int m = 0; m < MT; ++m)
              #pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int row = 16 * m + 4 * lgrp + r;
                if (s0 + row < S)
                  (dxtile + (16 * m + r) * (Tst * RNN_H))[dxlane] = fromF<T>(acc2[m][r]);
              }
          }
        } else {
          // CIN1 l0: the cross-wave sum of the partials reduced before the barrier
          if (wv == 0) {
            for (int sA = lane; sA < SEQ_TILE; sA += 64) {
              const float v = red[sA] + red[SEQ_TILE + sA] + red[2 * SEQ_TILE + sA] + red[3 * SEQ_TILE + sA];
              if (s0 + sA < S) dx[(long)(s0 + sA) * Tst + t] = fromF<T>(v);
            }
          }
        }

        // ---- stage-in: the stage's one wait on the save prefetch -----------
        if constexpr (REC) {
          #pragma unroll
          for (int m = 0; m < MT; ++m) {
            *(frag*)&gmine[m * 32 + 0] = gld[m][0];
            *(frag*)&gmine[m * 32 + 16] = gld[m][1];
            // LSTM: c_{t-2} replaces the dead c_t, same parity (at t == 1 the
            // repeated c_0 lands in the dead c_1 slot, which nobody reads)
            cmine(GRU ? t - 1 : t)[m] = cnext[m];
            if constexpr (UP) dhmine[m] = dhnext[m];
          }
          __syncthreads();   // the next pointwise phase overwrites dA / red
        }
      };
      // The last stage leaves the loop on its own edge: its dA stores are
      // still in flight, and if that state reached the loop header every
      // stage would drain its stores at the top.
      if (t == 0) {
        stage_rest(std::false_type{});
        break;
      }
      stage_rest(std::true_type{});
    }  // t loop
  };  // layer_body

  for (int layer = L - 1; layer >= 0; --layer) {
    rnn_uniform_bool(CIN1 && layer == 0, [&](auto scalar_c) {
      if (layer < L - 1) {
        layer_body(layer, scalar_c, std::integral_constant<int, DH_UP>{});
      } else {
        rnn_uniform_bool(ret_seq != 0, [&](auto seq_c) {
          layer_body(layer, scalar_c,
                     std::integral_constant<int, decltype(seq_c)::value ? DH_SEQ : DH_LAST>{});
        });
      }
    });
  }
}

extern "C" const char* stmgcn_lstm_bwd(void* stream, int dtype, const LstmBwdArgs& a) {
  if (!rnn_serves(a.S, a.Tst, a.L, a.cin))
    return "stmgcn_lstm_bwd: serves 1..8 layers, 1..16 steps, input width 1 or 64";
  const int nblk = (a.S + SEQ_TILE - 1) / SEQ_TILE;
  // the dA tile + the CIN1 dx reduction scratch + the lane-private parking of
  // the saves (gates 32 B per m-tile, dh and two cell parities 8 B each) +
  // W_hh^T of one layer: 76.5 KB, above the 64 KB a launch gets unasked
  const size_t lds_bytes = SEQ_TILE * 512 + 4 * SEQ_TILE * sizeof(float)
                           + 256 * (SEQ_TILE / 16) * (32 + 3 * 8)
                           + RNN_H * 4 * RNN_H * 2;
  return stm_dispatch_lowp("stmgcn_lstm_bwd: dtype code is not bf16/f16", dtype, [&](auto t) {
    using T = decltype(t);
    return rnn_dispatch_variant(a.cin, a.gru, [&](auto cin1, auto is_gru) {
      auto* kernel = lstm_bwd_kernel<T, decltype(cin1)::value, decltype(is_gru)::value>;
      if (const char* e = stm_status(hipFuncSetAttribute(
              (const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
              (int)lds_bytes)))
        return e;
      hipLaunchKernelGGL(kernel, dim3(nblk), dim3(256), lds_bytes, (hipStream_t)stream,
                         (const T*)a.dout, (const T*)a.x, (const T*)a.cseq,
                         (const T*)a.gates, a.w, (T*)a.dx, (T*)a.dA, (T*)a.dh, a.S,
                         a.Tst, a.L, a.ret_seq);
      return stm_launched();
    });
  });
}

// ===========================================================================
// Backward weight operands, one launch: lstm_bwd_kernel reads W_ih^T
// (cin_l, 4H) and W_hh^T (H, 4H) of every layer; this writes all 2L of them
// into one buffer (dst offsets in elements), replacing one transpose-copy
// launch per matrix. The weights change every step, so the transposes cannot
// be kept across steps. Pure 2-byte moves: the same kernel serves bf16 / f16.
// Grid (4 row tiles, 2L matrices), 256 threads; a 64 x 64 tile of the
// (4H, cols) source goes through LDS so both sides stay coalesced.
struct PackMats {
  const unsigned short* src[2 * MAX_LAYERS];
  long dst_off[2 * MAX_LAYERS];
  int cols[2 * MAX_LAYERS];
};

__global__ void __launch_bounds__(256)
lstm_pack_bwd_weights_kernel(PackMats pm, unsigned short* __restrict__ dst) {
  __shared__ unsigned short tile[64][66];
  const unsigned short* src = pm.src[blockIdx.y];
  unsigned short* out = dst + pm.dst_off[blockIdx.y];
  const int cols = pm.cols[blockIdx.y];     // 1 or 64
  const int r0 = blockIdx.x * 64;           // of the 4H = 256 source rows
  const int lo = threadIdx.x & 63, hi = threadIdx.x >> 6;
  for (int r = hi; r < 64; r += 4)
    if (lo < cols) tile[r][lo] = src[(long)(r0 + r) * cols + lo];
  __syncthreads();
  for (int c = hi; c < cols; c += 4)
    out[(long)c * 256 + r0 + lo] = tile[lo][c];
}

extern "C" const char* stmgcn_lstm_pack_bwd_weights(void* stream, const void** w_ih,
                                                    const void** w_hh, int L,
                                                    int cin, void* dst) {
  if (L < 1 || L > MAX_LAYERS) return "stmgcn_lstm_pack_bwd_weights: layer count outside 1..8";
  PackMats pm{};
  for (int i = 0; i < 2 * L; ++i) {   // all W_ih^T, then all W_hh^T
    pm.src[i] = (const unsigned short*)(i < L ? w_ih[i] : w_hh[i - L]);
    pm.cols[i] = i < L ? lstm_packT_cols(i, cin) : RNN_H;
    pm.dst_off[i] = lstm_packT_off(i, cin);
  }
  hipLaunchKernelGGL(lstm_pack_bwd_weights_kernel, dim3(4, 2 * L), dim3(256), 0,
                     (hipStream_t)stream, pm, (unsigned short*)dst);
  return stm_launched();
}
