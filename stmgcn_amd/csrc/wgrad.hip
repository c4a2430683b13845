// Weight-gradient (reduction-GEMM) kernels for CDNA4 (gfx950) — SURVEY K10.
//
// The wgrad shapes here are tall-skinny reductions: C[M<=256, N<=64] =
// A[rows, M]^T @ B[rows, N] with rows up to B*N*T (262k+). hipBLASLt serves
// these poorly (measured 437 us for (256,64|262k) bf16 on MI355X — see
// profiles/r01_bench1024_kernel_stats.md, 47.8% of step time); these kernels
// replace 15 library GEMM + 9 cat + 9 reduce launches per step with one
// launch per RNN branch + one per graph-conv.
//
// Scheme per workgroup: march a private chunk of the reduction dim in 64-row
// K-steps; stage the operands that need transposing as A^T / B^T tiles in LDS
// with an XOR swizzle that makes the 16B MFMA fragment reads
// bank-conflict-free; accumulate the full output in registers
// (v_mfma_f32_16x16x32, fp32 acc); one unsafeAtomicAdd(f32) per output element
// per workgroup at the end. Bias grads (column sums) ride along in the
// staging pass for free. Both kernels keep two named register sets (loop
// unrolled by two, no register copies), double-buffered LDS tiles with one
// barrier per K-step, and staging loads in which consecutive lanes take
// consecutive 16-byte blocks of one row. lstm_wgrad_kernel's loads are
// branch-free (clamped address, value selected at its use), so its waits are
// counted and two K-steps of loads stay in flight; atb_wgrad_kernel's loads
// are guarded, and the compiler drains the queue at every K-step there (the
// branch-free form measured no faster: profiles/wgrad_load_pipeline.md).
//
// LSTM variant reads the dA stream (L, Tst*S_pad, 4H) that lstm_bwd_kernel
// writes in wgrad A-fragment tile order (common.h) — dA goes global ->
// registers -> MFMA, only the hseq operands are transposed through LDS — and
// does ALL layers in one launch (grid.y = L). The h_{t-1} operand for dw_hh
// is hseq offset by -S_pad rows (zero for t == 0): the host-side torch.cat
// shift this replaces was 1.9% of step time.

#include "common.h"

namespace {

// Transposed-tile LDS addressing: column g (output dim) holds RB bytes of
// reduction rows (RB = 64: 32-row tiles, RB = 128: 64-row K-steps), off is the
// byte offset inside the column. The 256 / RB columns that share one 256 B
// line of the 64 banks keep their 16 B windows and successive lines XOR-rotate
// them, so an MFMA fragment read (16 consecutive g, 16 B each) hits 64
// distinct banks.
template <int RB>
__device__ __forceinline__ int tswz(int g, int off) {
  return g * RB + (off ^ ((((unsigned)g / (256 / RB)) & (RB / 16 - 1)) << 4));
}

// A-fragment (or B-fragment) read from a transposed LDS tile: output index g,
// reduction rows k = koff_bytes / 2 .. +8 -> the 16 B at tswz(g, koff_bytes).
template <typename T, int RB>
__device__ __forceinline__ typename Frag8<T>::type frag_from(
    const char* lds_tile, int g, int koff_bytes) {
  return *(const typename Frag8<T>::type*)&lds_tile[tswz<RB>(g, koff_bytes)];
}

// The layer forms of lstm_wgrad_kernel, dispatched once per workgroup: f gets
// the form as a std::integral_constant, so no stage holds another form's code.
enum : int { WG_SCALAR0 = 0, WG_DENSE0 = 1, WG_HANDOFF = 2 };
template <typename F>
__device__ __forceinline__ void wgrad_uniform_form(int form, F&& f) {
  if (form == WG_SCALAR0) f(std::integral_constant<int, WG_SCALAR0>{});
  else if (form == WG_DENSE0) f(std::integral_constant<int, WG_DENSE0>{});
  else f(std::integral_constant<int, WG_HANDOFF>{});
}

}  // namespace

// ===========================================================================
// Fused multi-layer LSTM weight gradients: one launch, grid (nchunks, L).
//   dwih[l] += dA_l^T @ (l == 0 ? x : hseq[l-1])      (4H, cin_l<=64)
//   dwhh[l] += dA_l^T @ hseq[l] shifted one step back (4H, H)
//   db[l]   += colsum(dA_l)                           (4H,)
// dA: (L, R=Tst*S_pad, 4H) in the TILED order of common.h; hseq: (L, R, H)
// natural; x: (S, Tst, Cin). Row r of the flat reduction dim maps to
// (t = r / S_pad, s = r % S_pad); R is a whole number of 32-row tiles.
//
// dA is already stored as MFMA A-fragments: lane (l16, lgrp) of gate g reads
// the 16 B at k' = 8*lgrp of the tile (a wave-load is 1 KiB contiguous),
// global -> registers with no LDS and no barrier. Only the B operands (hp =
// h_{t-1}, hx = layer input) go through LDS, transposed with their rows
// placed at k' = rho^-1(row) so both operands agree on the reduction order.
// Those two 8 KiB tiles per 64-row K-step are double-buffered: one barrier
// per K-step (the commit of step k+2 into the buffer step k read is ordered
// behind barrier k+1, which every wave reaches only after its step-k MFMAs).
// db is the fp32 sum of each A-fragment's 8 values, reduced across lgrp by
// two shuffles at the end.
//
// Every wave owns 32 gate rows (2 m-tiles), so the 8 waves of a 512-thread
// workgroup consume whole dA rows and hp/hx are staged once. One launch
// serves every layer, layer = blockIdx.y, in one of three workgroup-uniform
// forms with a straight-line K loop each: scalar-input layer 0 (cin1 != 0:
// x is (S, Tst, 1) and only column 0 of its dw_ih is live), dense layer 0,
// and hand-off layer (layer > 0 reads hseq[layer - 1]). A 256-thread
// gate-split form and a separate single-column launch for that layer 0 both
// measured slower (profiles/r03_da_stream_layout.md). Chunks are whole tiles
// (tpc per workgroup); the pair loop always runs both of its K-steps, and a
// K-step or K-half past the chunk end adds zeros.
//
// FIN (the finishing form): after its atomics every workgroup arrives at its
// layer's ticket (stm_last_arriver, common.h); the last one of a layer reads
// that layer's 129 KiB of fp32 sums back and writes dw_ih, dw_hh, db_ih,
// db_hh in the parameter dtype and in their final shapes into `fin.out`
// (layout: lstm_grads_layer_off, kernels.h). One ticket per layer, so up to L last
// arrivers share the conversion. GRU rows are un-packed on the way
// (q-slots [r|z|n_in|n_hid]: dw_ih/db_ih = rows [:3H], dw_hh/db_hh = rows
// [:2H] + [3H:]); LSTM writes the one bias sum to both db_ih and db_hh.
template <typename T>
struct LstmFin {
  unsigned* tickets;   // (L,) zero at launch, same fill as the accumulators
  T* out;              // flat parameter-dtype gradient buffer
  int gru, cin;
};

template <typename T, bool FIN>
__global__ void __launch_bounds__(512, 1)
lstm_wgrad_kernel(const T* __restrict__ dA, const T* __restrict__ hseq,
                  const T* __restrict__ x, float* __restrict__ dwih,
                  float* __restrict__ dwhh, float* __restrict__ db,
                  long R, long S_pad, int S, int Tst, int L, int cin1,
                  long tpc, LstmFin<T> fin) {
  using frag = typename Frag8<T>::type;
  constexpr int NTHR = 512;         // one wave per 32 of the 256 gate rows
  constexpr int MTG = 2;            // gate m-tiles per wave
  constexpr int KT = 64;            // K-step rows = two dA tiles
  constexpr int HT = 64 * 2 * KT;   // one transposed [64][KT] tile, bytes
  extern __shared__ char lds[];     // 2 x (hpT | hxT)

  const int layer = blockIdx.y;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l16 = lane & 15, lgrp = lane >> 4;
  const int gw = wv * 32;                     // this wave's first gate row
  const long ntile = R / SEQ_TILE;
  const long tb0 = (long)blockIdx.x * tpc;
  const long tb1 = (tb0 + tpc < ntile) ? tb0 + tpc : ntile;
  const long tp0 = S_pad / SEQ_TILE;          // tiles of t == 0 (no h_{t-1})
  // An empty chunk (the host's chunking leaves none) has nothing to add; in
  // the finishing form it still has to arrive, or its layer would never be
  // finished: it falls through with every load guarded off and adds zeros.
  if (!FIN && tb0 >= tb1) return;

  const T* dA_l = dA + (long)layer * R * STM_DA_GATES;
  const T* hp_l = hseq + (long)layer * R * 64;       // index r - S_pad
  const T* hx_l = (layer > 0) ? hseq + (long)(layer - 1) * R * 64 : nullptr;
  const bool l0 = layer == 0;
  const bool x1 = cin1 && l0;   // scalar layer-0 input

  f32x4 acc_hh[MTG][4], acc_ih[MTG][4];
  float dbp[MTG];
  #pragma unroll
  for (int mt = 0; mt < MTG; ++mt) {
    #pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc_hh[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc_ih[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    dbp[mt] = 0.f;
  }

  // hp/hx staging: one unit per thread per K-step (2 operands x 32 row pairs
  // x 8 column blocks): row pair p sits at k' = 2p, 2p+1 of K-half p >> 4,
  // i.e. tile rows rho(2(p&15)) and the next one (rho keeps even/odd k' pairs
  // adjacent). 8 consecutive lanes take the 8 column blocks of one row: 128 B
  // coalesced. Threads 0..255 (waves 0..3) stage hp, 256..511 stage hx.
  const int scb = threadIdx.x & 7, sp = (threadIdx.x >> 3) & 31;
  const int skh = sp >> 4, srow = stm_da_rho(2 * (sp & 15));
  const bool sop = threadIdx.x >= 256;

  // Register set of one K-step. No load stands under a branch: a row that
  // must read as zero (past the chunk end, t == 0 for h_{t-1}, a pad row
  // s >= S of x) is loaded from the first element of its own tensor instead
  // -- the ADDRESS is selected, so nothing outside the tensor is touched, and
  // every lane of a dead wave-load hits one line -- and the VALUE is selected
  // against zero where it is used (`live`; a select, so whatever the dead
  // address holds, NaN included, never reaches a sum). With every path
  // issuing the same loads the compiler counts its waits instead of
  // draining the queue at each join.
  struct KSet {
    frag h[2];                // rows r, r + 1 of hp (waves 0..3) or hx (4..7)
    unsigned short xs[2];     // scalar-input form: the two x values
    frag a[2][MTG];           // dA A-fragments [K-half = tile][m-tile]
    int live;                 // bit i: h[i] / xs[i] is a real row
  };

  auto load_h = [&](auto form, long tb, KSet& g) {
    constexpr int F = decltype(form)::value;
    const long tile = tb + skh;
    const bool tin = tile < tb1;
    const long r = tile * SEQ_TILE + srow;     // rows r, r + 1 (same tile)
    // h_{t-1}: hseq[l] offset -S_pad rows; t == 0 has none (for layer 0,
    // r - S_pad would point before the allocation)
    const bool hlive = tin && tile >= tp0 && !(F == WG_SCALAR0 && sop);
    const T* ph = hlive ? hp_l + (r - S_pad) * 64 : hp_l;
    const T *p0 = ph, *p1 = ph + 64;
    bool lv0 = hlive, lv1 = hlive;
    if constexpr (F == WG_HANDOFF) {
      const T* px = tin ? hx_l + r * 64 : hx_l;
      p0 = sop ? px : p0; p1 = sop ? px + 64 : p1;
      lv0 = lv1 = sop ? tin : hlive;
    } else {
      // layer 0 reads x (S, Tst, cin): t = tile / tp0, pad rows s >= S are dead
      const long t_ = (unsigned)tile / (unsigned)tp0;
      const long s_ = r - t_ * S_pad;
      const bool x0 = sop && tin && s_ < S, x1 = sop && tin && s_ + 1 < S;
      const long e0 = x0 ? s_ * Tst + t_ : 0, e1 = x1 ? (s_ + 1) * Tst + t_ : 0;
      if constexpr (F == WG_DENSE0) {
        p0 = sop ? x + e0 * 64 : p0; p1 = sop ? x + e1 * 64 : p1;
      } else {
        // Every wave issues both kinds of load, so the queue holds the same
        // count on every path: waves 4..7 take their x values here and send
        // their two fragment loads to the first row of hp, waves 0..3 send
        // these two to x[0]; the dead ones hit one line per wave.
        g.xs[0] = *(const unsigned short*)&x[e0];
        g.xs[1] = *(const unsigned short*)&x[e1];
      }
      lv0 = sop ? x0 : hlive; lv1 = sop ? x1 : hlive;
    }
    g.h[0] = *(const frag*)&p0[scb * 8];
    g.h[1] = *(const frag*)&p1[scb * 8];
    g.live = (lv0 ? 1 : 0) | (lv1 ? 2 : 0);
  };
  auto commit_h = [&](auto form, char* buf, const KSet& g) {
    constexpr int F = decltype(form)::value;
    const frag fz = {};
    char* tileT = buf + (sop ? HT : 0);
    const frag v0 = (g.live & 1) ? g.h[0] : fz;
    const frag v1 = (g.live & 2) ? g.h[1] : fz;
    // scalar input: the hx fragment is built here, only column 0 is live
    const int xw = ((g.live & 1) ? (int)g.xs[0] : 0) |
                   ((g.live & 2) ? (int)g.xs[1] << 16 : 0);
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      union { typename Frag8<T>::elem t2[2]; int i; } pk;
      pk.t2[0] = v0[j];
      pk.t2[1] = v1[j];
      int w = pk.i;
      if constexpr (F == WG_SCALAR0) w = sop ? ((j == 0 && scb == 0) ? xw : 0) : w;
      *(int*)&tileT[tswz<2 * KT>(scb * 8 + j, sp * 4)] = w;
    }
  };
  auto load_a = [&](long tb, KSet& g) {
    #pragma unroll
    for (int kh = 0; kh < 2; ++kh)
      #pragma unroll
      for (int mt = 0; mt < MTG; ++mt) {
        const long off = stm_da_tile_off((tb + kh) * SEQ_TILE) +
                         stm_da_elem(gw + mt * 16 + l16, 8 * lgrp);
        g.a[kh][mt] = *(const frag*)&dA_l[tb + kh < tb1 ? off : 0];
      }
  };

  // One K-step on register set g and LDS buffer buf, in this issue order:
  //   commit h(k) -> request h(k+2) -> barrier -> fragment reads and MFMAs on
  //   dA(k) -> request dA(k+2).
  // The set is refilled for the step TWO ahead as soon as each half has been
  // consumed, and the two sets alternate by name (loop unrolled by 2, no
  // register copies). With 2 h and 4 dA loads per thread per K-step the waits
  // before the commit are vmcnt(11) and (10): dA(k), h(k+1), dA(k+1) stay in
  // flight; the waits before the MFMAs on dA(k) run from vmcnt(11) to (8):
  // h(k+1), dA(k+1), h(k+2) stay in flight (13/12 and 15..12 in the
  // scalar-input form with its 4 h loads). No vmcnt(0) inside the loop: a CU
  // keeps two K-steps of 48 KB under way. The scheduling barriers pin the
  // commit, the two request points and the fragment-read groups.
  auto kstep = [&](auto form, long tb, char* buf, KSet& g) {
    char* hpT = buf;
    char* hxT = buf + HT;
    commit_h(form, buf, g);
    __builtin_amdgcn_sched_barrier(0);
    load_h(form, tb + 4, g);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    // Fragment reads run half a K-half ahead of their MFMAs: bh(1) is read
    // behind the hh MFMAs of half 0 and bx(1) behind its ih MFMAs, so at most
    // three of the four 16-register fragment groups are live at once. Every
    // accumulator still takes its products in the order kh = 0, 1.
    const frag fz = {};
    frag bh[2][4], bx[2][4], af[2][MTG];
    auto read_b = [&](frag (&b)[4], const char* tileT, int kh) {
      #pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        b[nt] = frag_from<T, 2 * KT>(tileT, nt * 16 + l16, kh * KT + lgrp * 16);
    };
    auto mfma_b = [&](f32x4 (&acc)[MTG][4], const frag (&b)[4], int kh) {
      #pragma unroll
      for (int mt = 0; mt < MTG; ++mt)
        #pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          acc[mt][nt] = mfma16x16x32(af[kh][mt], b[nt], acc[mt][nt]);
    };
    #pragma unroll
    for (int kh = 0; kh < 2; ++kh)
      #pragma unroll
      for (int mt = 0; mt < MTG; ++mt)   // past the chunk end: adds zeros
        af[kh][mt] = tb + kh < tb1 ? g.a[kh][mt] : fz;
    read_b(bh[0], hpT, 0);
    read_b(bx[0], hxT, 0);
    __builtin_amdgcn_sched_barrier(0);
    mfma_b(acc_hh, bh[0], 0);
    read_b(bh[1], hpT, 1);
    __builtin_amdgcn_sched_barrier(0);
    mfma_b(acc_ih, bx[0], 0);
    read_b(bx[1], hxT, 1);
    __builtin_amdgcn_sched_barrier(0);
    mfma_b(acc_hh, bh[1], 1);
    mfma_b(acc_ih, bx[1], 1);
    #pragma unroll
    for (int kh = 0; kh < 2; ++kh)
      #pragma unroll
      for (int mt = 0; mt < MTG; ++mt) {
        float sa = 0.f;
        #pragma unroll
        for (int j = 0; j < 8; ++j) sa += (float)af[kh][mt][j];
        dbp[mt] += sa;
      }
    __builtin_amdgcn_sched_barrier(0);
    load_a(tb + 4, g);
  };

  // One straight-line loop per workgroup-uniform layer form; the pair loop
  // runs both K-steps unconditionally (a K-step past the end adds zeros).
  wgrad_uniform_form(l0 ? (cin1 ? WG_SCALAR0 : WG_DENSE0) : WG_HANDOFF, [&](auto form) {
    KSet g0, g1;
    load_h(form, tb0, g0);
    load_a(tb0, g0);
    load_h(form, tb0 + 2, g1);
    load_a(tb0 + 2, g1);
    long tb = tb0;
    do {   // an empty chunk (finishing form only) runs one pair of zeros
      kstep(form, tb, lds, g0);
      kstep(form, tb + 2, lds + 2 * HT, g1);
      tb += 4;
    } while (tb < tb1);
  });

  // ---- writeback: one f32 atomic per output element per workgroup --------
  float* whh = dwhh + (long)layer * 256 * 64;
  float* wih = dwih + (long)layer * 256 * 64;
  #pragma unroll
  for (int mt = 0; mt < MTG; ++mt) {
    #pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      #pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int m = gw + mt * 16 + lgrp * 4 + rr;
        const int n = nt * 16 + l16;
        unsafeAtomicAdd(&whh[m * 64 + n], acc_hh[mt][nt][rr]);
        if (!x1 || n == 0)   // scalar input: one live column
          unsafeAtomicAdd(&wih[m * 64 + n], acc_ih[mt][nt][rr]);
      }
    // db: lane (l16, lgrp) holds the k' = 8*lgrp..+8 partial of gate l16
    float v = dbp[mt];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (lgrp == 0) unsafeAtomicAdd(&db[layer * 256 + gw + mt * 16 + l16], v);
  }

  if constexpr (FIN) {
    if (!stm_last_arriver(&fin.tickets[layer], gridDim.x, (int*)lds)) return;
    // packed gate row m -> output row (or -1: a zero GRU slot)
    const int GH = fin.gru ? 192 : 256;
    const int cin_l = l0 ? fin.cin : 64;
    auto row_ih = [&](int m) { return m < GH ? m : -1; };
    auto row_hh = [&](int m) {
      return !fin.gru ? m : (m < 128 ? m : (m >= 192 ? m - 64 : -1));
    };
    T* o_ih = fin.out + lstm_grads_layer_off(layer, GH, fin.cin);
    T* o_hh = o_ih + (long)GH * cin_l;
    T* o_bi = o_hh + (long)GH * 64;
    T* o_bh = o_bi + GH;
    const float* dbl = db + layer * 256;
    // Every load is issued before the first store (the outputs may alias the
    // sums as far as the compiler knows, so a load-store-load loop would pay
    // one memory round trip per iteration on this serial tail): float4 i of a
    // (256, 64) matrix is row i >> 4, columns 4 * (i & 15).
    // Threads 0..255 also carry one gate row's bias sum (and, for the scalar
    // input, its single dw_ih column).
    constexpr int IT = 256 * 16 / NTHR;   // float4 per thread per matrix
    const bool dense = cin_l == 64;
    const int mb = threadIdx.x;
    float4 vh[IT], vi[IT];
    #pragma unroll
    for (int k = 0; k < IT; ++k) {
      const int i = threadIdx.x + k * NTHR;
      vh[k] = *(const float4*)&whh[i * 4];
      vi[k] = dense ? *(const float4*)&wih[i * 4] : float4{0.f, 0.f, 0.f, 0.f};
    }
    const float vb = mb < 256 ? dbl[mb] : 0.f;
    const float vc = (!dense && mb < 256) ? wih[mb * 64] : 0.f;
    #pragma unroll
    for (int k = 0; k < IT; ++k) {
      const int i = threadIdx.x + k * NTHR;
      const int m = i >> 4, n4 = (i & 15) * 4;
      const int rh = row_hh(m), ri = row_ih(m);
      if (rh >= 0)
        stm_store4<T>(&o_hh[rh * 64 + n4], vh[k].x, vh[k].y, vh[k].z, vh[k].w);
      if (dense && ri >= 0)
        stm_store4<T>(&o_ih[ri * 64 + n4], vi[k].x, vi[k].y, vi[k].z, vi[k].w);
    }
    if (mb >= 256) return;
    const int ri = row_ih(mb), rh = row_hh(mb);
    if (ri >= 0) o_bi[ri] = fromF<T>(vb);
    if (rh >= 0) o_bh[rh] = fromF<T>(vb);
    if (!dense && ri >= 0) o_ih[ri] = fromF<T>(vc);
  }
}

// a.out == null: the accumulate-only form (fp32 sums left in a.ws)
extern "C" const char* stmgcn_lstm_wgrad(void* stream, int dtype, const LstmWgradArgs& a) {
  const long R = a.R;
  const int L = a.L;
  if (L < 1 || L > MAX_LAYERS) return "stmgcn_lstm_wgrad: layer count outside 1..8";
  if (R <= 0 || R % SEQ_TILE != 0)
    return "stmgcn_lstm_wgrad: R is not a whole number of dA tiles";
  // Chunks are whole 32-row tiles of the tiled dA stream: at most one per
  // 1024 rows, and at most 256 / L per layer, i.e. one workgroup per CU in a
  // single round. Two rounds of half-length chunks (512 / L) measured slower,
  // alone and in the step (profiles/wgrad_load_pipeline.md): twice the
  // prologues, dead prefetches and atomics for the same stream.
  const long ntile = R / SEQ_TILE;
  if (ntile >= (1L << 31)) return "stmgcn_lstm_wgrad: too many dA tiles";
  const long target = 256 / L;
  long nchunks = (R + 1023) / 1024;
  if (nchunks > target) nchunks = target;
  if (nchunks < 1) nchunks = 1;
  const long tpc = (ntile + nchunks - 1) / nchunks;   // tiles per workgroup
  nchunks = (ntile + tpc - 1) / tpc;
  const size_t lds = 2 * 2 * 8192;   // double-buffered hpT | hxT, 64-row steps
  const bool finishing = a.out != nullptr;
  const LstmWgradWs ws = lstm_wgrad_ws(L, finishing);
  unsigned* tickets = finishing ? (unsigned*)(a.ws + ws.tickets) : nullptr;
  return stm_dispatch_lowp("stmgcn_lstm_wgrad: dtype code is not bf16/f16", dtype, [&](auto t) {
    using T = decltype(t);
    const LstmFin<T> fin{tickets, (T*)a.out, finishing ? a.gru : 0, a.cin};
    return stm_dispatch_bool(finishing, [&](auto finc) {
      hipLaunchKernelGGL((lstm_wgrad_kernel<T, decltype(finc)::value>),
                         dim3((unsigned)nchunks, L), dim3(512), lds,
                         (hipStream_t)stream, (const T*)a.dA, (const T*)a.hseq,
                         (const T*)a.x, a.ws + ws.dwih, a.ws + ws.dwhh, a.ws + ws.db,
                         R, a.S_pad, a.S, a.Tst, L, a.cin == 1 ? 1 : 0, tpc, fin);
      return stm_launched();
    });
  });
}

// ===========================================================================
// Generic reduction GEMM: C[M,N] += A[rows,M]^T @ B[rows,N], optional
// db[N] += colsum(B). M <= 256, N <= 64 (zero-padded to 16-multiples in LDS).
// Serves the graph-conv dW = feat^T @ dZ and db = colsum(dZ) (SURVEY K2
// backward) — measured 465 us each as hipBLASLt calls.
//
// Multi-source form: A is up to 4 separate (rows, CA) tensors laid out as
// the column blocks of a virtual (rows, M = K*CA) matrix — the fused
// ChebConv wgrad passes its recurrence states [x, p_1, .., p_{K_s-1}] so
// ALL supports' dW_k land in one launch with dZ streamed ONCE (the
// (B,N,K_s,C) concat stack never exists). CA must be a multiple of 8 so
// every 8-col fragment stays within one source.
//
// 256 threads, 4 waves; wave wv owns the m-tiles wv, wv + 4, .. (up to 4) and
// all n-tiles. A K-step is 64 rows: its A^T [256][64] and B^T [64][64] tiles
// (40 KiB) are double-buffered, 80 KiB of LDS, one workgroup per CU. Staging
// unit = (row pair, 8-column block); a thread holds up to 4 A units and 1 B
// unit per register set, two 16-byte loads each, committed as 4-byte
// (row, row + 1) pairs. No scratch: accumulators and units are indexed at
// compile time, the tile loops are predicated on the wave-uniform counts.
//
// FIN (the finishing form): the workgroup that draws the launch's last ticket
// (stm_last_arriver, common.h) reads the <= 64 KiB of fp32 sums back and
// writes dW (M, N) and db (N,) in the parameter dtype. C, db and the ticket
// share one zero-filled fp32 workspace; two launches that share a workspace
// (the dual gconv's forward and backward source groups) take one ticket each
// and finish their own rows.
struct AtbSrc { const void* a[4]; };

template <typename T>
struct AtbFin {
  unsigned* ticket;   // zero at launch
  T *dW, *dbo;        // (M, N) and (N,) outputs; dbo null when db is
};

template <typename T, bool FIN>
__global__ void __launch_bounds__(256, 1)
atb_wgrad_kernel(AtbSrc As, int CA, const T* __restrict__ B,
                 float* __restrict__ C, float* __restrict__ db,
                 long rows, int M, int N, AtbFin<T> fin) {
  using frag = typename Frag8<T>::type;
  constexpr int KT = 64;                 // K-step rows
  constexpr int AT_B = 256 * 2 * KT;     // A^T tile [256][KT], bytes
  constexpr int BT_B = 64 * 2 * KT;      // B^T tile [64][KT]
  constexpr int BUF_B = AT_B + BT_B;
  constexpr int NUA = 4;                 // A units per thread: 32 pairs x 32 blocks / 256
  extern __shared__ char lds[];          // 2 x (A^T | B^T)
  float* red = (float*)lds;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l16 = lane & 15, lgrp = lane >> 4;
  const long chunk = (rows + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * chunk;
  const long r1 = (r0 + chunk < rows) ? r0 + chunk : rows;
  const int mtiles = (M + 15) / 16;       // <= 16
  const int ntiles = (N + 15) / 16;       // <= 4
  // wave wv handles m-tiles wv, wv+4, wv+8, wv+12
  const int mt_mine = (mtiles - wv + 3) / 4;

  f32x4 acc[4][4];
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[i][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbp[8];
  #pragma unroll
  for (int j = 0; j < 8; ++j) dbp[j] = 0.f;

  // Staging units of one K-step: (row pair p = 0..31, 8-column block cb). Unit
  // u = p * ncb + cb, so consecutive lanes take the consecutive 16-byte blocks
  // of one row (a source's CA columns are contiguous, then the next source's)
  // and the row pairs spread over the lane groups. ncb counts the zero-padded
  // blocks too (2 per 16-wide tile): a unit past M (or N) loads nothing and
  // commits zeros. A thread's units are the same in every K-step, so their
  // source, column and row pair are resolved once, here.
  const int ncba = mtiles * 2, ncbb = ntiles * 2;
  const T* ap[NUA];      // source + column offset, null: no such unit / padding
  int apair[NUA], acb[NUA];
  #pragma unroll
  for (int i = 0; i < NUA; ++i) {
    const int u = threadIdx.x + i * 256;
    apair[i] = u / ncba; acb[i] = u % ncba;
    ap[i] = nullptr;
    if (u < 32 * ncba && acb[i] * 8 < M)
      ap[i] = (const T*)As.a[(acb[i] * 8) / CA] + (acb[i] * 8) % CA;
  }
  const int bpair = threadIdx.x / ncbb, bcb = threadIdx.x % ncbb;
  const bool bunit = threadIdx.x < 32 * ncbb;       // commits (zeros past N)
  const T* bp = (bunit && bcb * 8 < N) ? B + bcb * 8 : nullptr;

  struct Regs { frag a[NUA][2]; frag b[2]; };
  auto load_tiles = [&](long kt, Regs& g) {
    const frag fz = {};
    #pragma unroll
    for (int i = 0; i < NUA; ++i) {
      g.a[i][0] = fz; g.a[i][1] = fz;
      const long ra = kt + apair[i] * 2;
      if (ap[i] != nullptr) {
        if (ra < r1) g.a[i][0] = *(const frag*)&ap[i][ra * CA];
        if (ra + 1 < r1) g.a[i][1] = *(const frag*)&ap[i][(ra + 1) * CA];
      }
    }
    g.b[0] = fz; g.b[1] = fz;
    const long rb = kt + bpair * 2;
    if (bp != nullptr) {
      if (rb < r1) g.b[0] = *(const frag*)&bp[rb * N];
      if (rb + 1 < r1) g.b[1] = *(const frag*)&bp[(rb + 1) * N];
    }
  };
  auto commit_tiles = [&](char* buf, const Regs& g) {
    char* AT = buf;
    char* BT = buf + AT_B;
    #pragma unroll
    for (int i = 0; i < NUA; ++i) {
      if (threadIdx.x + i * 256 < 32 * ncba) {
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          union { T t2[2]; int i; } pk;
          pk.t2[0] = ((const T*)&g.a[i][0])[j];
          pk.t2[1] = ((const T*)&g.a[i][1])[j];
          *(int*)&AT[tswz<2 * KT>(acb[i] * 8 + j, apair[i] * 4)] = pk.i;
        }
      }
    }
    if (bunit) {
      #pragma unroll
      for (int j = 0; j < 8; ++j) {
        union { T t2[2]; int i; } pk;
        pk.t2[0] = ((const T*)&g.b[0])[j];
        pk.t2[1] = ((const T*)&g.b[1])[j];
        *(int*)&BT[tswz<2 * KT>(bcb * 8 + j, bpair * 4)] = pk.i;
        if (db) dbp[j] += toF<T>(pk.t2[0]) + toF<T>(pk.t2[1]);
      }
    }
  };

  // One K-step on register set g and LDS buffer buf: the set is refilled for
  // the step TWO ahead as soon as it has been committed, and the two sets
  // alternate by name (loop unrolled by 2, no register copy). The loads stand
  // under their guards (unit, row end, second step of the pair), so at each
  // join the compiler waits vmcnt(0): a commit drains the queue, the refill
  // issued just before it included, and one K-step of loads is in flight at
  // a time. With four K-steps per workgroup the prologue, the atomics and
  // the finishing tail dominate; the branch-free form with counted waits
  // (lstm_wgrad_kernel's) measured no faster here and was not kept
  // (profiles/wgrad_load_pipeline.md). The LDS tiles are double-buffered: one
  // barrier per K-step (the commit of step k+2 into the buffer step k read is
  // ordered behind barrier k+1, which every wave reaches only after its
  // step-k MFMAs). Past the chunk end the loads issue nothing and leave
  // zeros. The tile loops are fully unrolled and predicated (wave-uniform),
  // so acc is indexed at compile time and a wave skips the m- and n-tiles M
  // and N do not reach (M = 24, N = 8: two waves run one MFMA pair per
  // K-half).
  auto kstep = [&](long kt, char* buf, Regs& g) {
    commit_tiles(buf, g);
    load_tiles(kt + 2 * KT, g);
    __syncthreads();
    const char* AT = buf;
    const char* BT = buf + AT_B;
    #pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      const int koff = kh * KT + lgrp * 16;   // byte offset of the K half
      frag bf[4];
      #pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        if (nt < ntiles) bf[nt] = frag_from<T, 2 * KT>(BT, nt * 16 + l16, koff);
      #pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < mt_mine) {
          const frag a = frag_from<T, 2 * KT>(AT, (wv + i * 4) * 16 + l16, koff);
          #pragma unroll
          for (int nt = 0; nt < 4; ++nt)
            if (nt < ntiles) acc[i][nt] = mfma16x16x32(a, bf[nt], acc[i][nt]);
        }
      }
    }
  };

  Regs g0, g1;
  load_tiles(r0, g0);
  load_tiles(r0 + KT, g1);
  for (long kt = r0; kt < r1; kt += 2 * KT) {
    kstep(kt, lds, g0);
    if (kt + KT < r1) kstep(kt + KT, lds + BUF_B, g1);   // WG-uniform
  }
  __syncthreads();   // red (and the ticket flag) reuse the tiles' LDS

  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i >= mt_mine) continue;
    const int mt = wv + i * 4;
    #pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      if (nt >= ntiles) continue;
      #pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int m = mt * 16 + lgrp * 4 + rr, n = nt * 16 + l16;
        if (m < M && n < N) unsafeAtomicAdd(&C[(long)m * N + n], acc[i][nt][rr]);
      }
    }
  }

  if (db) {
    // B-staging thread tid < 32 * ncbb held column block tid % ncbb
    #pragma unroll
    for (int j = 0; j < 8; ++j) red[threadIdx.x * 8 + j] = bunit ? dbp[j] : 0.f;
    __syncthreads();
    if (threadIdx.x < N) {
      const int n = threadIdx.x, cb = n >> 3, j = n & 7;
      float v = 0.f;
      for (int k = 0; k < 32; ++k) v += red[(k * ncbb + cb) * 8 + j];
      unsafeAtomicAdd(&db[n], v);
    }
  }

  if constexpr (FIN) {
    if (!stm_last_arriver(fin.ticket, gridDim.x, (int*)lds)) return;
    const int n4s = M * N / 4;   // N is a multiple of 8
    // four loads in flight per thread before their stores (see lstm_wgrad)
    for (int i0 = threadIdx.x; i0 < n4s; i0 += 4 * 256) {
      float4 v[4];
      #pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + k * 256;
        v[k] = i < n4s ? *(const float4*)&C[i * 4] : float4{0.f, 0.f, 0.f, 0.f};
      }
      #pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + k * 256;
        if (i < n4s) stm_store4<T>(&fin.dW[i * 4], v[k].x, v[k].y, v[k].z, v[k].w);
      }
    }
    if (db && threadIdx.x < N) fin.dbo[threadIdx.x] = fromF<T>(db[threadIdx.x]);
  }
}

// a.ws == null: the accumulate-into form (fp32 sums left in a.C / a.db)
extern "C" const char* stmgcn_atb_wgrad(void* stream, int dtype, const AtbWgradArgs& a) {
  if (a.nsrc < 1 || a.nsrc > ATB_MAX_SRC) return "stmgcn_atb_wgrad: source count outside 1..4";
  // 256 rows (four K-steps) per workgroup, at most 512 workgroups. At the
  // flagship shape (32768 rows, M = 192, N = 64) that is 128 workgroups and
  // 6.3 MB of float atomics; 128 rows (256 workgroups, twice the atomics) and
  // 512 rows (64 workgroups streaming) both measured slower, in isolation and
  // in the step (profiles/gconv_vector_tiles.md).
  const long rows = a.rows;
  long nchunks = (rows + 255) / 256;
  if (nchunks > 512) nchunks = 512;
  if (nchunks < 1) nchunks = 1;
  const dim3 grid((unsigned)nchunks), blk(256);
  const size_t lds = 2 * (256 + 64) * 128;   // double-buffered A^T | B^T, 64-row steps
  const int CA = a.CA, N = a.N, M = a.nsrc * CA;
  AtbSrc src{};
  for (int i = 0; i < a.nsrc; ++i) src.a[i] = a.As[i];
  // finishing form: this launch's rows of the shared workspace and of dW
  const bool finishing = a.ws != nullptr;
  const AtbWs ws = atb_ws(a.nsrc_all, CA, N);
  const long r0 = (long)a.src0 * CA * N;
  float* C = finishing ? a.ws + ws.C + r0 : a.C;
  float* db = finishing ? (a.dbo ? a.ws + ws.db : nullptr) : a.db;
  unsigned* ticket = finishing ? (unsigned*)(a.ws + ws.tickets) + (a.src0 ? 1 : 0) : nullptr;
  return stm_dispatch_lowp("stmgcn_atb_wgrad: dtype code is not bf16/f16", dtype, [&](auto t) {
    using T = decltype(t);
    const AtbFin<T> fin{ticket, finishing ? (T*)a.dW + r0 : nullptr, (T*)a.dbo};
    return stm_dispatch_bool(finishing, [&](auto finc) {
      auto* kernel = atb_wgrad_kernel<T, decltype(finc)::value>;
      if (const char* e = stm_status(hipFuncSetAttribute(
              (const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)))
        return e;
      hipLaunchKernelGGL(kernel, grid, blk, lds, (hipStream_t)stream, src, CA,
                         (const T*)a.B, C, db, rows, M, N, fin);
      return stm_launched();
    });
  });
}
