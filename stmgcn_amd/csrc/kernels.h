// Host/device contract of the stmgcn_amd HIP kernels: every extern "C" entry
// point that bindings.cpp calls, their argument structs and every workspace or
// output layout that both sides index. Plain C++ (no HIP, no torch), included
// by every .hip file (through common.h) and by bindings.cpp, so a definition
// that disagrees with its declaration is a compile error. `stream` is a
// hipStream_t, `dtype` a StmDtype.
//
// Every entry point returns a status: null when its kernels were launched,
// otherwise a static message with the cause (a refused argument, or HIP's own
// text for a failed attribute call or launch). Nothing was launched after the
// failing call; bindings.cpp raises on it.
#pragma once

#define SEQ_TILE 32     // sequences per RNN workgroup tile == dA tile rows
#define RNN_H 64        // hidden width of the fused RNN kernels
#define MAX_LAYERS 8    // RNN layers per launch
#define ATB_MAX_SRC 4   // A sources of one atb_wgrad launch

// CSR generator (or its transpose): rowptr (N + 1), colidx/vals (nnz)
struct StmCsr {
  const int *rowptr = nullptr, *colidx = nullptr;
  const float* vals = nullptr;
};

// A strided (B, N, C) slice: element strides between rows and between batches
struct StmSlice {
  const void* ptr = nullptr;
  long srow = 0, sbatch = 0;
};

// out = alpha * (g @ xin) + beta * p1 + gamma * p2 over strided slices
// (cheb_gconv.hip); a null slice drops its term
struct SpmmArgs {
  StmCsr g;
  StmSlice xin, p1, p2, out;   // out is written
  int B = 0, N = 0, C = 0;
  float alpha = 0.f, beta = 0.f, gamma = 0.f;
};

// One fused ChebConv forward step over (B, N, C) states (cheb_gconv.hip):
//   tile = alpha * (g @ xin) + beta * p1   (xin / p1 optional); pout = tile
//   W != null: y (+)= tile @ W[kofs:kofs+C] (+ x0 @ W[0:C]); `first` skips the
//   yacc read; yout != null makes this the last step: yout = act(y + bias).
struct ChebFwdArgs {
  StmCsr g;
  const void *xin = nullptr, *p1 = nullptr, *x0 = nullptr, *W = nullptr, *bias = nullptr;
  void *pout = nullptr, *yout = nullptr;
  float* yacc = nullptr;
  int B = 0, N = 0, C = 0, Cout = 0, kofs = 0;
  float alpha = 1.f, beta = 0.f;
  int first = 1, act = 0;
};

// One fused ChebConv backward (Clenshaw) step over the G^T CSR:
//   out = alpha * (g @ xin) + beta * p1 + dz @ W[kofs:kofs+C]^T
struct ChebBwdArgs {
  StmCsr g;
  const void *xin = nullptr, *p1 = nullptr, *dz = nullptr, *W = nullptr;
  void* out = nullptr;
  int B = 0, N = 0, C = 0, Cout = 0, kofs = 0;
  float alpha = 0.f, beta = 0.f;
};

// Dual random-walk steps (dual_gconv.hip): both generators per launch.
struct DualFwdArgs {
  StmCsr gf, gb;
  const void *xf = nullptr, *pf1 = nullptr, *xb = nullptr, *pb1 = nullptr;
  const void *x0 = nullptr, *W = nullptr, *bias = nullptr;
  void *pfout = nullptr, *pbout = nullptr, *yout = nullptr;
  float* yacc = nullptr;
  int B = 0, N = 0, C = 0, Cout = 0, kofs_f = 0, kofs_b = 0;
  float alpha = 1.f, beta = 0.f;
  int first = 1, act = 0;
};
struct DualBwdArgs {
  StmCsr gft, gbt;
  const void *xf = nullptr, *pf1 = nullptr, *xb = nullptr, *pb1 = nullptr;
  const void *dz = nullptr, *W = nullptr;
  void *outf = nullptr, *outb = nullptr;
  int B = 0, N = 0, C = 0, Cout = 0, kofs_f = 0, kofs_b = 0;
  float alpha = 0.f, beta = 0.f;
  int final_step = 0;
};

// ---- fused RNN (fused_rnn.hip) ---------------------------------------------
// Per-layer pointer tables of one launch, model dtype. Forward: w_ih (G*H, C_l)
// and w_hh (G*H, H) row-major, b_ih / b_hh (G*H,). Backward: w_ih / w_hh hold
// the transposes W_ih^T (C_l, 4H) / W_hh^T (H, 4H); the biases stay null.
struct RnnPtrs {
  const void* w_ih[MAX_LAYERS];
  const void* w_hh[MAX_LAYERS];
  const void* b_ih[MAX_LAYERS];
  const void* b_hh[MAX_LAYERS];
};

constexpr long rnn_s_pad(int S) { return (S + SEQ_TILE - 1L) / SEQ_TILE * SEQ_TILE; }

// x (S, Tst, cin) -> out (S, H) or, ret_seq, (S, Tst, H); hseq (L, Tst, S_pad,
// H) always; cseq (L, Tst, S_pad * H) and gates (L, Tst, S_pad * 4H) only when
// training (both null otherwise)
struct LstmFwdArgs {
  const void* x = nullptr;
  void *out = nullptr, *hseq = nullptr, *cseq = nullptr, *gates = nullptr;
  RnnPtrs w = {};
  int S = 0, Tst = 0, L = 0, cin = 0, ret_seq = 0, gru = 0;
};
// dx like x, dA (L, Tst, S_pad, 4H) in the tiled order of common.h, dh the
// (Tst * S_pad * H) cross-layer scratch (null for L == 1)
struct LstmBwdArgs {
  const void *dout = nullptr, *x = nullptr, *cseq = nullptr, *gates = nullptr;
  RnnPtrs w = {};
  void *dx = nullptr, *dA = nullptr, *dh = nullptr;
  int S = 0, Tst = 0, L = 0, cin = 0, ret_seq = 0, gru = 0;
};

// Packed backward weights, one buffer of 2-byte elements: matrix i < L is
// W_ih^T (cols(i), 4H) of layer i, matrix L + l is W_hh^T (H, 4H) of layer l.
constexpr int lstm_packT_cols(int i, int cin) { return i == 0 ? cin : RNN_H; }
constexpr long lstm_packT_off(int i, int cin) {   // i == 2L: the total
  return i == 0 ? 0 : 4L * RNN_H * (cin + (long)(i - 1) * RNN_H);
}

// ---- wgrad.hip -------------------------------------------------------------
// fp32 workspace of lstm_wgrad, one zero fill: dwih (L, 4H, H) | dwhh (L, 4H,
// H) | db (L, 4H), and for the finishing form 8 words whose first L are the
// per-layer tickets. Offsets and size in words.
struct LstmWgradWs { long dwih, dwhh, db, tickets, words; };
constexpr LstmWgradWs lstm_wgrad_ws(int L, bool finishing) {
  const long n_w = (long)L * 4 * RNN_H * RNN_H, n_b = (long)L * 4 * RNN_H;
  return {0, n_w, 2 * n_w, 2 * n_w + n_b, 2 * n_w + n_b + (finishing ? 8 : 0)};
}
// Flat parameter-dtype gradient buffer of the finishing form: per layer
// [dw_ih (GH, cin_l) | dw_hh (GH, H) | db_ih (GH) | db_hh (GH)], layers back to
// back; GH = 4H (LSTM) or 3H (GRU). Element offset of layer l's block; l == L
// gives the total.
constexpr long lstm_grads_layer_off(int l, int GH, int cin) {
  return l == 0 ? 0 : (long)GH * (cin + 64 + 2) + (long)(l - 1) * GH * (64 + 64 + 2);
}
struct LstmGradsLayer { long dw_ih, dw_hh, db_ih, db_hh; };
constexpr LstmGradsLayer lstm_grads_layer(int l, int GH, int cin) {
  const long o = lstm_grads_layer_off(l, GH, cin), cl = l == 0 ? cin : RNN_H;
  return {o, o + GH * cl, o + GH * cl + (long)GH * RNN_H, o + GH * cl + (long)GH * RNN_H + GH};
}
// All-layer weight gradients over the tiled dA stream (L, R = Tst * S_pad, 4H).
// out == null: the accumulate-only form, the fp32 sums stay in ws
// (lstm_wgrad_ws(L, false)); otherwise ws is lstm_wgrad_ws(L, true) and the last
// workgroup of each layer writes that layer's block of `out` in `dtype`.
struct LstmWgradArgs {
  const void *dA = nullptr, *hseq = nullptr, *x = nullptr;
  float* ws = nullptr;    // zero-filled
  void* out = nullptr;
  long R = 0, S_pad = 0;
  int S = 0, Tst = 0, L = 0, cin = 0, gru = 0;
};

// fp32 workspace of the finishing atb_wgrad, one zero fill: C (nsrc * CA, N) |
// db (N) | 8 words, the first two the tickets of its (up to) two launches
struct AtbWs { long C, db, tickets, words; };
constexpr AtbWs atb_ws(int nsrc, int CA, int N) {
  const long nW = (long)nsrc * CA * N;
  return {0, nW, nW + N, nW + N + 8};
}
// C[k*CA:(k+1)*CA, :] += As[k]^T @ B for nsrc <= 4 sources (rows, CA) and B
// (rows, N) in one launch; db += colsum(B).
// ws == null: the accumulate-only form into the caller's fp32 C (nsrc * CA, N)
// and db (N, or null).
// ws != null: the finishing form over atb_ws(nsrc_all, CA, N). This launch owns
// the sources [src0, src0 + nsrc) of nsrc_all, i.e. the rows from src0 * CA of
// C and of dW (nsrc_all * CA, N; `dtype`), which its last workgroup rounds; it
// draws ticket 0 (src0 == 0) or 1. dbo (N,) != null adds the bias gradient.
struct AtbWgradArgs {
  const void* As[ATB_MAX_SRC] = {};
  const void* B = nullptr;
  int nsrc = 0, CA = 0, N = 0;
  long rows = 0;
  float *C = nullptr, *db = nullptr;
  float* ws = nullptr;
  int nsrc_all = 0, src0 = 0;
  void *dW = nullptr, *dbo = nullptr;
};

// ---- pointwise.hip ---------------------------------------------------------
// fp32 workspaces of the gate, one zero fill each: forward z (B, Tst) | B
// tickets; backward dz (B, Tst) | B + 1 tickets
struct GateWs { long z, tickets, words; };
constexpr GateWs gate_ws(int B, int Tst, bool backward) {
  return {0, (long)B * Tst, (long)B * Tst + B + (backward ? 1 : 0)};
}
// node_major: out / dout are (B, N, T, C) instead of (B, T, N, C)
struct GateFwdArgs {
  const void *g = nullptr, *xs = nullptr, *fcw = nullptr, *fcb = nullptr, *obs = nullptr;
  float* ws = nullptr;              // gate_ws(B, Tst, false), zero-filled
  float *u = nullptr, *s = nullptr; // (B, Tst)
  void* out = nullptr;
  int B = 0, Tst = 0, N = 0, C = 0, node_major = 0;
};
// dw_f / db_f: fp32 sums over the batch, dw / db the same in `dtype`; dobs may
// be null (obs needs no gradient)
struct GateBwdArgs {
  const void *dout = nullptr, *obs = nullptr, *fcw = nullptr;
  const float *z = nullptr, *u = nullptr, *s = nullptr;
  float* ws = nullptr;              // gate_ws(B, Tst, true), zero-filled
  float *dw_part = nullptr, *db_part = nullptr;   // (B, Tst, Tst), (B, Tst)
  float *dw_f = nullptr, *db_f = nullptr;
  void *dw = nullptr, *db = nullptr, *dobs = nullptr, *dg = nullptr;
  int B = 0, Tst = 0, N = 0, C = 0, node_major = 0;
};

// fp32 workspace of the head wgrads, one zero fill. One column (O == 1): dw
// (64) | db (4) | ticket (4). Wide head: dw (O, G) | db (32) | ticket (8).
struct HeadWgradWs { long dw, db, ticket, words; };
constexpr HeadWgradWs head_wgrad_ws(int G, int O) {
  return O == 1 ? HeadWgradWs{0, 64, 68, 72}
                : HeadWgradWs{0, (long)O * G, (long)O * G + 32, (long)O * G + 40};
}
// dw = dy^T fsum, db = colsum(dy) over BN rows. dw_out == null: the
// accumulate-only form, the fp32 sums stay in ws; otherwise the last workgroup
// writes dw_out (O, G) / db_out (O,) in `dtype`. stmgcn_head_wgrad is the
// one-column kernel (O == 1, G <= 64), stmgcn_head_multi_wgrad the wide one.
struct HeadWgradArgs {
  const void *dy = nullptr, *fsum = nullptr;
  float* ws = nullptr;   // head_wgrad_ws(G, O), zero-filled
  void *dw_out = nullptr, *db_out = nullptr;
  int G = 0, O = 1;
  long BN = 0;
};

// masked loss workspace: zero-filled words
enum : int { MLOSS_WS_SUM = 0, MLOSS_WS_COUNT = 1, MLOSS_WS_TICKET = 2, MLOSS_WS_WORDS = 4 };

extern "C" {

// ---- cheb_gconv.hip / dual_gconv.hip ----
const char* stmgcn_spmm_step(void* stream, int dtype, const SpmmArgs& a);
const char* stmgcn_cheb_fused_fwd_step(void* stream, int dtype, const ChebFwdArgs& a);
const char* stmgcn_cheb_fused_bwd_step(void* stream, int dtype, const ChebBwdArgs& a);
// bf16/f16 only, C <= 64, Cout <= 64 (checked in bindings.cpp)
const char* stmgcn_dual_fused_fwd_step(void* stream, int dtype, const DualFwdArgs& a);
const char* stmgcn_dual_fused_bwd_step(void* stream, int dtype, const DualBwdArgs& a);

// ---- fused_rnn.hip ----
const char* stmgcn_lstm_fwd(void* stream, int dtype, const LstmFwdArgs& a);
const char* stmgcn_lstm_bwd(void* stream, int dtype, const LstmBwdArgs& a);
const char* stmgcn_mfma_probe(void* stream, const void* A, const void* B, void* D);
// the 2L transposes into dst in the lstm_packT_off order, one launch
const char* stmgcn_lstm_pack_bwd_weights(void* stream, const void** w_ih,
    const void** w_hh, int L, int cin, void* dst);

// ---- wgrad.hip ----
const char* stmgcn_lstm_wgrad(void* stream, int dtype, const LstmWgradArgs& a);
const char* stmgcn_atb_wgrad(void* stream, int dtype, const AtbWgradArgs& a);

// ---- pointwise.hip ----
const char* stmgcn_seqsum_permute(void* stream, int dtype, const void* obs, void* out,
    int B, int Tst, int N, int C);
const char* stmgcn_seqsum_permute_bwd(void* stream, int dtype, const void* dxs,
    void* dobs, int B, int Tst, int N, int C);
const char* stmgcn_gate_fwd(void* stream, int dtype, const GateFwdArgs& a);
const char* stmgcn_gate_bwd(void* stream, int dtype, const GateBwdArgs& a);
const char* stmgcn_head_fwd(void* stream, int dtype, const void* f0, const void* f1,
    const void* f2, const void* w, const void* bias, void* y, void* fsum, int G, long BN);
const char* stmgcn_head_bwd(void* stream, int dtype, const void* dy, const void* w,
    void* dfeat, int G, long BN);
const char* stmgcn_head_wgrad(void* stream, int dtype, const HeadWgradArgs& a);
// wide head: O = horizon * C output columns, 2 <= O <= 32, G <= 64 with
// G % 8 == 0, bf16/f16
const char* stmgcn_head_multi_fwd(void* stream, int dtype, const void* f0,
    const void* f1, const void* f2, const void* w, const void* bias, void* y, void* fsum,
    int G, int O, long BN);
const char* stmgcn_head_multi_bwd(void* stream, int dtype, const void* dy, const void* w,
    void* dfeat, int G, int O, long BN);
const char* stmgcn_head_multi_wgrad(void* stream, int dtype, const HeadWgradArgs& a);
// masked loss (NaN target = missing): kind 0 mse, 1 mae, 2 huber; ws =
// MLOSS_WS_WORDS zeroed words, res = {loss, 1 / max(count_valid, 1)}
const char* stmgcn_masked_loss_fwd(void* stream, int dtype, int kind, const void* pred,
    const void* tgt, float* ws, float* res, void* diff, long n);
const char* stmgcn_masked_loss_bwd(void* stream, int dtype, int kind, const void* diff,
    const float* res, const float* gscale, void* dpred, long n);
// dz = dy * (y > 0), bf16/f16
const char* stmgcn_relu_bwd(void* stream, int dtype, const void* dy, const void* y,
    void* dz, long n);
const char* stmgcn_mse_fwd(void* stream, int dtype, const void* pred, const void* tgt,
    float* loss, void* diff, long n);
const char* stmgcn_mse_bwd(void* stream, int dtype, const void* diff, const float* gscale,
    void* dpred, long n);
const char* stmgcn_adam(void* stream, int dtype, float* master, void* param,
    const void* grad, float* m, float* v, float* hyper, long n);
// nseg <= 64 segments per call
const char* stmgcn_gather_grads(void* stream, int dtype, const void** srcs,
    const long* ofs, const int* lens, int nseg, void* arena);

}  // extern "C"
