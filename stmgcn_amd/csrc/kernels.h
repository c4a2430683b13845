// Host/device contract of the stmgcn_amd HIP kernels: every extern "C" entry
// point that bindings.cpp calls and the argument structs of the fused gconv
// steps. Plain C++ (no HIP, no torch), included by every .hip file (through
// common.h) and by bindings.cpp, so a definition that disagrees with its
// declaration is a compile error. `stream` is a hipStream_t, `dtype` a StmDtype.
#pragma once

#define SEQ_TILE 32   // sequences per RNN workgroup tile == dA tile rows

// CSR generator (or its transpose): rowptr (N + 1), colidx/vals (nnz)
struct StmCsr {
  const int *rowptr = nullptr, *colidx = nullptr;
  const float* vals = nullptr;
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

extern "C" {

// ---- cheb_gconv.hip / dual_gconv.hip ----
// out = alpha * (G @ xin) + beta * p1 + gamma * p2 over strided (B, N, C)
// slices: s* = element stride between rows, b* = between batches.
void stmgcn_spmm_step(void* stream, int dtype, const int* rowptr, const int* colidx,
    const float* vals, const void* xin, const void* p1, const void* p2, void* out, int B,
    int N, int C, long sx, long s1, long s2, long so, long bx, long b1, long b2, long bo,
    float alpha, float beta, float gamma);
void stmgcn_cheb_fused_fwd_step(void* stream, int dtype, const ChebFwdArgs& a);
void stmgcn_cheb_fused_bwd_step(void* stream, int dtype, const ChebBwdArgs& a);
// bf16/f16 only, C <= 64, Cout <= 64 (checked in bindings.cpp)
void stmgcn_dual_fused_fwd_step(void* stream, int dtype, const DualFwdArgs& a);
void stmgcn_dual_fused_bwd_step(void* stream, int dtype, const DualBwdArgs& a);

// ---- fused_rnn.hip ----
void stmgcn_lstm_fwd(void* stream, int dtype, const void* x, void* out, void* hseq_g,
    void* cseq_g, void* gates_g, const void** w_ih, const void** w_hh, const void** b_ih,
    const void** b_hh, int S, int Tst, int L, int cin, int ret_seq, int gru);
void stmgcn_lstm_bwd(void* stream, int dtype, const void* dout, const void* x,
    const void* cseq_g, const void* gates_g, const void** w_ihT, const void** w_hhT,
    void* dx, void* dA_g, void* dh_g, int S, int Tst, int L, int cin, int ret_seq,
    int gru);
void stmgcn_mfma_probe(void* stream, const void* A, const void* B, void* D);
// W_ih^T (cin_l, 4H) of layers 0..L-1, then W_hh^T (H, 4H) of layers 0..L-1,
// back to back in dst (2-byte elements), one launch
void stmgcn_lstm_pack_bwd_weights(void* stream, const void** w_ih, const void** w_hh,
    int L, int cin, void* dst);

// ---- wgrad.hip ----
void stmgcn_lstm_wgrad(void* stream, int dtype, const void* dA, const void* hseq,
    const void* x, float* dwih, float* dwhh, float* db, long R, long S_pad, int S,
    int Tst, int L, int cin);
// finishing form: the last workgroup of each layer writes [dw_ih | dw_hh | db_ih |
// db_hh] of that layer to `out` in `dtype`, final shapes, layers back to back;
// dwih/dwhh/db/tickets are one zero-filled workspace (tickets: L words)
void stmgcn_lstm_wgrad_grads(void* stream, int dtype, const void* dA, const void* hseq,
    const void* x, float* dwih, float* dwhh, float* db, unsigned* tickets, void* out,
    long R, long S_pad, int S, int Tst, int L, int cin, int gru);
void stmgcn_atb_wgrad(void* stream, int dtype, const void* A, const void* B, float* C,
    float* db, long rows, int M, int N);
// finishing form: the last workgroup writes dW (nsrc*CA, N) and dbo (N,) in `dtype`
// from the zero-filled fp32 C / db / ticket workspace
void stmgcn_atb_wgrad_multi_grads(void* stream, int dtype, const void** As, int nsrc,
    int CA, const void* B, float* C, float* db, unsigned* ticket, void* dW, void* dbo,
    long rows, int N);
void stmgcn_atb_wgrad_multi(void* stream, int dtype, const void** As, int nsrc, int CA,
    const void* B, float* C, float* db, long rows, int N);

// ---- pointwise.hip ----
void stmgcn_seqsum_permute(void* stream, int dtype, const void* obs, void* out, int B,
    int Tst, int N, int C);
void stmgcn_seqsum_permute_bwd(void* stream, int dtype, const void* dxs, void* dobs,
    int B, int Tst, int N, int C);
// z | tickets (B) and dz | tickets (B + 1) are each one zero-filled allocation;
// node_major: out / dout are (B,N,T,C); dobs may be null; dw_f/db_f fp32, dw/db `dtype`
void stmgcn_gate_fwd(void* stream, int dtype, const void* g, const void* xs,
    const void* fcw, const void* fcb, const void* obs, float* z, float* u, float* s,
    unsigned* tickets, void* out, int B, int Tst, int N, int C, int node_major);
void stmgcn_gate_bwd(void* stream, int dtype, const void* dout, const void* obs,
    const void* fcw, const float* z, const float* u, const float* s, float* dz,
    float* dw_part, float* db_part, unsigned* tickets, float* dw_f, float* db_f,
    void* dw, void* db, void* dobs, void* dg, int B, int Tst, int N, int C,
    int node_major);
void stmgcn_head_fwd(void* stream, int dtype, const void* f0, const void* f1,
    const void* f2, const void* w, const void* bias, void* y, void* fsum, int G, long BN);
void stmgcn_head_bwd(void* stream, int dtype, const void* dy, const void* w, void* dfeat,
    int G, long BN);
void stmgcn_head_wgrad(void* stream, int dtype, const void* dy, const void* fsum,
    float* dw, float* db, int G, long BN);
void stmgcn_head_wgrad_grads(void* stream, int dtype, const void* dy, const void* fsum,
    float* dw, float* db, unsigned* ticket, void* dw_out, void* db_out, int G, long BN);
// wide head: O = horizon * C output columns, 2 <= O <= 32, G <= 64 with
// G % 8 == 0, bf16/f16. wgrad: ticket == null leaves the fp32 sums in dw / db
void stmgcn_head_multi_fwd(void* stream, int dtype, const void* f0, const void* f1,
    const void* f2, const void* w, const void* bias, void* y, void* fsum, int G, int O,
    long BN);
void stmgcn_head_multi_bwd(void* stream, int dtype, const void* dy, const void* w,
    void* dfeat, int G, int O, long BN);
void stmgcn_head_multi_wgrad(void* stream, int dtype, const void* dy, const void* fsum,
    float* dw, float* db, unsigned* ticket, void* dw_out, void* db_out, int G, int O,
    long BN);
// masked loss (NaN target = missing): kind 0 mse, 1 mae, 2 huber; ws = 3 zeroed
// words (sum, count, ticket), res = {loss, 1 / max(count_valid, 1)}
void stmgcn_masked_loss_fwd(void* stream, int dtype, int kind, const void* pred,
    const void* tgt, float* ws, float* res, void* diff, long n);
void stmgcn_masked_loss_bwd(void* stream, int dtype, int kind, const void* diff,
    const float* res, const float* gscale, void* dpred, long n);
// dz = dy * (y > 0), bf16/f16
void stmgcn_relu_bwd(void* stream, int dtype, const void* dy, const void* y, void* dz,
    long n);
void stmgcn_mse_fwd(void* stream, int dtype, const void* pred, const void* tgt,
    float* loss, void* diff, long n);
void stmgcn_mse_bwd(void* stream, int dtype, const void* diff, const float* gscale,
    void* dpred, long n);
void stmgcn_adam(void* stream, int dtype, float* master, void* param, const void* grad,
    float* m, float* v, float* hyper, long n);
void stmgcn_gather_grads(void* stream, int dtype, const void** srcs, const long* ofs,
    const int* lens, int nseg, void* arena);

}  // extern "C"
