// Python bindings + host-side sequencing for the stmgcn_amd HIP kernels.
// Device code lives in the .hip translation units (pure HIP, no torch);
// this file owns at::Tensor plumbing, stream lookup and launch ordering.
// The entry points and their argument structs are declared once, in kernels.h.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "kernels.h"

namespace {

int dtype_code(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return 0;
    case at::kBFloat16: return 1;
    case at::kHalf: return 2;
    default: TORCH_CHECK(false, "unsupported dtype for stmgcn kernels");
  }
}

void* stream() { return (void*)at::cuda::getCurrentCUDAStream().stream(); }

// The only way a binding obtains CSR pointers: the kernels index rowptr[0..N]
// and colidx/vals unchecked, so a CSR for another N must not reach them.
StmCsr csr_ptrs(const at::Tensor& rowptr, const at::Tensor& colidx,
                const at::Tensor& vals, int N) {
  TORCH_CHECK(rowptr.is_cuda() && colidx.is_cuda() && vals.is_cuda());
  TORCH_CHECK(rowptr.scalar_type() == at::kInt && colidx.scalar_type() == at::kInt &&
              vals.scalar_type() == at::kFloat);
  TORCH_CHECK(rowptr.is_contiguous() && colidx.is_contiguous() && vals.is_contiguous());
  TORCH_CHECK(rowptr.numel() == N + 1 && colidx.numel() == vals.numel());
  return {rowptr.data_ptr<int>(), colidx.data_ptr<int>(), vals.data_ptr<float>()};
}

// bias pointer for a fused forward; `keep` owns the contiguous copy for the
// duration of the binding (a temporary would be freed before the launches)
const void* bias_ptr(const c10::optional<at::Tensor>& bias, const at::Tensor& x,
                     int Cout, at::Tensor& keep) {
  if (!bias.has_value()) return nullptr;
  TORCH_CHECK(bias->scalar_type() == x.scalar_type() && bias->numel() == Cout);
  keep = bias->contiguous();
  return keep.data_ptr();
}

// optional fp32 (N,) accumulator of the wgrad kernels
float* db_ptr(const c10::optional<at::Tensor>& db, int N) {
  if (!db.has_value()) return nullptr;
  TORCH_CHECK(db->is_contiguous() && db->scalar_type() == at::kFloat && db->numel() == N);
  return db->data_ptr<float>();
}

struct Slice {
  const void* ptr;
  long srow, sbatch;
};
const Slice kNone{nullptr, 0, 0};

// one recurrence step: out_slice = alpha * G @ x_slice + beta*p1 + gamma*p2
struct SpmmStep {
  int dt;
  StmCsr g;
  int B, N, C;
  void operator()(Slice xin, Slice p1, Slice p2, Slice out, float alpha,
                  float beta, float gamma) const {
    stmgcn_spmm_step(stream(), dt, g.rowptr, g.colidx, g.vals, xin.ptr, p1.ptr,
                     p2.ptr, const_cast<void*>(out.ptr), B, N, C, xin.srow,
                     p1.srow, p2.srow, out.srow, xin.sbatch, p1.sbatch,
                     p2.sbatch, out.sbatch, alpha, beta, gamma);
  }
};

}  // namespace

// x: (B, N, C) -> S: (B, N, K_s, C); slice k of S is T_k(G) @ x.
// kind single (localpool): K_s == 1, S[...,0,:] = G @ x.
at::Tensor cheb_apply(at::Tensor x, at::Tensor rowptr, at::Tensor colidx,
                      at::Tensor vals, int64_t K_s, bool single) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.is_contiguous());
  const int B = x.size(0), N = x.size(1), C = x.size(2);
  const SpmmStep step{dtype_code(x), csr_ptrs(rowptr, colidx, vals, N), B, N, C};
  auto S = at::empty({B, N, K_s, C}, x.options());
  const long es = x.element_size();
  char* Sp = (char*)S.data_ptr();
  const long so = K_s * (long)C, bo = (long)N * K_s * C;  // S row/batch strides
  auto sl = [&](int k) -> Slice { return {Sp + (long)k * C * es, so, bo}; };
  const Slice xs{x.data_ptr(), C, (long)N * C};

  if (single) {
    TORCH_CHECK(K_s == 1);
    step(xs, kNone, kNone, sl(0), 1.f, 0.f, 0.f);
    return S;
  }
  step(kNone, kNone, xs, sl(0), 0.f, 0.f, 1.f);   // T_0 x = x (copy into slice 0)
  if (K_s > 1) step(xs, kNone, kNone, sl(1), 1.f, 0.f, 0.f);   // T_1 x = G x
  for (int k = 2; k < K_s; ++k)  // T_k x = 2 G (T_{k-1} x) - T_{k-2} x
    step(sl(k - 1), sl(k - 2), kNone, sl(k), 2.f, -1.f, 0.f);
  return S;
}

// U: (B, N, K_s, C) -> Z = sum_k T_k(G) @ U_k : (B, N, C), via the Clenshaw
// reverse recurrence (b_j = U_j + 2 G b_{j+1} - b_{j+2}; Z = U_0 + G b_1 - b_2).
// Pass the CSR of G^T here to get the gradient sum_k T_k(G)^T U_k.
at::Tensor cheb_combine(at::Tensor U, at::Tensor rowptr, at::Tensor colidx,
                        at::Tensor vals, bool single) {
  TORCH_CHECK(U.is_cuda() && U.dim() == 4 && U.is_contiguous());
  const int B = U.size(0), N = U.size(1), K_s = U.size(2), C = U.size(3);
  const SpmmStep step{dtype_code(U), csr_ptrs(rowptr, colidx, vals, N), B, N, C};
  auto Z = at::empty({B, N, C}, U.options());
  const long es = U.element_size();
  const char* Up = (const char*)U.data_ptr();
  const long su = (long)K_s * C, bu = (long)N * K_s * C;
  const long sz = C, bz = (long)N * C;
  auto ul = [&](int k) -> Slice { return {Up + (long)k * C * es, su, bu}; };
  const Slice Zs{Z.data_ptr(), sz, bz};

  if (single) {  // Z = G^T U_0
    step(ul(0), kNone, kNone, Zs, 1.f, 0.f, 0.f);
    return Z;
  }
  const int K = K_s - 1;
  if (K == 0) {  // T_0-only cheby: Z = U_0 (alpha 0 copy)
    step(kNone, kNone, ul(0), Zs, 0.f, 0.f, 1.f);
    return Z;
  }
  if (K == 1) {  // Z = U_0 + G U_1
    step(ul(1), kNone, ul(0), Zs, 1.f, 0.f, 1.f);
    return Z;
  }
  auto bk1 = at::empty({B, N, C}, U.options());   // b_{j+1}
  at::Tensor bk2;                                  // b_{j+2}; empty = virtual 0
  Slice sb1{bk1.data_ptr(), sz, bz}, sb2 = kNone;
  step(kNone, kNone, ul(K), sb1, 0.f, 0.f, 1.f);   // b_K = U_K  (copy)
  for (int j = K - 1; j >= 1; --j) {
    auto bnew = at::empty({B, N, C}, U.options());
    // b_j = 2 G b_{j+1} - b_{j+2} + U_j   (p1 = b_{j+2}, p2 = U_j);
    // b_{K+1} == 0 -> p1 skipped (beta 0) on the first iteration
    step(sb1, sb2, ul(j), {bnew.data_ptr(), sz, bz}, 2.f, sb2.ptr ? -1.f : 0.f, 1.f);
    bk2 = bk1; bk1 = bnew;
    sb1 = {bk1.data_ptr(), sz, bz}; sb2 = {bk2.data_ptr(), sz, bz};
  }
  step(sb1, sb2, ul(0), Zs, 1.f, -1.f, 1.f);   // Z = G b_1 - b_2 + U_0
  return Z;
}

// ---------------------------------------------------------------------------
// Fully fused ChebConv (SURVEY K1+K2): recurrence + MFMA mix + bias + act in
// one kernel chain; no support stack, no library GEMMs.
// A binding fills one argument struct (kernels.h) per call chain and changes
// only the per-step fields between launches.

// y = act(sum_k (T_k(G) x) @ W_k + b), fused: the K_s recurrence steps each
// fold their mix into an fp32 accumulator; the last adds bias + activation.
// Serves C <= 64, Cout <= 64 (every BASELINE config; the stack path in
// cheb_apply remains for parity tests / larger widths). training=true also
// returns the recurrence states p_1..p_{K_s-1} (p_0 == x) for the wgrad: their
// writes are mandatory anyway (cross-workgroup recurrence dependency), so
// keeping them costs no extra HBM traffic, unlike a (B,N,K_s,C) concat stack.
std::vector<at::Tensor> cheb_gconv_fused_fwd(
    at::Tensor x, at::Tensor rowptr, at::Tensor colidx, at::Tensor vals,
    at::Tensor W, c10::optional<at::Tensor> bias, int64_t K_s, bool single,
    int64_t act, bool training) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.is_contiguous());
  TORCH_CHECK(W.is_contiguous() && W.scalar_type() == x.scalar_type());
  const int B = x.size(0), N = x.size(1), C = x.size(2), Cout = W.size(1);
  TORCH_CHECK(C <= 64 && Cout <= 64, "fused ChebConv serves C/Cout <= 64");
  TORCH_CHECK(W.size(0) == K_s * C);
  const int dt = dtype_code(x);
  void* st = stream();
  auto y = at::empty({B, N, Cout}, x.options());
  at::Tensor bc;
  ChebFwdArgs a;   // the fields every step of the chain shares
  a.g = csr_ptrs(rowptr, colidx, vals, N);
  a.W = W.data_ptr();
  a.bias = bias_ptr(bias, x, Cout, bc);
  a.B = B; a.N = N; a.C = C; a.Cout = Cout; a.act = (int)act;

  if (single) {  // localpool: y = act((G @ x) @ W + b); p = G x kept if training
    TORCH_CHECK(K_s == 1);
    at::Tensor p;
    if (training) a.pout = (p = at::empty({B, N, C}, x.options())).data_ptr();
    a.xin = x.data_ptr(); a.yout = y.data_ptr();
    stmgcn_cheb_fused_fwd_step(st, dt, a);
    return training ? std::vector<at::Tensor>{y, p} : std::vector<at::Tensor>{y};
  }
  if (K_s == 1) {  // T_0 only: y = act(x @ W + b)
    a.p1 = x.data_ptr(); a.yout = y.data_ptr();
    a.alpha = 0.f; a.beta = 1.f;
    stmgcn_cheb_fused_fwd_step(st, dt, a);
    return {y};
  }
  // K_s - 1 launches: the T_0 mix (x @ W_0) rides the T_1 launch as its
  // x0 operand, so K_s == 2 needs no fp32 accumulator at all.
  at::Tensor yacc;
  if (K_s > 2) {
    yacc = at::empty({B, N, Cout}, x.options().dtype(at::kFloat));
    a.yacc = yacc.data_ptr<float>();
  }
  // training keeps every p_k, eval ping/pongs two buffers
  std::vector<at::Tensor> ps;
  const int nbuf = training ? (int)K_s - 1 : std::min<int>(2, (int)K_s - 1);
  for (int i = 0; i < nbuf; ++i)
    ps.push_back(at::empty({B, N, C}, x.options()));
  // k = 1: p_1 = G x; y (+)= x @ W_0 + p_1 @ W_1
  // k >= 2: p_k = 2 G p_{k-1} - p_{k-2}, y += p_k @ W_k; eval writes p_k over
  // p_{k-2} from k = 3 on (never over x): p1 == pout aliasing is element-safe
  const void* pm2 = nullptr;          // p_{k-2}
  a.xin = a.x0 = x.data_ptr();        // p_{k-1}
  for (int k = 1; k < K_s; ++k) {
    a.p1 = pm2;
    a.pout = (training || k <= 2) ? ps[k - 1].data_ptr() : const_cast<void*>(pm2);
    a.kofs = k * C;
    a.yout = k == K_s - 1 ? y.data_ptr() : nullptr;
    stmgcn_cheb_fused_fwd_step(st, dt, a);
    pm2 = a.xin; a.xin = a.pout; a.x0 = nullptr;
    a.alpha = 2.f; a.beta = -1.f; a.first = 0;
  }
  std::vector<at::Tensor> out{y};
  if (training) out.insert(out.end(), ps.begin(), ps.end());
  return out;
}

// dX = sum_k T_k(G)^T (dz W_k^T) via Clenshaw over the G^T CSR with the
// U_j = dz W_j^T term fused into every step (never materialized).
at::Tensor cheb_gconv_fused_bwd_dx(at::Tensor dz, at::Tensor W, at::Tensor rowptr_t,
                                   at::Tensor colidx_t, at::Tensor vals_t,
                                   int64_t K_s, bool single) {
  TORCH_CHECK(dz.is_cuda() && dz.dim() == 3 && dz.is_contiguous());
  TORCH_CHECK(W.is_contiguous() && W.scalar_type() == dz.scalar_type());
  const int B = dz.size(0), N = dz.size(1), Cout = dz.size(2);
  const int C = W.size(0) / K_s;
  TORCH_CHECK(C <= 64 && Cout <= 64 && (int)(K_s * C) == W.size(0));
  const int dt = dtype_code(dz);
  void* st = stream();
  auto dX = at::empty({B, N, C}, dz.options());
  ChebBwdArgs a;
  a.g = csr_ptrs(rowptr_t, colidx_t, vals_t, N);
  a.dz = dz.data_ptr(); a.W = W.data_ptr();
  a.B = B; a.N = N; a.C = C; a.Cout = Cout;

  auto bwd = [&](const void* xin, const void* p1, void* out, int kofs,
                 float alpha, float beta) {
    a.xin = xin; a.p1 = p1; a.out = out;
    a.kofs = kofs; a.alpha = alpha; a.beta = beta;
    stmgcn_cheb_fused_bwd_step(st, dt, a);
  };
  if (single) {  // dX = G^T U_0: materialize U_0, then one plain SpMM
    auto U0 = at::empty({B, N, C}, dz.options());
    bwd(nullptr, nullptr, U0.data_ptr(), 0, 0.f, 0.f);
    ChebFwdArgs s;   // W == null: no mix
    s.g = a.g;
    s.xin = U0.data_ptr();
    s.pout = dX.data_ptr();
    s.B = B; s.N = N; s.C = s.Cout = C;
    stmgcn_cheb_fused_fwd_step(st, dt, s);
    return dX;
  }
  const int K = (int)K_s - 1;
  if (K == 0) {  // dX = U_0
    bwd(nullptr, nullptr, dX.data_ptr(), 0, 0.f, 0.f);
    return dX;
  }
  // Clenshaw: b_K = U_K; b_j = U_j + 2 G^T b_{j+1} - b_{j+2};
  // dX = U_0 + G^T b_1 - b_2 (K == 1: dX = U_0 + G^T U_1, b_2 absent). Two
  // ping/pong buffers (one for K == 1); p1 aliasing is safe.
  auto bufA = at::empty({B, N, C}, dz.options());
  auto bufB = K > 1 ? at::empty({B, N, C}, dz.options()) : at::Tensor();
  void* bj1 = bufA.data_ptr();  // b_{j+1}
  void* bj2 = nullptr;          // b_{j+2}
  bwd(nullptr, nullptr, bj1, K * C, 0.f, 0.f);  // b_K
  void* other = K > 1 ? bufB.data_ptr() : nullptr;
  for (int j = K - 1; j >= 1; --j) {
    bwd(bj1, bj2, other, j * C, 2.f, bj2 ? -1.f : 0.f);
    bj2 = bj1;
    bj1 = other;
    other = bj2;  // overwritten next iteration (element-wise p1 read is safe)
  }
  bwd(bj1, bj2, dX.data_ptr(), 0, 1.f, bj2 ? -1.f : 0.f);
  return dX;
}

// ---------------------------------------------------------------------------
// Dual random-walk diffusion gconv (dual_gconv.hip): 2K+1 supports
// [I, T_1..T_K(G_f), T_1..T_K(G_b)], both generators advanced per launch.

// y = act(x W_0 + sum_k (T_k(G_f) x) W_k + (T_k(G_b) x) W_{K+k} + b) in K
// launches. training=true additionally returns pf_1..pf_K, pb_1..pb_K for the
// wgrad; eval ping/pongs two buffers per direction.
std::vector<at::Tensor> dual_gconv_fused_fwd(
    at::Tensor x, at::Tensor rpf, at::Tensor cif, at::Tensor vf,
    at::Tensor rpb, at::Tensor cib, at::Tensor vb, at::Tensor W,
    c10::optional<at::Tensor> bias, int64_t K, int64_t act, bool training) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf,
              "fused dual gconv serves bf16/f16");
  TORCH_CHECK(W.is_contiguous() && W.scalar_type() == x.scalar_type());
  const int B = x.size(0), N = x.size(1), C = x.size(2), Cout = W.size(1);
  TORCH_CHECK(K >= 1 && C <= 64 && Cout <= 64,
              "fused dual gconv serves K >= 1, C/Cout <= 64");
  TORCH_CHECK(W.size(0) == (2 * K + 1) * C);
  const int dt = dtype_code(x);
  void* st = stream();
  DualFwdArgs a;
  a.gf = csr_ptrs(rpf, cif, vf, N);
  a.gb = csr_ptrs(rpb, cib, vb, N);
  auto y = at::empty({B, N, Cout}, x.options());
  at::Tensor bc;
  a.W = W.data_ptr();
  a.bias = bias_ptr(bias, x, Cout, bc);
  a.B = B; a.N = N; a.C = C; a.Cout = Cout; a.act = (int)act;
  at::Tensor yacc;
  if (K > 1) {
    yacc = at::empty({B, N, Cout}, x.options().dtype(at::kFloat));
    a.yacc = yacc.data_ptr<float>();
  }
  const int nbuf = training ? (int)K : std::min<int>(2, (int)K);
  std::vector<at::Tensor> pf, pb;
  for (int i = 0; i < nbuf; ++i) {
    pf.push_back(at::empty({B, N, C}, x.options()));
    pb.push_back(at::empty({B, N, C}, x.options()));
  }
  // k = 1: p_1 = G x (both directions); acc = x W_0 + pf_1 W_1 + pb_1 W_{K+1}
  // k >= 2: p_k = 2 G p_{k-1} - p_{k-2}; eval writes p_k over p_{k-2} from
  // k = 3 on (never over x) — the p1 == pout aliasing the kernel allows
  const void *f2 = nullptr, *b2 = nullptr;   // p_{k-2}
  a.xf = a.xb = a.x0 = x.data_ptr();         // p_{k-1}
  for (int k = 1; k <= K; ++k) {
    a.pf1 = f2; a.pb1 = b2;
    const bool fresh = training || k <= 2;
    a.pfout = fresh ? pf[k - 1].data_ptr() : const_cast<void*>(f2);
    a.pbout = fresh ? pb[k - 1].data_ptr() : const_cast<void*>(b2);
    a.kofs_f = k * C; a.kofs_b = (int)(K + k) * C;
    a.yout = k == K ? y.data_ptr() : nullptr;
    stmgcn_dual_fused_fwd_step(st, dt, a);
    f2 = a.xf; b2 = a.xb; a.xf = a.pfout; a.xb = a.pbout; a.x0 = nullptr;
    a.alpha = 2.f; a.beta = -1.f; a.first = 0;
  }
  std::vector<at::Tensor> out{y};
  if (training) {
    out.insert(out.end(), pf.begin(), pf.end());
    out.insert(out.end(), pb.begin(), pb.end());
  }
  return out;
}

// dX = U_0 + sum_k T_k(G_f)^T U_k + T_k(G_b)^T U_{K+k}, U_j = dz W_j^T, via
// two Clenshaw chains over the transposed CSRs advanced together: K+1 launches.
at::Tensor dual_gconv_fused_bwd_dx(at::Tensor dz, at::Tensor W, at::Tensor rpf_t,
                                   at::Tensor cif_t, at::Tensor vf_t, at::Tensor rpb_t,
                                   at::Tensor cib_t, at::Tensor vb_t, int64_t K) {
  TORCH_CHECK(dz.is_cuda() && dz.dim() == 3 && dz.is_contiguous());
  TORCH_CHECK(dz.scalar_type() == at::kBFloat16 || dz.scalar_type() == at::kHalf,
              "fused dual gconv serves bf16/f16");
  TORCH_CHECK(W.is_contiguous() && W.scalar_type() == dz.scalar_type());
  const int B = dz.size(0), N = dz.size(1), Cout = dz.size(2);
  TORCH_CHECK(K >= 1 && W.size(0) % (2 * K + 1) == 0 && W.size(1) == Cout);
  const int C = W.size(0) / (2 * K + 1);
  TORCH_CHECK(C <= 64 && Cout <= 64);
  const int dt = dtype_code(dz);
  void* st = stream();
  DualBwdArgs a;
  a.gft = csr_ptrs(rpf_t, cif_t, vf_t, N);
  a.gbt = csr_ptrs(rpb_t, cib_t, vb_t, N);
  a.dz = dz.data_ptr(); a.W = W.data_ptr();
  a.B = B; a.N = N; a.C = C; a.Cout = Cout;
  auto dX = at::empty({B, N, C}, dz.options());

  auto bwd = [&](const void* xf, const void* pf1, const void* xb,
                 const void* pb1, void* outf, void* outb, int j, float alpha,
                 float beta) {
    a.xf = xf; a.pf1 = pf1; a.xb = xb; a.pb1 = pb1;
    a.outf = outf; a.outb = outb; a.final_step = j == 0;
    a.kofs_f = j * C; a.kofs_b = (int)(K + j) * C;
    a.alpha = alpha; a.beta = beta;
    stmgcn_dual_fused_bwd_step(st, dt, a);
  };
  // b_K = U_K; b_j = U_j + 2 G^T b_{j+1} - b_{j+2}; dX = U_0 + sum over both
  // chains of (G^T b_1 - b_2). Two ping/pong buffers per direction.
  const int nbuf = K > 1 ? 2 : 1;
  std::vector<at::Tensor> bufs;
  for (int i = 0; i < 2 * nbuf; ++i)
    bufs.push_back(at::empty({B, N, C}, dz.options()));
  void *f1 = bufs[0].data_ptr(), *g1 = bufs[1].data_ptr();   // b_{j+1}
  void *f2 = nullptr, *g2 = nullptr;                          // b_{j+2}
  bwd(nullptr, nullptr, nullptr, nullptr, f1, g1, (int)K, 0.f, 0.f);
  void* of = K > 1 ? bufs[2].data_ptr() : nullptr;
  void* og = K > 1 ? bufs[3].data_ptr() : nullptr;
  for (int j = (int)K - 1; j >= 1; --j) {
    bwd(f1, f2, g1, g2, of, og, j, 2.f, f2 ? -1.f : 0.f);
    f2 = f1; f1 = of; of = f2;   // overwritten next iteration (element-safe)
    g2 = g1; g1 = og; og = g2;
  }
  bwd(f1, f2, g1, g2, dX.data_ptr(), nullptr, 0, 1.f, f2 ? -1.f : 0.f);
  return dX;
}

// Plain axpby-SpMM on (B,N,C): out = alpha*(G @ xin) + beta*p1 — the
// recurrence-replay primitive for the fused wgrad (backward recompute).
at::Tensor spmm_axpby(at::Tensor xin, c10::optional<at::Tensor> p1,
                      at::Tensor rowptr, at::Tensor colidx, at::Tensor vals,
                      double alpha, double beta) {
  TORCH_CHECK(xin.is_cuda() && xin.dim() == 3 && xin.is_contiguous());
  const int B = xin.size(0), N = xin.size(1), C = xin.size(2);
  auto out = at::empty_like(xin);
  ChebFwdArgs a;   // W == null: no mix
  a.g = csr_ptrs(rowptr, colidx, vals, N);
  a.xin = xin.data_ptr();
  a.p1 = p1.has_value() ? p1->data_ptr() : nullptr;
  a.pout = out.data_ptr();
  a.B = B; a.N = N; a.C = a.Cout = C;
  a.alpha = (float)alpha; a.beta = (float)beta;
  stmgcn_cheb_fused_fwd_step(stream(), dtype_code(xin), a);
  return out;
}

// ---------------------------------------------------------------------------
// Fused LSTM: forward kernel + dgrad kernel + one batched
// wgrad kernel over the dA stream. lstm_bwd returns dA with logical shape
// (L, Tst, S_pad, 4H) but each 32-row sequence tile stored in the wgrad MFMA
// fragment order documented in csrc/common.h; lstm_wgrad expects that order.

static constexpr int kH = 64;

std::vector<at::Tensor> lstm_fwd(at::Tensor x, std::vector<at::Tensor> w_ih,
                                 std::vector<at::Tensor> w_hh,
                                 std::vector<at::Tensor> b_ih,
                                 std::vector<at::Tensor> b_hh, bool ret_seq,
                                 bool training, bool gru) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.is_contiguous());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf,
              "fused LSTM serves bf16/f16 (fp32 runs the torch path)");
  const int S = x.size(0), Tst = x.size(1), cin = x.size(2);
  const int L = (int)w_ih.size();
  TORCH_CHECK(L >= 1 && L <= 8 && Tst <= 16);
  TORCH_CHECK(cin == 1 || cin == kH, "C_in must be 1 or 64");
  for (int l = 0; l < L; ++l) {
    TORCH_CHECK(w_hh[l].size(0) == 4 * kH && w_hh[l].size(1) == kH,
                "hidden dim must be 64");
    TORCH_CHECK(w_ih[l].is_contiguous() && w_hh[l].is_contiguous());
    TORCH_CHECK(b_ih[l].scalar_type() == x.scalar_type() &&
                b_hh[l].scalar_type() == x.scalar_type());
  }
  const long nblk = (S + SEQ_TILE - 1) / SEQ_TILE;
  const long S_pad = nblk * SEQ_TILE;
  auto out = ret_seq ? at::empty({S, Tst, kH}, x.options())
                     : at::empty({S, kH}, x.options());
  at::Tensor hseq, cseq, gates;
  const void *wi[8], *wh[8], *bi[8], *bh[8];
  for (int l = 0; l < L; ++l) {
    wi[l] = w_ih[l].data_ptr(); wh[l] = w_hh[l].data_ptr();
    bi[l] = b_ih[l].data_ptr(); bh[l] = b_hh[l].data_ptr();
  }
  // hseq is the cross-layer hand-off in GLOBAL memory (LDS holds only the
  // live ping/pong slots) — allocated in eval too; cseq/gates only train.
  hseq = at::empty({L, Tst, S_pad, kH}, x.options());
  void* hp = hseq.data_ptr();
  void *cp = nullptr, *gp = nullptr;
  if (training) {
    cseq = at::empty({L, Tst, S_pad * kH}, x.options());
    gates = at::empty({L, Tst, S_pad * 4 * kH}, x.options());
    cp = cseq.data_ptr(); gp = gates.data_ptr();
  }
  stmgcn_lstm_fwd(stream(), dtype_code(x), x.data_ptr(), out.data_ptr(), hp,
                  cp, gp, wi, wh, bi, bh, S, Tst, L, cin, ret_seq ? 1 : 0,
                  gru ? 1 : 0);
  if (!training) return {out};
  return {out, hseq, cseq, gates};
}

std::vector<at::Tensor> lstm_bwd(at::Tensor dout, at::Tensor x,
                                 at::Tensor cseq, at::Tensor gates,
                                 std::vector<at::Tensor> w_ihT,
                                 std::vector<at::Tensor> w_hhT, bool ret_seq,
                                 bool gru) {
  TORCH_CHECK(dout.is_cuda() && x.is_contiguous());
  dout = dout.contiguous();
  const int S = x.size(0), Tst = x.size(1), cin = x.size(2);
  const int L = (int)w_ihT.size();
  const long nblk = (S + SEQ_TILE - 1) / SEQ_TILE;
  const long S_pad = nblk * SEQ_TILE;
  auto dx = at::empty_like(x);
  auto dA = at::empty({L, Tst, S_pad, 4 * kH}, x.options());
  // cross-layer dh hand-off scratch (global; LDS only holds dA tiles)
  at::Tensor dh;
  void* dhp = nullptr;
  if (L > 1) {
    dh = at::empty({(long)Tst * S_pad * kH}, x.options());
    dhp = dh.data_ptr();
  }
  const void *wi[8], *wh[8];
  for (int l = 0; l < L; ++l) {
    TORCH_CHECK(w_ihT[l].is_contiguous() && w_hhT[l].is_contiguous());
    wi[l] = w_ihT[l].data_ptr(); wh[l] = w_hhT[l].data_ptr();
  }
  stmgcn_lstm_bwd(stream(), dtype_code(x), dout.data_ptr(), x.data_ptr(),
                  cseq.data_ptr(), gates.data_ptr(), wi, wh, dx.data_ptr(),
                  dA.data_ptr(), dhp, S, Tst, L, cin, ret_seq ? 1 : 0,
                  gru ? 1 : 0);
  return {dx, dA};
}

// All-layer LSTM weight grads in ONE launch over the TILED dA stream (wgrad.hip):
// returns fp32 (dwih (L,4H,64), dwhh (L,4H,H), db (L,4H)); layer 0's live
// dwih columns are [:, :cin].
std::vector<at::Tensor> lstm_wgrad(at::Tensor dA, at::Tensor hseq, at::Tensor x) {
  TORCH_CHECK(dA.is_cuda() && dA.dim() == 4 && dA.is_contiguous());
  TORCH_CHECK(hseq.is_contiguous() && x.is_contiguous());
  const int L = dA.size(0), Tst = dA.size(1);
  const long S_pad = dA.size(2);
  const long R = (long)Tst * S_pad;
  const int S = x.size(0), cin = x.size(2);
  TORCH_CHECK(cin == 1 || cin == kH);
  TORCH_CHECK(dA.size(3) == 4 * kH && S_pad % SEQ_TILE == 0 && S <= S_pad,
              "dA must be (L, Tst, S_pad, 4H) with S_pad a multiple of 32");
  TORCH_CHECK(hseq.dim() == 4 && hseq.size(0) == L && hseq.size(1) == Tst &&
              hseq.size(2) == S_pad && hseq.size(3) == kH && x.size(1) == Tst);
  auto fopt = dA.options().dtype(at::kFloat);
  // one fill for all three atomic-accumulated outputs
  const long n_w = (long)L * 4 * kH * kH;
  auto flat = at::zeros({2 * n_w + (long)L * 4 * kH}, fopt);
  auto dwih = flat.narrow(0, 0, n_w).view({L, 4 * kH, kH});
  auto dwhh = flat.narrow(0, n_w, n_w).view({L, 4 * kH, kH});
  auto db = flat.narrow(0, 2 * n_w, (long)L * 4 * kH).view({L, 4 * kH});
  stmgcn_lstm_wgrad(stream(), dtype_code(dA), dA.data_ptr(), hseq.data_ptr(),
                    x.data_ptr(), dwih.data_ptr<float>(), dwhh.data_ptr<float>(),
                    db.data_ptr<float>(), R, S_pad, S, Tst, L, cin);
  return {dwih, dwhh, db};
}

// Finishing form of lstm_wgrad: the same launch, and its last workgroup per
// layer writes the gradients in the activations' dtype and in their final
// shapes. Returns [dw_ih_0, dw_hh_0, db_ih_0, db_hh_0, dw_ih_1, ...]: contiguous
// views of ONE flat buffer. One zero fill covers sums and tickets.
std::vector<at::Tensor> lstm_wgrad_grads(at::Tensor dA, at::Tensor hseq,
                                         at::Tensor x, bool gru) {
  TORCH_CHECK(dA.is_cuda() && dA.dim() == 4 && dA.is_contiguous());
  TORCH_CHECK(hseq.is_cuda() && x.is_cuda());
  TORCH_CHECK(hseq.is_contiguous() && x.is_contiguous() && x.dim() == 3);
  TORCH_CHECK(hseq.scalar_type() == dA.scalar_type() &&
              x.scalar_type() == dA.scalar_type());
  const int L = dA.size(0), Tst = dA.size(1);
  const long S_pad = dA.size(2);
  const long R = (long)Tst * S_pad;
  const int S = x.size(0), cin = x.size(2);
  TORCH_CHECK(L >= 1 && L <= 8 && (cin == 1 || cin == kH));
  TORCH_CHECK(dA.size(3) == 4 * kH && S_pad % SEQ_TILE == 0 && S <= S_pad,
              "dA must be (L, Tst, S_pad, 4H) with S_pad a multiple of 32");
  TORCH_CHECK(hseq.dim() == 4 && hseq.size(0) == L && hseq.size(1) == Tst &&
              hseq.size(2) == S_pad && hseq.size(3) == kH && x.size(1) == Tst);
  const long n_w = (long)L * 4 * kH * kH, n_b = (long)L * 4 * kH;
  auto ws = at::zeros({2 * n_w + n_b + 8}, dA.options().dtype(at::kFloat));
  float* wp = ws.data_ptr<float>();
  const long GH = (gru ? 3 : 4) * kH;
  const long total = GH * (cin + kH + 2) + (long)(L - 1) * GH * (2 * kH + 2);
  auto flat = at::empty({total}, dA.options());
  stmgcn_lstm_wgrad_grads(stream(), dtype_code(dA), dA.data_ptr(), hseq.data_ptr(),
                          x.data_ptr(), wp, wp + n_w, wp + 2 * n_w,
                          (unsigned*)(wp + 2 * n_w + n_b), flat.data_ptr(), R,
                          S_pad, S, Tst, L, cin, gru ? 1 : 0);
  std::vector<at::Tensor> out;
  long off = 0;
  for (int l = 0; l < L; ++l) {
    const long cl = l == 0 ? cin : kH;
    out.push_back(flat.narrow(0, off, GH * cl).view({GH, cl})); off += GH * cl;
    out.push_back(flat.narrow(0, off, GH * kH).view({GH, kH})); off += GH * kH;
    out.push_back(flat.narrow(0, off, GH)); off += GH;
    out.push_back(flat.narrow(0, off, GH)); off += GH;
  }
  return out;
}

// W_ih^T / W_hh^T of every layer (the operands lstm_bwd reads) in ONE launch
// into one buffer: returns [w_ihT_0.., w_hhT_0..] as views of it.
std::vector<at::Tensor> lstm_pack_bwd_weights(std::vector<at::Tensor> w_ih,
                                              std::vector<at::Tensor> w_hh) {
  const int L = (int)w_ih.size();
  TORCH_CHECK(L >= 1 && L <= 8 && (int)w_hh.size() == L);
  const auto dt = w_ih[0].scalar_type();
  TORCH_CHECK(dt == at::kBFloat16 || dt == at::kHalf);
  const int cin = w_ih[0].size(1);
  TORCH_CHECK(cin == 1 || cin == kH);
  const void *wi[8], *wh[8];
  for (int l = 0; l < L; ++l) {
    TORCH_CHECK(w_ih[l].is_cuda() && w_hh[l].is_cuda() && w_ih[l].is_contiguous() &&
                w_hh[l].is_contiguous() && w_ih[l].scalar_type() == dt &&
                w_hh[l].scalar_type() == dt);
    TORCH_CHECK(w_ih[l].dim() == 2 && w_ih[l].size(0) == 4 * kH &&
                w_ih[l].size(1) == (l == 0 ? cin : kH));
    TORCH_CHECK(w_hh[l].dim() == 2 && w_hh[l].size(0) == 4 * kH &&
                w_hh[l].size(1) == kH);
    wi[l] = w_ih[l].data_ptr(); wh[l] = w_hh[l].data_ptr();
  }
  const long total = 4L * kH * (cin + (long)(L - 1) * kH + (long)L * kH);
  auto flat = at::empty({total}, w_ih[0].options());
  stmgcn_lstm_pack_bwd_weights(stream(), wi, wh, L, cin, flat.data_ptr());
  std::vector<at::Tensor> out;
  long off = 0;
  for (int l = 0; l < L; ++l) {
    const long cl = l == 0 ? cin : kH;
    out.push_back(flat.narrow(0, off, 4 * kH * cl).view({cl, 4 * kH}));
    off += 4 * kH * cl;
  }
  for (int l = 0; l < L; ++l) {
    out.push_back(flat.narrow(0, off, 4L * kH * kH).view({kH, 4 * kH}));
    off += 4L * kH * kH;
  }
  return out;
}

// C = A^T @ B (+ db = colsum(B)) for tall-skinny wgrads (M<=256, N<=64).
std::vector<at::Tensor> atb_wgrad(at::Tensor A, at::Tensor B, bool want_db) {
  TORCH_CHECK(A.is_cuda() && A.dim() == 2 && B.dim() == 2);
  A = A.contiguous(); B = B.contiguous();
  const long rows = A.size(0);
  const int M = A.size(1), N = B.size(1);
  // M/N multiples of 8: the kernel reads 16-byte fragments at column
  // offsets cb*8; a ragged tail row would read past the end of A/B.
  TORCH_CHECK(B.size(0) == rows && M <= 256 && N <= 64 && M % 8 == 0 && N % 8 == 0);
  auto fopt = A.options().dtype(at::kFloat);
  auto C = at::zeros({M, N}, fopt);
  auto db = want_db ? at::zeros({N}, fopt) : at::Tensor();
  stmgcn_atb_wgrad(stream(), dtype_code(A), A.data_ptr(), B.data_ptr(),
                   C.data_ptr<float>(), want_db ? db.data_ptr<float>() : nullptr,
                   rows, M, N);
  return want_db ? std::vector<at::Tensor>{C, db} : std::vector<at::Tensor>{C};
}

// Accumulating variant: C (M,N) fp32 += A^T @ B, db (N,) fp32 += colsum(B).
// Caller provides (zeroed or accumulating) outputs — used by the fused
// ChebConv wgrad to land each support's dW_k slice in one flat buffer.
void atb_wgrad_into(at::Tensor A, at::Tensor B, at::Tensor C,
                    c10::optional<at::Tensor> db) {
  TORCH_CHECK(A.is_cuda() && A.dim() == 2 && B.dim() == 2);
  TORCH_CHECK(A.is_contiguous() && B.is_contiguous() && C.is_contiguous());
  TORCH_CHECK(C.scalar_type() == at::kFloat);
  const long rows = A.size(0);
  const int M = A.size(1), N = B.size(1);
  TORCH_CHECK(B.size(0) == rows && M <= 256 && N <= 64 && M % 8 == 0 && N % 8 == 0);
  TORCH_CHECK(C.size(0) == M && C.size(1) == N);
  float* dbp = db_ptr(db, N);
  stmgcn_atb_wgrad(stream(), dtype_code(A), A.data_ptr(), B.data_ptr(),
                   C.data_ptr<float>(), dbp, rows, M, N);
}

// Multi-source reduction GEMM: C[k*CA:(k+1)*CA, :] += As[k]^T @ B for up to
// 4 sources in ONE launch (B/dZ streamed once) + db += colsum(B). The fused
// ChebConv wgrad feeds the recurrence states [x, p_1, ..] here.
void atb_wgrad_multi(std::vector<at::Tensor> As, at::Tensor B, at::Tensor C,
                     c10::optional<at::Tensor> db) {
  TORCH_CHECK(!As.empty() && As.size() <= 4);
  const long rows = B.size(0);
  const int CA = As[0].size(1), N = B.size(1);
  const int M = (int)As.size() * CA;
  TORCH_CHECK(B.is_cuda() && B.is_contiguous() && B.dim() == 2);
  TORCH_CHECK(M <= 256 && N <= 64 && CA % 8 == 0 && N % 8 == 0);
  TORCH_CHECK(C.is_contiguous() && C.scalar_type() == at::kFloat &&
              C.size(0) == M && C.size(1) == N);
  const void* srcs[4];
  for (size_t i = 0; i < As.size(); ++i) {
    TORCH_CHECK(As[i].is_contiguous() && As[i].size(0) == rows &&
                As[i].size(1) == CA &&
                As[i].scalar_type() == B.scalar_type());
    srcs[i] = As[i].data_ptr();
  }
  float* dbp = db_ptr(db, N);
  stmgcn_atb_wgrad_multi(stream(), dtype_code(B), srcs, (int)As.size(), CA,
                         B.data_ptr(), C.data_ptr<float>(), dbp, rows, N);
}

// Finishing form of atb_wgrad_multi: returns dW (len(As)*CA, N) and, with
// want_db, db (N,) in the dtype of B. As[:split] (<= 4, with db) and As[split:]
// (<= 4) are one launch each over one zero-filled fp32 workspace of sums and
// tickets; each launch's last workgroup rounds its own rows.
std::vector<at::Tensor> atb_wgrad_multi_grads(std::vector<at::Tensor> As,
                                              at::Tensor B, int64_t split,
                                              bool want_db) {
  const int nsrc = (int)As.size();
  TORCH_CHECK(nsrc >= 1 && split >= 1 && split <= 4 && split <= nsrc &&
              nsrc - split <= 4);
  TORCH_CHECK(B.is_cuda() && B.is_contiguous() && B.dim() == 2);
  const long rows = B.size(0);
  const int CA = As[0].size(1), N = B.size(1);
  TORCH_CHECK(4 * CA <= 256 && N <= 64 && CA % 8 == 0 && N % 8 == 0);
  const void* srcs[8];
  for (int i = 0; i < nsrc; ++i) {
    TORCH_CHECK(As[i].is_cuda() && As[i].is_contiguous() && As[i].dim() == 2 &&
                As[i].size(0) == rows && As[i].size(1) == CA &&
                As[i].scalar_type() == B.scalar_type());
    srcs[i] = As[i].data_ptr();
  }
  const long nW = (long)nsrc * CA * N;
  auto ws = at::zeros({nW + N + 8}, B.options().dtype(at::kFloat));
  float* wp = ws.data_ptr<float>();
  unsigned* tickets = (unsigned*)(wp + nW + N);
  auto dW = at::empty({(long)nsrc * CA, (long)N}, B.options());
  at::Tensor db;
  if (want_db) db = at::empty({N}, B.options());
  const int dt = dtype_code(B);
  const long es = B.element_size();
  stmgcn_atb_wgrad_multi_grads(stream(), dt, srcs, (int)split, CA, B.data_ptr(), wp,
                               want_db ? wp + nW : nullptr, tickets, dW.data_ptr(),
                               want_db ? db.data_ptr() : nullptr, rows, N);
  if (split < nsrc) {
    const long r0 = split * CA * (long)N;
    stmgcn_atb_wgrad_multi_grads(stream(), dt, srcs + split, nsrc - (int)split, CA,
                                 B.data_ptr(), wp + r0, nullptr, tickets + 1,
                                 (char*)dW.data_ptr() + r0 * es, nullptr, rows, N);
  }
  return want_db ? std::vector<at::Tensor>{dW, db} : std::vector<at::Tensor>{dW};
}

// dz = dy * (y > 0) in one launch (the ReLU mask of the gconv backward)
at::Tensor relu_bwd(at::Tensor dy, at::Tensor y) {
  TORCH_CHECK(dy.is_cuda() && y.is_cuda() && dy.sizes() == y.sizes() &&
              dy.scalar_type() == y.scalar_type());
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 || dy.scalar_type() == at::kHalf,
              "relu_bwd serves bf16/f16");
  dy = dy.contiguous(); y = y.contiguous();
  auto dz = at::empty_like(dy);
  stmgcn_relu_bwd(stream(), dtype_code(dy), dy.data_ptr(), y.data_ptr(),
                  dz.data_ptr(), dy.numel());
  return dz;
}

at::Tensor mfma_probe(at::Tensor A, at::Tensor B) {
  TORCH_CHECK(A.is_cuda() && A.scalar_type() == at::kBFloat16);
  auto D = at::empty({16, 16}, A.options().dtype(at::kFloat));
  stmgcn_mfma_probe(stream(), A.contiguous().data_ptr(),
                    B.contiguous().data_ptr(), D.data_ptr());
  return D;
}

// ---------------------------------------------------------------------------
// pointwise.hip ops: K3 seqsum/permute, K4 gate, K7 head, K8 loss, K9 Adam

at::Tensor seqsum_permute(at::Tensor obs) {
  TORCH_CHECK(obs.is_cuda() && obs.dim() == 4 && obs.is_contiguous());
  const int B = obs.size(0), Tst = obs.size(1), N = obs.size(2), C = obs.size(3);
  auto out = at::empty({B, N, Tst}, obs.options());
  stmgcn_seqsum_permute(stream(), dtype_code(obs), obs.data_ptr(),
                        out.data_ptr(), B, Tst, N, C);
  return out;
}

at::Tensor seqsum_permute_bwd(at::Tensor dxs, int64_t C) {
  TORCH_CHECK(dxs.is_cuda() && dxs.dim() == 3);
  dxs = dxs.contiguous();
  const int B = dxs.size(0), N = dxs.size(1), Tst = dxs.size(2);
  auto dobs = at::empty({B, Tst, N, C}, dxs.options());
  stmgcn_seqsum_permute_bwd(stream(), dtype_code(dxs), dxs.data_ptr(),
                            dobs.data_ptr(), B, Tst, N, (int)C);
  return dobs;
}

// node_major: out is (B,N,T,C) — the sequence-major layout the RNN consumes —
// instead of (B,T,N,C). z is the pooled mean (fp32) either way.
std::vector<at::Tensor> gate_fwd(at::Tensor obs, at::Tensor g, at::Tensor xs,
                                 at::Tensor fcw, at::Tensor fcb, bool node_major) {
  TORCH_CHECK(obs.is_cuda() && obs.dim() == 4 && obs.is_contiguous());
  const int B = obs.size(0), Tst = obs.size(1), N = obs.size(2), C = obs.size(3);
  TORCH_CHECK(Tst <= 16, "gate kernel serves T <= 16");
  TORCH_CHECK(g.numel() == (long)B * N * Tst && xs.numel() == g.numel() &&
              fcw.numel() == Tst * Tst && fcb.numel() == Tst);
  TORCH_CHECK(g.is_cuda() && xs.is_cuda() && fcw.is_cuda() && fcb.is_cuda());
  TORCH_CHECK(g.scalar_type() == obs.scalar_type() &&
              xs.scalar_type() == obs.scalar_type() &&
              fcw.scalar_type() == obs.scalar_type() &&
              fcb.scalar_type() == obs.scalar_type());
  auto fopt = obs.options().dtype(at::kFloat);
  // z doubles as the multi-block zsum atomic target, followed by one arrival
  // ticket per batch row -> one zero fill for both
  auto zt = at::zeros({(long)B * Tst + B}, fopt);
  auto z = zt.narrow(0, 0, (long)B * Tst).view({B, Tst});
  auto u = at::empty({B, Tst}, fopt), s = at::empty({B, Tst}, fopt);
  auto out = node_major ? at::empty({B, N, Tst, C}, obs.options())
                        : at::empty_like(obs);
  auto gc = g.contiguous(), xc = xs.contiguous(), wc = fcw.contiguous(),
       bc = fcb.contiguous();
  stmgcn_gate_fwd(stream(), dtype_code(obs), gc.data_ptr(), xc.data_ptr(),
                  wc.data_ptr(), bc.data_ptr(), obs.data_ptr(),
                  zt.data_ptr<float>(), u.data_ptr<float>(), s.data_ptr<float>(),
                  (unsigned*)(zt.data_ptr<float>() + (long)B * Tst),
                  out.data_ptr(), B, Tst, N, C, node_major ? 1 : 0);
  return {out, z, u, s};
}

// Returns {dobs (undefined without want_dobs), dg, dw (T,T), db (T,), dw fp32,
// db fp32}: dw/db are summed over the batch in-kernel, in the dtype of obs and
// in fp32. node_major: dout is (B,N,T,C).
std::vector<at::Tensor> gate_bwd(at::Tensor dout, at::Tensor obs, at::Tensor fcw,
                                 at::Tensor z, at::Tensor u, at::Tensor s,
                                 bool node_major, bool want_dobs) {
  dout = dout.contiguous();
  TORCH_CHECK(obs.is_cuda() && obs.dim() == 4 && obs.is_contiguous());
  const int B = obs.size(0), Tst = obs.size(1), N = obs.size(2), C = obs.size(3);
  TORCH_CHECK(dout.is_cuda() && fcw.is_cuda() && z.is_cuda() && u.is_cuda() &&
              s.is_cuda() && z.scalar_type() == at::kFloat &&
              u.scalar_type() == at::kFloat && s.scalar_type() == at::kFloat);
  TORCH_CHECK(Tst <= 16 && dout.numel() == obs.numel() &&
              dout.scalar_type() == obs.scalar_type() &&
              fcw.scalar_type() == obs.scalar_type() && fcw.numel() == Tst * Tst);
  TORCH_CHECK(z.is_contiguous() && u.is_contiguous() && s.is_contiguous() &&
              z.numel() == (long)B * Tst && u.numel() == z.numel() &&
              s.numel() == z.numel());
  auto fopt = obs.options().dtype(at::kFloat);
  // dz doubles as the multi-block ds atomic target, followed by the B + 1
  // arrival tickets -> one zero fill for both
  auto dzt = at::zeros({(long)B * Tst + B + 1}, fopt);
  auto dw_part = at::empty({B, Tst, Tst}, fopt);
  auto db_part = at::empty({B, Tst}, fopt);
  auto dw_f = at::empty({Tst, Tst}, fopt), db_f = at::empty({Tst}, fopt);
  auto dw = at::empty({Tst, Tst}, obs.options()), db = at::empty({Tst}, obs.options());
  at::Tensor dobs;
  if (want_dobs) dobs = at::empty_like(obs);
  auto dg = at::empty({B, N, Tst}, obs.options());
  auto wc = fcw.contiguous();
  stmgcn_gate_bwd(stream(), dtype_code(obs), dout.data_ptr(), obs.data_ptr(),
                  wc.data_ptr(), z.data_ptr<float>(), u.data_ptr<float>(),
                  s.data_ptr<float>(), dzt.data_ptr<float>(),
                  dw_part.data_ptr<float>(), db_part.data_ptr<float>(),
                  (unsigned*)(dzt.data_ptr<float>() + (long)B * Tst),
                  dw_f.data_ptr<float>(), db_f.data_ptr<float>(), dw.data_ptr(),
                  db.data_ptr(), want_dobs ? dobs.data_ptr() : nullptr,
                  dg.data_ptr(), B, Tst, N, C, node_major ? 1 : 0);
  return {dobs, dg, dw, db, dw_f, db_f};
}

std::vector<at::Tensor> head_fwd(std::vector<at::Tensor> feats, at::Tensor w,
                                 at::Tensor bias) {
  auto f0 = feats[0].contiguous();
  TORCH_CHECK(f0.is_cuda() && f0.dim() == 3 && feats.size() >= 1 && feats.size() <= 3);
  const long BN = (long)f0.size(0) * f0.size(1);
  const int G = f0.size(2);
  TORCH_CHECK(G <= 64, "head kernel serves G <= 64");
  auto y = at::empty({f0.size(0), f0.size(1), 1}, f0.options());
  auto fsum = at::empty_like(f0);
  TORCH_CHECK(bias.scalar_type() == f0.scalar_type());
  stmgcn_head_fwd(stream(), dtype_code(f0), f0.data_ptr(),
                  feats.size() > 1 ? feats[1].contiguous().data_ptr() : nullptr,
                  feats.size() > 2 ? feats[2].contiguous().data_ptr() : nullptr,
                  w.contiguous().data_ptr(), bias.contiguous().data_ptr(),
                  y.data_ptr(), fsum.data_ptr(), G, BN);
  return {y, fsum};
}

at::Tensor head_bwd(at::Tensor dy, at::Tensor w, int64_t G) {
  dy = dy.contiguous();
  const long BN = (long)dy.size(0) * dy.size(1);
  auto dfeat = at::empty({dy.size(0), dy.size(1), G}, dy.options());
  stmgcn_head_bwd(stream(), dtype_code(dy), dy.data_ptr(),
                  w.contiguous().data_ptr(), dfeat.data_ptr(), (int)G, BN);
  return dfeat;
}

// dw[g] = sum_r dy[r] fsum[r,g]; db = sum dy — fp32 accumulated reduction.
std::vector<at::Tensor> head_wgrad(at::Tensor dy, at::Tensor fsum) {
  dy = dy.contiguous();
  fsum = fsum.contiguous();
  const long BN = (long)fsum.size(0) * fsum.size(1);
  const int G = fsum.size(2);
  auto fopt = dy.options().dtype(at::kFloat);
  auto dw = at::zeros({G}, fopt);
  auto db = at::zeros({1}, fopt);
  stmgcn_head_wgrad(stream(), dtype_code(dy), dy.data_ptr(), fsum.data_ptr(),
                    dw.data_ptr<float>(), db.data_ptr<float>(), G, BN);
  return {dw, db};
}

// Finishing form: dw (1, G) and db (1,) in the dtype of dy from one zero-filled
// fp32 workspace (sums + ticket); the kernel's last workgroup rounds them.
std::vector<at::Tensor> head_wgrad_grads(at::Tensor dy, at::Tensor fsum) {
  dy = dy.contiguous();
  fsum = fsum.contiguous();
  TORCH_CHECK(fsum.is_cuda() && dy.is_cuda() && fsum.dim() == 3 &&
              dy.scalar_type() == fsum.scalar_type());
  const long BN = (long)fsum.size(0) * fsum.size(1);
  const int G = fsum.size(2);
  TORCH_CHECK(G <= 64 && dy.numel() == BN);
  auto ws = at::zeros({64 + 8}, dy.options().dtype(at::kFloat));
  float* wp = ws.data_ptr<float>();
  auto dw = at::empty({1, G}, dy.options());
  auto db = at::empty({1}, dy.options());
  stmgcn_head_wgrad_grads(stream(), dtype_code(dy), dy.data_ptr(), fsum.data_ptr(),
                          wp, wp + 64, (unsigned*)(wp + 68), dw.data_ptr(),
                          db.data_ptr(), G, BN);
  return {dw, db};
}

std::vector<at::Tensor> mse_fwd(at::Tensor pred, at::Tensor tgt) {
  pred = pred.contiguous();
  auto loss = at::zeros({}, pred.options().dtype(at::kFloat));
  auto diff = at::empty_like(pred);
  stmgcn_mse_fwd(stream(), dtype_code(pred), pred.data_ptr(),
                 tgt.contiguous().data_ptr(), loss.data_ptr<float>(),
                 diff.data_ptr(), pred.numel());
  return {loss, diff};
}

at::Tensor mse_bwd(at::Tensor diff, at::Tensor gscale) {
  auto dpred = at::empty_like(diff);
  stmgcn_mse_bwd(stream(), dtype_code(diff), diff.data_ptr(),
                 gscale.contiguous().data_ptr<float>(), dpred.data_ptr(),
                 diff.numel());
  return dpred;
}

// ---- wide head (multi-step horizon): O = fc_weight.size(0), 2 <= O <= 32 ----
static void head_multi_check(const at::Tensor& a, int64_t G, int64_t O) {
  TORCH_CHECK(a.is_cuda() && (a.scalar_type() == at::kBFloat16 ||
                              a.scalar_type() == at::kHalf),
              "wide head serves bf16/f16");
  TORCH_CHECK(O >= 2 && O <= 32 && G >= 8 && G <= 64 && G % 8 == 0,
              "wide head serves 2 <= O <= 32, G <= 64 with G % 8 == 0");
}

// {y (B, N, O), fsum (B, N, G)}
std::vector<at::Tensor> head_multi_fwd(std::vector<at::Tensor> feats,
                                       at::Tensor w, at::Tensor bias) {
  TORCH_CHECK(feats.size() >= 1 && feats.size() <= 3 && w.dim() == 2);
  auto f0 = feats[0].contiguous();
  TORCH_CHECK(f0.dim() == 3);
  const long BN = (long)f0.size(0) * f0.size(1);
  const int G = f0.size(2), O = w.size(0);
  head_multi_check(f0, G, O);
  TORCH_CHECK(w.size(1) == G && bias.numel() == O &&
              w.scalar_type() == f0.scalar_type() &&
              bias.scalar_type() == f0.scalar_type() && w.is_cuda() &&
              bias.is_cuda());
  std::vector<at::Tensor> fc{f0};
  for (size_t m = 1; m < feats.size(); ++m) {
    TORCH_CHECK(feats[m].sizes() == f0.sizes() && feats[m].is_cuda() &&
                feats[m].scalar_type() == f0.scalar_type());
    fc.push_back(feats[m].contiguous());
  }
  auto wc = w.contiguous(), bc = bias.contiguous();
  auto y = at::empty({f0.size(0), f0.size(1), O}, f0.options());
  auto fsum = at::empty_like(f0);
  stmgcn_head_multi_fwd(stream(), dtype_code(f0), fc[0].data_ptr(),
                        fc.size() > 1 ? fc[1].data_ptr() : nullptr,
                        fc.size() > 2 ? fc[2].data_ptr() : nullptr,
                        wc.data_ptr(), bc.data_ptr(), y.data_ptr(),
                        fsum.data_ptr(), G, O, BN);
  return {y, fsum};
}

at::Tensor head_multi_bwd(at::Tensor dy, at::Tensor w) {
  TORCH_CHECK(dy.dim() == 3 && w.dim() == 2 && w.is_cuda());
  dy = dy.contiguous();
  const long BN = (long)dy.size(0) * dy.size(1);
  const int O = w.size(0), G = w.size(1);
  head_multi_check(dy, G, O);
  TORCH_CHECK(dy.size(2) == O && w.scalar_type() == dy.scalar_type());
  auto wc = w.contiguous();
  auto dfeat = at::empty({dy.size(0), dy.size(1), G}, dy.options());
  stmgcn_head_multi_bwd(stream(), dtype_code(dy), dy.data_ptr(), wc.data_ptr(),
                        dfeat.data_ptr(), G, O, BN);
  return dfeat;
}

static long head_multi_wgrad_check(at::Tensor& dy, at::Tensor& fsum) {
  TORCH_CHECK(dy.dim() == 3 && fsum.dim() == 3 && fsum.is_cuda() &&
              dy.scalar_type() == fsum.scalar_type() &&
              dy.size(0) == fsum.size(0) && dy.size(1) == fsum.size(1));
  dy = dy.contiguous();
  fsum = fsum.contiguous();
  head_multi_check(dy, fsum.size(2), dy.size(2));
  return (long)fsum.size(0) * fsum.size(1);
}

// dW (O, G) = dy^T fsum and db (O,) = colsum(dy) as fp32 sums
std::vector<at::Tensor> head_multi_wgrad(at::Tensor dy, at::Tensor fsum) {
  const long BN = head_multi_wgrad_check(dy, fsum);
  const int G = fsum.size(2), O = dy.size(2);
  auto fopt = dy.options().dtype(at::kFloat);
  auto dw = at::zeros({O, G}, fopt);
  auto db = at::zeros({O}, fopt);
  stmgcn_head_multi_wgrad(stream(), dtype_code(dy), dy.data_ptr(),
                          fsum.data_ptr(), dw.data_ptr<float>(),
                          db.data_ptr<float>(), nullptr, nullptr, nullptr, G, O,
                          BN);
  return {dw, db};
}

// Finishing form: dW (O, G) and db (O,) in the dtype of dy from one zero-filled
// fp32 workspace (O*G sums, 32 db slots, ticket); the last workgroup rounds.
std::vector<at::Tensor> head_multi_wgrad_grads(at::Tensor dy, at::Tensor fsum) {
  const long BN = head_multi_wgrad_check(dy, fsum);
  const int G = fsum.size(2), O = dy.size(2);
  auto ws = at::zeros({(long)O * G + 32 + 8}, dy.options().dtype(at::kFloat));
  float* wp = ws.data_ptr<float>();
  auto dw = at::empty({O, G}, dy.options());
  auto db = at::empty({O}, dy.options());
  stmgcn_head_multi_wgrad(stream(), dtype_code(dy), dy.data_ptr(),
                          fsum.data_ptr(), wp, wp + (long)O * G,
                          (unsigned*)(wp + (long)O * G + 32), dw.data_ptr(),
                          db.data_ptr(), G, O, BN);
  return {dw, db};
}

// ---- masked loss: {res (2,) fp32 = loss, 1 / max(count_valid, 1); diff} ----
std::vector<at::Tensor> masked_loss_fwd(at::Tensor pred, at::Tensor tgt,
                                        int64_t kind) {
  TORCH_CHECK(pred.is_cuda() && tgt.is_cuda() && pred.sizes() == tgt.sizes() &&
              pred.scalar_type() == tgt.scalar_type());
  TORCH_CHECK(kind >= 0 && kind <= 2, "masked loss kind: 0 mse, 1 mae, 2 huber");
  // count_valid is a 32-bit integer sum
  TORCH_CHECK(pred.numel() > 0 && pred.numel() < (1LL << 32));
  pred = pred.contiguous();
  tgt = tgt.contiguous();
  auto fopt = pred.options().dtype(at::kFloat);
  auto ws = at::zeros({4}, fopt);     // sum, count, ticket: one fill
  auto res = at::empty({2}, fopt);
  auto diff = at::empty_like(pred);
  stmgcn_masked_loss_fwd(stream(), dtype_code(pred), (int)kind, pred.data_ptr(),
                         tgt.data_ptr(), ws.data_ptr<float>(),
                         res.data_ptr<float>(), diff.data_ptr(), pred.numel());
  return {res, diff};
}

at::Tensor masked_loss_bwd(at::Tensor diff, at::Tensor res, at::Tensor gscale,
                           int64_t kind) {
  TORCH_CHECK(diff.is_cuda() && diff.is_contiguous() && res.is_cuda() &&
              gscale.is_cuda() && res.scalar_type() == at::kFloat &&
              gscale.scalar_type() == at::kFloat && res.numel() == 2 &&
              res.is_contiguous() && gscale.numel() == 1);
  TORCH_CHECK(kind >= 0 && kind <= 2 && diff.numel() > 0);
  auto dpred = at::empty_like(diff);
  stmgcn_masked_loss_bwd(stream(), dtype_code(diff), (int)kind, diff.data_ptr(),
                         res.data_ptr<float>(), gscale.data_ptr<float>(),
                         dpred.data_ptr(), diff.numel());
  return dpred;
}

// Pack per-param grads (or zeros for undefined) into the flat grad arena.
// grads: list aligned with the arena layout; offsets/lens in elements.
void gather_grads(std::vector<at::Tensor> grads, std::vector<int64_t> ofs,
                  std::vector<int64_t> lens, at::Tensor arena) {
  TORCH_CHECK(arena.is_cuda() && arena.is_contiguous());
  const int n = (int)ofs.size();
  const void* srcs[64];
  long o[64];
  int l[64];
  int dt = dtype_code(arena);
  for (int base = 0; base < n; base += 64) {
    const int cnt = std::min(64, n - base);
    for (int i = 0; i < cnt; ++i) {
      const auto& g = grads[base + i];
      if (g.defined() && g.numel() > 0) {
        TORCH_CHECK(g.is_contiguous() && g.scalar_type() == arena.scalar_type());
        srcs[i] = g.data_ptr();
      } else {
        srcs[i] = nullptr;   // no grad flowed -> zero-fill the segment
      }
      o[i] = ofs[base + i];
      l[i] = (int)lens[base + i];
    }
    stmgcn_gather_grads(stream(), dt, srcs, o, l, cnt, arena.data_ptr());
  }
}

void adam_step(at::Tensor master, at::Tensor param, at::Tensor grad,
               at::Tensor m, at::Tensor v, at::Tensor hyper) {
  TORCH_CHECK(master.is_cuda() && master.scalar_type() == at::kFloat);
  TORCH_CHECK(hyper.numel() == 9 && hyper.scalar_type() == at::kFloat);
  stmgcn_adam(stream(), dtype_code(param), master.data_ptr<float>(),
              param.data_ptr(), grad.data_ptr(), m.data_ptr<float>(),
              v.data_ptr<float>(), hyper.data_ptr<float>(), master.numel());
}
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("lstm_fwd", &lstm_fwd, "Fused multi-layer LSTM forward (persistent)");
  m.def("lstm_bwd", &lstm_bwd, "Fused LSTM dgrad (BPTT in-kernel)");
  m.def("lstm_wgrad", &lstm_wgrad, "All-layer LSTM weight grads, one launch");
  m.def("lstm_wgrad_grads", &lstm_wgrad_grads,
        "All-layer LSTM/GRU weight grads, finished in-kernel: final dtype/shapes");
  m.def("lstm_pack_bwd_weights", &lstm_pack_bwd_weights,
        "W_ih^T / W_hh^T of every layer in one launch (lstm_bwd operands)");
  m.def("atb_wgrad_multi_grads", &atb_wgrad_multi_grads,
        "All-support wgrad finished in-kernel: dW / db in the parameter dtype");
  m.def("relu_bwd", &relu_bwd, "dz = dy * (y > 0)");
  m.def("head_wgrad_grads", &head_wgrad_grads,
        "K7: dw/db reduction finished in-kernel (parameter dtype)");
  m.def("atb_wgrad", &atb_wgrad, "C = A^T B reduction GEMM (+colsum(B))");
  m.def("mfma_probe", &mfma_probe, "16x16x32 bf16 MFMA fragment-layout probe");
  m.def("seqsum_permute", &seqsum_permute, "K3: feature-sum + transpose");
  m.def("seqsum_permute_bwd", &seqsum_permute_bwd);
  m.def("gate_fwd", &gate_fwd, "K4: fused contextual gate forward",
        py::arg("obs"), py::arg("g"), py::arg("xs"), py::arg("fcw"),
        py::arg("fcb"), py::arg("node_major") = false);
  m.def("gate_bwd", &gate_bwd, "K4: fused contextual gate backward",
        py::arg("dout"), py::arg("obs"), py::arg("fcw"), py::arg("z"),
        py::arg("u"), py::arg("s"), py::arg("node_major") = false,
        py::arg("want_dobs") = true);
  m.def("head_fwd", &head_fwd, "K7: branch-sum + FC head forward");
  m.def("head_bwd", &head_bwd, "K7: head backward (dfeat)");
  m.def("head_wgrad", &head_wgrad, "K7: dw/db reduction (no library GEMM)");
  m.def("head_multi_fwd", &head_multi_fwd,
        "K7 wide: branch-sum + FC head forward, 2 <= O <= 32 columns (MFMA)");
  m.def("head_multi_bwd", &head_multi_bwd, "K7 wide: dfeat = dy W (MFMA)");
  m.def("head_multi_wgrad", &head_multi_wgrad,
        "K7 wide: dW / db reduction, fp32 sums");
  m.def("head_multi_wgrad_grads", &head_multi_wgrad_grads,
        "K7 wide: dW / db reduction finished in-kernel (parameter dtype)");
  m.def("masked_loss_fwd", &masked_loss_fwd,
        "K8 masked: MSE / MAE / Huber over non-NaN targets, loss on the device");
  m.def("masked_loss_bwd", &masked_loss_bwd, "K8 masked: fused grad");
  m.def("mse_fwd", &mse_fwd, "K8: fused MSE loss forward");
  m.def("mse_bwd", &mse_bwd, "K8: fused MSE grad");
  m.def("adam_step", &adam_step, "K9: multi-tensor Adam over flat arena");
  m.def("gather_grads", &gather_grads, "K9b: pack per-param grads into arena");
  m.def("cheb_apply", &cheb_apply,
        "Support stack S[b,n,k,c] = (T_k(G) x)[b,n,c] via in-kernel recurrence");
  m.def("cheb_combine", &cheb_combine,
        "Z = sum_k T_k(G) U_k via Clenshaw (pass G^T CSR for gradients)");
  m.def("cheb_gconv_fused_fwd", &cheb_gconv_fused_fwd,
        "Fused ChebConv fwd: recurrence + MFMA mix + bias + act, no stack");
  m.def("cheb_gconv_fused_bwd_dx", &cheb_gconv_fused_bwd_dx,
        "Fused ChebConv dX: Clenshaw over G^T with in-kernel U = dz W^T");
  m.def("dual_gconv_fused_fwd", &dual_gconv_fused_fwd,
        "Fused dual random-walk gconv fwd: both recurrences + mix per launch");
  m.def("dual_gconv_fused_bwd_dx", &dual_gconv_fused_bwd_dx,
        "Fused dual random-walk gconv dX: both Clenshaw chains per launch");
  m.def("spmm_axpby", &spmm_axpby,
        "out = alpha*(G @ xin) + beta*p1 on (B,N,C) (recurrence replay)");
  m.def("atb_wgrad_into", &atb_wgrad_into,
        "C += A^T B (+db += colsum B) into caller-provided fp32 buffers");
  m.def("atb_wgrad_multi", &atb_wgrad_multi,
        "All-support wgrad: C[k] += As[k]^T B in one launch, B read once");
}
