// Python bindings + host-side sequencing for the stmgcn_amd HIP kernels.
// Device code lives in the .hip translation units (pure HIP, no torch);
// this file owns at::Tensor plumbing, stream lookup and launch ordering.
// The entry points, their argument structs and every workspace layout are
// declared once, in kernels.h; pointers come from the checked accessors below.
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

// Every entry point reports a status (kernels.h); a non-null one is raised.
void launched(const char* entry, const char* status) {
  TORCH_CHECK(status == nullptr, entry, " failed: ", status);
}
#define STM_LAUNCH(entry, ...) launched(#entry, entry(__VA_ARGS__))

bool is_lowp(const at::Tensor& t) {
  return t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kHalf;
}

// The only code in this file that calls data_ptr. A binding builds one Ptrs
// from its name and its first tensor, which fixes the device, and obtains every
// pointer it hands to a launcher here, with the element count that launcher
// will index: the kernels index unchecked, so a tensor for another shape, dtype
// or device must not reach them.
class Ptrs {
 public:
  Ptrs(const char* fn, const at::Tensor& first) : fn_(fn) {
    TORCH_CHECK(first.defined() && first.is_cuda(), fn, ": tensors must be on a GPU");
    dev_ = first.device();
  }
  // t on the binding's device, of dtype dt, contiguous, exactly n elements
  template <typename T = void>
  T* in(const at::Tensor& t, const char* name, at::ScalarType dt, int64_t n) const {
    TORCH_CHECK(t.defined() && t.device() == dev_, fn_, ": ", name, " must be on ", dev_);
    TORCH_CHECK(t.scalar_type() == dt, fn_, ": ", name, " must be ", dt, ", is ",
                t.scalar_type());
    TORCH_CHECK(t.is_contiguous(), fn_, ": ", name, " must be contiguous");
    TORCH_CHECK(t.numel() == n, fn_, ": ", name, " must have ", n, " elements, has ",
                t.numel());
    return static_cast<T*>(t.data_ptr());
  }
  // an optional tensor: null when absent
  template <typename T = void>
  T* opt(const c10::optional<at::Tensor>& t, const char* name, at::ScalarType dt,
         int64_t n) const {
    return t.has_value() ? in<T>(*t, name, dt, n) : nullptr;
  }
  // a possibly strided tensor: `keep` receives the contiguous copy and must
  // outlive the launches (a temporary would be freed before they run)
  template <typename T = void>
  T* copy(const at::Tensor& t, const char* name, at::ScalarType dt, int64_t n,
          at::Tensor& keep) const {
    TORCH_CHECK(t.defined(), fn_, ": ", name, " is undefined");
    keep = t.contiguous();
    return in<T>(keep, name, dt, n);
  }
  template <typename T = void>
  T* opt_copy(const c10::optional<at::Tensor>& t, const char* name, at::ScalarType dt,
              int64_t n, at::Tensor& keep) const {
    return t.has_value() ? copy<T>(*t, name, dt, n, keep) : nullptr;
  }
  // a tensor the binding allocated itself (undefined: null)
  template <typename T = void> static T* own(const at::Tensor& t) {
    return t.defined() ? static_cast<T*>(t.data_ptr()) : nullptr;
  }
  // rowptr (N + 1), colidx / vals (nnz) of one generator
  StmCsr csr(const at::Tensor& rowptr, const at::Tensor& colidx, const at::Tensor& vals,
             int N) const {
    return {in<int>(rowptr, "rowptr", at::kInt, N + 1),
            in<int>(colidx, "colidx", at::kInt, vals.defined() ? vals.numel() : 0),
            in<float>(vals, "vals", at::kFloat, colidx.numel())};
  }

 private:
  const char* fn_;
  c10::Device dev_{c10::kCPU};
};

// one recurrence step: out_slice = alpha * G @ x_slice + beta*p1 + gamma*p2
struct SpmmStep {
  int dt;
  SpmmArgs a;   // g, B, N, C fixed per binding
  void operator()(StmSlice xin, StmSlice p1, StmSlice p2, StmSlice out, float alpha,
                  float beta, float gamma) {
    a.xin = xin; a.p1 = p1; a.p2 = p2; a.out = out;
    a.alpha = alpha; a.beta = beta; a.gamma = gamma;
    STM_LAUNCH(stmgcn_spmm_step, stream(), dt, a);
  }
};
const StmSlice kNone{};

}  // namespace

// x: (B, N, C) -> S: (B, N, K_s, C); slice k of S is T_k(G) @ x.
// kind single (localpool): K_s == 1, S[...,0,:] = G @ x.
at::Tensor cheb_apply(at::Tensor x, at::Tensor rowptr, at::Tensor colidx,
                      at::Tensor vals, int64_t K_s, bool single) {
  TORCH_CHECK(x.dim() == 3 && K_s >= 1);
  const Ptrs p("cheb_apply", x);
  const int B = x.size(0), N = x.size(1), C = x.size(2);
  SpmmStep step{dtype_code(x), {}};
  step.a.g = p.csr(rowptr, colidx, vals, N);
  step.a.B = B; step.a.N = N; step.a.C = C;
  auto S = at::empty({B, N, K_s, C}, x.options());
  const long es = x.element_size();
  char* Sp = p.own<char>(S);
  const long so = K_s * (long)C, bo = (long)N * K_s * C;  // S row/batch strides
  auto sl = [&](int k) -> StmSlice { return {Sp + (long)k * C * es, so, bo}; };
  const StmSlice xs{p.in(x, "x", x.scalar_type(), x.numel()), C, (long)N * C};

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
  TORCH_CHECK(U.dim() == 4);
  const Ptrs p("cheb_combine", U);
  const int B = U.size(0), N = U.size(1), K_s = U.size(2), C = U.size(3);
  SpmmStep step{dtype_code(U), {}};
  step.a.g = p.csr(rowptr, colidx, vals, N);
  step.a.B = B; step.a.N = N; step.a.C = C;
  auto Z = at::empty({B, N, C}, U.options());
  const long es = U.element_size();
  const char* Up = p.in<const char>(U, "U", U.scalar_type(), U.numel());
  const long su = (long)K_s * C, bu = (long)N * K_s * C;
  const long sz = C, bz = (long)N * C;
  auto ul = [&](int k) -> StmSlice { return {Up + (long)k * C * es, su, bu}; };
  const StmSlice Zs{p.own(Z), sz, bz};

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
  StmSlice sb1{p.own(bk1), sz, bz}, sb2 = kNone;
  step(kNone, kNone, ul(K), sb1, 0.f, 0.f, 1.f);   // b_K = U_K  (copy)
  for (int j = K - 1; j >= 1; --j) {
    auto bnew = at::empty({B, N, C}, U.options());
    // b_j = 2 G b_{j+1} - b_{j+2} + U_j   (p1 = b_{j+2}, p2 = U_j);
    // b_{K+1} == 0 -> p1 skipped (beta 0) on the first iteration
    step(sb1, sb2, ul(j), {p.own(bnew), sz, bz}, 2.f, sb2.ptr ? -1.f : 0.f, 1.f);
    bk2 = bk1; bk1 = bnew;
    sb2 = sb1; sb1 = {p.own(bk1), sz, bz};
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
  TORCH_CHECK(x.dim() == 3 && W.dim() == 2);
  const Ptrs p("cheb_gconv_fused_fwd", x);
  const auto xt = x.scalar_type();
  const int B = x.size(0), N = x.size(1), C = x.size(2), Cout = W.size(1);
  TORCH_CHECK(C <= 64 && Cout <= 64, "fused ChebConv serves C/Cout <= 64");
  TORCH_CHECK(K_s >= 1 && W.size(0) == K_s * C);
  const int dt = dtype_code(x);
  void* st = stream();
  const void* xp = p.in(x, "x", xt, x.numel());
  auto y = at::empty({B, N, Cout}, x.options());
  at::Tensor bc;
  ChebFwdArgs a;   // the fields every step of the chain shares
  a.g = p.csr(rowptr, colidx, vals, N);
  a.W = p.in(W, "W", xt, K_s * C * Cout);
  a.bias = p.opt_copy(bias, "bias", xt, Cout, bc);
  a.B = B; a.N = N; a.C = C; a.Cout = Cout; a.act = (int)act;

  if (single) {  // localpool: y = act((G @ x) @ W + b); p = G x kept if training
    TORCH_CHECK(K_s == 1);
    at::Tensor p1;
    if (training) a.pout = p.own(p1 = at::empty({B, N, C}, x.options()));
    a.xin = xp; a.yout = p.own(y);
    STM_LAUNCH(stmgcn_cheb_fused_fwd_step, st, dt, a);
    return training ? std::vector<at::Tensor>{y, p1} : std::vector<at::Tensor>{y};
  }
  if (K_s == 1) {  // T_0 only: y = act(x @ W + b)
    a.p1 = xp; a.yout = p.own(y);
    a.alpha = 0.f; a.beta = 1.f;
    STM_LAUNCH(stmgcn_cheb_fused_fwd_step, st, dt, a);
    return {y};
  }
  // K_s - 1 launches: the T_0 mix (x @ W_0) rides the T_1 launch as its
  // x0 operand, so K_s == 2 needs no fp32 accumulator at all.
  at::Tensor yacc;
  if (K_s > 2) {
    yacc = at::empty({B, N, Cout}, x.options().dtype(at::kFloat));
    a.yacc = p.own<float>(yacc);
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
  a.xin = a.x0 = xp;                  // p_{k-1}
  for (int k = 1; k < K_s; ++k) {
    a.p1 = pm2;
    a.pout = (training || k <= 2) ? p.own(ps[k - 1]) : const_cast<void*>(pm2);
    a.kofs = k * C;
    a.yout = k == K_s - 1 ? p.own(y) : nullptr;
    STM_LAUNCH(stmgcn_cheb_fused_fwd_step, st, dt, a);
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
  TORCH_CHECK(dz.dim() == 3 && W.dim() == 2 && K_s >= 1);
  const Ptrs p("cheb_gconv_fused_bwd_dx", dz);
  const int B = dz.size(0), N = dz.size(1), Cout = dz.size(2);
  const int C = W.size(0) / K_s;
  TORCH_CHECK(C <= 64 && Cout <= 64 && (int)(K_s * C) == W.size(0));
  const int dt = dtype_code(dz);
  void* st = stream();
  auto dX = at::empty({B, N, C}, dz.options());
  ChebBwdArgs a;
  a.g = p.csr(rowptr_t, colidx_t, vals_t, N);
  a.dz = p.in(dz, "dz", dz.scalar_type(), dz.numel());
  a.W = p.in(W, "W", dz.scalar_type(), K_s * C * Cout);
  a.B = B; a.N = N; a.C = C; a.Cout = Cout;

  auto bwd = [&](const void* xin, const void* p1, void* out, int kofs,
                 float alpha, float beta) {
    a.xin = xin; a.p1 = p1; a.out = out;
    a.kofs = kofs; a.alpha = alpha; a.beta = beta;
    STM_LAUNCH(stmgcn_cheb_fused_bwd_step, st, dt, a);
  };
  if (single) {  // dX = G^T U_0: materialize U_0, then one plain SpMM
    auto U0 = at::empty({B, N, C}, dz.options());
    bwd(nullptr, nullptr, p.own(U0), 0, 0.f, 0.f);
    ChebFwdArgs s;   // W == null: no mix
    s.g = a.g;
    s.xin = p.own(U0);
    s.pout = p.own(dX);
    s.B = B; s.N = N; s.C = s.Cout = C;
    STM_LAUNCH(stmgcn_cheb_fused_fwd_step, st, dt, s);
    return dX;
  }
  const int K = (int)K_s - 1;
  if (K == 0) {  // dX = U_0
    bwd(nullptr, nullptr, p.own(dX), 0, 0.f, 0.f);
    return dX;
  }
  // Clenshaw: b_K = U_K; b_j = U_j + 2 G^T b_{j+1} - b_{j+2};
  // dX = U_0 + G^T b_1 - b_2 (K == 1: dX = U_0 + G^T U_1, b_2 absent). Two
  // ping/pong buffers (one for K == 1); p1 aliasing is safe.
  auto bufA = at::empty({B, N, C}, dz.options());
  auto bufB = K > 1 ? at::empty({B, N, C}, dz.options()) : at::Tensor();
  void* bj1 = p.own(bufA);      // b_{j+1}
  void* bj2 = nullptr;          // b_{j+2}
  bwd(nullptr, nullptr, bj1, K * C, 0.f, 0.f);  // b_K
  void* other = p.own(bufB);
  for (int j = K - 1; j >= 1; --j) {
    bwd(bj1, bj2, other, j * C, 2.f, bj2 ? -1.f : 0.f);
    bj2 = bj1;
    bj1 = other;
    other = bj2;  // overwritten next iteration (element-wise p1 read is safe)
  }
  bwd(bj1, bj2, p.own(dX), 0, 1.f, bj2 ? -1.f : 0.f);
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
  TORCH_CHECK(x.dim() == 3 && W.dim() == 2);
  const Ptrs p("dual_gconv_fused_fwd", x);
  TORCH_CHECK(is_lowp(x), "fused dual gconv serves bf16/f16");
  const auto xt = x.scalar_type();
  const int B = x.size(0), N = x.size(1), C = x.size(2), Cout = W.size(1);
  TORCH_CHECK(K >= 1 && C <= 64 && Cout <= 64,
              "fused dual gconv serves K >= 1, C/Cout <= 64");
  TORCH_CHECK(W.size(0) == (2 * K + 1) * C);
  const int dt = dtype_code(x);
  void* st = stream();
  const void* xp = p.in(x, "x", xt, x.numel());
  DualFwdArgs a;
  a.gf = p.csr(rpf, cif, vf, N);
  a.gb = p.csr(rpb, cib, vb, N);
  auto y = at::empty({B, N, Cout}, x.options());
  at::Tensor bc;
  a.W = p.in(W, "W", xt, (2 * K + 1) * C * Cout);
  a.bias = p.opt_copy(bias, "bias", xt, Cout, bc);
  a.B = B; a.N = N; a.C = C; a.Cout = Cout; a.act = (int)act;
  at::Tensor yacc;
  if (K > 1) {
    yacc = at::empty({B, N, Cout}, x.options().dtype(at::kFloat));
    a.yacc = p.own<float>(yacc);
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
  a.xf = a.xb = a.x0 = xp;                   // p_{k-1}
  for (int k = 1; k <= K; ++k) {
    a.pf1 = f2; a.pb1 = b2;
    const bool fresh = training || k <= 2;
    a.pfout = fresh ? p.own(pf[k - 1]) : const_cast<void*>(f2);
    a.pbout = fresh ? p.own(pb[k - 1]) : const_cast<void*>(b2);
    a.kofs_f = k * C; a.kofs_b = (int)(K + k) * C;
    a.yout = k == K ? p.own(y) : nullptr;
    STM_LAUNCH(stmgcn_dual_fused_fwd_step, st, dt, a);
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
  TORCH_CHECK(dz.dim() == 3 && W.dim() == 2);
  const Ptrs p("dual_gconv_fused_bwd_dx", dz);
  TORCH_CHECK(is_lowp(dz), "fused dual gconv serves bf16/f16");
  const int B = dz.size(0), N = dz.size(1), Cout = dz.size(2);
  TORCH_CHECK(K >= 1 && W.size(0) % (2 * K + 1) == 0 && W.size(1) == Cout);
  const int C = W.size(0) / (2 * K + 1);
  TORCH_CHECK(C <= 64 && Cout <= 64);
  const int dt = dtype_code(dz);
  void* st = stream();
  DualBwdArgs a;
  a.gft = p.csr(rpf_t, cif_t, vf_t, N);
  a.gbt = p.csr(rpb_t, cib_t, vb_t, N);
  a.dz = p.in(dz, "dz", dz.scalar_type(), dz.numel());
  a.W = p.in(W, "W", dz.scalar_type(), W.numel());
  a.B = B; a.N = N; a.C = C; a.Cout = Cout;
  auto dX = at::empty({B, N, C}, dz.options());

  auto bwd = [&](const void* xf, const void* pf1, const void* xb,
                 const void* pb1, void* outf, void* outb, int j, float alpha,
                 float beta) {
    a.xf = xf; a.pf1 = pf1; a.xb = xb; a.pb1 = pb1;
    a.outf = outf; a.outb = outb; a.final_step = j == 0;
    a.kofs_f = j * C; a.kofs_b = (int)(K + j) * C;
    a.alpha = alpha; a.beta = beta;
    STM_LAUNCH(stmgcn_dual_fused_bwd_step, st, dt, a);
  };
  // b_K = U_K; b_j = U_j + 2 G^T b_{j+1} - b_{j+2}; dX = U_0 + sum over both
  // chains of (G^T b_1 - b_2). Two ping/pong buffers per direction.
  const int nbuf = K > 1 ? 2 : 1;
  std::vector<at::Tensor> bufs;
  for (int i = 0; i < 2 * nbuf; ++i)
    bufs.push_back(at::empty({B, N, C}, dz.options()));
  void *f1 = p.own(bufs[0]), *g1 = p.own(bufs[1]);           // b_{j+1}
  void *f2 = nullptr, *g2 = nullptr;                          // b_{j+2}
  bwd(nullptr, nullptr, nullptr, nullptr, f1, g1, (int)K, 0.f, 0.f);
  void* of = K > 1 ? p.own(bufs[2]) : nullptr;
  void* og = K > 1 ? p.own(bufs[3]) : nullptr;
  for (int j = (int)K - 1; j >= 1; --j) {
    bwd(f1, f2, g1, g2, of, og, j, 2.f, f2 ? -1.f : 0.f);
    f2 = f1; f1 = of; of = f2;   // overwritten next iteration (element-safe)
    g2 = g1; g1 = og; og = g2;
  }
  bwd(f1, f2, g1, g2, p.own(dX), nullptr, 0, 1.f, f2 ? -1.f : 0.f);
  return dX;
}

// Plain axpby-SpMM on (B,N,C): out = alpha*(G @ xin) + beta*p1 — the
// recurrence-replay primitive for the fused wgrad (backward recompute).
at::Tensor spmm_axpby(at::Tensor xin, c10::optional<at::Tensor> p1,
                      at::Tensor rowptr, at::Tensor colidx, at::Tensor vals,
                      double alpha, double beta) {
  TORCH_CHECK(xin.dim() == 3);
  const Ptrs p("spmm_axpby", xin);
  const int B = xin.size(0), N = xin.size(1), C = xin.size(2);
  auto out = at::empty_like(xin);
  ChebFwdArgs a;   // W == null: no mix
  a.g = p.csr(rowptr, colidx, vals, N);
  a.xin = p.in(xin, "xin", xin.scalar_type(), xin.numel());
  a.p1 = p.opt(p1, "p1", xin.scalar_type(), xin.numel());
  a.pout = p.own(out);
  a.B = B; a.N = N; a.C = a.Cout = C;
  a.alpha = (float)alpha; a.beta = (float)beta;
  STM_LAUNCH(stmgcn_cheb_fused_fwd_step, stream(), dtype_code(xin), a);
  return out;
}

// ---------------------------------------------------------------------------
// Fused LSTM: forward kernel + dgrad kernel + one batched
// wgrad kernel over the dA stream. lstm_bwd returns dA with logical shape
// (L, Tst, S_pad, 4H) but each 32-row sequence tile stored in the wgrad MFMA
// fragment order documented in csrc/common.h; lstm_wgrad expects that order.

static constexpr int kH = RNN_H;

// x (S, Tst, cin) of a fused-RNN binding: the shapes the kernels serve
static void rnn_check_x(const at::Tensor& x, int64_t L) {
  TORCH_CHECK(x.dim() == 3 && is_lowp(x),
              "fused LSTM serves bf16/f16 (fp32 runs the torch path)");
  TORCH_CHECK(x.size(0) >= 1 && L >= 1 && L <= MAX_LAYERS && x.size(1) >= 1 &&
              x.size(1) <= 16, "fused LSTM serves 1..8 layers, T <= 16");
  TORCH_CHECK(x.size(2) == 1 || x.size(2) == kH, "C_in must be 1 or 64");
}

std::vector<at::Tensor> lstm_fwd(at::Tensor x, std::vector<at::Tensor> w_ih,
                                 std::vector<at::Tensor> w_hh,
                                 std::vector<at::Tensor> b_ih,
                                 std::vector<at::Tensor> b_hh, bool ret_seq,
                                 bool training, bool gru) {
  const Ptrs p("lstm_fwd", x);
  const int L = (int)w_ih.size();
  rnn_check_x(x, L);
  TORCH_CHECK((int)w_hh.size() == L && (int)b_ih.size() == L && (int)b_hh.size() == L,
              "lstm_fwd: w_ih, w_hh, b_ih, b_hh must list the same layers");
  const auto xt = x.scalar_type();
  LstmFwdArgs a;
  a.S = x.size(0); a.Tst = x.size(1); a.cin = x.size(2); a.L = L;
  a.ret_seq = ret_seq ? 1 : 0; a.gru = gru ? 1 : 0;
  a.x = p.in(x, "x", xt, x.numel());
  for (int l = 0; l < L; ++l) {
    a.w.w_ih[l] = p.in(w_ih[l], "w_ih", xt, 4L * kH * (l == 0 ? a.cin : kH));
    a.w.w_hh[l] = p.in(w_hh[l], "w_hh", xt, 4L * kH * kH);
    a.w.b_ih[l] = p.in(b_ih[l], "b_ih", xt, 4 * kH);
    a.w.b_hh[l] = p.in(b_hh[l], "b_hh", xt, 4 * kH);
  }
  const long S_pad = rnn_s_pad(a.S);
  auto out = ret_seq ? at::empty({a.S, a.Tst, kH}, x.options())
                     : at::empty({a.S, kH}, x.options());
  // hseq is the cross-layer hand-off in GLOBAL memory (LDS holds only the
  // live ping/pong slots) — allocated in eval too; cseq/gates only train.
  at::Tensor hseq = at::empty({L, a.Tst, S_pad, kH}, x.options()), cseq, gates;
  if (training) {
    cseq = at::empty({L, a.Tst, S_pad * kH}, x.options());
    gates = at::empty({L, a.Tst, S_pad * 4 * kH}, x.options());
  }
  a.out = p.own(out); a.hseq = p.own(hseq);
  a.cseq = p.own(cseq); a.gates = p.own(gates);
  STM_LAUNCH(stmgcn_lstm_fwd, stream(), dtype_code(x), a);
  if (!training) return {out};
  return {out, hseq, cseq, gates};
}

std::vector<at::Tensor> lstm_bwd(at::Tensor dout, at::Tensor x,
                                 at::Tensor cseq, at::Tensor gates,
                                 std::vector<at::Tensor> w_ihT,
                                 std::vector<at::Tensor> w_hhT, bool ret_seq,
                                 bool gru) {
  const Ptrs p("lstm_bwd", x);
  const int L = (int)w_ihT.size();
  rnn_check_x(x, L);
  TORCH_CHECK((int)w_hhT.size() == L, "lstm_bwd: w_ihT and w_hhT must list the same layers");
  const auto xt = x.scalar_type();
  LstmBwdArgs a;
  a.S = x.size(0); a.Tst = x.size(1); a.cin = x.size(2); a.L = L;
  a.ret_seq = ret_seq ? 1 : 0; a.gru = gru ? 1 : 0;
  const long S_pad = rnn_s_pad(a.S), LT = (long)L * a.Tst;
  a.x = p.in(x, "x", xt, x.numel());
  a.dout = p.copy(dout, "dout", xt, (long)a.S * (ret_seq ? a.Tst : 1) * kH, dout);
  a.cseq = p.in(cseq, "cseq", xt, LT * S_pad * kH);
  a.gates = p.in(gates, "gates", xt, LT * S_pad * 4 * kH);
  for (int l = 0; l < L; ++l) {
    a.w.w_ih[l] = p.in(w_ihT[l], "w_ihT", xt, (l == 0 ? a.cin : kH) * 4L * kH);
    a.w.w_hh[l] = p.in(w_hhT[l], "w_hhT", xt, kH * 4L * kH);
  }
  auto dx = at::empty_like(x);
  auto dA = at::empty({L, a.Tst, S_pad, 4 * kH}, x.options());
  // cross-layer dh hand-off scratch (global; LDS only holds dA tiles)
  at::Tensor dh;
  if (L > 1) dh = at::empty({(long)a.Tst * S_pad * kH}, x.options());
  a.dx = p.own(dx); a.dA = p.own(dA); a.dh = p.own(dh);
  STM_LAUNCH(stmgcn_lstm_bwd, stream(), dtype_code(x), a);
  return {dx, dA};
}

// dA (L, Tst, S_pad, 4H) tiled, hseq (L, Tst, S_pad, H), x (S, Tst, cin): the
// inputs of both lstm_wgrad forms, checked and entered into `a`
static void lstm_wgrad_inputs(const Ptrs& p, const at::Tensor& dA, const at::Tensor& hseq,
                              const at::Tensor& x, LstmWgradArgs& a) {
  TORCH_CHECK(dA.dim() == 4 && x.dim() == 3 && is_lowp(dA), "lstm_wgrad serves bf16/f16");
  a.L = dA.size(0); a.Tst = dA.size(1); a.S_pad = dA.size(2);
  a.R = (long)a.Tst * a.S_pad;
  a.S = x.size(0); a.cin = x.size(2);
  TORCH_CHECK(a.L >= 1 && a.L <= MAX_LAYERS && (a.cin == 1 || a.cin == kH));
  TORCH_CHECK(dA.size(3) == 4 * kH && a.S_pad % SEQ_TILE == 0 && a.S <= a.S_pad,
              "dA must be (L, Tst, S_pad, 4H) with S_pad a multiple of 32");
  TORCH_CHECK(x.size(1) == a.Tst, "x must be (S, Tst, cin)");
  const auto dt = dA.scalar_type();
  a.dA = p.in(dA, "dA", dt, dA.numel());
  a.hseq = p.in(hseq, "hseq", dt, (long)a.L * a.R * kH);
  a.x = p.in(x, "x", dt, (long)a.S * a.Tst * a.cin);
}

// All-layer LSTM weight grads in ONE launch over the TILED dA stream (wgrad.hip):
// returns fp32 (dwih (L,4H,64), dwhh (L,4H,H), db (L,4H)); layer 0's live
// dwih columns are [:, :cin].
std::vector<at::Tensor> lstm_wgrad(at::Tensor dA, at::Tensor hseq, at::Tensor x) {
  const Ptrs p("lstm_wgrad", dA);
  LstmWgradArgs a;
  lstm_wgrad_inputs(p, dA, hseq, x, a);
  const int L = a.L;
  // one fill for all three atomic-accumulated outputs
  const LstmWgradWs ws = lstm_wgrad_ws(L, false);
  auto flat = at::zeros({ws.words}, dA.options().dtype(at::kFloat));
  a.ws = p.own<float>(flat);
  STM_LAUNCH(stmgcn_lstm_wgrad, stream(), dtype_code(dA), a);
  return {flat.narrow(0, ws.dwih, ws.dwhh - ws.dwih).view({L, 4 * kH, kH}),
          flat.narrow(0, ws.dwhh, ws.db - ws.dwhh).view({L, 4 * kH, kH}),
          flat.narrow(0, ws.db, ws.words - ws.db).view({L, 4 * kH})};
}

// Finishing form of lstm_wgrad: the same launch, and its last workgroup per
// layer writes the gradients in the activations' dtype and in their final
// shapes. Returns [dw_ih_0, dw_hh_0, db_ih_0, db_hh_0, dw_ih_1, ...]: contiguous
// views of ONE flat buffer. One zero fill covers sums and tickets.
std::vector<at::Tensor> lstm_wgrad_grads(at::Tensor dA, at::Tensor hseq,
                                         at::Tensor x, bool gru) {
  const Ptrs p("lstm_wgrad_grads", dA);
  LstmWgradArgs a;
  lstm_wgrad_inputs(p, dA, hseq, x, a);
  a.gru = gru ? 1 : 0;
  auto ws = at::zeros({lstm_wgrad_ws(a.L, true).words}, dA.options().dtype(at::kFloat));
  const int GH = (gru ? 3 : 4) * kH;
  auto flat = at::empty({lstm_grads_layer_off(a.L, GH, a.cin)}, dA.options());
  a.ws = p.own<float>(ws);
  a.out = p.own(flat);
  STM_LAUNCH(stmgcn_lstm_wgrad, stream(), dtype_code(dA), a);
  std::vector<at::Tensor> out;
  for (int l = 0; l < a.L; ++l) {
    const LstmGradsLayer o = lstm_grads_layer(l, GH, a.cin);
    const long cl = l == 0 ? a.cin : kH;
    out.push_back(flat.narrow(0, o.dw_ih, GH * cl).view({GH, cl}));
    out.push_back(flat.narrow(0, o.dw_hh, (long)GH * kH).view({GH, kH}));
    out.push_back(flat.narrow(0, o.db_ih, GH));
    out.push_back(flat.narrow(0, o.db_hh, GH));
  }
  return out;
}

// W_ih^T / W_hh^T of every layer (the operands lstm_bwd reads) in ONE launch
// into one buffer: returns [w_ihT_0.., w_hhT_0..] as views of it.
std::vector<at::Tensor> lstm_pack_bwd_weights(std::vector<at::Tensor> w_ih,
                                              std::vector<at::Tensor> w_hh) {
  const int L = (int)w_ih.size();
  TORCH_CHECK(L >= 1 && L <= MAX_LAYERS && (int)w_hh.size() == L);
  const Ptrs p("lstm_pack_bwd_weights", w_ih[0]);
  const auto dt = w_ih[0].scalar_type();
  TORCH_CHECK(is_lowp(w_ih[0]) && w_ih[0].dim() == 2);
  const int cin = w_ih[0].size(1);
  TORCH_CHECK(cin == 1 || cin == kH);
  const void *wi[MAX_LAYERS], *wh[MAX_LAYERS];
  for (int l = 0; l < L; ++l) {
    wi[l] = p.in(w_ih[l], "w_ih", dt, 4L * kH * lstm_packT_cols(l, cin));
    wh[l] = p.in(w_hh[l], "w_hh", dt, 4L * kH * kH);
  }
  auto flat = at::empty({lstm_packT_off(2 * L, cin)}, w_ih[0].options());
  STM_LAUNCH(stmgcn_lstm_pack_bwd_weights, stream(), wi, wh, L, cin, p.own(flat));
  std::vector<at::Tensor> out;
  for (int i = 0; i < 2 * L; ++i) {
    const long cols = i < L ? lstm_packT_cols(i, cin) : kH;
    out.push_back(flat.narrow(0, lstm_packT_off(i, cin), 4 * kH * cols).view({cols, 4 * kH}));
  }
  return out;
}

// (rows, CA) sources and B (rows, N) of an atb_wgrad binding, checked; the
// kernel reads 16-byte fragments at column offsets cb*8, so CA and N are
// multiples of 8 (a ragged tail row would read past the end of A / B)
static void atb_inputs(const Ptrs& p, const std::vector<at::Tensor>& As, size_t first,
                       size_t count, const at::Tensor& B, AtbWgradArgs& a) {
  TORCH_CHECK(B.dim() == 2 && count >= 1 && count <= ATB_MAX_SRC &&
              first + count <= As.size());
  a.rows = B.size(0); a.N = B.size(1);
  a.nsrc = (int)count;
  a.CA = As[first].dim() == 2 ? As[first].size(1) : 0;
  TORCH_CHECK(a.CA >= 8 && a.CA % 8 == 0 && a.nsrc * a.CA <= 256 && a.N >= 8 &&
              a.N <= 64 && a.N % 8 == 0,
              "atb_wgrad serves M <= 256, N <= 64, both multiples of 8");
  a.B = p.in(B, "B", B.scalar_type(), a.rows * a.N);
  for (size_t i = 0; i < count; ++i) {
    const at::Tensor& A = As[first + i];
    TORCH_CHECK(A.dim() == 2 && A.size(1) == a.CA, "atb_wgrad: sources must be (rows, CA)");
    a.As[i] = p.in(A, "A", B.scalar_type(), a.rows * a.CA);
  }
}

// C = A^T @ B (+ db = colsum(B)) for tall-skinny wgrads (M<=256, N<=64).
std::vector<at::Tensor> atb_wgrad(at::Tensor A, at::Tensor B, bool want_db) {
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(0) == B.size(0));
  const Ptrs p("atb_wgrad", A);
  A = A.contiguous(); B = B.contiguous();
  AtbWgradArgs a;
  atb_inputs(p, {A}, 0, 1, B, a);
  auto fopt = A.options().dtype(at::kFloat);
  auto C = at::zeros({a.CA, a.N}, fopt);
  auto db = want_db ? at::zeros({a.N}, fopt) : at::Tensor();
  a.C = p.own<float>(C); a.db = p.own<float>(db);
  STM_LAUNCH(stmgcn_atb_wgrad, stream(), dtype_code(A), a);
  return want_db ? std::vector<at::Tensor>{C, db} : std::vector<at::Tensor>{C};
}

// Multi-source reduction GEMM: C[k*CA:(k+1)*CA, :] += As[k]^T @ B for up to
// 4 sources in ONE launch (B/dZ streamed once) + db += colsum(B). The fused
// ChebConv wgrad feeds the recurrence states [x, p_1, ..] here.
void atb_wgrad_multi(std::vector<at::Tensor> As, at::Tensor B, at::Tensor C,
                     c10::optional<at::Tensor> db) {
  const Ptrs p("atb_wgrad_multi", B);
  AtbWgradArgs a;
  atb_inputs(p, As, 0, As.size(), B, a);
  a.C = p.in<float>(C, "C", at::kFloat, (long)a.nsrc * a.CA * a.N);
  a.db = p.opt<float>(db, "db", at::kFloat, a.N);
  STM_LAUNCH(stmgcn_atb_wgrad, stream(), dtype_code(B), a);
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
  const Ptrs p("atb_wgrad_multi_grads", B);
  AtbWgradArgs a, b;
  atb_inputs(p, As, 0, split, B, a);
  if (split < nsrc) {
    atb_inputs(p, As, split, nsrc - split, B, b);
    TORCH_CHECK(b.CA == a.CA, "atb_wgrad_multi_grads: sources differ in width");
  }
  TORCH_CHECK(4 * a.CA <= 256);
  auto ws = at::zeros({atb_ws(nsrc, a.CA, a.N).words}, B.options().dtype(at::kFloat));
  auto dW = at::empty({(long)nsrc * a.CA, (long)a.N}, B.options());
  at::Tensor db;
  if (want_db) db = at::empty({a.N}, B.options());
  const int dt = dtype_code(B);
  a.ws = b.ws = p.own<float>(ws);
  a.dW = b.dW = p.own(dW);
  a.nsrc_all = b.nsrc_all = nsrc;
  a.dbo = p.own(db);
  STM_LAUNCH(stmgcn_atb_wgrad, stream(), dt, a);
  if (split < nsrc) {
    b.src0 = (int)split;
    STM_LAUNCH(stmgcn_atb_wgrad, stream(), dt, b);
  }
  return want_db ? std::vector<at::Tensor>{dW, db} : std::vector<at::Tensor>{dW};
}

// dz = dy * (y > 0) in one launch (the ReLU mask of the gconv backward)
at::Tensor relu_bwd(at::Tensor dy, at::Tensor y) {
  const Ptrs p("relu_bwd", dy);
  TORCH_CHECK(dy.sizes() == y.sizes() && is_lowp(dy), "relu_bwd serves bf16/f16");
  const auto dt = dy.scalar_type();
  const long n = dy.numel();
  const void* dyp = p.copy(dy, "dy", dt, n, dy);
  const void* yp = p.copy(y, "y", dt, n, y);
  auto dz = at::empty_like(dy);
  STM_LAUNCH(stmgcn_relu_bwd, stream(), dtype_code(dy), dyp, yp, p.own(dz), n);
  return dz;
}

at::Tensor mfma_probe(at::Tensor A, at::Tensor B) {
  const Ptrs p("mfma_probe", A);
  const void* Ap = p.copy(A, "A", at::kBFloat16, 16 * 32, A);
  const void* Bp = p.copy(B, "B", at::kBFloat16, 32 * 16, B);
  auto D = at::empty({16, 16}, A.options().dtype(at::kFloat));
  STM_LAUNCH(stmgcn_mfma_probe, stream(), Ap, Bp, p.own(D));
  return D;
}

// ---------------------------------------------------------------------------
// pointwise.hip ops: K3 seqsum/permute, K4 gate, K7 head, K8 loss, K9 Adam

at::Tensor seqsum_permute(at::Tensor obs) {
  TORCH_CHECK(obs.dim() == 4);
  const Ptrs p("seqsum_permute", obs);
  const int B = obs.size(0), Tst = obs.size(1), N = obs.size(2), C = obs.size(3);
  const void* op = p.in(obs, "obs", obs.scalar_type(), obs.numel());
  auto out = at::empty({B, N, Tst}, obs.options());
  STM_LAUNCH(stmgcn_seqsum_permute, stream(), dtype_code(obs), op, p.own(out), B, Tst,
             N, C);
  return out;
}

at::Tensor seqsum_permute_bwd(at::Tensor dxs, int64_t C) {
  TORCH_CHECK(dxs.dim() == 3 && C >= 1);
  const Ptrs p("seqsum_permute_bwd", dxs);
  const int B = dxs.size(0), N = dxs.size(1), Tst = dxs.size(2);
  const void* dp = p.copy(dxs, "dxs", dxs.scalar_type(), dxs.numel(), dxs);
  auto dobs = at::empty({B, Tst, N, C}, dxs.options());
  STM_LAUNCH(stmgcn_seqsum_permute_bwd, stream(), dtype_code(dxs), dp, p.own(dobs), B,
             Tst, N, (int)C);
  return dobs;
}

// node_major: out is (B,N,T,C) — the sequence-major layout the RNN consumes —
// instead of (B,T,N,C). z is the pooled mean (fp32) either way.
std::vector<at::Tensor> gate_fwd(at::Tensor obs, at::Tensor g, at::Tensor xs,
                                 at::Tensor fcw, at::Tensor fcb, bool node_major) {
  TORCH_CHECK(obs.dim() == 4);
  const Ptrs p("gate_fwd", obs);
  const auto dt = obs.scalar_type();
  GateFwdArgs a;
  a.B = obs.size(0); a.Tst = obs.size(1); a.N = obs.size(2); a.C = obs.size(3);
  a.node_major = node_major ? 1 : 0;
  TORCH_CHECK(a.Tst <= 16, "gate kernel serves T <= 16");
  const long BNT = (long)a.B * a.N * a.Tst;
  a.obs = p.in(obs, "obs", dt, obs.numel());
  a.g = p.copy(g, "g", dt, BNT, g);
  a.xs = p.copy(xs, "xs", dt, BNT, xs);
  a.fcw = p.copy(fcw, "fcw", dt, a.Tst * a.Tst, fcw);
  a.fcb = p.copy(fcb, "fcb", dt, a.Tst, fcb);
  auto fopt = obs.options().dtype(at::kFloat);
  // z doubles as the multi-block zsum atomic target, followed by one arrival
  // ticket per batch row -> one zero fill for both
  const GateWs ws = gate_ws(a.B, a.Tst, false);
  auto zt = at::zeros({ws.words}, fopt);
  auto z = zt.narrow(0, ws.z, ws.tickets - ws.z).view({a.B, a.Tst});
  auto u = at::empty({a.B, a.Tst}, fopt), s = at::empty({a.B, a.Tst}, fopt);
  auto out = node_major ? at::empty({a.B, a.N, a.Tst, a.C}, obs.options())
                        : at::empty_like(obs);
  a.ws = p.own<float>(zt); a.u = p.own<float>(u); a.s = p.own<float>(s);
  a.out = p.own(out);
  STM_LAUNCH(stmgcn_gate_fwd, stream(), dtype_code(obs), a);
  return {out, z, u, s};
}

// Returns {dobs (undefined without want_dobs), dg, dw (T,T), db (T,), dw fp32,
// db fp32}: dw/db are summed over the batch in-kernel, in the dtype of obs and
// in fp32. node_major: dout is (B,N,T,C).
std::vector<at::Tensor> gate_bwd(at::Tensor dout, at::Tensor obs, at::Tensor fcw,
                                 at::Tensor z, at::Tensor u, at::Tensor s,
                                 bool node_major, bool want_dobs) {
  TORCH_CHECK(obs.dim() == 4);
  const Ptrs p("gate_bwd", obs);
  const auto dt = obs.scalar_type();
  GateBwdArgs a;
  a.B = obs.size(0); a.Tst = obs.size(1); a.N = obs.size(2); a.C = obs.size(3);
  a.node_major = node_major ? 1 : 0;
  TORCH_CHECK(a.Tst <= 16, "gate kernel serves T <= 16");
  const long BT = (long)a.B * a.Tst;
  a.obs = p.in(obs, "obs", dt, obs.numel());
  a.dout = p.copy(dout, "dout", dt, obs.numel(), dout);
  a.fcw = p.copy(fcw, "fcw", dt, a.Tst * a.Tst, fcw);
  a.z = p.in<float>(z, "z", at::kFloat, BT);
  a.u = p.in<float>(u, "u", at::kFloat, BT);
  a.s = p.in<float>(s, "s", at::kFloat, BT);
  auto fopt = obs.options().dtype(at::kFloat);
  // dz doubles as the multi-block ds atomic target, followed by the B + 1
  // arrival tickets -> one zero fill for both
  auto dzt = at::zeros({gate_ws(a.B, a.Tst, true).words}, fopt);
  auto dw_part = at::empty({a.B, a.Tst, a.Tst}, fopt);
  auto db_part = at::empty({a.B, a.Tst}, fopt);
  auto dw_f = at::empty({a.Tst, a.Tst}, fopt), db_f = at::empty({a.Tst}, fopt);
  auto dw = at::empty({a.Tst, a.Tst}, obs.options()), db = at::empty({a.Tst}, obs.options());
  at::Tensor dobs;
  if (want_dobs) dobs = at::empty_like(obs);
  auto dg = at::empty({a.B, a.N, a.Tst}, obs.options());
  a.ws = p.own<float>(dzt);
  a.dw_part = p.own<float>(dw_part); a.db_part = p.own<float>(db_part);
  a.dw_f = p.own<float>(dw_f); a.db_f = p.own<float>(db_f);
  a.dw = p.own(dw); a.db = p.own(db); a.dobs = p.own(dobs); a.dg = p.own(dg);
  STM_LAUNCH(stmgcn_gate_bwd, stream(), dtype_code(obs), a);
  return {dobs, dg, dw, db, dw_f, db_f};
}

// The 1..3 branch feature maps (B, N, G) of a head forward: contiguous copies
// in fc (their owner), pointers in f (null past the last)
static void head_feats(const Ptrs& p, const std::vector<at::Tensor>& feats,
                       std::vector<at::Tensor>& fc, const void* f[3]) {
  const at::Tensor& f0 = feats[0];
  fc.resize(feats.size());
  for (size_t m = 0; m < 3; ++m) {
    f[m] = nullptr;
    if (m >= feats.size()) continue;
    TORCH_CHECK(feats[m].defined() && feats[m].sizes() == f0.sizes(),
                "head: the feature maps differ in shape");
    f[m] = p.copy(feats[m], "feats", f0.scalar_type(), f0.numel(), fc[m]);
  }
}

std::vector<at::Tensor> head_fwd(std::vector<at::Tensor> feats, at::Tensor w,
                                 at::Tensor bias) {
  TORCH_CHECK(feats.size() >= 1 && feats.size() <= 3 && feats[0].dim() == 3);
  const Ptrs p("head_fwd", feats[0]);
  const at::Tensor& f0 = feats[0];
  const long BN = (long)f0.size(0) * f0.size(1);
  const int G = f0.size(2);
  TORCH_CHECK(G <= 64, "head kernel serves G <= 64");
  std::vector<at::Tensor> fc;
  const void* f[3];
  head_feats(p, feats, fc, f);
  const void* wp = p.copy(w, "w", f0.scalar_type(), G, w);
  const void* bp = p.copy(bias, "bias", f0.scalar_type(), 1, bias);
  auto y = at::empty({f0.size(0), f0.size(1), 1}, f0.options());
  auto fsum = at::empty_like(fc[0]);
  STM_LAUNCH(stmgcn_head_fwd, stream(), dtype_code(f0), f[0], f[1], f[2], wp, bp,
             p.own(y), p.own(fsum), G, BN);
  return {y, fsum};
}

at::Tensor head_bwd(at::Tensor dy, at::Tensor w, int64_t G) {
  TORCH_CHECK(dy.dim() >= 2 && G >= 1);
  const Ptrs p("head_bwd", dy);
  const long BN = (long)dy.size(0) * dy.size(1);
  const void* dyp = p.copy(dy, "dy", dy.scalar_type(), BN, dy);
  const void* wp = p.copy(w, "w", dy.scalar_type(), G, w);
  auto dfeat = at::empty({dy.size(0), dy.size(1), G}, dy.options());
  STM_LAUNCH(stmgcn_head_bwd, stream(), dtype_code(dy), dyp, wp, p.own(dfeat), (int)G, BN);
  return dfeat;
}

// dy (B, N, O) and fsum (B, N, G) of a head wgrad binding, checked (contiguous
// copies left in dy / fsum) and entered into `a`
static void head_wgrad_inputs(const Ptrs& p, at::Tensor& dy, at::Tensor& fsum, int O,
                              HeadWgradArgs& a) {
  TORCH_CHECK(fsum.dim() == 3);
  a.BN = (long)fsum.size(0) * fsum.size(1);
  a.G = fsum.size(2); a.O = O;
  a.fsum = p.copy(fsum, "fsum", fsum.scalar_type(), fsum.numel(), fsum);
  a.dy = p.copy(dy, "dy", fsum.scalar_type(), a.BN * O, dy);
}

// dw[g] = sum_r dy[r] fsum[r,g]; db = sum dy — fp32 accumulated reduction.
std::vector<at::Tensor> head_wgrad(at::Tensor dy, at::Tensor fsum) {
  const Ptrs p("head_wgrad", fsum);
  HeadWgradArgs a;
  head_wgrad_inputs(p, dy, fsum, 1, a);
  TORCH_CHECK(a.G <= 64, "head kernel serves G <= 64");
  const HeadWgradWs ws = head_wgrad_ws(a.G, 1);
  auto sums = at::zeros({ws.words}, dy.options().dtype(at::kFloat));
  a.ws = p.own<float>(sums);
  STM_LAUNCH(stmgcn_head_wgrad, stream(), dtype_code(dy), a);
  return {sums.narrow(0, ws.dw, a.G), sums.narrow(0, ws.db, 1)};
}

// Finishing form: dw (1, G) and db (1,) in the dtype of dy from one zero-filled
// fp32 workspace (sums + ticket); the kernel's last workgroup rounds them.
std::vector<at::Tensor> head_wgrad_grads(at::Tensor dy, at::Tensor fsum) {
  const Ptrs p("head_wgrad_grads", fsum);
  HeadWgradArgs a;
  head_wgrad_inputs(p, dy, fsum, 1, a);
  TORCH_CHECK(a.G <= 64, "head kernel serves G <= 64");
  auto ws = at::zeros({head_wgrad_ws(a.G, 1).words}, dy.options().dtype(at::kFloat));
  auto dw = at::empty({1, a.G}, dy.options());
  auto db = at::empty({1}, dy.options());
  a.ws = p.own<float>(ws); a.dw_out = p.own(dw); a.db_out = p.own(db);
  STM_LAUNCH(stmgcn_head_wgrad, stream(), dtype_code(dy), a);
  return {dw, db};
}

std::vector<at::Tensor> mse_fwd(at::Tensor pred, at::Tensor tgt) {
  const Ptrs p("mse_fwd", pred);
  const auto dt = pred.scalar_type();
  const long n = pred.numel();
  const void* pp = p.copy(pred, "pred", dt, n, pred);
  const void* tp = p.copy(tgt, "tgt", dt, n, tgt);
  auto loss = at::zeros({}, pred.options().dtype(at::kFloat));
  auto diff = at::empty_like(pred);
  STM_LAUNCH(stmgcn_mse_fwd, stream(), dtype_code(pred), pp, tp, p.own<float>(loss),
             p.own(diff), n);
  return {loss, diff};
}

at::Tensor mse_bwd(at::Tensor diff, at::Tensor gscale) {
  const Ptrs p("mse_bwd", diff);
  const long n = diff.numel();
  const void* dp = p.in(diff, "diff", diff.scalar_type(), n);
  const float* gp = p.copy<float>(gscale, "gscale", at::kFloat, 1, gscale);
  auto dpred = at::empty_like(diff);
  STM_LAUNCH(stmgcn_mse_bwd, stream(), dtype_code(diff), dp, gp, p.own(dpred), n);
  return dpred;
}

// ---- wide head (multi-step horizon): O = fc_weight.size(0), 2 <= O <= 32 ----
static void head_multi_check(const at::Tensor& a, int64_t G, int64_t O) {
  TORCH_CHECK(is_lowp(a), "wide head serves bf16/f16");
  TORCH_CHECK(O >= 2 && O <= 32 && G >= 8 && G <= 64 && G % 8 == 0,
              "wide head serves 2 <= O <= 32, G <= 64 with G % 8 == 0");
}

// {y (B, N, O), fsum (B, N, G)}
std::vector<at::Tensor> head_multi_fwd(std::vector<at::Tensor> feats,
                                       at::Tensor w, at::Tensor bias) {
  TORCH_CHECK(feats.size() >= 1 && feats.size() <= 3 && w.dim() == 2 &&
              feats[0].dim() == 3);
  const Ptrs p("head_multi_fwd", feats[0]);
  const at::Tensor& f0 = feats[0];
  const long BN = (long)f0.size(0) * f0.size(1);
  const int G = f0.size(2), O = w.size(0);
  head_multi_check(f0, G, O);
  TORCH_CHECK(w.size(1) == G);
  std::vector<at::Tensor> fc;
  const void* f[3];
  head_feats(p, feats, fc, f);
  const void* wp = p.copy(w, "w", f0.scalar_type(), (long)O * G, w);
  const void* bp = p.copy(bias, "bias", f0.scalar_type(), O, bias);
  auto y = at::empty({f0.size(0), f0.size(1), O}, f0.options());
  auto fsum = at::empty_like(fc[0]);
  STM_LAUNCH(stmgcn_head_multi_fwd, stream(), dtype_code(f0), f[0], f[1], f[2], wp, bp,
             p.own(y), p.own(fsum), G, O, BN);
  return {y, fsum};
}

at::Tensor head_multi_bwd(at::Tensor dy, at::Tensor w) {
  TORCH_CHECK(dy.dim() == 3 && w.dim() == 2);
  const Ptrs p("head_multi_bwd", dy);
  const long BN = (long)dy.size(0) * dy.size(1);
  const int O = w.size(0), G = w.size(1);
  head_multi_check(dy, G, O);
  const void* dyp = p.copy(dy, "dy", dy.scalar_type(), BN * O, dy);
  const void* wp = p.copy(w, "w", dy.scalar_type(), (long)O * G, w);
  auto dfeat = at::empty({dy.size(0), dy.size(1), G}, dy.options());
  STM_LAUNCH(stmgcn_head_multi_bwd, stream(), dtype_code(dy), dyp, wp, p.own(dfeat), G,
             O, BN);
  return dfeat;
}

static void head_multi_wgrad_inputs(const Ptrs& p, at::Tensor& dy, at::Tensor& fsum,
                                    HeadWgradArgs& a) {
  TORCH_CHECK(dy.dim() == 3 && fsum.dim() == 3 && dy.size(0) == fsum.size(0) &&
              dy.size(1) == fsum.size(1));
  head_multi_check(fsum, fsum.size(2), dy.size(2));
  head_wgrad_inputs(p, dy, fsum, dy.size(2), a);
}

// dW (O, G) = dy^T fsum and db (O,) = colsum(dy) as fp32 sums
std::vector<at::Tensor> head_multi_wgrad(at::Tensor dy, at::Tensor fsum) {
  const Ptrs p("head_multi_wgrad", fsum);
  HeadWgradArgs a;
  head_multi_wgrad_inputs(p, dy, fsum, a);
  const HeadWgradWs ws = head_wgrad_ws(a.G, a.O);
  auto sums = at::zeros({ws.words}, dy.options().dtype(at::kFloat));
  a.ws = p.own<float>(sums);
  STM_LAUNCH(stmgcn_head_multi_wgrad, stream(), dtype_code(dy), a);
  return {sums.narrow(0, ws.dw, (long)a.O * a.G).view({a.O, a.G}),
          sums.narrow(0, ws.db, a.O)};
}

// Finishing form: dW (O, G) and db (O,) in the dtype of dy from one zero-filled
// fp32 workspace (O*G sums, 32 db slots, ticket); the last workgroup rounds.
std::vector<at::Tensor> head_multi_wgrad_grads(at::Tensor dy, at::Tensor fsum) {
  const Ptrs p("head_multi_wgrad_grads", fsum);
  HeadWgradArgs a;
  head_multi_wgrad_inputs(p, dy, fsum, a);
  auto ws = at::zeros({head_wgrad_ws(a.G, a.O).words}, dy.options().dtype(at::kFloat));
  auto dw = at::empty({a.O, a.G}, dy.options());
  auto db = at::empty({a.O}, dy.options());
  a.ws = p.own<float>(ws); a.dw_out = p.own(dw); a.db_out = p.own(db);
  STM_LAUNCH(stmgcn_head_multi_wgrad, stream(), dtype_code(dy), a);
  return {dw, db};
}

// ---- masked loss: {res (2,) fp32 = loss, 1 / max(count_valid, 1); diff} ----
std::vector<at::Tensor> masked_loss_fwd(at::Tensor pred, at::Tensor tgt,
                                        int64_t kind) {
  const Ptrs p("masked_loss_fwd", pred);
  TORCH_CHECK(pred.sizes() == tgt.sizes());
  TORCH_CHECK(kind >= 0 && kind <= 2, "masked loss kind: 0 mse, 1 mae, 2 huber");
  // count_valid is a 32-bit integer sum
  const long n = pred.numel();
  TORCH_CHECK(n > 0 && n < (1LL << 32));
  const void* pp = p.copy(pred, "pred", pred.scalar_type(), n, pred);
  const void* tp = p.copy(tgt, "tgt", pred.scalar_type(), n, tgt);
  auto fopt = pred.options().dtype(at::kFloat);
  auto ws = at::zeros({MLOSS_WS_WORDS}, fopt);     // sum, count, ticket: one fill
  auto res = at::empty({2}, fopt);
  auto diff = at::empty_like(pred);
  STM_LAUNCH(stmgcn_masked_loss_fwd, stream(), dtype_code(pred), (int)kind, pp, tp,
             p.own<float>(ws), p.own<float>(res), p.own(diff), n);
  return {res, diff};
}

at::Tensor masked_loss_bwd(at::Tensor diff, at::Tensor res, at::Tensor gscale,
                           int64_t kind) {
  const Ptrs p("masked_loss_bwd", diff);
  const long n = diff.numel();
  TORCH_CHECK(kind >= 0 && kind <= 2 && n > 0);
  const void* dp = p.in(diff, "diff", diff.scalar_type(), n);
  const float* rp = p.in<float>(res, "res", at::kFloat, 2);
  const float* gp = p.in<float>(gscale, "gscale", at::kFloat, 1);
  auto dpred = at::empty_like(diff);
  STM_LAUNCH(stmgcn_masked_loss_bwd, stream(), dtype_code(diff), (int)kind, dp, rp, gp,
             p.own(dpred), n);
  return dpred;
}

// Pack per-param grads (or zeros for undefined) into the flat grad arena.
// grads: list aligned with the arena layout; offsets/lens in elements.
void gather_grads(std::vector<at::Tensor> grads, std::vector<int64_t> ofs,
                  std::vector<int64_t> lens, at::Tensor arena) {
  const Ptrs p("gather_grads", arena);
  const size_t n = ofs.size();
  TORCH_CHECK(grads.size() == n && lens.size() == n,
              "gather_grads: grads, ofs and lens differ in length");
  void* ap = p.in(arena, "arena", arena.scalar_type(), arena.numel());
  std::vector<const void*> srcs(n);
  std::vector<long> o(n);
  std::vector<int> l(n);
  for (size_t i = 0; i < n; ++i) {   // every segment is checked before any launch
    TORCH_CHECK(ofs[i] >= 0 && lens[i] >= 0 && lens[i] < (1LL << 31) &&
                ofs[i] + lens[i] <= arena.numel(),
                "gather_grads: segment ", i, " lies outside the arena");
    const auto& g = grads[i];
    // no grad flowed -> null: the segment is zero-filled
    srcs[i] = (g.defined() && g.numel() > 0)
                  ? p.in(g, "grad", arena.scalar_type(), lens[i]) : nullptr;
    o[i] = ofs[i];
    l[i] = (int)lens[i];
  }
  const int dt = dtype_code(arena);
  for (size_t base = 0; base < n; base += 64)
    STM_LAUNCH(stmgcn_gather_grads, stream(), dt, srcs.data() + base, o.data() + base,
               l.data() + base, (int)std::min<size_t>(64, n - base), ap);
}

void adam_step(at::Tensor master, at::Tensor param, at::Tensor grad,
               at::Tensor m, at::Tensor v, at::Tensor hyper) {
  const Ptrs p("adam_step", master);
  const long n = master.numel();
  float* mp = p.in<float>(master, "master", at::kFloat, n);
  void* pp = p.in(param, "param", param.scalar_type(), n);
  const void* gp = p.in(grad, "grad", param.scalar_type(), n);
  float* m1 = p.in<float>(m, "m", at::kFloat, n);
  float* m2 = p.in<float>(v, "v", at::kFloat, n);
  float* hp = p.in<float>(hyper, "hyper", at::kFloat, 9);
  STM_LAUNCH(stmgcn_adam, stream(), dtype_code(param), mp, pp, gp, m1, m2, hp, n);
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
  m.def("atb_wgrad_multi", &atb_wgrad_multi,
        "All-support wgrad: C[k] += As[k]^T B in one launch, B read once");
}
