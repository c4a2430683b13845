"""ChebConv kernels at the shapes where tiles are partial and dispatch
changes: fused forward/backward against the float64 oracle with bounds from
_lowp_oracle, eval-vs-train bit equality, the stack path at channel counts
that do not divide the 256-thread block, and atb_wgrad_multi called directly.
"""
import pytest
import torch

import _lowp_oracle as lo

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _run_gconv(r, training=True):
    from stmgcn_amd.ops.hip_ops import ChebGconvFn
    csr_d = r.extra["csr"].to(DEV)
    t = {k: v.to(DEV).requires_grad_(True) for k, v in r.inputs.items()}
    y = ChebGconvFn.apply(t["x"], t["W"], t["b"], csr_d, "relu", training)
    return y, t


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", lo.CHEB_CASES, ids=str)
def test_fused_gconv_edges(case, dtype):
    """Forward, dX, dW, db at partial tiles / every MFMA-vs-scalar dispatch."""
    r = lo.cheb_reference(case, dtype)
    y, t = _run_gconv(r)
    (y.float() ** 2).sum().backward()
    r.check({"out": y, "dx": t["x"].grad, "dW": t["W"].grad, "db": t["b"].grad},
            f"chebconv {case} {lo.dtype_name(dtype)}")


def test_wide_stack_path_bf16():
    """cin = 80 > 64: cheb_apply stack + atb_wgrad at KC = 240 + cheb_combine."""
    r = lo.cheb_reference(lo.CHEB_WIDE_CASE, lo.BF16)
    y, t = _run_gconv(r)
    (y.float() ** 2).sum().backward()
    r.check({"out": y, "dx": t["x"].grad, "dW": t["W"].grad, "db": t["b"].grad},
            f"chebconv-stack {lo.CHEB_WIDE_CASE}")


# ---- eval == train, bit for bit -------------------------------------------
EVAL_CASES = [(33, 2, c, c, kernel, K)
              for c in (64, 8)
              for kernel, K in (("chebyshev", 1), ("chebyshev", 2),
                                ("chebyshev", 3), ("localpool", 2))]


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", EVAL_CASES, ids=str)
def test_eval_equals_train_bitwise(case, dtype):
    """training=False only changes which state buffers exist (K_s = 4: the
    last state overwrites p_1); y must not change by a bit."""
    from stmgcn_amd.ops import gconv_mix
    r = lo.cheb_reference(case, dtype)
    y_train, _ = _run_gconv(r, training=True)
    y_eval, _ = _run_gconv(r, training=False)
    assert torch.equal(y_eval, y_train)
    assert lo.relerr(y_train, r.want["out"]) <= r.tol("out")

    csr_d = r.extra["csr"].to(DEV)
    x = r.inputs["x"].to(DEV)
    W = r.inputs["W"].to(DEV).requires_grad_(True)
    b = r.inputs["b"].to(DEV).requires_grad_(True)
    y_grad = gconv_mix(csr_d, x, W, b, "relu")
    assert y_grad.grad_fn is not None
    with torch.no_grad():
        y_ng = gconv_mix(csr_d, x, W, b, "relu")
    assert y_ng.grad_fn is None and not y_ng.requires_grad
    assert torch.equal(y_ng, y_grad)
    assert torch.equal(y_ng, y_train)


# ---- stack path (fp32) at channel counts that do not divide 256 -----------
@pytest.mark.parametrize("C,N,B,K", [(24, 33, 2, 3), (48, 33, 2, 2),
                                     (300, 10, 1, 2)])
def test_stack_path_odd_channels_fp32(C, N, B, K):
    """C = 24/48: the last 16 threads of a block own no row. C = 300: the
    C > 256 branch, one row per block with a channel loop."""
    from stmgcn_amd.ops import reference_impl as ref
    from stmgcn_amd.ops.functional import require_hip
    _C = require_hip()
    csr = lo.csr_graph(n=N, K=K)
    csr_d = csr.to(DEV)
    g = lo._gen("stack", C, N, B, K)
    x = torch.randn(B, N, C, generator=g)
    S = _C.cheb_apply(x.to(DEV), csr_d.row_ptr, csr_d.col_idx, csr_d.vals,
                      csr_d.K_supports, False)
    assert S.shape == (B, N, csr.K_supports, C)
    S_ref = ref.cheb_supports_apply(csr, x.double())          # (B, K, N, C)
    torch.testing.assert_close(S.permute(0, 2, 1, 3).cpu().double(), S_ref,
                               rtol=1e-5, atol=1e-5)

    U = torch.randn(B, N, csr.K_supports, C, generator=g)
    Z = _C.cheb_combine(U.to(DEV), csr_d.row_ptr, csr_d.col_idx, csr_d.vals, False)
    dense = csr.dense_supports().double()
    Z_ref = sum(torch.einsum("ij,bjc->bic", dense[k], U[:, :, k].double())
                for k in range(csr.K_supports))
    torch.testing.assert_close(Z.cpu().double(), Z_ref, rtol=1e-4, atol=1e-4)


# ---- atb_wgrad_multi called directly ---------------------------------------
def _check_atb_multi(nsrc, CA, N, rows, dtype):
    from stmgcn_amd.ops.functional import require_hip
    _C = require_hip()
    g = lo._gen("atb", nsrc, CA, N, rows, lo.dtype_name(dtype))
    As = [(torch.randn(rows, CA, generator=g) * 0.5).to(dtype) for _ in range(nsrc)]
    Bm = (torch.randn(rows, N, generator=g) * 0.5).to(dtype)
    C0 = torch.randn(nsrc * CA, N, generator=g)
    db0 = torch.randn(N, generator=g)
    Cg, dbg = C0.to(DEV), db0.to(DEV)
    _C.atb_wgrad_multi([a.to(DEV) for a in As], Bm.to(DEV), Cg, dbg)
    want = C0.double() + torch.cat([a.double().T @ Bm.double() for a in As])
    db_want = db0.double() + Bm.double().sum(dim=0)
    tol = dict(rtol=2e-2, atol=2e-2 * rows ** 0.5)   # test_atb_wgrad_matches_gemm
    torch.testing.assert_close(Cg.cpu().double(), want, **tol)
    torch.testing.assert_close(dbg.cpu().double(), db_want, **tol)
    # without db the call must leave C accumulation unchanged
    Cg2 = C0.to(DEV)
    _C.atb_wgrad_multi([a.to(DEV) for a in As], Bm.to(DEV), Cg2, None)
    torch.testing.assert_close(Cg2.cpu().double(), want, **tol)


@pytest.mark.parametrize("N", [8, 40, 64])
@pytest.mark.parametrize("CA", [8, 24, 64])
@pytest.mark.parametrize("nsrc", [1, 3, 4])
def test_atb_wgrad_multi_small_rows(nsrc, CA, N):
    """One row, a ragged 32-row k-step, and 129 rows (two workgroups, the
    second with a single row); C and db arrive non-zero and are added to."""
    for rows in (1, 31, 129):
        _check_atb_multi(nsrc, CA, N, rows, lo.BF16)
    _check_atb_multi(nsrc, CA, N, 31, lo.F16)


@pytest.mark.parametrize("nsrc,CA,N,dtype", [
    (1, 64, 64, lo.BF16), (3, 24, 40, lo.BF16), (4, 64, 8, lo.F16),
    (4, 8, 64, lo.BF16)], ids=str)
def test_atb_wgrad_multi_empty_tail_chunks(nsrc, CA, N, dtype):
    """65537 rows -> 512 chunks of 129 rows: chunks 509..511 start past the
    end and must add nothing."""
    _check_atb_multi(nsrc, CA, N, 65537, dtype)


# ---- the binding boundary: CSR validation, bias lifetime --------------------
def test_csr_validation_at_every_binding():
    """Every binding that takes a CSR refuses one whose rowptr is not N + 1
    long or whose vals and colidx differ in length, before it launches. Both
    malformed inputs only append an entry, so nothing indexes past valid data
    even without the check."""
    from stmgcn_amd.ops.functional import require_hip
    _C = require_hip()
    csr = lo.csr_graph(n=5, K=2).to(DEV)
    K_s = csr.K_supports
    g = lo._gen("csr-validation")
    x = torch.randn(1, 5, 8, generator=g).to(DEV)
    W = torch.randn(K_s * 8, 8, generator=g).to(DEV)
    U = torch.randn(1, 5, K_s, 8, generator=g).to(DEV)
    calls = {
        "cheb_apply": lambda rp, ci, v: _C.cheb_apply(x, rp, ci, v, K_s, False),
        "cheb_combine": lambda rp, ci, v: _C.cheb_combine(U, rp, ci, v, False),
        "cheb_gconv_fused_fwd": lambda rp, ci, v: _C.cheb_gconv_fused_fwd(
            x, rp, ci, v, W, None, K_s, False, 0, False),
        "cheb_gconv_fused_bwd_dx": lambda rp, ci, v: _C.cheb_gconv_fused_bwd_dx(
            x, W, rp, ci, v, K_s, False),
        "spmm_axpby": lambda rp, ci, v: _C.spmm_axpby(x, None, rp, ci, v, 1.0, 0.0),
    }
    rp, ci, v = csr.row_ptr, csr.col_idx, csr.vals
    long_rp = torch.cat([rp, rp[-1:]])
    long_v = torch.cat([v, v[-1:]])
    for name, call in calls.items():
        call(rp, ci, v)                       # the call itself is well-formed
        with pytest.raises(RuntimeError):
            call(long_rp, ci, v)
        with pytest.raises(RuntimeError):
            call(rp, ci, long_v)
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,B,C,Cout", [(5, 1, 8, 8), (33, 2, 64, 64)])
def test_fused_fwd_noncontiguous_bias(N, B, C, Cout):
    """A strided bias view is made contiguous inside the binding; that copy
    must outlive the launches. At the small shape y is allocated from the
    block a freed copy would have returned to the allocator."""
    from stmgcn_amd.ops.functional import require_hip
    _C = require_hip()
    csr = lo.csr_graph(n=N, K=2).to(DEV)
    K_s = csr.K_supports
    g = lo._gen("strided-bias", N, B, C, Cout)
    x = torch.randn(B, N, C, generator=g).to(lo.BF16).to(DEV)
    W = (torch.randn(K_s * C, Cout, generator=g) * 0.1).to(lo.BF16).to(DEV)
    full = torch.randn(2 * Cout, generator=g).to(lo.BF16).to(DEV)
    bias = full[::2]
    assert not bias.is_contiguous()

    def fwd(b):
        return _C.cheb_gconv_fused_fwd(x, csr.row_ptr, csr.col_idx, csr.vals, W,
                                       b, K_s, False, 1, False)[0]
    y_strided = fwd(bias)
    y_contig = fwd(bias.contiguous())
    assert torch.equal(y_strided, y_contig)
