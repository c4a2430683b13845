"""The wide head on the GPU (head_multi_fwd / _bwd / _wgrad, 2 <= O <= 32
output columns): every case of _horizon_oracle in bf16 and f16 against the
float64 oracle under the rule of _lowp_oracle, the finishing wgrad against its
fp32 binding, workspace and ticket hygiene across calls, eval against
training, and the public path that refused these widths before."""
import pytest
import torch

import _horizon_oracle as ho
import _lowp_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gpu(inputs, names):
    return {k: v.to(DEV).requires_grad_(k in names) for k, v in inputs.items()}


def _names(M):
    return tuple(f"f{m}" for m in range(M)) + ("w", "b")


def _fwd_bwd(t, M):
    from stmgcn_amd import ops
    y = ops.branch_fuse_head([t[f"f{m}"] for m in range(M)], t["w"], t["b"])
    (y.float() ** 2).sum().backward()
    got = {"out": y.detach()}
    for k in _names(M):
        got["d" + k] = t[k].grad
    return got


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", ho.HEAD_MULTI_CASES, ids=str)
def test_head_multi_cases(case, dtype, monkeypatch):
    from stmgcn_amd.ops import hip_ops
    monkeypatch.delenv("STMGCN_ALLOW_FALLBACK", raising=False)
    B, N, G, M, O = case
    r = ho.head_multi_reference(case, dtype)
    hip_ops.reset_fallback_count()
    t = _gpu(r.inputs, _names(M))
    got = _fwd_bwd(t, M)
    assert hip_ops.fallback_count() == 0
    assert got["out"].shape == (B, N, O) and got["dw"].shape == (O, G)
    assert got["db"].shape == (O,) and got["df0"].shape == (B, N, G)
    r.check(got, f"head-multi {case} {lo.dtype_name(dtype)}")
    # eval (no autograd) gives the training output bit for bit
    with torch.no_grad():
        from stmgcn_amd import ops
        y_eval = ops.branch_fuse_head([t[f"f{m}"].detach() for m in range(M)],
                                      t["w"].detach(), t["b"].detach())
    assert torch.equal(y_eval, got["out"])


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", [(2, 25, 64, 3, 32), (2, 515, 40, 3, 12),
                                  (3, 11, 24, 2, 7)], ids=str)
def test_head_multi_wgrad_finish_matches_fp32_form(case, dtype):
    """The finishing form rounds the same fp32 sums the accumulate-only
    binding returns. The two launches add their partials in their own order,
    so the sums differ by fp32 reassociation: at most (partials) * 2^-24 of
    sum |terms| <= 2^-16 max|dW| here (<= 5 partials, |terms| summed over
    <= 1030 rows against a maximum of that order). On top of that comes the
    one rounding to the output dtype, half an ulp = eps / 2 relative; eps is
    allowed, which also covers a sum that sits next to a rounding boundary."""
    from stmgcn_amd.ops import require_hip
    C = require_hip()
    B, N, G, M, O = case
    g = lo._gen("head_multi_wgrad", case)
    dy = torch.randn(B, N, O, generator=g).to(dtype).to(DEV)
    fsum = torch.randn(B, N, G, generator=g).to(dtype).to(DEV)
    dwf, dbf = C.head_multi_wgrad(dy, fsum)
    dw, db = C.head_multi_wgrad_grads(dy, fsum)
    assert dwf.dtype == torch.float32 and dwf.shape == (O, G) and dbf.shape == (O,)
    assert dw.dtype == dtype and dw.shape == (O, G) and db.shape == (O,)
    # the fp32 sums themselves against float64 on the CPU
    dy64, f64 = dy.double().cpu().view(-1, O), fsum.double().cpu().view(-1, G)
    assert lo.relerr(dwf, dy64.t() @ f64) < 1e-5
    assert lo.relerr(dbf, dy64.sum(0)) < 1e-5
    for fin, f32 in ((dw, dwf), (db, dbf)):
        err = (fin.double() - f32.double()).abs()
        lim = lo.EPS[dtype] * f32.double().abs() + 2.0 ** -16 * f32.abs().max().item()
        print(f"{case} {lo.dtype_name(dtype)}: worst excess "
              f"{(err - lim).max().item():.3e}")
        assert (err <= lim).all()


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
def test_head_multi_back_to_back_calls(dtype):
    """Two calls in a row, the second with every branch doubled (exact in both
    dtypes) and judged against its own float64 reference: a sum or a ticket
    left over from the first call would put dW / db of the second (about 4x
    the first's) far outside the bound."""
    case = (2, 515, 40, 3, 12)
    M = case[3]
    r = ho.head_multi_reference(case, dtype)
    first = _fwd_bwd(_gpu(r.inputs, _names(M)), M)
    r.check(first, f"first call {lo.dtype_name(dtype)}")
    twice = {k: (v * 2 if k.startswith("f") else v) for k, v in r.inputs.items()}
    want = lo.fwd_bwd(lo.head_oracle, twice, _names(M), torch.float64)
    low = lo.fwd_bwd(lo.head_oracle, twice, _names(M), dtype)
    second = _fwd_bwd(_gpu(twice, _names(M)), M)
    bad = []
    for k in sorted(want):
        cap = lo.CAP_OUT if k == "out" else lo.CAP_GRAD
        tol = lo.bound(lo.relerr(low[k], want[k]), dtype, cap)
        e = lo.relerr(second[k], want[k])
        print(f"second call {k}: err {e:.5f} tol {tol:.5f}")
        if not e <= tol:
            bad.append(f"{k}: err {e:.5f} > tol {tol:.5f}")
    assert not bad, "; ".join(bad)
    # and a third call on the first inputs reproduces the first call's
    # forward bit for bit (nothing of the forward depends on earlier calls)
    third = _fwd_bwd(_gpu(r.inputs, _names(M)), M)
    assert torch.equal(third["out"], first["out"])
    assert torch.equal(third["df0"], first["df0"])
    r.check(third, f"third call {lo.dtype_name(dtype)}")


def test_head_three_columns_is_served(monkeypatch):
    """Refused before the wide head existed: C_out = 3 on the GPU without
    STMGCN_ALLOW_FALLBACK raised RuntimeError from branch_fuse_head_hip."""
    from stmgcn_amd import ops
    from stmgcn_amd.ops import hip_ops
    monkeypatch.delenv("STMGCN_ALLOW_FALLBACK", raising=False)
    hip_ops.reset_fallback_count()
    g = lo._gen("head3")
    feats = [torch.randn(2, 16, 8, generator=g).to(lo.BF16).to(DEV) for _ in range(2)]
    w = (torch.randn(3, 8, generator=g) * 0.3).to(lo.BF16).to(DEV)
    b = (torch.randn(3, generator=g) * 0.1).to(lo.BF16).to(DEV)
    y = ops.branch_fuse_head(feats, w, b)
    assert y.shape == (2, 16, 3) and hip_ops.fallback_count() == 0
    want = torch.nn.functional.linear((feats[0].double() + feats[1].double()).cpu(),
                                      w.double().cpu(), b.double().cpu())
    assert lo.relerr(y, want) < 4 * lo.EPS[lo.BF16]
    # outside the served range it is still an error that names the range
    w40 = torch.randn(40, 8, device=DEV, dtype=lo.BF16)
    with pytest.raises(RuntimeError, match="2<=C_out<=32"):
        ops.branch_fuse_head(feats, w40, torch.zeros(40, device=DEV, dtype=lo.BF16))
    with pytest.raises(RuntimeError, match="STMGCN_ALLOW_FALLBACK"):
        ops.branch_fuse_head([f.float() for f in feats], w.float(), b.float())


def test_st_mgcn_horizon_forward_on_gpu():
    """ST_MGCN(horizon=3) did not exist (TypeError); bf16 on the HIP path it
    returns (B, N, P, C) with no fallback."""
    from stmgcn_amd.models import ST_MGCN
    from stmgcn_amd.ops import hip_ops
    N = 33
    torch.manual_seed(3)
    model = ST_MGCN(M=2, seq_len=4, n_nodes=N, input_dim=1, lstm_hidden_dim=64,
                    lstm_num_layers=1, gcn_hidden_dim=64,
                    sta_kernel_config={"kernel_type": "chebyshev", "K": 2},
                    horizon=3).to(device=DEV, dtype=lo.BF16)
    adjs = [lo.csr_graph(n=N, seed=m, K=2).to(DEV) for m in range(2)]
    hip_ops.reset_fallback_count()
    out = model(torch.randn(2, 4, N, 1, device=DEV, dtype=lo.BF16), adjs)
    assert out.shape == (2, N, 3, 1) and torch.isfinite(out.float()).all()
    assert hip_ops.fallback_count() == 0
