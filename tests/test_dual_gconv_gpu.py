"""Dual random-walk diffusion gconv on the GPU (dual_gconv.hip + its stack
path) against the float64 dense oracle, with the bounds of _lowp_oracle:
every MFMA/scalar dispatch pair, partial tiles, empty CSR rows in either
direction, eval == train, the stack path, swapped directions, and the model.
"""
import pytest
import torch

import _dual_oracle as do
import _lowp_oracle as lo

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _run(r, training=True, activation="relu"):
    from stmgcn_amd.ops.hip_ops import ChebGconvFn
    csr_d = r.extra["csr"].to(DEV)
    t = {k: v.to(DEV).requires_grad_(True) for k, v in r.inputs.items()}
    y = ChebGconvFn.apply(t["x"], t["W"], t["b"], csr_d, activation, training)
    return y, t


def _check_fwd_bwd(r, label):
    y, t = _run(r)
    (y.float() ** 2).sum().backward()
    r.check({"out": y, "dx": t["x"].grad, "dW": t["W"].grad, "db": t["b"].grad},
            label)


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", do.DUAL_CASES, ids=str)
def test_fused_dual_gconv(case, dtype):
    """y, dX, dW, db of the fused path at every dispatch pair."""
    from stmgcn_amd.ops import hip_ops
    hip_ops.reset_fallback_count()
    _check_fwd_bwd(do.dual_reference(case, dtype),
                   f"dual {case} {lo.dtype_name(dtype)}")
    assert hip_ops.fallback_count() == 0


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", do.DUAL_CASES, ids=str)
def test_eval_equals_train_bitwise(case, dtype):
    """no_grad only changes which state buffers exist (K = 3: pf_3/pb_3
    overwrite pf_1/pb_1); y must not change by a bit."""
    from stmgcn_amd.ops import gconv_mix
    r = do.dual_reference(case, dtype)
    csr_d = r.extra["csr"].to(DEV)
    x = r.inputs["x"].to(DEV)
    W = r.inputs["W"].to(DEV).requires_grad_(True)
    b = r.inputs["b"].to(DEV).requires_grad_(True)
    y_train = gconv_mix(csr_d, x, W, b, "relu")
    assert y_train.grad_fn is not None
    with torch.no_grad():
        y_eval = gconv_mix(csr_d, x, W, b, "relu")
    assert y_eval.grad_fn is None
    assert torch.equal(y_eval, y_train)
    assert lo.relerr(y_train, r.want["out"]) <= r.tol("out")


def test_stack_path_fp32():
    """fp32, C = 5: cheb_apply / cheb_combine once per generator. Tolerances
    of test_gpu_kernels.py::test_cheb_gconv_forward_backward (fp32)."""
    from stmgcn_amd.ops import hip_ops
    from stmgcn_amd.ops import reference_impl as ref
    from stmgcn_amd.ops.hip_ops import ChebGconvFn
    N, B, C, Cout, K = do.DUAL_STACK_FP32
    csr = do.dual_graph(N, K)
    g = lo._gen("dual-stack-fp32")
    base = {"x": torch.randn(B, N, C, generator=g),
            "W": torch.randn(csr.K_supports * C, Cout, generator=g) * 0.2,
            "b": torch.randn(Cout, generator=g) * 0.1}
    hip_ops.reset_fallback_count()
    t = {k: v.to(DEV).requires_grad_(True) for k, v in base.items()}
    y = ChebGconvFn.apply(t["x"], t["W"], t["b"], csr.to(DEV), "relu")
    (y ** 2).sum().backward()
    assert hip_ops.fallback_count() == 0
    tr = {k: v.clone().requires_grad_(True) for k, v in base.items()}
    y_ref = ref.gconv_mix_dense(csr.dense_supports(), tr["x"], tr["W"], tr["b"], "relu")
    (y_ref ** 2).sum().backward()
    rtol, atol = 1e-4, 1e-5
    torch.testing.assert_close(y.cpu(), y_ref.detach(), rtol=rtol, atol=atol * 10)
    for k in ("x", "W", "b"):
        torch.testing.assert_close(t[k].grad.cpu(), tr[k].grad,
                                   rtol=rtol * 10, atol=atol * 50)


def test_stack_path_bf16_k4():
    """K = 4 > 3 leaves the fused path (wgrad source limit): stack path."""
    from stmgcn_amd.ops import hip_ops
    hip_ops.reset_fallback_count()
    _check_fwd_bwd(do.dual_reference(do.DUAL_STACK_K4, lo.BF16),
                   f"dual-stack {do.DUAL_STACK_K4} bf16")
    assert hip_ops.fallback_count() == 0


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
def test_direction_swap_is_visible(dtype):
    """Forward-half weights 8x the backward half: exchanging the halves (what
    swapped generators or transposes amount to) moves y by far more than the
    bound, and the kernel agrees with the oracle of the unswapped W."""
    from stmgcn_amd.ops.hip_ops import ChebGconvFn
    r = do.dual_reference(do.DUAL_SWAP_CASE, dtype, True)
    label = f"dual-swap {lo.dtype_name(dtype)}"
    y, t = _run(r, activation=None)
    (y.float() ** 2).sum().backward()
    # the run with the halves exchanged; its dX goes through the transposes
    xs = r.inputs["x"].to(DEV).requires_grad_(True)
    y_sw = ChebGconvFn.apply(xs, r.extra["W_swapped"].to(DEV), t["b"].detach(),
                             r.extra["csr"].to(DEV), None, True)
    (y_sw.float() ** 2).sum().backward()
    d_out, d_dx = lo.relerr(y_sw, y), lo.relerr(xs.grad, t["x"].grad)
    print(f"{label}: swapped-vs-not out {d_out:.5f} dx {d_dx:.5f}")
    assert d_out > r.tol("out") and d_dx > r.tol("dx")
    r.check({"out": y, "dx": t["x"].grad, "dW": t["W"].grad, "db": t["b"].grad},
            label)


def _directed_model_setup(n, M, T, hidden, layers):
    from stmgcn_amd.graph import SupportGenerator
    from stmgcn_amd.models import ST_MGCN
    gen = SupportGenerator("dual_random_walk", 2)
    csr = [gen.process_csr(do.directed_adj(n, seed=s)) for s in range(M)]
    torch.manual_seed(0)
    model = ST_MGCN(M=M, seq_len=T, n_nodes=n, input_dim=1,
                    lstm_hidden_dim=hidden, lstm_num_layers=layers,
                    gcn_hidden_dim=hidden,
                    sta_kernel_config={"kernel_type": "dual_random_walk", "K": 2})
    return model, csr


def test_model_bf16_gpu_vs_cpu_fp32():
    """ST_MGCN (M=2, N=33, B=2, T=8) forward + backward, bf16 on the GPU
    through the fused dual path, against the same weights on the CPU in fp32.
    One eager step. Thresholds are those of the bf16 model parity test
    test_gpu_kernels.py::test_full_model_bf16_hip_vs_torch_impl (0.06 output,
    0.12 fc-weight gradient, max-normalised): the fp32 model test's 1e-4 is
    below the half-ulp of bf16 (2^-9) and cannot apply to a bf16 run; it is
    applied to the fp32 run in test_model_fp32_gpu_vs_cpu below."""
    import copy
    from stmgcn_amd.ops import hip_ops
    n, M, T, B = 33, 2, 8, 2
    model, csr = _directed_model_setup(n, M, T, 64, 3)
    model = model.to(torch.bfloat16)              # round the weights once
    x = torch.randn(B, T, n, 1).to(torch.bfloat16)
    cpu = copy.deepcopy(model).float()
    y_cpu = cpu(x.float(), csr)
    g_cpu = torch.autograd.grad((y_cpu ** 2).sum(), cpu.fc.weight)[0]

    hip_ops.reset_fallback_count()
    gpu = model.to(DEV)
    y_gpu = gpu(x.to(DEV), [c.to(DEV) for c in csr])
    g_gpu = torch.autograd.grad((y_gpu.float() ** 2).sum(), gpu.fc.weight)[0]
    assert hip_ops.fallback_count() == 0
    rel, relg = lo.relerr(y_gpu, y_cpu), lo.relerr(g_gpu, g_cpu)
    print(f"model bf16 vs cpu fp32: out {rel:.5f} fc grad {relg:.5f}")
    assert rel < 0.06, f"forward rel err {rel}"
    assert relg < 0.12, f"fc grad rel err {relg}"


def test_model_fp32_gpu_vs_cpu(monkeypatch):
    """Same model in fp32 (dual stack path) at the tolerance of
    test_gpu_kernels.py::test_model_gpu_matches_cpu_fp32; like that test it
    opts into the counted torch fallback for the fp32 RNN only."""
    monkeypatch.setenv("STMGCN_ALLOW_FALLBACK", "1")
    n, M, T, B = 33, 2, 8, 2
    model, csr = _directed_model_setup(n, M, T, 16, 2)
    x = torch.randn(B, T, n, 1)
    y_cpu = model(x, csr)
    y_gpu = model.to(DEV)(x.to(DEV), [c.to(DEV) for c in csr])
    torch.testing.assert_close(y_gpu.cpu(), y_cpu, rtol=1e-4, atol=1e-4)


def test_csr_validation_at_dual_bindings():
    """Both dual bindings refuse, for either generator, a rowptr that is not
    N + 1 long and a vals longer than colidx, before they launch. Both
    malformed inputs only append an entry: nothing would index past valid
    data even without the check."""
    from stmgcn_amd.ops.functional import require_hip
    _C = require_hip()
    csr = do.dual_graph(5, 2).to(DEV)
    gb = csr.dual
    K = gb.K_supports - 1
    g = lo._gen("dual-csr-validation")
    x = torch.randn(1, 5, 8, generator=g).to(lo.BF16).to(DEV)
    W = torch.randn(csr.K_supports * 8, 8, generator=g).to(lo.BF16).to(DEV)
    fwd_csr = [csr.row_ptr, csr.col_idx, csr.vals, gb.row_ptr, gb.col_idx, gb.vals]
    bwd_csr = [csr.row_ptr_t, csr.col_idx_t, csr.vals_t,
               gb.row_ptr_t, gb.col_idx_t, gb.vals_t]
    calls = [
        (fwd_csr, lambda c: _C.dual_gconv_fused_fwd(x, *c, W, None, K, 0, False)),
        (bwd_csr, lambda c: _C.dual_gconv_fused_bwd_dx(x, W, *c, K)),
    ]
    for good, call in calls:
        call(good)                            # the call itself is well-formed
        for d in (0, 3):                      # forward / backward generator
            long_rp = list(good)
            long_rp[d] = torch.cat([good[d], good[d][-1:]])
            with pytest.raises(RuntimeError):
                call(long_rp)
            long_v = list(good)
            long_v[d + 2] = torch.cat([good[d + 2], good[d + 2][-1:]])
            with pytest.raises(RuntimeError):
                call(long_v)
    torch.cuda.synchronize()
