"""Pointwise kernels (gate, head, MSE, seqsum) and FusedAdam at the sizes
where their launch geometry changes: more than one reduce chunk, more than
one block of the per-batch kernels, single elements, low-precision dtypes,
more than 64 gather segments and the strided gather loop."""
import pytest
import torch

import _lowp_oracle as lo

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALL_DTYPES = (lo.F32,) + lo.LOWP


def _gpu(inputs, dtype, wrt):
    return {k: v.to(DEV, dtype).requires_grad_(k in wrt) for k, v in inputs.items()}


def _check_fp32(got, want, relmax=None, out_tol=None, grad_tol=None):
    """fp32 cases keep the older tests' tolerances for the same op."""
    for name in sorted(want):
        if relmax is not None:
            e = lo.relerr(got[name], want[name])
            print(name, "err", e)
            assert e < relmax, f"{name}: rel err {e}"
        else:
            tol = out_tol if name == "out" else grad_tol
            torch.testing.assert_close(got[name].detach().cpu().double(),
                                       want[name], rtol=tol, atol=tol)


# ---- contextual gate ------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=lo.dtype_name)
@pytest.mark.parametrize("case", lo.GATE_CASES, ids=str)
def test_gate_edges(case, dtype):
    from stmgcn_amd.ops.hip_ops import GateFn
    wrt = ("obs", "g", "w", "b")
    if dtype == lo.F32:
        inputs = lo.gate_inputs(case)
        want = lo.fwd_bwd(lo.gate_oracle, inputs, wrt, torch.float64)
    else:
        r = lo.gate_reference(case, dtype)
        inputs = r.inputs
    t = _gpu(inputs, dtype, wrt)
    out = GateFn.apply(t["obs"], t["g"], t["w"], t["b"])
    (out.float() ** 2).sum().backward()
    got = {"out": out, "dobs": t["obs"].grad, "dg": t["g"].grad,
           "dw": t["w"].grad, "db": t["b"].grad}
    if dtype == lo.F32:
        _check_fp32(got, want, relmax=3e-4)     # test_gate_kernel_matches_oracle
    else:
        r.check(got, f"gate {case} {lo.dtype_name(dtype)}")


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=lo.dtype_name)
@pytest.mark.parametrize("case", lo.GATE_CASES, ids=str)
def test_gate_node_mean_is_exact_to_fp32(case, dtype):
    """The pooled z = mean_n(g + x_seq) that gate_fwd returns is fp32 whatever
    the dtype. One node counted twice or dropped by the chunked reduction
    moves z by |term| / N but moves `out` only through a sigmoid, far below
    any output tolerance, so z is compared directly. Bound: every partial sum
    passes through at most ceil(2048 / 256) serial adds, 6 shuffle levels, 4
    waves and the per-chunk atomics, under 32 roundings in all, so
    |z - z_ref| <= 32 * 2^-24 * mean_n|term| (mean_n|term| bounds every
    partial sum divided by N)."""
    from stmgcn_amd.ops.functional import require_hip
    _C = require_hip()
    inp = lo.gate_inputs(case)
    obs = inp["obs"].to(DEV, dtype)
    g = inp["g"].to(DEV, dtype)
    xs = _C.seqsum_permute(obs)
    _, z, _, _ = _C.gate_fwd(obs, g, xs, inp["w"].to(DEV, dtype),
                             inp["b"].to(DEV, dtype))
    assert z.dtype == torch.float32
    term = g.double().cpu() + xs.double().cpu()               # (B, N, T)
    err = (z.double().cpu() - term.mean(dim=1)).abs()
    lim = 32 * 2.0 ** -24 * term.abs().mean(dim=1)
    print("z err/limit max", (err / lim).max().item())
    assert (err <= lim).all()


# ---- head -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=lo.dtype_name)
@pytest.mark.parametrize("case", lo.HEAD_CASES, ids=str)
def test_head_edges(case, dtype):
    from stmgcn_amd.ops.hip_ops import HeadFn
    M = case[3]
    names = tuple(f"f{m}" for m in range(M)) + ("w", "b")
    if dtype == lo.F32:
        inputs = lo.head_inputs(case)
        want = lo.fwd_bwd(lo.head_oracle, inputs, names, torch.float64)
    else:
        r = lo.head_reference(case, dtype)
        inputs = r.inputs
    t = _gpu(inputs, dtype, names)
    y = HeadFn.apply(t["w"], t["b"], *[t[f"f{m}"] for m in range(M)])
    (y.float() ** 2).sum().backward()
    got = {"out": y}
    for k in names:
        got["d" + k] = t[k].grad
    if dtype == lo.F32:
        _check_fp32(got, want, out_tol=1e-4, grad_tol=1e-3)   # test_head_kernel_*
    else:
        r.check(got, f"head {case} {lo.dtype_name(dtype)}")


# ---- MSE ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("n", lo.MSE_CASES)
def test_mse_lowp(n, dtype):
    from stmgcn_amd.ops.hip_ops import FusedMSELossFn
    r = lo.mse_reference(n, dtype)
    pred = r.inputs["pred"].to(DEV).requires_grad_(True)
    loss = FusedMSELossFn.apply(pred, r.inputs["tgt"].to(DEV))
    (d,) = torch.autograd.grad(loss * lo.MSE_UPSTREAM, pred)
    r.check({"out": loss, "dpred": d}, f"mse {n} {lo.dtype_name(dtype)}")


# ---- seqsum ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", lo.SEQSUM_CASES, ids=str)
def test_seqsum_lowp(case, dtype):
    from stmgcn_amd.ops.hip_ops import SeqsumPermuteFn
    r = lo.seqsum_reference(case, dtype)
    obs = r.inputs["obs"].to(DEV).requires_grad_(True)
    out = SeqsumPermuteFn.apply(obs)
    (d,) = torch.autograd.grad(out, obs, r.inputs["gout"].to(DEV))
    r.check({"out": out, "dobs": d}, f"seqsum {case} {lo.dtype_name(dtype)}")


# ---- FusedAdam ------------------------------------------------------------
# 70 small segments + one of 20000 elements: two gather launches (64 + 7
# segments), and 20000 > 8 x 2048 so the first launch's blocks loop.
ADAM_SIZES = [1 + (7 * i) % 40 for i in range(70)]
ADAM_SIZES.insert(5, 20000)
ADAM_STEPS = 5
ADAM_TOL = dict(rtol=1e-5, atol=1e-6)      # test_fused_adam_matches_torch_adam


def _adam_data(dtype):
    """Initial values and per-step grads, rounded to dtype. Every third
    parameter gets no grad."""
    g = lo._gen("adam")
    base = [torch.randn(n, generator=g).to(dtype) for n in ADAM_SIZES]
    grads = [[None if i % 3 == 2 else torch.randn(n, generator=g).to(dtype)
              for i, n in enumerate(ADAM_SIZES)] for _ in range(ADAM_STEPS)]
    return base, grads


def _fused_step(opt, params, gs):
    opt.zero_grad()
    for p, g in zip(params, gs):
        if g is not None:
            p.grad = g.to(DEV)
    opt.step()


def _torch_adam_fp32(base, grads):
    """torch.optim.Adam in fp32 on the same (rounded) values; a parameter
    without grad gets an explicit zero grad, because FusedAdam zero-fills
    where torch would skip the parameter."""
    ps = [torch.nn.Parameter(b.float().to(DEV)) for b in base]
    opt = torch.optim.Adam(ps, lr=1e-2, weight_decay=1e-2)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.zeros_like(p) if g is None else g.float().to(DEV)
        opt.step()
    return ps


def _segments(opt, flat):
    return [flat[o:o + n] for o, n in zip(opt._offsets, opt._lens)]


def test_fused_adam_many_segments_and_missing_grads():
    from stmgcn_amd.train import FusedAdam
    base, grads = _adam_data(lo.F32)
    ps = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    opt = FusedAdam(ps, lr=1e-2, weight_decay=1e-2)
    for gs in grads:
        _fused_step(opt, ps, gs)
    for i, (pf, pt) in enumerate(zip(ps, _torch_adam_fp32(base, grads))):
        torch.testing.assert_close(pf.data, pt.data, msg=lambda m: f"param {i}: {m}",
                                   **ADAM_TOL)


def test_fused_adam_bf16_model_fp32_master():
    from stmgcn_amd.train import FusedAdam
    base, grads = _adam_data(lo.BF16)
    ps = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    opt = FusedAdam(ps, lr=1e-2, weight_decay=1e-2)
    assert opt.master.dtype == torch.float32
    for gs in grads:
        _fused_step(opt, ps, gs)
    masters = _segments(opt, opt.master)
    for i, (pf, mf, pt) in enumerate(zip(ps, masters, _torch_adam_fp32(base, grads))):
        torch.testing.assert_close(mf, pt.data, msg=lambda m: f"master {i}: {m}",
                                   **ADAM_TOL)
        assert pf.dtype == torch.bfloat16
        assert torch.equal(pf.data, mf.bfloat16()), f"param {i} != master.bfloat16()"


@pytest.mark.parametrize("dtype", [lo.F32, lo.BF16], ids=lo.dtype_name)
def test_fused_adam_state_round_trip(dtype):
    """state_dict -> new optimizer -> load_state_dict -> one more step equals
    the uninterrupted run bit for bit."""
    from stmgcn_amd.train import FusedAdam
    base, grads = _adam_data(dtype)
    ps_a = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    opt_a = FusedAdam(ps_a, lr=1e-2, weight_decay=1e-2)
    for gs in grads[:-1]:
        _fused_step(opt_a, ps_a, gs)
    sd = {k: v.clone() for k, v in opt_a.state_dict().items()}
    ps_b = [torch.nn.Parameter(torch.zeros_like(b).to(DEV)) for b in base]
    opt_b = FusedAdam(ps_b, lr=1e-2, weight_decay=1e-2)
    opt_b.load_state_dict(sd)
    for pa, pb in zip(ps_a, ps_b):
        assert torch.equal(pa.data, pb.data)
    _fused_step(opt_a, ps_a, grads[-1])
    _fused_step(opt_b, ps_b, grads[-1])
    for pa, pb in zip(ps_a, ps_b):
        assert torch.equal(pa.data, pb.data)
    for k in ("master", "m", "v", "hyper"):
        assert torch.equal(opt_a.state_dict()[k], opt_b.state_dict()[k]), k
