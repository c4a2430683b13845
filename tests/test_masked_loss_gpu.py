"""The fused masked loss on the GPU (masked_loss_fwd / _bwd): MSE, MAE and
Huber over the targets that are not NaN, against the float64 oracle under the
rule of _lowp_oracle, with an upstream gradient of 3.0."""
import pytest
import torch

import _horizon_oracle as ho
import _lowp_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(inputs, kind):
    from stmgcn_amd import ops
    pred = inputs["pred"].to(DEV).requires_grad_(True)
    loss = ops.masked_loss(pred, inputs["tgt"].to(DEV), kind)
    (d,) = torch.autograd.grad(loss * ho.LOSS_UPSTREAM, pred)
    return loss.detach(), d


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("n", ho.LOSS_NUMELS)
@pytest.mark.parametrize("kind", ho.LOSS_KINDS)
def test_masked_loss_cases(kind, n, dtype):
    r = ho.loss_reference(kind, n, dtype)
    loss, d = _run(r.inputs, kind)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and d.dtype == dtype
    r.check({"out": loss, "dpred": d}, f"masked-{kind} {n} {lo.dtype_name(dtype)}")
    masked = torch.isnan(r.inputs["tgt"]).to(DEV)
    assert (n == 1) == (int(masked.sum()) == 0)
    # exactly 0 at every masked index, never NaN anywhere
    assert torch.equal(d[masked], torch.zeros(int(masked.sum()), dtype=dtype, device=DEV))
    assert torch.isfinite(d.float()).all() and torch.isfinite(loss)


@pytest.mark.parametrize("dtype", lo.LOWP + (lo.F32,), ids=lo.dtype_name)
@pytest.mark.parametrize("kind", ho.LOSS_KINDS)
def test_masked_loss_all_masked(kind, dtype):
    g = lo._gen("all-masked")
    inputs = {"pred": torch.randn(3, 257, generator=g).to(dtype),
              "tgt": torch.full((3, 257), float("nan"), dtype=dtype)}
    loss, d = _run(inputs, kind)
    assert loss.item() == 0.0
    assert d.shape == (3, 257)
    assert torch.equal(d, torch.zeros(3, 257, dtype=dtype, device=DEV))


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("n", ho.LOSS_NUMELS)
def test_masked_mse_without_nan_matches_mse_loss(n, dtype):
    """NaN-free targets: kind = mse is ops.mse_loss, under the bound of the
    NaN-free reference (both kernels are judged against the same float64
    values)."""
    from stmgcn_amd import ops
    r = ho.loss_reference("mse", n, dtype, 0.0)
    assert not torch.isnan(r.inputs["tgt"]).any()
    loss, d = _run(r.inputs, "mse")
    r.check({"out": loss, "dpred": d}, f"masked-mse nan-free {n}")
    pred = r.inputs["pred"].to(DEV).requires_grad_(True)
    plain = ops.mse_loss(pred, r.inputs["tgt"].to(DEV))
    (dp,) = torch.autograd.grad(plain * ho.LOSS_UPSTREAM, pred)
    r.check({"out": plain, "dpred": dp}, f"mse_loss {n}")
    e_out, e_d = lo.relerr(loss, plain), lo.relerr(d, dp)
    print(f"masked vs mse_loss {n} {lo.dtype_name(dtype)}: out {e_out:.2e} dpred {e_d:.2e}")
    assert e_out <= r.tol("out") and e_d <= r.tol("dpred")


def test_masked_loss_fp32_matches_oracle():
    """The fp32 form (the parity dtype) against the float64 oracle."""
    from stmgcn_amd.ops import reference_impl as ref
    for kind in ho.LOSS_KINDS:
        inputs = ho.loss_inputs(70001, lo.F32)
        loss, d = _run(inputs, kind)
        p = inputs["pred"].double().requires_grad_(True)
        want = ref.masked_loss(p, inputs["tgt"].double(), kind)
        (dw,) = torch.autograd.grad(want * ho.LOSS_UPSTREAM, p)
        assert lo.relerr(loss, want) < 1e-5 and lo.relerr(d, dw) < 1e-5
