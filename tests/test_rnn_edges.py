"""Fused LSTM/GRU at the limits the binding allows (T = 16, L = 8), at
T = 1, at ragged and sub-tile S, and on the eval path, against the float64
oracle with bounds from _lowp_oracle."""
import pytest
import torch

import _lowp_oracle as lo

DEV = "cuda"


def _to_gpu(r, grad=True):
    x = r.inputs["x"].to(DEV).requires_grad_(grad)
    n = len(r.inputs) - 1
    ws = [r.inputs[f"w{i}"].to(DEV).requires_grad_(grad) for i in range(n)]
    return x, ws


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", lo.RNN_CASES, ids=str)
@pytest.mark.parametrize("cell", lo.RNN_CELLS)
def test_fused_rnn_edges(cell, case, dtype):
    """Output, dx and every weight/bias gradient, each under its own bound."""
    from stmgcn_amd.ops.hip_ops import FusedLSTMFn
    r = lo.rnn_reference(cell, case, dtype)
    x, ws = _to_gpu(r)
    out = FusedLSTMFn.apply(x, cell, case[4], True, *ws)
    (out.float() ** 2).sum().backward()
    got = {"out": out, "dx": x.grad}
    for i, w in enumerate(ws):
        got[f"dw{i}"] = w.grad
    r.check(got, f"{cell} {case} {lo.dtype_name(dtype)}")


EVAL_CASES = [(33, 16, 2, 1), (40, 3, 2, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("shape", EVAL_CASES, ids=str)
@pytest.mark.parametrize("cell", lo.RNN_CELLS)
def test_eval_equals_train_bitwise(cell, shape, dtype):
    """training=False only drops the cseq/gates saves and the dead top-layer
    hseq store: the output must not change by a bit, and must be right."""
    from stmgcn_amd.ops.hip_ops import FusedLSTMFn
    for ret_seq in (False, True):
        r = lo.rnn_reference(cell, shape + (ret_seq,), dtype)
        x, ws = _to_gpu(r, grad=False)
        y_train = FusedLSTMFn.apply(x, cell, ret_seq, True, *ws)
        y_eval = FusedLSTMFn.apply(x, cell, ret_seq, False, *ws)
        assert torch.equal(y_eval, y_train)
        e = lo.relerr(y_eval, r.want["out"])
        print(cell, shape, ret_seq, "eval err", e, "tol", r.tol("out"))
        assert e <= r.tol("out")


@pytest.mark.gpu
@pytest.mark.parametrize("cell", lo.RNN_CELLS)
def test_dispatcher_no_grad_and_weight_only_grad(cell):
    """rnn_forward picks eval under no_grad, and picks training when only the
    weights require grad; the weight gradients are then still right."""
    from stmgcn_amd.ops import rnn_forward
    case = (40, 3, 2, 64, True)
    S, T, L, cin, ret_seq = case
    r = lo.rnn_reference(cell, case, lo.BF16)
    x, ws = _to_gpu(r, grad=False)
    for w in ws:
        w.requires_grad_(True)
    h0 = torch.zeros(L, S, lo.H, device=DEV, dtype=lo.BF16)
    y = rnn_forward(cell, x, ws, h0, h0.clone(), ret_seq)
    assert y.grad_fn is not None
    with torch.no_grad():
        y_ng = rnn_forward(cell, x, ws, h0, h0.clone(), ret_seq)
    assert y_ng.grad_fn is None and not y_ng.requires_grad
    assert torch.equal(y_ng, y)
    (y.float() ** 2).sum().backward()
    assert x.grad is None
    got = {"out": y}
    for i, w in enumerate(ws):
        got[f"dw{i}"] = w.grad
    r.check(got, f"dispatcher {cell} {case}", skip=("dx",))
