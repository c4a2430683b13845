"""lstm_fwd's stage bodies: the shapes at which a (layer, t) stage takes each
of its straight-line forms (scalar-input layer 0 / dense input, training saves
/ eval, top layer, with / without the recurrent term and the input prefetch),
against the float64 oracle with the bounds of _lowp_oracle; eval against
train, a staleness check of the recycled buffers, and saturated activations
(the unclamped tanh)."""
import pytest
import torch

import _lowp_oracle as lo

DEV = "cuda"

# (S, T, L, cin, ret_seq)
SCHEDULE_CASES = [
    # scalar layer 0, two dense layers, a one-row tail
    (33, 2, 3, 1, False),
    # the prefetch with a stage before and after it
    (33, 3, 3, 1, False),
    # T = 1: no prefetch, no recurrent term, ret_seq stores in every stage
    (64, 1, 3, 64, True),
    # a single row, dense guarded layer 0
    (1, 2, 2, 64, False),
    # the flagship's T and L, three full tiles
    (96, 8, 3, 1, False),
]
SATURATION_CASE = (33, 2, 2, 1, True)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", SCHEDULE_CASES, ids=str)
@pytest.mark.parametrize("cell", lo.RNN_CELLS)
def test_fwd_schedule_cases(cell, case, dtype):
    """Output, dx and every weight/bias gradient, each under its own bound."""
    from stmgcn_amd.ops.hip_ops import FusedLSTMFn
    r = lo.rnn_reference(cell, case, dtype)
    x = r.inputs["x"].to(DEV).requires_grad_(True)
    ws = [r.inputs[f"w{i}"].to(DEV).requires_grad_(True)
          for i in range(len(r.inputs) - 1)]
    out = FusedLSTMFn.apply(x, cell, case[4], True, *ws)
    (out.float() ** 2).sum().backward()
    got = {"out": out, "dx": x.grad}
    for i, w in enumerate(ws):
        got[f"dw{i}"] = w.grad
    r.check(got, f"{cell} {case} {lo.dtype_name(dtype)}")


def packed_weights(cell, ws):
    """(w_ih, w_hh, b_ih, b_hh) per-layer lists as the raw binding takes them;
    GRU in the 4-slot packing of FusedLSTMFn: [r | z | n_input | n_hidden]."""
    w_ih, w_hh, b_ih, b_hh = (list(ws[i::4]) for i in range(4))
    if cell == "lstm":
        return w_ih, w_hh, b_ih, b_hh
    H = lo.H
    for l in range(len(w_ih)):
        wi, wh, bi, bh = w_ih[l], w_hh[l], b_ih[l], b_hh[l]
        w_ih[l] = torch.cat([wi, torch.zeros_like(wi[:H])])
        w_hh[l] = torch.cat([wh[:2 * H], torch.zeros_like(wh[:H]), wh[2 * H:]])
        b_ih[l] = torch.cat([bi, torch.zeros_like(bi[:H])])
        b_hh[l] = torch.cat([bh[:2 * H], torch.zeros_like(bh[:H]), bh[2 * H:]])
    return w_ih, w_hh, b_ih, b_hh


def raw_inputs(cell, case, dtype, seed):
    S, T, L, cin, _ = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, T, cin, generator=g).to(dtype)
    ws = [w.to(dtype) for w in lo.rnn_weights(cell, L, cin, g)]
    return x, ws


def raw_fwd(C, cell, case, x, ws, training=True):
    """lstm_fwd through the raw binding: [out] in eval, [out, hseq, cseq,
    gates] in training, on the CPU; the device buffers are dropped on return,
    so the allocator hands the same blocks to the next call."""
    w = [[t.to(DEV).contiguous() for t in lst] for lst in packed_weights(cell, ws)]
    outs = C.lstm_fwd(x.to(DEV), *w, case[4], training, cell == "gru")
    return [o.cpu() for o in outs]


# (cell, dtype, case) of the raw-binding tests
RAW_CASES = [("lstm", lo.BF16, (33, 3, 3, 1, False)),
             ("gru", lo.F16, (40, 3, 2, 64, True))]
RAW_IDS = [f"{c}-{lo.dtype_name(d)}-{s}" for c, d, s in RAW_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("cell,dtype,case", RAW_CASES, ids=RAW_IDS)
def test_fwd_eval_equals_train(cell, dtype, case):
    """The eval bodies (no saves, top layer's sequence not handed off) give
    the bits of the training bodies."""
    from stmgcn_amd.ops.functional import require_hip
    C = require_hip()
    x, ws = raw_inputs(cell, case, dtype, 21)
    out_train = raw_fwd(C, cell, case, x, ws, True)[0]
    (out_eval,) = raw_fwd(C, cell, case, x, ws, False)
    assert torch.equal(out_eval, out_train)


@pytest.mark.gpu
@pytest.mark.parametrize("cell,dtype,case", RAW_CASES, ids=RAW_IDS)
def test_fwd_no_stale_state(cell, dtype, case):
    """A, then B (other weights and inputs), then A again on the recycled
    buffers: lstm_fwd has no atomics, so all four outputs of the two A runs are
    bit-equal, the padding rows of the last tile included, unless a weight
    fragment, a prefetched input or an LDS slot of B's run (or of a
    neighbouring stage or layer) leaks into A's."""
    from stmgcn_amd.ops.functional import require_hip
    C = require_hip()
    xa, wa = raw_inputs(cell, case, dtype, 11)
    xb, wb = raw_inputs(cell, case, dtype, 12)
    a1 = raw_fwd(C, cell, case, xa, wa)
    b = raw_fwd(C, cell, case, xb, wb)
    a2 = raw_fwd(C, cell, case, xa, wa)
    assert not torch.equal(b[0], a1[0]), "B must differ from A for the test to bite"
    for name, t1, t2 in zip(("out", "hseq", "cseq", "gates"), a1, a2):
        assert torch.equal(t1, t2), name


def saturation_inputs(cell, dtype):
    """x = randn * m, m cycling over the rows through 1, 20, 1e3 and the
    largest scale the dtype takes (1e30 / 2e4); the rounded f16 input is
    clamped to +-6e4 so that no input is infinite."""
    S, T, L, cin, _ = SATURATION_CASE
    g = lo._gen("rnn-saturation", cell, lo.dtype_name(dtype))
    big = 1e30 if dtype == lo.BF16 else 2e4
    m = torch.tensor([1.0, 20.0, 1e3, big])[torch.arange(S) % 4].view(S, 1, 1)
    x = (torch.randn(S, T, cin, generator=g) * m).to(dtype)
    if dtype == lo.F16:
        x = x.float().clamp(-6e4, 6e4).to(dtype)
    assert torch.isfinite(x.float()).all()
    ws = [w.to(dtype) for w in lo.rnn_weights(cell, L, cin, g)]
    return x, ws


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("cell", lo.RNN_CELLS)
def test_fwd_saturation(cell, dtype):
    """Gate pre-activations far beyond where exp overflows: the output is
    finite and within the bound the all-low-precision CPU run gives. Forward
    only: the saturated gradients are zero and a relative error against them
    means nothing."""
    from stmgcn_amd.ops.hip_ops import FusedLSTMFn
    _, _, L, _, ret_seq = SATURATION_CASE
    x, ws = saturation_inputs(cell, dtype)
    t = {"x": x, **{f"w{i}": w for i, w in enumerate(ws)}}
    want = lo.rnn_oracle(cell, {k: v.double() for k, v in t.items()}, L, ret_seq)
    low = lo.rnn_oracle(cell, t, L, ret_seq)
    assert torch.isfinite(want).all()
    floor = lo.relerr(low, want)
    tol = lo.bound(floor, dtype, lo.CAP_OUT)
    out = FusedLSTMFn.apply(x.to(DEV), cell, ret_seq, False,
                            *[w.to(DEV) for w in ws])
    assert torch.isfinite(out.float()).all()
    err = lo.relerr(out, want)
    print(f"{cell} {lo.dtype_name(dtype)} saturation out: err {err:.5f} "
          f"floor {floor:.5f} tol {tol:.5f}")
    assert err <= tol
    # the training bodies round the saturated gates and cell into their saves
    from stmgcn_amd.ops.functional import require_hip
    saves = raw_fwd(require_hip(), cell, SATURATION_CASE, x, ws, True)
    assert torch.equal(saves[0], out.cpu())
    for name, t in zip(("out", "hseq", "cseq", "gates"), saves):
        assert torch.isfinite(t.float()).all(), name
