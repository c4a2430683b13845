"""lstm_bwd's pointwise bodies: one straight-line body per layer form (where
dh comes from: the layer above, dout at every stage, dout at the last
timestep only; scalar-input layer 0 or not). The shapes below reach the forms
the other lists do not, against the float64 oracle with the bounds of
_lowp_oracle; plus the padding rows of the dA stream and a staleness check of
the form that reads dout at every stage and reduces the scalar-input dx."""
import pytest
import torch

import _lowp_oracle as lo

DEV = "cuda"

# (S, T, L, cin, ret_seq)
LAYER_FORM_CASES = [
    # top layer and scalar-input layer 0 in one, dout in the layer prologue
    (33, 2, 1, 1, False),
    # the same layer form with dout at every stage
    (33, 3, 1, 1, True),
    # dense single layer, dout in the prologue
    (33, 2, 1, 64, False),
    # dense single layer, dout at every stage
    (33, 3, 1, 64, True),
    # dense layer 0 under two hand-offs, one-row tail
    (33, 3, 3, 64, False),
    # scalar-input layer 0 under a ret_seq top layer
    (33, 3, 3, 1, True),
    # three tiles, one live row in the last
    (65, 2, 2, 1, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", LAYER_FORM_CASES, ids=str)
@pytest.mark.parametrize("cell", lo.RNN_CELLS)
def test_bwd_layer_forms(cell, case, dtype):
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


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", LAYER_FORM_CASES, ids=str)
@pytest.mark.parametrize("cell", lo.RNN_CELLS)
def test_layer_form_bounds_come_from_the_floor(cell, case, dtype):
    """No cap decides a bound of the cases above: 3 * floor <= cap for every
    tensor (worst: 0.82 of the cap, GRU bf16 (33, 2, 1, 64, False) `out`)."""
    r = lo.rnn_reference(cell, case, dtype)
    for name, floor in r.floor.items():
        assert 3 * floor <= r.cap[name], (name, floor, r.cap[name])


def _raw_inputs(case, seed):
    S, T, L, cin, ret_seq = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, T, cin, generator=g).to(lo.BF16).to(DEV)
    ws = [w.to(lo.BF16).to(DEV) for w in lo.rnn_weights("lstm", L, cin, g)]
    dshape = (S, T, lo.H) if ret_seq else (S, lo.H)
    dout = torch.randn(*dshape, generator=g).to(lo.BF16).to(DEV)
    return x, ws, dout


def _raw_bwd(C, case, x, ws, dout):
    """forward saves -> packed transposes -> dgrad, through the raw bindings;
    every intermediate is dropped on return, so the allocator hands the same
    blocks to the next call."""
    L, ret_seq = case[2], case[4]
    w_ih, w_hh = ws[0::4], ws[1::4]
    _, _, cseq, gates = C.lstm_fwd(x, w_ih, w_hh, ws[2::4], ws[3::4], ret_seq,
                                   True, False)
    wT = C.lstm_pack_bwd_weights(w_ih, w_hh)
    dx, dA = C.lstm_bwd(dout, x, cseq, gates, wT[:L], wT[L:], ret_seq, False)
    return dx.cpu(), dA.cpu()


def _da_rows(dA):
    """The tiled dA stream (csrc/common.h) as (L, T, S_pad, 4H) rows: inside a
    32-row tile, element (gate g, k') is row rho(k') of the tile."""
    L, T, S_pad, G = dA.shape
    kp = torch.arange(32)
    rho = 16 * ((kp >> 2) & 1) + 4 * (kp >> 3) + (kp & 3)
    tiles = dA.reshape(L, T, S_pad // 32, G, 32)
    rows = torch.empty(L, T, S_pad // 32, 32, G, dtype=dA.dtype)
    rows[:, :, :, rho, :] = tiles.transpose(3, 4)
    return rows.reshape(L, T, S_pad, G)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(33, 2, 3, 1, False), (33, 3, 1, 64, True)],
                         ids=str)
def test_bwd_padding_rows_are_zero(case):
    """Rows of dA at or beyond S: the dout mask makes dh zero there, every dA
    term carries dh or dc, and a zero dA row hands a zero dh down."""
    from stmgcn_amd.ops.functional import require_hip
    C = require_hip()
    S = case[0]
    x, ws, dout = _raw_inputs(case, 21)
    _, dA = _raw_bwd(C, case, x, ws, dout)
    rows = _da_rows(dA)
    assert rows.shape[2] == 64
    assert rows[:, :, :S].float().abs().max() > 0
    assert torch.equal(rows[:, :, S:], torch.zeros_like(rows[:, :, S:]))


@pytest.mark.gpu
def test_bwd_seq_scalar_form_no_stale_state():
    """A, then B (other weights and dout), then A again on the recycled
    buffers, in the form that reads dout at every stage and reduces the
    scalar-input dx: dx and dA of the two A runs are bit-equal."""
    from stmgcn_amd.ops.functional import require_hip
    C = require_hip()
    case = (33, 3, 1, 1, True)
    xa, wa, da = _raw_inputs(case, 11)
    xb, wb, db = _raw_inputs(case, 12)
    dx1, dA1 = _raw_bwd(C, case, xa, wa, da)
    dxb, _ = _raw_bwd(C, case, xb, wb, db)
    dx2, dA2 = _raw_bwd(C, case, xa, wa, da)
    assert not torch.equal(dxb, dx1), "B must differ from A for the test to bite"
    assert torch.equal(dx1, dx2)
    assert torch.equal(dA1, dA2)
