"""lstm_bwd's stage schedule: the shapes at which the BPTT stage takes each of
its paths (with / without the recurrent GEMM, with / without the input GEMM,
with / without a layer above, every arm of the save prefetch and of the cell
parity slots), against the float64 oracle with the bounds of _lowp_oracle,
and a staleness check of the lane-private LDS parking and the prefetch."""
import pytest
import torch

import _lowp_oracle as lo

DEV = "cuda"

# (S, T, L, cin, ret_seq)
SCHEDULE_CASES = [
    # the flagship's structure at its smallest: two tiles with a one-row tail,
    # one stage with and one without GEMM1, both edges of the c rotation, two
    # layer hand-offs, the scalar-input reduction
    (33, 2, 3, 1, False),
    # the t >= 2 arm of the c prefetch
    (33, 3, 3, 1, False),
    # T = 1: no GEMM1 and no prefetch is ever issued, the layer prologue still
    # runs for every layer, dout is read at every stage
    (64, 1, 3, 64, True),
    # a single row
    (1, 2, 2, 64, False),
    # the flagship's T and L, three full tiles
    (96, 8, 3, 1, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", SCHEDULE_CASES, ids=str)
@pytest.mark.parametrize("cell", lo.RNN_CELLS)
def test_bwd_schedule_cases(cell, case, dtype):
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


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(33, 3, 3, 1, False), (40, 3, 2, 64, True)],
                         ids=str)
def test_bwd_no_stale_state(case):
    """A, then B (other weights and dout), then A again on the recycled
    buffers: lstm_bwd has no atomics, so dx and dA of the two A runs are
    bit-equal unless a weight, a parked save or a prefetched word of B's run
    (or of a neighbouring stage) leaks into A's."""
    from stmgcn_amd.ops.functional import require_hip
    C = require_hip()
    xa, wa, da = _raw_inputs(case, 11)
    xb, wb, db = _raw_inputs(case, 12)
    dx1, dA1 = _raw_bwd(C, case, xa, wa, da)
    dxb, _ = _raw_bwd(C, case, xb, wb, db)
    dx2, dA2 = _raw_bwd(C, case, xa, wa, da)
    assert not torch.equal(dxb, dx1), "B must differ from A for the test to bite"
    assert torch.equal(dx1, dx2)
    # rows of dA past S are padding of the last tile: compare the whole tensor
    # anyway, the kernel writes every element of it deterministically
    assert torch.equal(dA1, dA2)
