"""The reduction kernels that finish their own outputs ("last arriver
finishes", stmgcn_amd/csrc/common.h) against the kept fp32 bindings, plus the
two small kernels that replace glue launches (weight pack, ReLU mask).

A finishing binding runs the same partial sums as its fp32 sibling; only the
order in which the workgroups' atomics arrive differs, and the place of the
final rounding. The bound is therefore one rounding step of the output dtype,
per element:  |new - old.to(dtype)| <= 2 * EPS[dtype] * |old.to(dtype)|.

Inputs of the multi-chunk cases are non-negative: every partial then has the
sign of the total, so the fp32 order error (a few 2^-24 of the total) stays
far below one output ulp. With signed inputs an element whose partials cancel
to ~1e-5 of their size would turn that same fp32 error into several output
ulps, which says nothing about the epilogue. One- and two-workgroup cases
(fp32 addition is commutative) use signed inputs and must match exactly.
Non-negative inputs also make a lost partial visible: with c chunks it lowers
an element by about 1/c, far outside the bound.
"""
import pytest
import torch

from _lowp_oracle import BF16, EPS, F16, H, dtype_name

pytestmark = pytest.mark.gpu
DTYPES = [BF16, F16]
ids = dtype_name


def _C():
    from stmgcn_amd.ops.functional import require_hip
    return require_hip()


def _rand(shape, dtype, scale, signed, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g) * scale
    return (t if signed else t.abs()).to(dtype).cuda()


def _within_one_rounding(new, old_f32, dtype, label):
    old = old_f32.to(dtype)
    assert new.dtype == dtype and new.shape == old.shape, (label, new.shape, old.shape)
    assert new.is_contiguous(), label
    diff = (new.double() - old.double()).abs()
    lim = 2.0 * EPS[dtype] * old.double().abs()
    worst = (diff - lim).max().item()
    print(f"{label}: max|new-old| {diff.max().item():.3e}, "
          f"worst (diff - bound) {worst:.3e}")
    assert bool((diff <= lim).all()), f"{label}: {int((diff > lim).sum())} elements out"


# --------------------------------------------------------------------------
# lstm_wgrad_grads vs lstm_wgrad
def _lstm_inputs(S, T, L, cin, dtype, signed, seed=0):
    S_pad = (S + 31) // 32 * 32
    dA = _rand((L, T, S_pad, 4 * H), dtype, 0.25, signed, seed)
    hseq = _rand((L, T, S_pad, H), dtype, 0.25, signed, seed + 1)
    x = _rand((S, T, cin), dtype, 0.25, signed, seed + 2)
    return dA, hseq, x


def _lstm_old(C, dA, hseq, x, gru):
    """What FusedLSTMFn.backward builds from the fp32 binding, still fp32."""
    dwih, dwhh, dbf = C.lstm_wgrad(dA, hseq, x)
    L, cin = dA.shape[0], x.shape[2]
    out = []
    for l in range(L):
        cl = cin if l == 0 else H
        if gru:
            out += [dwih[l, :3 * H, :cl],
                    torch.cat([dwhh[l, :2 * H], dwhh[l, 3 * H:]]),
                    dbf[l, :3 * H],
                    torch.cat([dbf[l, :2 * H], dbf[l, 3 * H:]])]
        else:
            out += [dwih[l, :, :cl], dwhh[l], dbf[l], dbf[l]]
    return [o.contiguous() for o in out]


LSTM_CASES = [
    # (S, T, L, cin, gru, signed)
    (300, 8, 3, 1, False, False),   # 3 chunks per layer, S_pad = 320 pads rows
    (300, 8, 2, 64, True, False),   # GRU un-packing, dense layer-0 input
    (5, 1, 1, 1, False, True),      # one chunk: the last arriver is the only one
]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("case", LSTM_CASES, ids=str)
def test_lstm_wgrad_grads_matches_fp32_binding(case, dtype):
    S, T, L, cin, gru, signed = case
    C = _C()
    dA, hseq, x = _lstm_inputs(S, T, L, cin, dtype, signed)
    old = _lstm_old(C, dA, hseq, x, gru)
    new = C.lstm_wgrad_grads(dA, hseq, x, gru)
    assert len(new) == 4 * L
    base = new[0].untyped_storage().data_ptr()
    for i, (n, o) in enumerate(zip(new, old)):
        assert n.untyped_storage().data_ptr() == base, "views of one flat buffer"
        _within_one_rounding(n, o, dtype, f"lstm {case} grad {i}")
        if signed:   # single workgroup per layer: same sums, same rounding
            assert torch.equal(n, o.to(dtype))


# --------------------------------------------------------------------------
# atb_wgrad_multi_grads vs atb_wgrad_multi
ATB_CASES = [
    # (rows, nsrc, CA, N, split, signed)
    (400, 3, 8, 8, 3, False),        # 4 chunks
    (65537, 4, 64, 64, 4, False),    # 512 chunks, ragged last row
    (1, 3, 8, 8, 3, True),           # one chunk
    (400, 7, 8, 16, 4, False),       # dual form: two launches, one workspace
]


def _atb_inputs(rows, nsrc, CA, N, dtype, signed, seed=10):
    As = [_rand((rows, CA), dtype, 0.25, signed, seed + i) for i in range(nsrc)]
    return As, _rand((rows, N), dtype, 0.25, signed, seed + 9)


def _atb_old(C, As, B, split):
    CA, N = As[0].shape[1], B.shape[1]
    dW = torch.zeros(len(As) * CA, N, device="cuda")
    db = torch.zeros(N, device="cuda")
    C.atb_wgrad_multi(As[:split], B, dW[:split * CA], db)
    if split < len(As):
        C.atb_wgrad_multi(As[split:], B, dW[split * CA:], None)
    return dW, db


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("case", ATB_CASES, ids=str)
def test_atb_wgrad_multi_grads_matches_fp32_binding(case, dtype):
    rows, nsrc, CA, N, split, signed = case
    C = _C()
    As, B = _atb_inputs(rows, nsrc, CA, N, dtype, signed)
    dW_old, db_old = _atb_old(C, As, B, split)
    dW, db = C.atb_wgrad_multi_grads(As, B, split, True)
    _within_one_rounding(dW, dW_old, dtype, f"atb {case} dW")
    _within_one_rounding(db, db_old, dtype, f"atb {case} db")
    (dW_nob,) = C.atb_wgrad_multi_grads(As, B, split, False)
    _within_one_rounding(dW_nob, dW_old, dtype, f"atb {case} dW (no db)")
    if signed:
        assert torch.equal(dW, dW_old.to(dtype)) and torch.equal(db, db_old.to(dtype))


# --------------------------------------------------------------------------
# head_wgrad_grads vs head_wgrad
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("B,N,G", [(1, 1, 64), (2, 515, 40)], ids=str)
def test_head_wgrad_grads_matches_fp32_binding(B, N, G, dtype):
    C = _C()
    signed = B * N == 1
    dy = _rand((B, N, 1), dtype, 0.25, signed, 20)
    fsum = _rand((B, N, G), dtype, 0.25, signed, 21)
    dw_old, db_old = C.head_wgrad(dy, fsum)
    dw, db = C.head_wgrad_grads(dy, fsum)
    _within_one_rounding(dw, dw_old.view(1, G), dtype, f"head {B * N} dw")
    _within_one_rounding(db, db_old, dtype, f"head {B * N} db")
    if signed:
        assert torch.equal(dw, dw_old.view(1, G).to(dtype))


# --------------------------------------------------------------------------
# Staleness: 20 back-to-back calls alternating two input sets whose results
# differ by exactly 2x. The allocator hands the same workspace and output
# buffers back, so a finishing read that misses a partial (about -1/chunks)
# or sees the previous call's data (2x off) is far outside the bound.
def _alternate(run, refs, dtype, label):
    """run(k) -> list of outputs for input set k; refs[k] the fp32 lists."""
    lows = [[o.to(dtype).double() for o in r] for r in refs]
    bad = torch.zeros((), device="cuda")
    for call in range(20):
        k = call & 1
        for n, o in zip(run(k), lows[k]):
            bad += ((n.double() - o).abs() > 2.0 * EPS[dtype] * o.abs()).sum()
    assert int(bad.item()) == 0, f"{label}: {int(bad.item())} elements out"


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_lstm_wgrad_grads_no_stale_reads(dtype):
    C = _C()
    dA, hseq, x = _lstm_inputs(300, 8, 3, 1, dtype, False)
    sets = [(dA, hseq, x), (dA * 2, hseq, x)]
    refs = [_lstm_old(C, *s, False) for s in sets]
    # the sets really are 2x apart (up to the fp32 atomics' arrival order)
    torch.testing.assert_close(refs[1][1], refs[0][1] * 2, rtol=1e-5, atol=0)
    _alternate(lambda k: C.lstm_wgrad_grads(*sets[k], False), refs, dtype, "lstm")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("nsrc,split", [(3, 3), (7, 4)])
def test_atb_wgrad_multi_grads_no_stale_reads(nsrc, split, dtype):
    C = _C()
    As, B = _atb_inputs(400, nsrc, 8, 8, dtype, False)
    sets = [(As, B), (As, B * 2)]
    refs = [list(_atb_old(C, a, b, split)) for a, b in sets]
    _alternate(lambda k: C.atb_wgrad_multi_grads(*sets[k], split, True), refs,
               dtype, "atb")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_head_wgrad_grads_no_stale_reads(dtype):
    C = _C()
    dy = _rand((2, 515, 1), dtype, 0.25, False, 20)
    fsum = _rand((2, 515, 40), dtype, 0.25, False, 21)
    sets = [(dy, fsum), (dy * 2, fsum)]
    refs = []
    for s in sets:
        dw, db = C.head_wgrad(*s)
        refs.append([dw.view(1, 40), db])
    _alternate(lambda k: C.head_wgrad_grads(*sets[k]), refs, dtype, "head")


# --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("cin", [1, 64])
@pytest.mark.parametrize("L", [1, 3, 8])
def test_pack_bwd_weights_is_the_transposes(L, cin, dtype):
    C = _C()
    w_ih = [_rand((4 * H, cin if l == 0 else H), dtype, 1.0, True, 30 + l)
            for l in range(L)]
    w_hh = [_rand((4 * H, H), dtype, 1.0, True, 40 + l) for l in range(L)]
    out = C.lstm_pack_bwd_weights(w_ih, w_hh)
    assert len(out) == 2 * L
    for got, w in zip(out, w_ih + w_hh):
        assert got.is_contiguous()
        assert torch.equal(got, w.t().contiguous())


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("n", [8, 4096, 1003, 70001])
def test_relu_bwd_is_the_mask(n, dtype):
    C = _C()
    dy = _rand((n + 1,), dtype, 1.0, True, 50)
    y = torch.relu(_rand((n + 1,), dtype, 1.0, True, 51))
    y[::7] = 0.0
    y[3::7] = -0.0
    y[5::11] = -1.5          # not a ReLU output, but the mask is defined
    for a, b in ((dy[:n], y[:n]),        # 16-byte aligned
                 (dy[1:], y[1:])):       # 2-byte offset: scalar path
        got = C.relu_bwd(a, b)
        assert torch.equal(got, a * (b > 0))
    d3, y3 = dy[:n // 8 * 8].view(-1, 8), y[:n // 8 * 8].view(-1, 8)
    assert torch.equal(C.relu_bwd(d3, y3), d3 * (y3 > 0))


def test_relu_bwd_unaligned_path_is_linear():
    """The element-wise path (a base pointer off the 16-byte grid) must do each
    thread's own 8 elements and no more. It moves the same bytes as the vector
    path with 8x the memory instructions, each a 2-byte access whose cache
    line the thread's next seven accesses reuse: at most 8-16x the time, so 32x
    is the bound (the aligned time floored at 5 us, since both calls are near
    the launch cost at this size). A loop that ran on to the end of the tensor
    would do n / 16 = 16384 times the work; n is kept at 2^18 so that even then
    the call ends within a fraction of a second."""
    C = _C()
    n = 1 << 18
    dy = _rand((n + 8,), BF16, 1.0, True, 60)
    y = _rand((n + 8,), BF16, 1.0, True, 61)

    def gpu_ms(a, b):
        C.relu_bwd(a, b)
        best = float("inf")
        for _ in range(5):
            t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            t0.record()
            out = C.relu_bwd(a, b)
            t1.record()
            t1.synchronize()
            best = min(best, t0.elapsed_time(t1))
        return best, out

    t_al, out_al = gpu_ms(dy[:n], y[:n])
    t_un, out_un = gpu_ms(dy[1:n + 1], y[1:n + 1])
    print(f"relu_bwd n={n}: aligned {t_al * 1e3:.1f} us, unaligned {t_un * 1e3:.1f} us")
    assert torch.equal(out_al, dy[:n] * (y[:n] > 0))
    assert torch.equal(out_un, dy[1:n + 1] * (y[1:n + 1] > 0))
    assert t_un <= 32 * max(t_al, 5e-3), (t_un, t_al)
