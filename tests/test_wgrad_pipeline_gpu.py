"""The wgrad kernels' branch-free loads (stmgcn_amd/csrc/wgrad.hip): every row
that must read as zero -- past a chunk's end, t == 0 of h_{t-1}, a pad row of
x, a thread without a staging unit -- is loaded from a clamped address inside
its own tensor and dropped by a select where it is used.

Reference and bound. The reference is float64 from the same rounded inputs.
A workgroup accumulates its share of the R products (exact in fp32) in fp32,
and at most two workgroups add their sums into a zero, so per element

    |err| <= R * 2^-23 * (|A|^T @ |B|)  (+ 2^-149 for exact zeros)

which is twice the textbook (R - 1) * 2^-24 * sum|a_i b_i|. No fitted
tolerance.

Poison. Every input is a contiguous slice out of the middle of a larger
allocation whose other elements are NaN (S_pad * 64 or more on each side): a
load that leaves its tensor, a clamped load whose value leaks, or a mask by
multiplication shows up as NaN, which fails the comparison. Pad rows inside
hseq / dA are finite random values, as in the other wgrad tests.
"""
import functools
import zlib

import pytest
import torch

from _lowp_oracle import BF16, F16, H, dtype_name

pytestmark = pytest.mark.gpu
DTYPES = [BF16, F16]
TILE = 32
U23 = 2.0 ** -23
TINY = 2.0 ** -149


def _C():
    from stmgcn_amd.ops.functional import require_hip
    return require_hip()


def _poisoned(values, pad):
    """values (CPU, low precision) as a contiguous CUDA view with `pad` NaN
    elements before and after it in the same allocation (pad % 8 == 0 keeps
    the 16-byte alignment the kernels' fragment loads need)."""
    assert pad % 8 == 0
    n = values.numel()
    big = torch.full((pad + n + pad,), float("nan"), dtype=values.dtype)
    big[pad:pad + n] = values.reshape(-1)
    view = big.cuda()[pad:pad + n].view(values.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


def _within(got, want, lim, label):
    err = (got.double().cpu() - want).abs()
    worst = (err - lim).max().item()
    print(f"{label}: max err {err.max().item():.3e}, max bound {lim.max().item():.3e}, "
          f"worst (err - bound) {worst:.3e}")
    assert bool((err <= lim).all()), f"{label}: {int((~(err <= lim)).sum())} elements out"


# --------------------------------------------------------------------------
# lstm_wgrad / lstm_wgrad_grads
def _rho(kp):
    return 16 * ((kp >> 2) & 1) + 4 * (kp >> 3) + (kp & 3)


def _tile_dA(dA):
    """Natural (L, T, S_pad, 4H) -> the tile order of csrc/common.h."""
    L, T, Sp, G = dA.shape
    rows = torch.tensor([_rho(kp) for kp in range(TILE)])
    blk = dA.reshape(L, T, Sp // TILE, TILE, G).index_select(3, rows).transpose(3, 4)
    return blk.contiguous().reshape(L, T, Sp, G)


LSTM_SHAPES = [
    # (T, S, S_pad, L)
    (1, 5, 32, 2),      # one tile: half a K-step, and all of it t == 0
    (1, 64, 64, 2),     # one whole K-step
    (3, 70, 96, 2),     # 9 tiles: odd tail; tp0 = 3 splits a K-step at t == 0; ragged S
    (2, 150, 160, 2),   # 10 tiles, tp0 = 5: more than two loop rounds, ends on a full pair
]
LSTM_CASES = [s + (cin,) for s in LSTM_SHAPES for cin in (1, 64)] + [
    (3, 352, 352, 1, 1),    # R = 1056: two chunks of 17 and 16 tiles
]


@functools.lru_cache(maxsize=None)
def _lstm_case(case, dtype):
    """Poisoned device inputs, float64 sums and their bounds."""
    T, S, S_pad, L, cin = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    dA = (torch.randn(L, T, S_pad, 4 * H, generator=g) * 0.5).to(dtype)
    hseq = (torch.randn(L, T, S_pad, H, generator=g) * 0.5).to(dtype)
    x = (torch.randn(S, T, cin, generator=g) * 0.5).to(dtype)
    R = T * S_pad
    x_pad = torch.zeros(S_pad, T, cin, dtype=torch.float64)
    x_pad[:S] = x.double()
    x_rows = x_pad.transpose(0, 1).reshape(R, cin)       # row r = t * S_pad + s
    want, lim = [], []
    for l in range(L):
        a = dA[l].double().reshape(R, 4 * H)
        hp = torch.zeros(T, S_pad, H, dtype=torch.float64)
        hp[1:] = hseq[l, :-1].double()                   # h_{t-1}, zero at t == 0
        hp = hp.reshape(R, H)
        hx = x_rows if l == 0 else hseq[l - 1].double().reshape(R, H)
        for b in (hx, hp):
            want.append(a.T @ b)
            lim.append(R * U23 * (a.abs().T @ b.abs()) + TINY)
        want.append(a.sum(0))
        lim.append(R * U23 * a.abs().sum(0) + TINY)
    pad = S_pad * 64
    dev = (_poisoned(_tile_dA(dA), pad), _poisoned(hseq, pad), _poisoned(x, pad))
    return dev, want, lim


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_name)
@pytest.mark.parametrize("case", LSTM_CASES, ids=str)
def test_lstm_wgrad_clamped_loads(case, dtype):
    T, S, S_pad, L, cin = case
    C = _C()
    (dA, hseq, x), want, lim = _lstm_case(case, dtype)
    dwih, dwhh, db = C.lstm_wgrad(dA, hseq, x)
    fp32 = []
    for l in range(L):
        cl = cin if l == 0 else H
        fp32 += [dwih[l, :, :cl], dwhh[l], db[l]]
    for i, (got, w, b) in enumerate(zip(fp32, want, lim)):
        _within(got, w, b, f"lstm_wgrad {case} layer {i // 3} {'ih hh b'.split()[i % 3]}")
    # the finishing form: the same sums (at most two workgroups per layer, so
    # the order of their atomics does not matter), rounded once
    new = C.lstm_wgrad_grads(dA, hseq, x, False)
    assert len(new) == 4 * L
    for l in range(L):
        ih, hh, b = fp32[3 * l:3 * l + 3]
        for n, o in zip(new[4 * l:4 * l + 4], (ih, hh, b, b)):
            assert n.dtype == dtype and torch.equal(n, o.contiguous().to(dtype))


# --------------------------------------------------------------------------
# atb_wgrad_multi / atb_wgrad_multi_grads
ATB_SHAPES = [(3, 64, 64),   # (nsrc, CA, N)
              (3, 8, 8)]     # M = 24: threads with no A unit, two live waves
ATB_ROWS = [1, 63, 65, 193, 255, 256, 321]   # odd ends, 1..4 K-steps, two workgroups


@functools.lru_cache(maxsize=None)
def _atb_case(shape, rows, dtype):
    nsrc, CA, N = shape
    g = torch.Generator().manual_seed(2000 + rows)
    As = [(torch.randn(rows, CA, generator=g) * 0.5).to(dtype) for _ in range(nsrc)]
    B = (torch.randn(rows, N, generator=g) * 0.5).to(dtype)
    a, b = torch.cat(As, 1).double(), B.double()
    want = (a.T @ b, b.sum(0))
    lim = (rows * U23 * (a.abs().T @ b.abs()) + TINY, rows * U23 * b.abs().sum(0) + TINY)
    dev = ([_poisoned(A, 4096) for A in As], _poisoned(B, 4096))
    return dev, want, lim


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_name)
@pytest.mark.parametrize("rows", ATB_ROWS)
@pytest.mark.parametrize("shape", ATB_SHAPES, ids=str)
def test_atb_wgrad_clamped_loads(shape, rows, dtype):
    nsrc, CA, N = shape
    C = _C()
    (As, B), (w_dW, w_db), (l_dW, l_db) = _atb_case(shape, rows, dtype)
    label = f"atb_wgrad {shape} rows {rows}"
    dW = torch.zeros(nsrc * CA, N, device="cuda")
    db = torch.zeros(N, device="cuda")
    C.atb_wgrad_multi(As, B, dW, db)
    _within(dW, w_dW, l_dW, label + " dW")
    _within(db, w_db, l_db, label + " db")
    dW_nob = torch.zeros(nsrc * CA, N, device="cuda")
    C.atb_wgrad_multi(As, B, dW_nob, None)
    assert torch.equal(dW_nob, dW)
    # the finishing form: same sums (at most two workgroups), rounded once
    g_dW, g_db = C.atb_wgrad_multi_grads(As, B, nsrc, True)
    assert g_dW.dtype == dtype and torch.equal(g_dW, dW.to(dtype))
    assert torch.equal(g_db, db.to(dtype))
    (g_nob,) = C.atb_wgrad_multi_grads(As, B, nsrc, False)
    assert torch.equal(g_nob, dW.to(dtype))
