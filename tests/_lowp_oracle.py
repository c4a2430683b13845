"""Shared cases, float64 oracles and bounds for the kernel edge-case tests
(test_chebconv_edges.py, test_rnn_edges.py, test_pointwise_edges.py).

Every bf16/f16 case is compared the same way. The inputs are rounded to the
low-precision dtype once; the kernel and the oracle both get those rounded
values. The oracle is the matching ``reference_impl`` function in float64 on
the CPU. The metric is, per tensor, ``max|got - ref| / (max|ref| + 1e-6)``.
The bound comes from the reference alone:

    tol = min(max(3 * floor, 2 * eps), cap)

``floor`` is the same metric for the same reference function run entirely in
the low-precision dtype on the CPU. The kernels keep fp32 accumulators and
round only where they store, so they should sit at or below that. The factor
3 covers roundings falling in different places and the max over a few
thousand elements moving by about 2x between rounding patterns. ``2 * eps``
(four half-ulp roundings at the largest magnitude) keeps the bound from
collapsing on tiny cases. ``cap`` is the threshold the older tests use
(0.05 output, 0.08 gradients, 0.1 for f16 RNN gradients), so a new bound is
never looser than an old one; test_lowp_bounds.py asserts that on the CPU.

``python -m tests._lowp_oracle --print`` regenerates the floor table of
docs/TESTING.md.
"""
from __future__ import annotations

import functools
import os
import sys
import zlib

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from stmgcn_amd.data.synthetic import _random_sparse_sym_adj  # noqa: E402
from stmgcn_amd.graph import SupportGenerator  # noqa: E402
from stmgcn_amd.ops import reference_impl as ref  # noqa: E402

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
LOWP = (BF16, F16)
EPS = {BF16: 2.0 ** -8, F16: 2.0 ** -10}
CAP_OUT = 0.05
CAP_GRAD = 0.08
CAP_GRAD_RNN_F16 = 0.1
H = 64


def dtype_name(dt):
    return {BF16: "bf16", F16: "f16", F32: "fp32"}[dt]


def relerr(got, want):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return ((got - want).abs().max() / (want.abs().max() + 1e-6)).item()


def bound(floor, dtype, cap):
    return min(max(3.0 * floor, 2.0 * EPS[dtype]), cap)


def csr_graph(n=64, seed=0, kernel="chebyshev", K=2):
    """Same graph builder as test_gpu_kernels._csr."""
    rng = np.random.default_rng(seed)
    A = torch.from_numpy(_random_sparse_sym_adj(n, 8, rng, weighted=True))
    return SupportGenerator(kernel, K).process_csr(A)


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


class Reference:
    """Rounded inputs, float64 results and low-precision floors of one case.

    inputs: name -> CPU tensor of the case dtype (already rounded).
    want:   name -> float64 tensor ("out" and "d<input>" for each gradient).
    floor:  name -> metric of the all-low-precision CPU run against ``want``.
    cap:    name -> the older suite's threshold for that tensor.
    """

    def __init__(self, dtype, inputs, want, floor, cap, extra=None):
        self.dtype, self.inputs, self.want = dtype, inputs, want
        self.floor, self.cap, self.extra = floor, cap, extra or {}

    def tol(self, name):
        return bound(self.floor[name], self.dtype, self.cap[name])

    def check(self, got, label="", skip=()):
        """Print every figure, then assert all of them."""
        bad = []
        names = set(self.want) - set(skip)
        assert set(got) == names, (sorted(got), sorted(names))
        for name in sorted(names):
            e, t = relerr(got[name], self.want[name]), self.tol(name)
            print(f"{label} {name}: err {e:.5f} floor {self.floor[name]:.5f} "
                  f"tol {t:.5f}")
            if not e <= t:          # also catches NaN
                bad.append(f"{name}: err {e:.5f} > tol {t:.5f}")
        assert not bad, f"{label}: " + "; ".join(bad)


def fwd_bwd(fn, inputs, wrt, dt):
    """Run fn on copies of inputs cast to dt; loss = sum(out^2) as the suite
    does. Returns {"out": .., "d<name>": ..}."""
    ts = {k: v.to(dt).clone().requires_grad_(k in wrt) for k, v in inputs.items()}
    out = fn(ts)
    acc = torch.float64 if dt == torch.float64 else torch.float32
    (out.to(acc) ** 2).sum().backward()
    res = {"out": out.detach()}
    for k in wrt:
        res["d" + k] = ts[k].grad
    return res


def make_reference(fn, inputs, wrt, dtype, cap_grad=CAP_GRAD, extra=None):
    want = fwd_bwd(fn, inputs, wrt, torch.float64)
    low = fwd_bwd(fn, inputs, wrt, dtype)
    floor = {k: relerr(low[k], want[k]) for k in want}
    cap = {k: (CAP_OUT if k == "out" else cap_grad) for k in want}
    return Reference(dtype, inputs, want, floor, cap, extra)


# --------------------------------------------------------------------------
# Fused ChebConv: (N, B, cin, cout, kernel, K)
CHEB_CASES = [
    (33, 3, 64, 64, "chebyshev", 2),
    (31, 1, 32, 16, "chebyshev", 2),
    (33, 2, 32, 48, "chebyshev", 2),
    (50, 2, 48, 64, "chebyshev", 2),
    (33, 2, 24, 40, "chebyshev", 2),
    (33, 2, 64, 8, "chebyshev", 2),
    (50, 2, 64, 64, "chebyshev", 3),
    (33, 2, 64, 64, "chebyshev", 1),
    (33, 2, 16, 64, "localpool", 2),
    (5, 1, 8, 8, "chebyshev", 2),
]
# bf16 only: cin > 64 takes the stack path (cheb_apply + atb_wgrad at KC=240)
CHEB_WIDE_CASE = (33, 2, 80, 64, "chebyshev", 2)


@functools.lru_cache(maxsize=None)
def cheb_graph(N, kernel, K):
    return csr_graph(n=N, kernel=kernel, K=K)


@functools.lru_cache(maxsize=None)
def cheb_reference(case, dtype):
    N, B, cin, cout, kernel, K = case
    csr = cheb_graph(N, kernel, K)
    g = _gen("cheb", case)
    inputs = {
        "x": torch.randn(B, N, cin, generator=g).to(dtype),
        "W": (torch.randn(csr.K_supports * cin, cout, generator=g) * 0.15).to(dtype),
        "b": (torch.randn(cout, generator=g) * 0.1).to(dtype),
    }
    dense = csr.dense_supports()

    def fn(t):
        return ref.gconv_mix_dense(dense.to(t["x"].dtype), t["x"], t["W"],
                                   t["b"], "relu")

    return make_reference(fn, inputs, ("x", "W", "b"), dtype, extra={"csr": csr})


# --------------------------------------------------------------------------
# Fused RNN: (S, T, L, cin, ret_seq)
RNN_CASES = [
    (5, 1, 1, 1, False),
    (31, 16, 1, 1, True),
    (33, 2, 8, 1, False),
    (40, 3, 2, 64, True),
    (33, 16, 2, 64, False),
    (70, 4, 3, 1, True),
    (40, 2, 8, 64, False),
]
RNN_CELLS = ("lstm", "gru")


def rnn_weights(cell, L, cin, g):
    """Same scales as the suite's _lstm_oracle_weights / _gru_weights."""
    gm = 4 if cell == "lstm" else 3
    ws = []
    for l in range(L):
        in_l = cin if l == 0 else H
        ws += [torch.randn(gm * H, in_l, generator=g) * 0.2,
               torch.randn(gm * H, H, generator=g) * 0.2,
               torch.randn(gm * H, generator=g) * 0.1,
               torch.randn(gm * H, generator=g) * 0.1]
    return ws


def rnn_oracle(cell, t, L, ret_seq):
    x = t["x"]
    ws = [t[f"w{i}"] for i in range(4 * L)]
    h0 = torch.zeros(L, x.shape[0], H, dtype=x.dtype)
    if cell == "lstm":
        return ref.lstm_forward(x, ws, h0, h0.clone(), ret_seq)
    return ref.gru_forward(x, ws, h0, ret_seq)


@functools.lru_cache(maxsize=None)
def rnn_reference(cell, case, dtype):
    S, T, L, cin, ret_seq = case
    g = _gen("rnn", cell, case)
    inputs = {"x": torch.randn(S, T, cin, generator=g).to(dtype)}
    for i, w in enumerate(rnn_weights(cell, L, cin, g)):
        inputs[f"w{i}"] = w.to(dtype)
    cap = CAP_GRAD_RNN_F16 if dtype == F16 else CAP_GRAD
    return make_reference(lambda t: rnn_oracle(cell, t, L, ret_seq), inputs,
                          tuple(inputs), dtype, cap_grad=cap)


# --------------------------------------------------------------------------
# Contextual gate: (B, T, N, C)
GATE_CASES = [
    (2, 1, 40, 3),
    (2, 16, 40, 3),
    (65, 2, 8, 1),      # B > 64: two blocks of the per-batch FC kernels
    (2, 3, 2100, 1),    # N > 2048: two forward reduce chunks of 1050
    (2, 2, 300, 8),     # N*C > 2048: two backward reduce chunks
    # the deep variant's blocks 2..n: obs is the previous block's C = 64 output
    (2, 4, 33, 64),     # N*C = 2112: two backward chunks of 1056, split in node 16
    (1, 16, 35, 64),    # T = 16 with C = 64
    (2, 4, 33, 6),      # C neither 1 nor a multiple of 4
]


def gate_inputs(case):
    B, T, N, C = case
    g = _gen("gate", case)
    return {"obs": torch.randn(B, T, N, C, generator=g),
            "g": torch.randn(B, N, T, generator=g),
            "w": torch.randn(T, T, generator=g) * 0.4,
            "b": torch.randn(T, generator=g) * 0.1}


def gate_oracle(t):
    return ref.contextual_gate(t["obs"], t["g"], t["w"], t["b"])


@functools.lru_cache(maxsize=None)
def gate_reference(case, dtype):
    inputs = {k: v.to(dtype) for k, v in gate_inputs(case).items()}
    return make_reference(gate_oracle, inputs, ("obs", "g", "w", "b"), dtype)


# --------------------------------------------------------------------------
# Head: (B, N, G, M)
HEAD_CASES = [(2, 25, G, M) for M in (1, 2, 3) for G in (8, 40, 64)] + [
    (1, 1, 64, 3),       # B*N = 1
    (2, 515, 40, 3),     # B*N = 1030: five wgrad blocks of 206 rows
]


def head_inputs(case):
    B, N, G, M = case
    g = _gen("head", case)
    d = {f"f{m}": torch.randn(B, N, G, generator=g) for m in range(M)}
    d["w"] = torch.randn(1, G, generator=g) * 0.3
    d["b"] = torch.randn(1, generator=g) * 0.1
    return d


def head_oracle(t):
    feats = [t[k] for k in sorted(t) if k.startswith("f")]
    return ref.branch_fuse_head(feats, t["w"], t["b"])


@functools.lru_cache(maxsize=None)
def head_reference(case, dtype):
    inputs = {k: v.to(dtype) for k, v in head_inputs(case).items()}
    return make_reference(head_oracle, inputs, tuple(inputs), dtype)


# --------------------------------------------------------------------------
# MSE: numel; upstream gradient 3.0 as in test_mse_kernel_matches_torch
MSE_CASES = [1, 257, 70001]
MSE_UPSTREAM = 3.0


@functools.lru_cache(maxsize=None)
def mse_reference(n, dtype):
    g = _gen("mse", n)
    inputs = {"pred": torch.randn(n, generator=g).to(dtype),
              "tgt": torch.randn(n, generator=g).to(dtype)}

    def run(dt):
        p = inputs["pred"].to(dt).requires_grad_(True)
        loss = F.mse_loss(p, inputs["tgt"].to(dt))
        (d,) = torch.autograd.grad(loss * MSE_UPSTREAM, p)
        return {"out": loss.detach(), "dpred": d}

    want, low = run(torch.float64), run(dtype)
    floor = {k: relerr(low[k], want[k]) for k in want}
    return Reference(dtype, inputs, want, floor,
                     {"out": CAP_OUT, "dpred": CAP_GRAD})


# --------------------------------------------------------------------------
# Seqsum: (B, T, N, C) with B*T*N = 615, not a multiple of the 256-thread block
# C = 64: 16 rounds of the 4-wide loop; C = 6: one round and a tail of 2
SEQSUM_CASES = [(3, 5, 41, C) for C in (1, 3, 4, 5, 64, 6)]


@functools.lru_cache(maxsize=None)
def seqsum_reference(case, dtype):
    B, T, N, C = case
    g = _gen("seqsum", case)
    inputs = {"obs": torch.randn(B, T, N, C, generator=g).to(dtype),
              "gout": torch.randn(B, N, T, generator=g).to(dtype)}

    def run(dt):
        o = inputs["obs"].to(dt).requires_grad_(True)
        out = o.sum(-1).permute(0, 2, 1)
        (d,) = torch.autograd.grad(out, o, inputs["gout"].to(dt))
        return {"out": out.detach(), "dobs": d}

    want, low = run(torch.float64), run(dtype)
    floor = {k: relerr(low[k], want[k]) for k in want}
    return Reference(dtype, inputs, want, floor,
                     {"out": CAP_OUT, "dobs": CAP_GRAD})


# --------------------------------------------------------------------------
def all_lowp_references():
    """(label, Reference) for every bf16/f16 case of the three modules."""
    for dt in LOWP:
        n = dtype_name(dt)
        for c in CHEB_CASES:
            yield f"chebconv {c} {n}", cheb_reference(c, dt)
        for cell in RNN_CELLS:
            for c in RNN_CASES:
                yield f"{cell} {c} {n}", rnn_reference(cell, c, dt)
        for c in GATE_CASES:
            yield f"gate {c} {n}", gate_reference(c, dt)
        for c in HEAD_CASES:
            yield f"head {c} {n}", head_reference(c, dt)
        for c in MSE_CASES:
            yield f"mse {c} {n}", mse_reference(c, dt)
        for c in SEQSUM_CASES:
            yield f"seqsum {c} {n}", seqsum_reference(c, dt)
    yield (f"chebconv-stack {CHEB_WIDE_CASE} bf16",
           cheb_reference(CHEB_WIDE_CASE, BF16))


def floor_table():
    """Markdown table: worst output floor and worst gradient floor per case,
    and the bounds they give."""
    rows = ["| case | out floor | out tol | worst grad floor | grad tol |",
            "|---|---|---|---|---|"]
    for label, r in all_lowp_references():
        grads = [k for k in r.floor if k != "out"]
        worst = max(grads, key=lambda k: r.floor[k])
        rows.append(f"| {label} | {r.floor['out']:.4f} | {r.tol('out'):.4f} | "
                    f"{r.floor[worst]:.4f} ({worst}) | {r.tol(worst):.4f} |")
    return "\n".join(rows)


if __name__ == "__main__":
    if sys.argv[1:] == ["--print"]:
        print(floor_table())
    else:
        sys.exit("usage: python -m tests._lowp_oracle --print")
