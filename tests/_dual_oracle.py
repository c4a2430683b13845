"""Cases, graph and float64 references of the dual random-walk gconv tests
(test_dual_random_walk.py on the CPU, test_dual_gconv_gpu.py on the GPU).

Judged by the rule of _lowp_oracle: inputs rounded once to the dtype, oracle
= gconv_mix_dense over csr.dense_supports() in float64 on the CPU, metric
max|got - ref| / (max|ref| + 1e-6) per tensor, bound
min(max(3 floor, 2 eps), cap).
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import _lowp_oracle as lo
from stmgcn_amd.graph import SupportGenerator
from stmgcn_amd.ops import reference_impl as ref

# (N, B, C, Cout, K)
DUAL_CASES = [
    (33, 3, 64, 64, 2),    # MFMA both ways, partial tile
    (31, 1, 32, 16, 1),    # MFMA forward, scalar backward, no yacc
    (33, 2, 24, 40, 2),    # scalar both ways
    (50, 2, 64, 64, 3),    # 4+3 wgrad sources, deepest ping/pong
    (5, 1, 8, 8, 2),       # one tile, mostly padding
    (33, 2, 16, 64, 1),    # scalar forward, MFMA backward
]
# stack path: fp32 (C = 5 as in the reference preset's temporal gconv), K > 3
DUAL_STACK_FP32 = (33, 2, 5, 5, 2)
DUAL_STACK_K4 = (33, 2, 16, 16, 4)


def directed_adj(N, seed=0):
    """Directed weighted adjacency, about 4 out-edges per node. Node 1 has no
    in-edge and node N-2 no out-edge, so each generator and each transpose
    has an empty CSR row. Out-degrees cycle through 2..5 (capped by N), so
    the 4-wide gather and its tail both run."""
    rng = np.random.default_rng(1000 + seed)
    A = np.zeros((N, N), dtype=np.float32)
    for i in range(N):
        others = np.array([j for j in range(N) if j != i])
        deg = min(2 + i % 4, len(others))
        cols = rng.choice(others, size=deg, replace=False)
        A[i, cols] = rng.uniform(0.1, 1.0, size=deg).astype(np.float32)
    A[:, 1] = 0.0
    A[N - 2, :] = 0.0
    return torch.from_numpy(A)


@functools.lru_cache(maxsize=None)
def dual_graph(N, K):
    return SupportGenerator("dual_random_walk", K).process_csr(directed_adj(N))


def row_counts(csr):
    """nnz per row of the four CSR arrays: G_f, G_f^T, G_b, G_b^T."""
    return [torch.diff(rp).tolist() for rp in
            (csr.row_ptr, csr.row_ptr_t, csr.dual.row_ptr, csr.dual.row_ptr_t)]


@functools.lru_cache(maxsize=None)
def dual_reference(case, dtype, swap=False):
    """swap=True is the direction-swap case: no activation, the backward-half
    rows of W at 1/8 of the forward half's magnitude; extra["W_swapped"] has
    the two halves exchanged."""
    N, B, cin, cout, K = case
    csr = dual_graph(N, K)
    g = lo._gen("dual", case)
    inputs = {
        "x": torch.randn(B, N, cin, generator=g).to(dtype),
        "W": (torch.randn(csr.K_supports * cin, cout, generator=g) * 0.15).to(dtype),
        "b": (torch.randn(cout, generator=g) * 0.1).to(dtype),
    }
    extra = {"csr": csr}
    if swap:
        W = inputs["W"]
        W[(K + 1) * cin:] *= 0.125                    # exact in bf16 and f16
        extra["W_swapped"] = torch.cat(
            [W[:cin], W[(K + 1) * cin:], W[cin:(K + 1) * cin]])
    dense = csr.dense_supports()

    def fn(t):
        return ref.gconv_mix_dense(dense.to(t["x"].dtype), t["x"], t["W"],
                                   t["b"], None if swap else "relu")

    return lo.make_reference(fn, inputs, ("x", "W", "b"), dtype, extra=extra)


DUAL_SWAP_CASE = (33, 2, 64, 64, 2)


def all_dual_references():
    """(label, Reference) for every bf16/f16 case the GPU module judges with
    a floor-derived bound."""
    for dt in lo.LOWP:
        for c in DUAL_CASES:
            yield f"dual {c} {lo.dtype_name(dt)}", dual_reference(c, dt)
        yield (f"dual-swap {DUAL_SWAP_CASE} {lo.dtype_name(dt)}",
               dual_reference(DUAL_SWAP_CASE, dt, True))
    yield (f"dual-stack {DUAL_STACK_K4} bf16",
           dual_reference(DUAL_STACK_K4, lo.BF16))


if __name__ == "__main__":
    # python tests/_dual_oracle.py: the floor rows of docs/TESTING.md
    for label, r in all_dual_references():
        worst = max((k for k in r.floor if k != "out"), key=lambda k: r.floor[k])
        print(f"| {label} | {r.floor['out']:.4f} | {r.tol('out'):.4f} | "
              f"{r.floor[worst]:.4f} ({worst}) | {r.tol(worst):.4f} |")
