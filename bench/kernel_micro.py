"""Standalone kernel microbenchmarks (GPU) — per-kernel wall time via HIP
events, for tuning without running the whole model.

Usage: python bench/kernel_micro.py [--kernel lstm_wgrad|atb_wgrad|lstm|dual_gconv|cheb|all]
Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def timeit(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def bench_lstm_wgrad(C):
    # bench-1024 shape: S = 32*1024, T = 8, L = 3, cin = 1
    S, T, L, H = 32 * 1024, 8, 3, 64
    S_pad = (S + 63) // 64 * 64
    R = T * S_pad
    dA = torch.randn(L, T, S_pad, 4 * H, device="cuda", dtype=torch.bfloat16)
    hseq = torch.randn(L, T, S_pad, H, device="cuda", dtype=torch.bfloat16)
    x = torch.randn(S, T, 1, device="cuda", dtype=torch.bfloat16)
    us = timeit(lambda: C.lstm_wgrad(dA, hseq, x))
    gb = (dA.numel() + hseq.numel() + x.numel()) * 2 / 1e9
    print(json.dumps({"kernel": "lstm_wgrad", "us": round(us, 1),
                      "eff_tb_s": round(gb / (us * 1e-6) / 1e3, 2)}))


def bench_atb(C):
    for rows, M, N in [(32768, 192, 64), (32768, 24, 8)]:
        A = torch.randn(rows, M, device="cuda", dtype=torch.bfloat16)
        B = torch.randn(rows, N, device="cuda", dtype=torch.bfloat16)
        us = timeit(lambda: C.atb_wgrad(A, B, True))
        gb = (A.numel() + B.numel()) * 2 / 1e9
        print(json.dumps({"kernel": f"atb_{M}x{N}", "us": round(us, 1),
                          "eff_tb_s": round(gb / (us * 1e-6) / 1e3, 2)}))
        # library comparison
        us2 = timeit(lambda: (A.float().T @ B.float(), B.sum(0)))
        print(json.dumps({"kernel": f"atb_{M}x{N}_torch", "us": round(us2, 1)}))


def bench_lstm(C):
    from stmgcn_amd.ops.hip_ops import FusedLSTMFn
    S, T, L = 32 * 1024, 8, 3
    x = torch.randn(S, T, 1, device="cuda", dtype=torch.bfloat16)
    ws = []
    for l in range(L):
        in_l = 1 if l == 0 else 64
        ws += [torch.randn(256, in_l, device="cuda", dtype=torch.bfloat16) * 0.1,
               torch.randn(256, 64, device="cuda", dtype=torch.bfloat16) * 0.1,
               torch.randn(256, device="cuda", dtype=torch.bfloat16) * 0.1,
               torch.randn(256, device="cuda", dtype=torch.bfloat16) * 0.1]
    us = timeit(lambda: FusedLSTMFn.apply(x, "lstm", False, False, *ws), iters=30)
    print(json.dumps({"kernel": "lstm_fwd_infer", "us": round(us, 1)}))

    def train_step():
        xg = x.clone().requires_grad_(True)
        wsg = [w.clone().requires_grad_(True) for w in ws]
        out = FusedLSTMFn.apply(xg, "lstm", False, True, *wsg)
        out.float().square().sum().backward()
    us = timeit(train_step, iters=20, warmup=5)
    print(json.dumps({"kernel": "lstm_fwd_bwd_wgrad", "us": round(us, 1)}))


def bench_dual_gconv(C):
    """Fused dual random-walk gconv fwd+bwd at the bench-1024 gconv shape on
    a directed graph, next to the fused chebyshev K=2 gconv on a graph of the
    same nnz per row (the yardstick: 1 generator, 3 supports)."""
    import numpy as np
    from stmgcn_amd.data.synthetic import _random_sparse_directed_adj
    from stmgcn_amd.graph import SupportGenerator
    from stmgcn_amd.ops.hip_ops import ChebGconvFn
    B, N, Cin, Cout, K = 32, 1024, 64, 64, 2
    A = torch.from_numpy(_random_sparse_directed_adj(
        N, 9, np.random.default_rng(0)))
    dual = SupportGenerator("dual_random_walk", K).process_csr(A).to("cuda")
    # chebyshev wants a symmetric adjacency: symmetrizing 4 out-edges + ring
    # gives ~10 nnz per generator row, as 9 out-edges + ring do per direction
    A2 = torch.from_numpy(_random_sparse_directed_adj(
        N, 4, np.random.default_rng(1)))
    cheb = SupportGenerator("chebyshev", K).process_csr(
        torch.maximum(A2, A2.T)).to("cuda")
    res = {}
    for name, csr in (("dual_gconv", dual), ("cheb_gconv_k2", cheb)):
        x = torch.randn(B, N, Cin, device="cuda", dtype=torch.bfloat16,
                        requires_grad=True)
        W = (torch.randn(csr.K_supports * Cin, Cout, device="cuda",
                         dtype=torch.bfloat16) * 0.1).requires_grad_(True)
        b = torch.zeros(Cout, device="cuda", dtype=torch.bfloat16,
                        requires_grad=True)
        dy = torch.randn(B, N, Cout, device="cuda", dtype=torch.bfloat16)

        def step():
            y = ChebGconvFn.apply(x, W, b, csr, "relu", True)
            torch.autograd.grad(y, (x, W, b), dy)
        res[name] = timeit(step, iters=300, warmup=30)
        nnz = [csr.nnz] + ([csr.dual.nnz] if csr.dual is not None else [])
        print(json.dumps({"kernel": name + "_fwd_bwd", "us": round(res[name], 1),
                          "supports": csr.K_supports,
                          "nnz_per_row": [round(z / N, 2) for z in nnz]}))
    print(json.dumps({"kernel": "dual_over_cheb_ratio",
                      "ratio": round(res["dual_gconv"] / res["cheb_gconv_k2"], 3)}))


def bench_cheb(C):
    """Fused ChebConv at the bench-1024 gconv shape (B = 32, N = 1024,
    C = Cout = 64, bf16, K_s = 3, training) on the preset's three graphs:
    forward, then dX + the finishing wgrad, as the train step runs them.
    This is the case the SQ wait counters of cheb_fused_fwd / cheb_fused_bwd /
    atb_wgrad are collected on."""
    from stmgcn_amd import PRESETS
    from stmgcn_amd.data.synthetic import make_synthetic_dataset
    from stmgcn_amd.graph import SupportGenerator
    from stmgcn_amd.ops.hip_ops import ChebGconvFn
    cfg = PRESETS["bench-1024"]
    B, N, Cin, Cout = cfg.batch_size, cfg.n_nodes, 64, 64
    raw = make_synthetic_dataset(n_nodes=N, n_steps=64, m_graphs=cfg.m_graphs,
                                 seed=7, day_timesteps=1)
    gen = SupportGenerator(cfg.kernel_type, cfg.cheby_K, cfg.lambda_max_mode)
    for key in [k for k in raw if k.endswith("_adj")]:
        csr = gen.process_csr(torch.from_numpy(raw[key]).float()).to("cuda")
        x = torch.randn(B, N, Cin, device="cuda", dtype=torch.bfloat16,
                        requires_grad=True)
        W = (torch.randn(csr.K_supports * Cin, Cout, device="cuda",
                         dtype=torch.bfloat16) * 0.1).requires_grad_(True)
        b = torch.zeros(Cout, device="cuda", dtype=torch.bfloat16,
                        requires_grad=True)
        dy = torch.randn(B, N, Cout, device="cuda", dtype=torch.bfloat16)

        def fwd():
            with torch.no_grad():
                ChebGconvFn.apply(x, W, b, csr, "relu", True)

        def step():
            y = ChebGconvFn.apply(x, W, b, csr, "relu", True)
            torch.autograd.grad(y, (x, W, b), dy)
        us_f = timeit(fwd, iters=200, warmup=20)
        us_s = timeit(step, iters=200, warmup=20)
        print(json.dumps({"kernel": "cheb_gconv_" + key, "fwd_us": round(us_f, 1),
                          "fwd_bwd_us": round(us_s, 1),
                          "supports": csr.K_supports,
                          "nnz_per_row": round(csr.nnz / N, 2)}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--kernel", default="all")
    args = p.parse_args()
    from stmgcn_amd.ops.functional import require_hip
    C = require_hip()
    if args.kernel in ("lstm_wgrad", "all"):
        bench_lstm_wgrad(C)
    if args.kernel in ("atb_wgrad", "all"):
        bench_atb(C)
    if args.kernel in ("lstm", "all"):
        bench_lstm(C)
    if args.kernel in ("dual_gconv", "all"):
        bench_dual_gconv(C)
    if args.kernel in ("cheb", "all"):
        bench_cheb(C)


if __name__ == "__main__":
    main()
