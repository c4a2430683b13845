"""Cases and float64 references of the multi-step horizon tests: the wide head
(test_horizon_head_gpu.py), the masked loss (test_masked_loss_gpu.py) and the
floor-against-cap check on the CPU (test_horizon.py).

Judged by the rule of _lowp_oracle: inputs rounded once to the dtype, oracle =
the reference_impl function in float64 on the CPU, metric
max|got - ref| / (max|ref| + 1e-6) per tensor, bound
min(max(3 floor, 2 eps), cap) with cap 0.05 for outputs and 0.08 for
gradients. The head's loss is sum(out^2); the loss tests use the upstream
gradient 3.0 of mse_reference.
"""
from __future__ import annotations

import functools

import torch

import _lowp_oracle as lo
from stmgcn_amd.ops import reference_impl as ref

# Wide head: (B, N, G, M, O), O = horizon * C output columns
HEAD_MULTI_CASES = [
    (2, 25, 8, 1, 3),
    (2, 25, 40, 2, 12),
    (2, 25, 64, 3, 24),
    (2, 25, 64, 3, 32),     # both column tiles full
    (1, 1, 64, 3, 2),       # a single row
    (2, 515, 40, 3, 12),    # 1030 rows: five wgrad chunks, a 6-row tile tail
    (3, 11, 24, 2, 7),      # O odd, 33 rows
]


def head_multi_inputs(case):
    """Same scales as _lowp_oracle.head_inputs. The single-row case has two
    outputs, each a sum of 64 products of magnitude ~0.5 (typical |out| ~ 4):
    a draw in which they cancel to a few tenths has an all-bf16 floor above
    cap / 3, where the cap and not the floor would decide. This key's draw has
    out = (-3.5, 8.7); test_horizon.py asserts 3 floor <= cap for every case."""
    B, N, G, M, O = case
    g = lo._gen("horizon_head", case)
    d = {f"f{m}": torch.randn(B, N, G, generator=g) for m in range(M)}
    d["w"] = torch.randn(O, G, generator=g) * 0.3
    d["b"] = torch.randn(O, generator=g) * 0.1
    return d


@functools.lru_cache(maxsize=None)
def head_multi_reference(case, dtype):
    inputs = {k: v.to(dtype) for k, v in head_multi_inputs(case).items()}
    return lo.make_reference(lo.head_oracle, inputs, tuple(inputs), dtype)


# Masked loss: kind x numel. About 30 % of the targets are NaN for numel > 1;
# pred ~ 1.5 N(0,1) so that Huber sees |d| < 1 and |d| >= 1.
LOSS_KINDS = ("mse", "mae", "huber")
LOSS_NUMELS = [1, 257, 70001]
LOSS_UPSTREAM = lo.MSE_UPSTREAM
NAN_FRACTION = 0.3


def loss_inputs(n, dtype, nan_fraction=NAN_FRACTION):
    g = lo._gen("masked_loss", n)
    pred = (1.5 * torch.randn(n, generator=g)).to(dtype)
    tgt = torch.randn(n, generator=g).to(dtype)
    if n > 1 and nan_fraction > 0:
        tgt[torch.rand(n, generator=g) < nan_fraction] = float("nan")
    return {"pred": pred, "tgt": tgt}


@functools.lru_cache(maxsize=None)
def loss_reference(kind, n, dtype, nan_fraction=NAN_FRACTION):
    inputs = loss_inputs(n, dtype, nan_fraction)

    def run(dt):
        p = inputs["pred"].to(dt).requires_grad_(True)
        loss = ref.masked_loss(p, inputs["tgt"].to(dt), kind)
        (d,) = torch.autograd.grad(loss * LOSS_UPSTREAM, p)
        return {"out": loss.detach(), "dpred": d}

    want, low = run(torch.float64), run(dtype)
    floor = {k: lo.relerr(low[k], want[k]) for k in want}
    return lo.Reference(dtype, inputs, want, floor,
                        {"out": lo.CAP_OUT, "dpred": lo.CAP_GRAD})


def all_horizon_references():
    """(label, Reference) for every bf16/f16 case of the two GPU modules."""
    for dt in lo.LOWP:
        n = lo.dtype_name(dt)
        for c in HEAD_MULTI_CASES:
            yield f"head-multi {c} {n}", head_multi_reference(c, dt)
        for kind in LOSS_KINDS:
            for numel in LOSS_NUMELS:
                yield (f"masked-{kind} {numel} {n}",
                       loss_reference(kind, numel, dt))


if __name__ == "__main__":
    # python tests/_horizon_oracle.py: the floor rows of docs/TESTING.md
    for label, r in all_horizon_references():
        worst = max((k for k in r.floor if k != "out"), key=lambda k: r.floor[k])
        print(f"| {label} | {r.floor['out']:.4f} | {r.tol('out'):.4f} | "
              f"{r.floor[worst]:.4f} ({worst}) | {r.tol(worst):.4f} |")
