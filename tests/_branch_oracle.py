"""Cases and float64 references of one model branch, the composition the
deep variant runs from its second block on: CG_LSTM (seqsum -> temporal
gconv -> contextual gate, node-major -> fused RNN) followed by its GCN,
reshaped as STMGCNBlock / ST_MGCN do (test_branch_composite_gpu.py on the
GPU, test_lowp_bounds.py for the floors on the CPU).

Judged by the rule of _lowp_oracle. The modules' parameters and obs are
rounded to the dtype once. The oracle takes a deep copy of the same modules
to float64 on the CPU and runs reference_branch over csr.dense_supports():
the modules' parameters, but not their forward methods -- the composition is
written out again from the reference_impl functions, so a mistake in the
wiring of CG_LSTM.forward (a detached x_seq, say) is not mirrored by the
oracle. The floor is another copy run the same way entirely in the
low-precision dtype on the CPU. Metric, per tensor,
max|got - ref| / (max|ref| + 1e-6); bound min(max(3 floor, 2 eps), cap).

``python tests/_branch_oracle.py --print`` prints the floor rows of
docs/TESTING.md, ``--find-seeds`` the draw each case uses (BRANCH_SEEDS).
"""
from __future__ import annotations

import copy
import functools
import sys

import torch

import _lowp_oracle as lo
from stmgcn_amd.models.stmgcn import CG_LSTM, GCN
from stmgcn_amd.ops import reference_impl as ref

G = 64      # gcn_hidden_dim: a block's output width, the next block's C
# (B, T, N, C, L, cell, ret_seq, K)
BRANCH_CASES = [
    (2, 8, 33, 1, 2, "lstm", False, 2),   # ST_MGCN's branch; fused temporal gconv (T = 8)
    (1, 8, 50, 1, 2, "gru", True, 2),     # block 1 of the deep variant
    (2, 4, 33, 64, 2, "gru", True, 2),    # block 2..n: C = 64, dobs, gate chunk splits node 16
    (2, 4, 33, 64, 2, "lstm", True, 2),
    (2, 3, 40, 64, 1, "gru", True, 3),    # odd T, four supports, one layer
]
# eval forward == training forward, bit for bit
EVAL_CASES = [c for c in BRANCH_CASES if c[3] == 64 and c[4] == 2]

# Which draw of weights and obs each case uses. Two ReLUs of a branch feed
# gradients that do not vanish at the kink: the temporal gconv's (B*N*T
# elements, a few hundred here; its incoming gradient dg is one value per
# (b, t)) and the one inside the gate's tied FC (B*T elements). Where a
# pre-activation lies within rounding of zero, its mask is a coin toss between
# two correct implementations, and one flipped element moves the
# few-hundred-row gradients behind it (temporal gconv W / b, fc, dobs) by
# 0.03 to 0.2 of their maximum -- in f16 as in bf16, on the CPU floor run as
# on the GPU. Such a draw measures the toss, not the kernels. A draw is
# therefore used only if, in the float64 oracle, every pre-activation p of
# both ReLUs has
#     |p| > EPS[bf16] * (sum of the absolute values of p's terms)
# (relu_margin below), and if 3 x floor is under the cap for every tensor in
# both dtypes. EPS is two half-ulp roundings of every term: the two stores
# that separate a kernel's pre-activation from the oracle's on the same
# rounded inputs, x_seq and the support stack T_k x_seq (the accumulators are
# fp32), all errors taken with the same sign. The seed is the first one from
# 0 that qualifies (``--find-seeds`` recomputes them); test_lowp_bounds.py
# asserts both conditions. Nothing measured on a GPU enters the choice.
BRANCH_SEEDS = dict(zip(BRANCH_CASES, (74, 31, 8, 0, 1)))
RELU_MARGIN = lo.EPS[lo.BF16]


def branch_graph(case):
    return lo.csr_graph(n=case[2], K=case[7])


def build_branch(case, seed):
    """fp32 modules of one branch, seeded by the case. Both gconv biases are
    non-zero: their zero initialisation would hide a dropped bias."""
    B, T, N, C, L, cell, ret_seq, K = case
    g = lo._gen("branch", case, seed)
    torch.manual_seed(int(g.initial_seed()) % (2 ** 31))
    rnn = CG_LSTM(K + 1, T, C, lo.H, L, cell=cell)
    gcn = GCN(K + 1, lo.H, G)
    with torch.no_grad():
        rnn.gconv_temporal_feats.b.copy_(torch.randn(T, generator=g) * 0.1)
        gcn.b.copy_(torch.randn(G, generator=g) * 0.1)
    return rnn, gcn


def run_branch(rnn, gcn, adj, obs, ret_seq):
    """One branch as STMGCNBlock.forward (ret_seq) / ST_MGCN.forward run it."""
    B, T, N, _ = obs.shape
    h = rnn(adj, obs, return_sequences=ret_seq)
    if not ret_seq:
        return gcn(adj, h)                                   # (B, N, G)
    flat = h.reshape(B * T, N, h.shape[-1])
    return gcn(adj, flat).reshape(B, T, N, -1)               # (B, T, N, G)


def reference_branch(rnn, gcn, dense, obs, ret_seq):
    """The same branch from the modules' parameters alone, composed of the
    reference_impl functions over a dense (K, N, N) support stack."""
    B, T, N, C = obs.shape
    tg = rnn.gconv_temporal_feats
    x_seq = obs.sum(dim=-1).permute(0, 2, 1)                          # (B,N,T)
    g = ref.gconv_mix_dense(dense, x_seq, tg.W, tg.b, tg.activation)
    gated = ref.contextual_gate(obs, g, rnn.fc.weight, rnn.fc.bias)   # (B,T,N,C)
    flat = gated.permute(0, 2, 1, 3).reshape(B * N, T, C)
    ws = rnn.lstm.flat_weights()
    h0 = obs.new_zeros(rnn.num_layers, B * N, rnn.hidden_dim)
    if rnn.cell == "lstm":
        h = ref.lstm_forward(flat, ws, h0, h0.clone(), ret_seq)
    else:
        h = ref.gru_forward(flat, ws, h0, ret_seq)
    if not ret_seq:
        return ref.gconv_mix_dense(dense, h.reshape(B, N, -1), gcn.W, gcn.b,
                                   gcn.activation)
    seq = h.reshape(B, N, T, -1).permute(0, 2, 1, 3).reshape(B * T, N, -1)
    return ref.gconv_mix_dense(dense, seq, gcn.W, gcn.b,
                               gcn.activation).reshape(B, T, N, -1)


def param_names(rnn, gcn):
    return ([f"d rnn.{n}" for n, _ in rnn.named_parameters()]
            + [f"d gcn.{n}" for n, _ in gcn.named_parameters()])


def fwd_bwd(rnn, gcn, adj, obs, ret_seq, want_dobs, forward=run_branch):
    """loss = sum(out.float()^2) (float64 for the oracle). Returns
    {"out", "dobs" if want_dobs, "d rnn.<param>", "d gcn.<param>"}."""
    obs = obs.detach().clone().requires_grad_(want_dobs)
    for p in list(rnn.parameters()) + list(gcn.parameters()):
        p.grad = None
    out = forward(rnn, gcn, adj, obs, ret_seq)
    acc = torch.float64 if out.dtype == torch.float64 else torch.float32
    (out.to(acc) ** 2).sum().backward()
    res = {"out": out.detach()}
    if want_dobs:
        res["dobs"] = obs.grad
    for name, (_, p) in zip(param_names(rnn, gcn),
                            list(rnn.named_parameters())
                            + list(gcn.named_parameters())):
        assert p.grad is not None, name
        res[name] = p.grad
    return res


def _cap(name, dtype):
    if name == "out":
        return lo.CAP_OUT
    if dtype == lo.F16 and name.startswith("d rnn.lstm."):
        return lo.CAP_GRAD_RNN_F16
    return lo.CAP_GRAD


def relu_margin(rnn, dense, obs):
    """min over both gradient-carrying ReLUs (temporal gconv, gate FC) of
    |pre-activation| / (sum of |terms|), in float64."""
    rnn, dense, obs = copy.deepcopy(rnn).double(), dense.double(), obs.double()
    with torch.no_grad():
        tg = rnn.gconv_temporal_feats
        xs = obs.sum(-1).permute(0, 2, 1)
        feat = torch.cat([torch.einsum("ij,bjp->bip", dense[k], xs)
                          for k in range(dense.shape[0])], dim=-1)
        pre = feat @ tg.W + tg.b
        mag = feat.abs() @ tg.W.abs() + tg.b.abs()
        z = (torch.relu(pre) + xs).mean(dim=1)
        fw, fb = rnn.fc.weight, rnn.fc.bias
        pre_u = z @ fw.T + fb
        mag_u = z.abs() @ fw.abs().T + fb.abs()
        return min((pre.abs() / mag).min().item(),
                   (pre_u.abs() / mag_u).min().item())


def _draw(case, dtype, seed):
    B, T, N, C = case[:4]
    rnn, gcn = build_branch(case, seed)
    rnn, gcn = rnn.to(dtype), gcn.to(dtype)                  # rounded once
    g = lo._gen("branch-obs", case, seed)
    obs = torch.randn(B, T, N, C, generator=g)
    obs = (obs * 0.5 if C > 1 else obs).to(dtype)
    return rnn, gcn, obs


@functools.lru_cache(maxsize=None)
def branch_reference(case, dtype, seed=None):
    """extra: "csr", "modules" = the (rnn, gcn) holding the rounded parameter
    values (deep-copy before use), and "relu_margin"."""
    B, T, N, C, L, cell, ret_seq, K = case
    csr = branch_graph(case)
    rnn, gcn, obs = _draw(case, dtype,
                          BRANCH_SEEDS[case] if seed is None else seed)
    dense = csr.dense_supports()
    want_dobs = C > 1

    def run(dt):
        r, c = copy.deepcopy(rnn).to(dt), copy.deepcopy(gcn).to(dt)
        return fwd_bwd(r, c, dense.to(dt), obs.to(dt), ret_seq, want_dobs,
                       forward=reference_branch)

    want, low = run(torch.float64), run(dtype)
    floor = {k: lo.relerr(low[k], want[k]) for k in want}
    cap = {k: _cap(k, dtype) for k in want}
    return lo.Reference(dtype, {"obs": obs}, want, floor, cap,
                        extra={"csr": csr, "modules": (rnn, gcn),
                               "relu_margin": relu_margin(rnn, dense, obs)})


def find_seed(case, limit=20000):
    """First seed whose draw is clear of both kinks and keeps 3 x floor under
    the cap, in both dtypes."""
    dense = branch_graph(case).dense_supports()
    for seed in range(limit):
        draws = [_draw(case, dt, seed) for dt in lo.LOWP]
        if any(relu_margin(rnn, dense, obs) <= RELU_MARGIN
               for rnn, _, obs in draws):
            continue
        refs = [branch_reference(case, dt, seed) for dt in lo.LOWP]
        if all(3.0 * fl <= r.cap[k] for r in refs for k, fl in r.floor.items()):
            return seed
    raise RuntimeError(f"no seed below {limit} for {case}")


def all_branch_references():
    for dt in lo.LOWP:
        for c in BRANCH_CASES:
            yield f"branch {c} {lo.dtype_name(dt)}", branch_reference(c, dt)


if __name__ == "__main__":
    if sys.argv[1:] == ["--find-seeds"]:
        for c in BRANCH_CASES:
            print(f"    {c}: {find_seed(c)},", flush=True)
        sys.exit(0)
    if sys.argv[1:] != ["--print"]:
        sys.exit("usage: python tests/_branch_oracle.py --print | --find-seeds")
    for label, r in all_branch_references():
        worst = max((k for k in r.floor if k != "out"), key=lambda k: r.floor[k])
        print(f"| {label} | {r.floor['out']:.4f} | {r.tol('out'):.4f} | "
              f"{r.floor[worst]:.4f} ({worst}) | {r.tol(worst):.4f} |")
