"""The train step as it is benchmarked: M branches on their own HIP streams,
the whole step (forward, fused MSE, backward, gradient gather, FusedAdam)
captured once and replayed, the bias correction advancing on the device.
Every kernel test runs eagerly on one stream; this module runs the same step
in three modes and compares them:

  (i)   eager, STMGCN_DETERMINISTIC=1 (one stream) -- the serialized twin,
  (ii)  eager, one stream per branch,
  (iii) ModelTrainer(use_graph=True): two eager steps (the second on a side
        stream, followed by the capture), then replays (ST_MGCN only, see
        REPLAY_MODELS).

Each mode has its own deep copy of the model and its own FusedAdam. Before
every step the serialized twin's optimizer state (master, m, v, hyper, and
with them the arena) is copied into the other two, so every step is compared
from identical state, and every step gets a batch of its own, so a replay
that read a stale batch would miss on the loss.

Tiny shapes (N = 33; B = 2 for ST_MGCN, B = 1 for the stacked model): every
fp32 reduction has at most two partials, and two partials added atomically
to zero give the same sum in either order, so the three modes agree bit for
bit on the loss, the output, the whole grad_arena and arena / master / m / v
after the step. The partial counts, from the launch code:
  atb_wgrad (gconv dW / db)   ceil(rows / 128) workgroups; rows = B*N = 66,
                              or B*T*N = 132 for the stacked model's
                              post-RNN gconv: 1 or 2
  lstm_wgrad                  ceil(T * S_pad / 1024) = 1
  gate forward / backward     ceil(N / 2048) = 1, ceil(N*C / 2048) <= 2
                              (N*C = 2112 in the stacked model's block 2)
  head_wgrad                  ceil(B*N / 256) = 1
  mse_fwd                     ceil(numel / 256) = 1
The stacked model's final nn.Linear and its T = 4 temporal gconv (C_in = 4
takes the support-stack path) run library GEMMs; they are held to the same
equality.

Chunked shape (B = 4, N = 200): several arrivers per ticket while the
branches run concurrently. The forward is still deterministic (one gate
forward chunk), so the output stays bit-equal; the loss has four partials and
is held to 4 ulp of fp32. The atomically summed gradients may differ between
modes by fp32 reassociation, so each parameter's segment of grad_arena is held
to max|a - b| <= 2 * EPS[dtype] * max|a| -- one ulp at the top binade. (The
gate's backward sums ds the same way, over N*C / 2048 = 7 chunks in the
stacked model's block 2, so dg and dobs there, and the gradients behind them,
fall under the same rule and not under bit equality.)

Under replay the Adam update is recomputed on the CPU from the pre-step state
and the step's own gradients, with the bias-correction powers advanced in
fp32 as adam_prep_kernel does.
"""
import copy

import pytest
import torch

import _lowp_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, WD = 5e-3, 1e-4
N_STEPS = 5             # steps 0, 1 of mode (iii) are eager, 2.. are replays

MODELS = {
    "st_mgcn": dict(dtype=lo.BF16, cfg=dict(
        seq_len=8, m_graphs=3, lstm_num_layers=2, rnn_cell="lstm", n_blocks=1)),
    "stacked": dict(dtype=lo.F16, cfg=dict(
        seq_len=4, m_graphs=2, lstm_num_layers=2, rnn_cell="gru", n_blocks=2)),
}
# Models whose step is also captured and replayed. The stacked model is not
# among them: the first replay of its captured step (B = 4, N = 200) ended the
# process with a segmentation fault inside the HIP runtime's graph launch in
# one of two runs, the other run and both runs at B = 1, N = 33 passed, and the
# cause is not known. Its graph differs from ST_MGCN's in nesting two
# fork/join blocks and in holding library GEMMs (the T = 4 temporal gconv's
# support-stack path, the final nn.Linear) on the branch streams. Until the
# cause is found the stacked model runs modes (i) and (ii) only.
REPLAY_MODELS = ("st_mgcn",)
# (B, N) per model
SHAPES = {
    "tiny": {"st_mgcn": (2, 33), "stacked": (1, 33)},
    "chunked": {"st_mgcn": (4, 200), "stacked": (4, 200)},
}


def _setup(model_key, shape_key):
    from stmgcn_amd.config import STMGCNConfig
    from stmgcn_amd.models import build_model
    B, N = SHAPES[shape_key][model_key]
    spec = MODELS[model_key]
    cfg = STMGCNConfig(n_nodes=N, cheby_K=2, **spec["cfg"])
    torch.manual_seed(11)
    base = build_model(cfg).to(spec["dtype"])           # CPU, rounded once
    csr = [lo.csr_graph(n=N, seed=m, K=2) for m in range(cfg.m_graphs)]
    g = lo._gen("modes", model_key, shape_key)
    n_batches = N_STEPS + 2
    xs = torch.randn(n_batches, B, cfg.seq_len, N, 1, generator=g).to(spec["dtype"])
    ys = torch.randn(n_batches, B, N, 1, generator=g).to(spec["dtype"])
    return base, csr, xs, ys, spec["dtype"]


class _Twin:
    """One mode: its model copy, its trainer (which owns the FusedAdam) and
    the output of its last forward."""

    def __init__(self, base, use_graph):
        from stmgcn_amd.ops import mse_loss
        from stmgcn_amd.train import FusedAdam, ModelTrainer
        self.model = copy.deepcopy(base).to(DEV)
        self.model.train()
        self.tr = ModelTrainer(model=self.model, loss=mse_loss,
                               optimizer=FusedAdam, lr=LR, wd=WD, n_epochs=1,
                               use_graph=use_graph)
        self.opt = self.tr.optimizer
        self.eager_out = self.graph_out = None
        self.model.register_forward_hook(self._keep)

    def _keep(self, module, args, output):
        # detach(): a view without autograd history. The one taken during the
        # capture keeps the output's block of the graph's pool from being
        # reused, so after a replay it holds that replay's output.
        if torch.cuda.is_current_stream_capturing():
            self.graph_out = output.detach()
        else:
            self.eager_out = output.detach()

    def step(self, x, y, adjs):
        """Returns (loss, out, grad_arena, state after the step), cloned."""
        replayed = (tuple(x.shape), tuple(y.shape)) in self.tr._graphs
        loss = self.tr._train_step(x, y, adjs)
        torch.cuda.synchronize()
        out = self.graph_out if replayed else self.eager_out
        state = {k: v.clone() for k, v in self.opt.state_dict().items()}
        state["arena"] = self.opt.arena.clone()
        return loss, out.clone(), self.opt.grad_arena.clone(), state

    def segments(self):
        names = [n for n, _ in self.model.named_parameters()]
        assert len(names) == len(self.opt._offsets)
        return list(zip(names, self.opt._offsets, self.opt._lens))


def _adam_expected(pre, grad):
    """The update of adam_kernel in float64 from the pre-step state, with the
    hyper row advanced in fp32 as adam_prep_kernel does."""
    h = pre["hyper"].float().cpu()
    one = torch.tensor(1.0, dtype=torch.float32)
    b1pow, b2pow = h[7] * h[1], h[8] * h[2]              # fp32 products
    bc1, bc2 = one - b1pow, one - b2pow                   # fp32
    hyper = h.clone()
    hyper[5], hyper[6], hyper[7], hyper[8] = bc1, bc2, b1pow, b2pow
    lr, b1, b2, eps, wd = (float(h[i]) for i in range(5))
    p = pre["master"].double().cpu()
    g = grad.double().cpu() + wd * p
    m = b1 * pre["m"].double().cpu() + float(one - h[1]) * g
    v = b2 * pre["v"].double().cpu() + float(one - h[2]) * g * g
    pn = p - lr * (m / float(bc1)) / (torch.sqrt(v / float(bc2)) + eps)
    return {"hyper": hyper, "master": pn, "m": m, "v": v}


def _check_adam(pre, grad, post, dtype, label, bad):
    want = _adam_expected(pre, grad)
    # lr, betas, eps, wd untouched and the two powers exactly the fp32
    # products. bc = 1 - pow: the compiler may contract the product into the
    # subtraction (an fma skips the product's rounding, at most half an ulp of
    # a value below 1, 2^-25), and the difference rounds once more: 2^-24.
    hp, hw = post["hyper"].cpu(), want["hyper"]
    keep = [0, 1, 2, 3, 4, 7, 8]
    if not torch.equal(hp[keep], hw[keep]):
        bad.append(f"{label} hyper {hp.tolist()} != {hw.tolist()}")
    if not ((hp[5:7].double() - hw[5:7].double()).abs() <= 2.0 ** -24).all():
        bad.append(f"{label} bias corrections {hp[5:7].tolist()} != "
                   f"{hw[5:7].tolist()}")
    for k in ("master", "m", "v"):
        got = post[k].double().cpu()
        # the tolerance of test_fused_adam_matches_torch_adam
        err = (got - want[k]).abs() - (1e-6 + 1e-5 * want[k].abs())
        print(f"{label} adam {k}: worst excess over rtol 1e-5 / atol 1e-6 "
              f"{err.max().item():.3e}")
        if not (err <= 0).all():
            bad.append(f"{label} adam {k}: off by {err.max().item():.3e} over "
                       f"the tolerance")
    if not torch.equal(post["arena"], post["master"].to(dtype)):
        bad.append(f"{label} arena != master.to(dtype)")


def _compare(ref_res, res, segs, dtype, exact, loss_exact, label, bad, worst):
    (l0, out0, g0, s0), (l1, out1, g1, s1) = ref_res, res
    if loss_exact:
        if l0 != l1:
            bad.append(f"{label} loss {l1!r} != {l0!r}")
    elif not abs(l0 - l1) <= 4 * 2.0 ** -23 * abs(l0):
        bad.append(f"{label} loss {l1!r} vs {l0!r}: over 4 ulp of fp32")
    if not torch.equal(out0, out1):
        bad.append(f"{label} output differs, max "
                   f"{(out0.float() - out1.float()).abs().max().item():.3e}")
    if exact:
        if not torch.equal(g0, g1):
            diff = [n for n, o, k in segs if not torch.equal(g0[o:o + k], g1[o:o + k])]
            bad.append(f"{label} grad_arena differs in {diff}")
        for k in ("arena", "master", "m", "v", "hyper"):
            if not torch.equal(s0[k], s1[k]):
                bad.append(f"{label} {k} after the step differs")
        return
    for name, o, k in segs:
        a, b = g0[o:o + k].double(), g1[o:o + k].double()
        d, lim = (a - b).abs().max().item(), 2 * lo.EPS[dtype] * a.abs().max().item()
        frac = d / lim if lim > 0 else (0.0 if d == 0 else float("inf"))
        worst[0] = max(worst[0], frac)
        if not d <= lim:
            bad.append(f"{label} grad {name}: max|a-b| {d:.3e} > {lim:.3e}")


@pytest.mark.parametrize("shape_key", list(SHAPES))
@pytest.mark.parametrize("model_key", list(MODELS))
def test_modes_agree_and_adam_advances_under_replay(model_key, shape_key,
                                                    monkeypatch):
    from stmgcn_amd.models.stmgcn import deterministic_mode
    from stmgcn_amd.ops import hip_ops
    base, csr, xs, ys, dtype = _setup(model_key, shape_key)
    adjs = [c.to(DEV) for c in csr]
    xs, ys = xs.to(DEV), ys.to(DEV)
    B = xs.shape[1]
    exact = shape_key == "tiny"
    loss_exact = B * xs.shape[3] <= 512         # at most two mse_fwd blocks

    hip_ops.reset_fallback_count()
    ser, multi = _Twin(base, False), _Twin(base, False)
    replay = _Twin(base, True) if model_key in REPLAY_MODELS else None
    others = [t for t in (multi, replay) if t is not None]
    segs = ser.segments()
    bad, worst = [], [0.0]

    def one_step(i, label, replays):
        pre = {k: v.clone() for k, v in ser.opt.state_dict().items()}
        for t in others:
            t.opt.load_state_dict(pre)                  # arena follows master
        monkeypatch.setenv("STMGCN_DETERMINISTIC", "1")
        assert deterministic_mode()
        r_ser = ser.step(xs[i], ys[i], adjs)
        monkeypatch.delenv("STMGCN_DETERMINISTIC")
        assert not deterministic_mode()
        r_multi = multi.step(xs[i], ys[i], adjs)
        print(f"{label} loss ser {r_ser[0]!r} multi {r_multi[0]!r}")
        _compare(r_ser, r_multi, segs, dtype, exact, loss_exact,
                 f"{label} multi-stream", bad, worst)
        if replay is None:
            return r_ser
        r_replay = replay.step(xs[i], ys[i], adjs)
        print(f"{label} loss replay {r_replay[0]!r}")
        _compare(r_ser, r_replay, segs, dtype, exact, loss_exact,
                 f"{label} {'replay' if replays else 'graph twin, eager'}",
                 bad, worst)
        if replays:
            _check_adam(pre, r_replay[2], r_replay[3], dtype, label, bad)
        return r_ser

    first = None
    for i in range(N_STEPS):
        replays = i >= 2
        r = one_step(i, f"step {i}", replays)
        first = first or r
        if i == 1 and replay is not None:
            assert replay.tr.use_graph and len(replay.tr._graphs) == 1, \
                "the step was not captured"
    assert not ser.tr._graphs and not multi.tr._graphs
    # distinct batches gave distinct losses: the comparison can see a stale one
    assert first[0] != r[0]

    # a ragged batch runs eagerly and must leave the captured graph's buffers
    # alone: the next full-size replay still equals the serialized twin.
    # (B = 1 has no smaller batch.)
    if B > 1 and replay is not None:
        i = N_STEPS
        replay.opt.load_state_dict(ser.opt.state_dict())
        v = replay.tr._train_step(xs[i, :B - 1], ys[i, :B - 1], adjs)
        assert v == v and len(replay.tr._graphs) == 1
        one_step(N_STEPS + 1, "after ragged", True)

    assert hip_ops.fallback_count() == 0
    if not exact:
        print(f"{model_key} {shape_key}: worst gradient difference between "
              f"modes = {worst[0]:.3f} of the bound")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape_key", list(SHAPES))
def test_stacked_model_matches_fp32_cpu(shape_key, monkeypatch):
    """The deep variant's GPU parity check: one serialized f16 train step
    against the same weights in fp32 on the CPU over dense supports, at the
    thresholds of test_full_model_bf16_hip_vs_torch_impl. (The all-f16 CPU
    run of this model is within 0.005 on the output and 0.04 on the fc
    gradients.)"""
    import torch.nn.functional as F
    from stmgcn_amd.ops import hip_ops
    base, csr, xs, ys, dtype = _setup("stacked", shape_key)
    cpu = copy.deepcopy(base).float()
    out_c = cpu(xs[0].float(), [c.dense_supports() for c in csr])
    F.mse_loss(out_c, ys[0].float()).backward()

    monkeypatch.setenv("STMGCN_DETERMINISTIC", "1")
    hip_ops.reset_fallback_count()
    twin = _Twin(base, False)
    _, out_g, grads, _ = twin.step(xs[0].to(DEV), ys[0].to(DEV),
                                   [c.to(DEV) for c in csr])
    assert hip_ops.fallback_count() == 0
    e = lo.relerr(out_g, out_c)
    print(f"stacked {shape_key} out: err {e:.5f}")
    assert e < 0.06
    want = dict(cpu.named_parameters())
    for name, o, k in twin.segments():
        if name.startswith("fc."):
            e = lo.relerr(grads[o:o + k].view_as(want[name]), want[name].grad)
            print(f"stacked {shape_key} d {name}: err {e:.5f}")
            assert e < 0.12, name
