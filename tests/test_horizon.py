"""Multi-step forecast horizon on the CPU: windowing, NaN marking of missing
readings, the widened head's column order, the masked-loss oracle, masked
metrics, the CLI, and the floors of the GPU cases against their caps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _horizon_oracle as ho
import _lowp_oracle as lo
from stmgcn_amd import ops
from stmgcn_amd.config import STMGCNConfig
from stmgcn_amd.data import DataGenerator, DataInput
from stmgcn_amd.data.container import sliding_windows
from stmgcn_amd.models import ST_MGCN, StackedSTMGCN, build_model
from stmgcn_amd.ops import reference_impl as ref
from stmgcn_amd.train.metrics import MAE, MAPE, MSE, RMSE, masked_metrics

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KCONF = {"kernel_type": "chebyshev", "K": 2}


def _series(T=80, N=4, C=2, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(T, N, C)).astype(np.float32)


# ------------------------------------------------------------------ windowing
def test_sliding_windows_horizon_matches_loop():
    data = _series()
    serial, daily, weekly, day_ts, P = 3, 1, 0, 24, 3
    x, y = sliding_windows(data, serial, daily, weekly, day_ts, horizon=P)
    start = max(serial, daily * day_ts, weekly * day_ts * 7)
    anchors = list(range(start, data.shape[0] - P + 1))
    assert anchors[-1] + P - 1 == data.shape[0] - 1      # last step is used
    assert x.shape == (len(anchors), serial + daily, 4, 2)
    assert y.shape == (len(anchors), 4, P, 2)
    for s, a in enumerate(anchors):
        for n in range(4):
            for p in range(P):
                for c in range(2):
                    assert y[s, n, p, c] == data[a + p, n, c]
        want_x = [data[a - daily * day_ts]] + [data[a - k] for k in (3, 2, 1)]
        assert np.array_equal(x[s], np.stack(want_x))
    assert y.flags["C_CONTIGUOUS"]


def test_sliding_windows_horizon_one_is_unchanged():
    data = _series()
    x0, y0 = sliding_windows(data, 3, 1, 1, 2)
    x1, y1 = sliding_windows(data, 3, 1, 1, 2, horizon=1)
    assert x0.shape == x1.shape and y0.shape == y1.shape == (x0.shape[0], 4, 2)
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1)
    start = max(3, 2, 14)
    assert np.array_equal(y0, data[start:])
    gen = DataGenerator(dt=12, obs_len=(3, 1, 1), train_test_dates=["0101", "0110", "0111", "0112"])
    xg, yg = gen.window(data)
    assert np.array_equal(xg, x0) and np.array_equal(yg, y0)
    with pytest.raises(ValueError):
        sliding_windows(data, 3, 1, 1, 2, horizon=0)


def test_null_value_marks_targets_not_inputs():
    raw = np.abs(_series(T=60, N=3, C=1)) + 0.5
    raw[7, 1, 0] = 0.0
    raw[30, 2, 0] = 0.0
    din = DataInput(M_adj=0, data_dir="unused", null_value=0.0)
    data = din.load_dict({"taxi": raw})
    assert not np.isnan(data["taxi"]).any()               # x is left as loaded
    tgt = data["taxi_target"]
    assert np.isnan(tgt).sum() == 2 and np.isnan(tgt[7, 1, 0]) and np.isnan(tgt[30, 2, 0])
    keep = ~np.isnan(tgt)
    assert np.array_equal(tgt[keep], data["taxi"][keep])
    # the marking is decided on the raw values: the normalised null is -1
    assert data["taxi"][7, 1, 0] == -1.0
    # without a null value nothing is added
    plain = DataInput(M_adj=0, data_dir="unused").load_dict({"taxi": raw})
    assert "taxi_target" not in plain

    gen = DataGenerator(dt=12, obs_len=(3, 0, 0), horizon=2,
                        train_test_dates=["0101", "0110", "0111", "0112"])
    loaders = gen.get_data_loader(data, 8, torch.device("cpu"))
    ys = torch.cat([y for _, y in loaders["train"]] + [y for _, y in loaders["validate"]]
                   + [y for _, y in loaders["test"]])
    xs = torch.cat([x for x, _ in loaders["train"]])
    assert ys.shape[1:] == (3, 2, 1) and not torch.isnan(xs).any()
    # raw step 7 is the target of anchor 7 (p = 0) and of anchor 6 (p = 1)
    assert torch.isnan(ys[7 - 3, 1, 0, 0]) and torch.isnan(ys[6 - 3, 1, 1, 0])
    # over all windows, each of the two missing readings is a target twice
    _, y_all = gen.window(data["taxi"], data["taxi_target"])
    assert np.isnan(y_all).sum() == 4
    # NaN survives the casts to the low-precision dtypes
    for dt in lo.LOWP:
        assert torch.equal(torch.isnan(ys.to(dt)), torch.isnan(ys))


# ---------------------------------------------------------------------- model
def _adjs(N, M):
    return [lo.csr_graph(n=N, seed=m, K=2).dense_supports() for m in range(M)]


def test_st_mgcn_horizon_shape_and_column_order():
    torch.manual_seed(0)
    B, T, N, C, P, G = 2, 4, 9, 2, 3, 8
    model = ST_MGCN(M=2, seq_len=T, n_nodes=N, input_dim=C, lstm_hidden_dim=8,
                    lstm_num_layers=1, gcn_hidden_dim=G, sta_kernel_config=KCONF,
                    horizon=P)
    assert model.fc.weight.shape == (P * C, G)
    feats = []
    hook = model.gcn_list[0].register_forward_hook(lambda m, a, o: feats.append(o))
    hook2 = model.gcn_list[1].register_forward_hook(lambda m, a, o: feats.append(o))
    x = torch.randn(B, T, N, C)
    out = model(x, _adjs(N, 2))
    hook.remove(), hook2.remove()
    assert out.shape == (B, N, P, C)
    fused = feats[0] + feats[1]
    for p in range(P):
        rows = slice(p * C, (p + 1) * C)                  # o = p*C + c
        step = F.linear(fused, model.fc.weight[rows], model.fc.bias[rows])
        torch.testing.assert_close(out[:, :, p], step, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        ST_MGCN(M=1, seq_len=T, n_nodes=N, input_dim=C, lstm_hidden_dim=8,
                lstm_num_layers=1, gcn_hidden_dim=G, sta_kernel_config=KCONF,
                horizon=0)


def test_stacked_horizon_shape_and_column_order():
    torch.manual_seed(0)
    B, T, N, C, P, G = 2, 4, 9, 1, 2, 8
    model = StackedSTMGCN(M=2, seq_len=T, n_nodes=N, input_dim=C, lstm_hidden_dim=8,
                          lstm_num_layers=1, gcn_hidden_dim=G,
                          sta_kernel_config=KCONF, n_blocks=2, horizon=P)
    assert model.fc.weight.shape == (P * C, G)
    last = []
    hook = model.fc.register_forward_hook(lambda m, a, o: last.append(a[0]))
    out = model(torch.randn(B, T, N, C), _adjs(N, 2))
    hook.remove()
    assert out.shape == (B, N, P, C)
    for p in range(P):
        rows = slice(p * C, (p + 1) * C)
        step = F.linear(last[0], model.fc.weight[rows], model.fc.bias[rows])
        torch.testing.assert_close(out[:, :, p], step, rtol=1e-5, atol=1e-6)


def test_horizon_one_keeps_state_dict_schema_and_shape():
    with open(os.path.join(REPO, "tests", "golden",
                           "reference_state_dict_schema.json")) as f:
        schema = json.load(f)
    cfg = STMGCNConfig()
    assert cfg.horizon == 1 and cfg.null_value is None
    model = build_model(cfg)
    keys = schema["keys"] if isinstance(schema, dict) and "keys" in schema else schema
    names = [k if isinstance(k, str) else k[0] for k in keys]
    assert sorted(model.state_dict().keys()) == sorted(names)
    wide = build_model(cfg.replace(horizon=4))
    assert sorted(wide.state_dict().keys()) == sorted(names)
    assert wide.fc.weight.shape == (4 * cfg.input_dim, cfg.gcn_hidden_dim)
    N = 9
    small = build_model(cfg.replace(n_nodes=N, m_graphs=1, lstm_num_layers=1))
    out = small(torch.randn(2, cfg.seq_len, N, 1), _adjs(N, 1))
    assert out.shape == (2, N, 1)                          # not (B, N, 1, C)


# ---------------------------------------------------------------- masked loss
@pytest.mark.parametrize("kind,torch_loss", [
    ("mse", F.mse_loss), ("mae", F.l1_loss), ("huber", F.smooth_l1_loss)])
def test_masked_loss_without_nan_is_the_torch_loss(kind, torch_loss):
    g = lo._gen("masked-cpu", kind)
    pred = (1.5 * torch.randn(4, 7, 3, dtype=torch.float64, generator=g)).requires_grad_(True)
    tgt = torch.randn(4, 7, 3, dtype=torch.float64, generator=g)
    got = ref.masked_loss(pred, tgt, kind)
    (dg,) = torch.autograd.grad(got, pred)
    p2 = pred.detach().clone().requires_grad_(True)
    want = torch_loss(p2, tgt)
    (dw,) = torch.autograd.grad(want, p2)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(dg, dw, rtol=1e-12, atol=1e-14)
    # the dispatcher takes the same path on the CPU
    torch.testing.assert_close(ops.masked_loss(pred, tgt, kind), got, rtol=0, atol=0)


@pytest.mark.parametrize("kind", ho.LOSS_KINDS)
def test_masked_loss_masks_and_stays_finite(kind):
    g = lo._gen("masked-cpu-nan", kind)
    pred = (1.5 * torch.randn(300, dtype=torch.float64, generator=g))
    pred[5] = 0.25                                        # an exact tie: sign(0) = 0
    tgt = torch.randn(300, dtype=torch.float64, generator=g)
    tgt[5] = 0.25
    mask = torch.rand(300, generator=g) < 0.3
    mask[5] = False
    tgt[mask] = float("nan")
    p = pred.clone().requires_grad_(True)
    loss = ref.masked_loss(p, tgt, kind)
    (d,) = torch.autograd.grad(loss * 3.0, p)
    assert torch.isfinite(loss) and torch.isfinite(d).all()
    assert torch.equal(d[mask], torch.zeros(int(mask.sum()), dtype=torch.float64))
    assert d[5] == 0
    # written out on the valid elements alone
    keep = ~mask
    dv = pred[keep] - tgt[keep]
    n = int(keep.sum())
    if kind == "mse":
        lv, gv = dv * dv, 2 * dv
    elif kind == "mae":
        lv, gv = dv.abs(), torch.sign(dv)
    else:
        lv = torch.where(dv.abs() < 1, 0.5 * dv * dv, dv.abs() - 0.5)
        gv = torch.where(dv.abs() < 1, dv, torch.sign(dv))
        assert (dv.abs() < 1).any() and (dv.abs() >= 1).any()
    torch.testing.assert_close(loss, lv.sum() / n, rtol=1e-12, atol=0)
    torch.testing.assert_close(d[keep], 3.0 * gv / n, rtol=1e-12, atol=0)


@pytest.mark.parametrize("kind", ho.LOSS_KINDS)
def test_masked_loss_all_masked_is_zero(kind):
    pred = torch.randn(4, 5, requires_grad=True)
    tgt = torch.full((4, 5), float("nan"))
    loss = ref.masked_loss(pred, tgt, kind)
    loss.backward()
    assert loss.item() == 0.0
    assert torch.equal(pred.grad, torch.zeros(4, 5))
    with pytest.raises(ValueError):
        ops.masked_loss(pred, tgt, "rmse")
    with pytest.raises(ValueError):
        ops.masked_loss(pred, tgt[:2], kind)


def test_masked_metrics():
    rng = np.random.default_rng(3)
    pr, gt = rng.normal(size=(6, 5, 3, 1)) + 5, rng.normal(size=(6, 5, 3, 1)) + 5
    plain = masked_metrics(pr, gt)
    assert plain == {"MSE": MSE(pr, gt), "RMSE": RMSE(pr, gt),
                     "MAE": MAE(pr, gt), "MAPE": MAPE(pr, gt)}
    gt2 = gt.copy()
    gt2[0, 1, 2, 0] = np.nan
    gt2[4, 0, 0, 0] = np.nan
    keep = ~np.isnan(gt2)
    m = masked_metrics(pr, gt2)
    assert m["MSE"] == pytest.approx(np.mean((pr[keep] - gt[keep]) ** 2), rel=1e-12)
    assert m["MAE"] == pytest.approx(np.mean(np.abs(pr[keep] - gt[keep])), rel=1e-12)
    assert m["RMSE"] == pytest.approx(np.sqrt(m["MSE"]), rel=1e-12)
    assert all(np.isfinite(v) for v in m.values())
    empty = masked_metrics(pr, np.full_like(gt, np.nan))
    assert all(np.isnan(v) for v in empty.values())


# ------------------------------------------------------------------------ CLI
def test_main_cli_horizon_and_null_value(tmp_path):
    """Pattern of test_trainer.py::test_main_cli_end_to_end."""
    out_dir = tmp_path / "output"
    metrics = tmp_path / "metrics.jsonl"
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "Main.py"), "-device", "cpu",
         "--synthetic", "--preset", "cpu-small", "--epochs", "1",
         "--nodes", "12", "-cpt", "3", "1", "1",
         "-date", "0101", "0109", "0110", "0112",
         "--horizon", "3", "--null-value", "0", "--loss", "MAE",
         "--model-dir", str(out_dir), "--metrics", str(metrics)],
        capture_output=True, text=True, timeout=420, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (out_dir / "ST_MGCN_best_model.pkl").exists()
    assert "test step 3 true MSE: " in r.stdout
    assert "test true MAPE: " in r.stdout and "nan" not in r.stdout.lower()
    recs = [json.loads(l) for l in metrics.read_text().splitlines()]
    test = [x for x in recs if x.get("test_mode") == "test"]
    assert [x.get("step") for x in test] == [0, 1, 2, None]
    assert all(np.isfinite(x["MAE"]) for x in test)
    saved = torch.load(out_dir / "ST_MGCN_best_model.pkl", weights_only=False)
    assert saved["state_dict"]["fc.weight"].shape[0] == 3


# -------------------------------------------------------- floors against caps
def test_floors_leave_the_caps_idle():
    """3 * floor <= cap for every tensor of every GPU case in both dtypes, so
    the bound of each is decided by the reference's own error (or 2 eps),
    never by the cap."""
    worst = (0.0, "")
    for label, r in ho.all_horizon_references():
        for name, fl in r.floor.items():
            frac = 3.0 * fl / r.cap[name]
            worst = max(worst, (frac, f"{label} {name}"))
            assert 3.0 * fl <= r.cap[name], (label, name, fl)
            assert r.tol(name) <= r.cap[name]
    print("worst 3 * floor / cap = %.2f (%s)" % worst)
    # about 30 % of the loss targets are masked, and Huber sees both branches
    for n in ho.LOSS_NUMELS[1:]:
        t = ho.loss_inputs(n, lo.BF16)
        frac = torch.isnan(t["tgt"]).float().mean().item()
        assert 0.2 < frac < 0.4
        d = (t["pred"].float() - t["tgt"].float())[~torch.isnan(t["tgt"])].abs()
        assert (d < 1).any() and (d >= 1).any()
