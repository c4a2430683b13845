"""Training runtime — API and observable-behavior parity with the reference
ModelTrainer (Model_Trainer.py:8-114), rebuilt for MI355X.

Parity kept:
  - constructor signature (model, loss, optimizer, lr, wd, n_epochs)
    (Model_Trainer.py:9-14; `optimizer` is the class, e.g. torch.optim.Adam)
  - train(data_loader, sta_adj_list, modes, model_dir, early_stopper=10):
    best-val checkpointing to {model_dir}/{cls}_best_model.pkl with payload
    {'epoch': int, 'state_dict': ...}; patience reset on improvement;
    exact epoch print strings (Model_Trainer.py:47-60)
  - test(...) reloads the best checkpoint, prints denormalized
    MSE/RMSE/MAE/MAPE with the reference's formats (Model_Trainer.py:92-95)
  - class-name dispatch: only 'ST_MGCN'-named models accepted (quirk 9)

Reference quirks intentionally FIXED (documented in SURVEY Appendix A):
  - running_loss accumulates a detached float, not a live tensor (quirk 6)
  - test()/validate run under torch.no_grad() (quirk 7)

MI355X additions:
  - data-parallel awareness: an optional GradReducer all-reduces gradients
    after backward; loss scalars are all-reduced for identical early-stop
    decisions on every rank; only rank 0 writes checkpoints/prints
  - per-step HIP-event timing and JSONL metrics stream (samples/sec, val
    loss) for the scaling-curve report (SURVEY §5 observability)
"""
from __future__ import annotations

import json
import os
import time
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import nn

from .metrics import MSE, RMSE, MAE, MAPE, PCC, masked_metrics


class ModelTrainer:
    SUPPORTED_MODELS = ("ST_MGCN", "StackedSTMGCN")

    def __init__(self, model: nn.Module, loss: nn.Module, optimizer, lr: float,
                 wd: float, n_epochs: int, grad_reducer=None, rank: int = 0,
                 world_size: int = 1, metrics_path: Optional[str] = None,
                 use_graph: bool = False):
        self.model = model
        self.model_name = model.__class__.__name__
        if self.model_name not in self.SUPPORTED_MODELS:
            raise ValueError(f"unsupported model class {self.model_name!r}")
        self.criterion = loss
        self.optimizer = optimizer(params=model.parameters(), lr=lr, weight_decay=wd)
        self.n_epochs = n_epochs
        self.grad_reducer = grad_reducer
        self.rank, self.world = rank, world_size
        self.metrics_path = metrics_path
        self._metrics_f = None
        # whole-step hipGraph capture for full-size train batches (the
        # bench-grade path: fwd+loss+bwd(+all-reduce)+Adam as one replay);
        # ragged last batches and eval run eagerly. Requires the FusedAdam
        # path (device-side bias correction) on GPU.
        self.use_graph = use_graph and torch.cuda.is_available()
        self._graphs = {}             # shape -> (graph, x_static, y_static, loss_static)
        self._eager_seen = set()      # shapes that ran their one eager warmup
        self._resume_best_val = np.inf

    # ------------------------------------------------------------------ utils
    def _log(self, *args):
        if self.rank == 0:
            print(*args)

    def _emit(self, record: dict):
        if self.rank != 0 or self.metrics_path is None:
            return
        if self._metrics_f is None:
            os.makedirs(os.path.dirname(self.metrics_path) or ".", exist_ok=True)
            self._metrics_f = open(self.metrics_path, "a")
        self._metrics_f.write(json.dumps(record) + "\n")
        self._metrics_f.flush()

    def _allreduce_scalar(self, value: float) -> float:
        if self.world <= 1:
            return value
        import torch.distributed as dist
        if not dist.is_initialized():
            return value
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([value], dtype=torch.float64, device=dev)
        dist.all_reduce(t)
        return float(t.item()) / self.world

    def _forward(self, x, sta_adj_list):
        return self.model(obs_seq=x, sta_adj_list=sta_adj_list)

    def _train_step_eager(self, x, y_true, sta_adj_list):
        if self.grad_reducer is not None:
            self.grad_reducer.zero_grad()
        elif hasattr(self.optimizer, "reduce"):
            self.optimizer.zero_grad()           # FusedAdam arena
        else:
            self.optimizer.zero_grad(set_to_none=True)
        y_pred = self._forward(x, sta_adj_list)
        loss = self.criterion(y_pred, y_true)
        loss.backward()
        if self.grad_reducer is not None:
            self.grad_reducer.reduce()
        elif hasattr(self.optimizer, "reduce") and self.world > 1:
            self.optimizer.reduce()              # one flat RCCL all-reduce
        self.optimizer.step()
        return loss

    def _train_step(self, x, y_true, sta_adj_list) -> float:
        """Returns the step loss as a FLOAT — never a live tensor: a loss
        held by the caller across iterations keeps the autograd graph (and
        its default-stream AccumulateGrad nodes) alive, which breaks hipGraph
        capture of the next step. Graphs are cached PER SHAPE (the ragged
        last batch of an epoch gets its own graph and never clobbers the
        full-batch one); each shape pays one eager warmup step, then its
        second sighting is the warmup-before-capture step — the capture
        itself records without executing and is NOT replayed on that batch,
        so every batch is trained exactly once."""
        if not self.use_graph:
            return float(self._train_step_eager(x, y_true, sta_adj_list).detach())
        shape = (tuple(x.shape), tuple(y_true.shape))
        entry = self._graphs.get(shape)
        if entry is not None:
            g, xs, ys, ls = entry
            xs.copy_(x)
            ys.copy_(y_true)
            g.replay()
            return float(ls.detach())
        if shape not in self._eager_seen:        # first sighting: eager warmup
            self._eager_seen.add(shape)
            return float(self._train_step_eager(x, y_true, sta_adj_list).detach())
        # second sighting of the shape: the side-stream warmup IS this
        # batch's (single) real training step; then record the graph.
        try:
            xs, ys = x.clone(), y_true.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                warm_loss = self._train_step_eager(xs, ys, sta_adj_list)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            warm = float(warm_loss.detach())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                ls = self._train_step_eager(xs, ys, sta_adj_list)
            torch.cuda.synchronize()
            self._graphs[shape] = (g, xs, ys, ls)
            return warm
        except Exception as e:
            self._log(f"# hipGraph capture unavailable, eager fallback: {e}")
            self.use_graph = False
            return float(self._train_step_eager(x, y_true, sta_adj_list).detach())

    def _ckpt_path(self, model_dir: str) -> str:
        return os.path.join(model_dir, f"{self.model_name}_best_model.pkl")

    def _optim_path(self, model_dir: str) -> str:
        # sidecar file: the reference-format best_model.pkl stays
        # byte-compatible ({'epoch', 'state_dict'} only — SURVEY §5)
        return os.path.join(model_dir, f"{self.model_name}_best_model.optim.pkl")

    def resume(self, model_dir: str) -> int:
        """Failure recovery: reload the best-val checkpoint (and
        optimizer state if its sidecar exists) and return the epoch to
        continue from. No-op (returns 0) when no checkpoint exists."""
        path = self._ckpt_path(model_dir)
        if not os.path.exists(path):
            return 0
        saved = torch.load(path, weights_only=False, map_location="cpu")
        dev = next(self.model.parameters()).device
        dt = next(self.model.parameters()).dtype
        self.model.load_state_dict(
            {k: v.to(device=dev, dtype=dt) for k, v in saved["state_dict"].items()})
        opath = self._optim_path(model_dir)
        if os.path.exists(opath):
            payload = torch.load(opath, weights_only=False, map_location=dev)
            if isinstance(payload, dict) and "optimizer" in payload:
                self.optimizer.load_state_dict(payload["optimizer"])
                # seed the best-val floor so the first post-resume epoch
                # cannot overwrite a better pre-crash checkpoint
                self._resume_best_val = float(payload.get("best_val_loss", np.inf))
            else:                     # legacy sidecar: bare optimizer state
                self.optimizer.load_state_dict(payload)
        self._log(f"Resumed from {path} (epoch {saved['epoch']})")
        return int(saved["epoch"])

    # ------------------------------------------------------------------ train
    def train(self, data_loader: Dict, sta_adj_list: List, modes: List[str],
              model_dir: str, early_stopper: int = 10, start_epoch: int = 0):
        patience = early_stopper
        # cloned snapshot (not live references): the unconditional final save
        # must never write weights from a later epoch under this epoch number
        checkpoint = {"epoch": start_epoch,
                      "state_dict": {k: v.detach().clone()
                                     for k, v in self.model.state_dict().items()}}
        val_loss = self._resume_best_val
        self._log("Training starts at: ", time.ctime())

        for epoch in range(start_epoch + 1, self.n_epochs + 1):
            running_loss = {mode: 0.0 for mode in modes}
            t_epoch = time.perf_counter()
            n_train_samples = 0
            for mode in modes:
                self.model.train() if mode == "train" else self.model.eval()
                step = 0
                for x, y_true in data_loader[mode]:
                    if mode == "train":
                        lval = self._train_step(x, y_true, sta_adj_list)
                    else:
                        with torch.no_grad():
                            lval = float(self.criterion(
                                self._forward(x, sta_adj_list), y_true).detach())
                    running_loss[mode] += lval * y_true.shape[0]
                    step += y_true.shape[0]
                if mode == "train":
                    n_train_samples = step * self.world

                if mode == "validate":
                    epoch_val = self._allreduce_scalar(running_loss[mode] / max(step, 1))
                    dt = time.perf_counter() - t_epoch
                    self._emit({"epoch": epoch, "val_loss": epoch_val,
                                "train_loss": running_loss.get("train", 0.0) / max(n_train_samples // max(self.world, 1), 1),
                                "samples_per_sec": n_train_samples / dt if dt > 0 else 0.0,
                                "wall_s": dt})
                    if epoch_val <= val_loss:
                        self._log(f"Epoch {epoch}, Val_loss drops from {val_loss:.5} "
                                  f"to {epoch_val:.5}. Update model checkpoint..")
                        val_loss = epoch_val
                        # snapshot (clone) the best-epoch weights: the
                        # reference keeps live references here, so its final
                        # save silently writes LAST-epoch weights under the
                        # best epoch number — quirk fixed like 6/7
                        checkpoint.update(
                            epoch=epoch,
                            state_dict={k: v.detach().clone()
                                        for k, v in self.model.state_dict().items()})
                        if self.rank == 0:
                            torch.save(checkpoint, self._ckpt_path(model_dir))
                            torch.save({"optimizer": self.optimizer.state_dict(),
                                        "best_val_loss": val_loss},
                                       self._optim_path(model_dir))
                        patience = early_stopper
                    else:
                        self._log(f"Epoch {epoch}, Val_loss does not improve from {val_loss:.5}.")
                        patience -= 1
                        if patience == 0:
                            self._log(f"Early stopping at epoch {epoch}..")
                            return

        self._log("Training ends at: ", time.ctime())
        if self.rank == 0:
            torch.save(checkpoint, self._ckpt_path(model_dir))

    # ------------------------------------------------------------------- test
    def test(self, data_loader: Dict, sta_adj_list: List, modes: List[str],
             model_dir: str, data_class):
        saved = torch.load(self._ckpt_path(model_dir), weights_only=False)
        self.model.load_state_dict(saved["state_dict"])
        self.model.eval()
        self._log("Testing starts at: ", time.ctime())
        results = {}
        with torch.no_grad():
            for mode in modes:
                truths, preds = [], []
                for x, y_true in data_loader[mode]:
                    y_pred = self._forward(x, sta_adj_list)
                    truths.append(y_true.float().cpu().numpy())
                    preds.append(y_pred.float().cpu().numpy())
                gt = data_class.minmax_denormalize(np.concatenate(truths, axis=0))
                pr = data_class.minmax_denormalize(np.concatenate(preds, axis=0))
                if gt.ndim == 4:
                    # horizon P > 1, (S, N, P, C): one record per step ahead,
                    # then the aggregate over all steps below
                    for p in range(gt.shape[2]):
                        m = masked_metrics(pr[:, :, p], gt[:, :, p])
                        self._log(f"{mode} step {p + 1} true MSE: ", m["MSE"],
                                  " RMSE: ", m["RMSE"], " MAE: ", m["MAE"],
                                  " MAPE: ", m["MAPE"] * 100, "%")
                        self._emit({"test_mode": mode, "step": p, **m})
                results[mode] = masked_metrics(pr, gt)
                self._log(f"{mode} true MSE: ", results[mode]["MSE"])
                self._log(f"{mode} true RMSE: ", results[mode]["RMSE"])
                self._log(f"{mode} true MAE: ", results[mode]["MAE"])
                self._log(f"{mode} true MAPE: ", results[mode]["MAPE"] * 100, "%")
                self._emit({"test_mode": mode, **results[mode]})
        self._log("Testing ends at: ", time.ctime())
        return results

    # static metric surface (reference Model_Trainer.py:100-114)
    MSE = staticmethod(MSE)
    RMSE = staticmethod(RMSE)
    MAE = staticmethod(MAE)
    MAPE = staticmethod(MAPE)
    PCC = staticmethod(PCC)
