"""Evaluation metrics — formula parity with reference Model_Trainer.py:100-114.

Computed on DENORMALIZED predictions (reference Model_Trainer.py:89-90).
MAPE uses the reference's unusually large epsilon=1.0 (quirk 11).
PCC exists in the reference but is never called; kept for capability parity.
"""
from __future__ import annotations

import numpy as np


def MSE(y_pred: np.ndarray, y_true: np.ndarray) -> float:
    return float(np.mean(np.square(y_pred - y_true)))


def RMSE(y_pred: np.ndarray, y_true: np.ndarray) -> float:
    return float(np.sqrt(np.mean(np.square(y_pred - y_true))))


def MAE(y_pred: np.ndarray, y_true: np.ndarray) -> float:
    return float(np.mean(np.abs(y_pred - y_true)))


def MAPE(y_pred: np.ndarray, y_true: np.ndarray, epsilon: float = 1e-0) -> float:
    return float(np.mean(np.abs(y_pred - y_true) / (y_true + epsilon)))


def masked_metrics(y_pred: np.ndarray, y_true: np.ndarray) -> dict:
    """MSE / RMSE / MAE / MAPE over the valid elements: a NaN in y_true marks a
    missing reading. Without NaN the arrays go to the metrics untouched, so the
    figures are exactly the unmasked ones; every element masked gives NaN."""
    valid = ~np.isnan(y_true)
    if not valid.all():
        if not valid.any():
            return {k: float("nan") for k in ("MSE", "RMSE", "MAE", "MAPE")}
        y_pred, y_true = y_pred[valid], y_true[valid]
    return {"MSE": MSE(y_pred, y_true), "RMSE": RMSE(y_pred, y_true),
            "MAE": MAE(y_pred, y_true), "MAPE": MAPE(y_pred, y_true)}


def PCC(y_pred: np.ndarray, y_true: np.ndarray) -> float:
    return float(np.corrcoef(y_pred.flatten(), y_true.flatten())[0, 1])
