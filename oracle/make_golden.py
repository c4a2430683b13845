"""Record the reference implementation's results as test fixtures.

    python oracle/make_golden.py --reference /path/to/ST-MGCN

imports the upstream ST-MGCN modules (GCN, STMGCN, Data_Container,
Model_Trainer) from the given directory — nothing of theirs is copied — runs
them on fixed, seeded inputs and stores inputs and results in
tests/golden/reference_parity.npz (+ reference_state_dict_schema.json).
tests/test_reference_parity.py then checks this package against the stored
results, so the suite needs no reference checkout. Re-run only when the
parity cases change; the fixtures are committed.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)

KERNEL = {"kernel_type": "chebyshev", "K": 2}


def _adj(n=24, seed=3):
    from stmgcn_amd.data.synthetic import _random_sparse_sym_adj
    rng = np.random.default_rng(seed)
    return torch.from_numpy(_random_sparse_sym_adj(n, 6, rng, weighted=True)).float()


def _ref_model(ref_stmgcn, n_nodes, hidden, seq_len=5):
    return ref_stmgcn.ST_MGCN(M=3, seq_len=seq_len, n_nodes=n_nodes, input_dim=1,
                              lstm_hidden_dim=hidden, lstm_num_layers=3,
                              gcn_hidden_dim=hidden, sta_kernel_config=KERNEL,
                              gconv_use_bias=True, gconv_activation=torch.nn.ReLU)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reference", required=True,
                   help="directory of the upstream ST-MGCN checkout")
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    import GCN as ref_gcn
    import STMGCN as ref_stmgcn
    import Data_Container as ref_dc
    import Model_Trainer as ref_mt

    out = {}

    # ---- adjacency preprocessing ------------------------------------------
    A = _adj()
    out["adj/A"] = A.numpy()
    out["adj/chebyshev_K2"] = ref_gcn.Adj_Preprocessor("chebyshev", 2).process(A).numpy()
    out["adj/localpool"] = ref_gcn.Adj_Preprocessor("localpool", 2).process(A).numpy()

    # ---- full model forward + input grad ----------------------------------
    from stmgcn_amd.models import ST_MGCN as OurModel
    N, M, T = 24, 3, 5
    torch.manual_seed(0)
    ours = OurModel(M=M, seq_len=T, n_nodes=N, input_dim=1, lstm_hidden_dim=32,
                    lstm_num_layers=3, gcn_hidden_dim=32, sta_kernel_config=KERNEL)
    theirs = _ref_model(ref_stmgcn, N, 32, T)
    theirs.load_state_dict(ours.state_dict(), strict=True)
    adjs = [ref_gcn.Adj_Preprocessor("chebyshev", 2).process(_adj(N, seed=s))
            for s in range(M)]
    x = torch.randn(4, T, N, 1)
    x2 = x.clone().requires_grad_(True)
    y_ref = theirs(x2, adjs)
    g_ref = torch.autograd.grad(y_ref.pow(2).sum(), x2)[0]
    for k, v in ours.state_dict().items():
        out[f"model/weights/{k}"] = v.numpy()
    out["model/adjs"] = torch.stack(adjs).numpy()
    out["model/x"] = x.numpy()
    out["model/y"] = y_ref.detach().numpy()
    out["model/grad_x"] = g_ref.numpy()

    # ---- state_dict schema (names and shapes only) -------------------------
    schema = {k: list(v.shape)
              for k, v in _ref_model(ref_stmgcn, 58, 64).state_dict().items()}

    # ---- data pipeline -----------------------------------------------------
    from stmgcn_amd.data.synthetic import make_synthetic_dataset
    raw = make_synthetic_dataset(n_nodes=16, m_graphs=1, n_steps=24 * 30, seed=11)
    with tempfile.TemporaryDirectory() as tmp:
        npz = os.path.join(tmp, "data_dict.npz")
        np.savez(npz, **raw)
        ref_in = ref_dc.DataInput(M_adj=1, data_dir=npz, norm_opt=True)
        ref_data = ref_in.load_data()
    ref_gen = ref_dc.DataGenerator(dt=1, obs_len=(3, 1, 1),
                                   train_test_dates=["0101", "0115", "0116", "0120"],
                                   val_ratio=0.2)
    loaders = ref_gen.get_data_loader(data=ref_data, batch_size=8,
                                      device=torch.device("cpu"))
    for k, v in raw.items():
        out[f"data/raw/{k}"] = np.asarray(v)
    out["data/taxi_norm"] = np.asarray(ref_data["taxi"])
    for mode in ["train", "validate", "test"]:
        batches = list(loaders[mode])
        out[f"data/{mode}/batch_sizes"] = np.array([len(bx) for bx, _ in batches])
        out[f"data/{mode}/x"] = torch.cat([bx for bx, _ in batches]).numpy()
        out[f"data/{mode}/y"] = torch.cat([by for _, by in batches]).numpy()
    z = np.linspace(-1, 1, 13, dtype=np.float32)
    out["data/denorm_in"] = z
    out["data/denorm_out"] = np.asarray(ref_in.minmax_denormalize(z))

    # ---- metric formulas ---------------------------------------------------
    rng = np.random.default_rng(4)
    y_pred = rng.normal(50, 20, (100, 16, 1)).astype(np.float32)
    y_true = np.abs(rng.normal(50, 20, (100, 16, 1))).astype(np.float32)
    out["metrics/y_pred"], out["metrics/y_true"] = y_pred, y_true
    for name in ["MSE", "RMSE", "MAE", "MAPE", "PCC"]:
        out[f"metrics/{name}"] = np.asarray(
            getattr(ref_mt.ModelTrainer, name)(y_pred, y_true), dtype=np.float64)

    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(GOLDEN, "reference_parity.npz"), **out)
    with open(os.path.join(GOLDEN, "reference_state_dict_schema.json"), "w") as f:
        json.dump(schema, f, indent=1)
        f.write("\n")
    print("wrote", len(out), "arrays and", len(schema), "schema entries to", GOLDEN)


if __name__ == "__main__":
    main()
