"""Device launches of one eager train step. The glue around the HIP kernels
(dtype converts, zero fills, transposes, masks, small reductions) used to be
two thirds of a step's launches; it now lives in the kernels' epilogues. This
test keeps it there: a change that brings per-parameter converts or copies
back shows up as a higher count long before it shows up in a benchmark."""
import pytest
import torch

# Kernel launches (memcpy / memset events not counted) of one step of the model
# below, measured with this file's own counter on an MI355X:
#   before the epilogue work:  197 (44 bf16 copies, 25 fp32 fills, 24 strided
#                              copies, 6 reduces, 12 mask kernels, ...)
#   with it:                    86 (18 fp32 fills: one per reduction workspace;
#                              every other launch is one of the project's kernels)
PARENT_LAUNCHES = 197
MEASURED_LAUNCHES = 86


def count_step_launches():
    """One eager train step of a tiny ST_MGCN (M=3, N=64, B=2, T=8, L=3, bf16,
    HIP path, FusedAdam) under torch.profiler -> {kernel name: launches}."""
    from collections import Counter
    from stmgcn_amd import PRESETS
    from stmgcn_amd.data.synthetic import make_synthetic_dataset
    from stmgcn_amd.graph import SupportGenerator
    from stmgcn_amd.models import build_model
    from stmgcn_amd.ops import mse_loss
    from stmgcn_amd.train import FusedAdam

    dev = torch.device("cuda")
    cfg = PRESETS["bench-1024"].replace(n_nodes=64, batch_size=2)
    assert (cfg.m_graphs, cfg.seq_len, cfg.lstm_num_layers) == (3, 8, 3)
    raw = make_synthetic_dataset(n_nodes=cfg.n_nodes, n_steps=64,
                                 m_graphs=cfg.m_graphs, seed=7, day_timesteps=1)
    gen = SupportGenerator(cfg.kernel_type, cfg.cheby_K, cfg.lambda_max_mode)
    adjs = [gen.process_csr(torch.from_numpy(raw[k]).float()).to(dev)
            for k in raw if k.endswith("_adj")]
    torch.manual_seed(0)
    model = build_model(cfg).to(device=dev, dtype=torch.bfloat16)
    x = torch.randn(cfg.batch_size, cfg.seq_len, cfg.n_nodes, cfg.input_dim,
                    device=dev, dtype=torch.bfloat16)
    y = torch.randn(cfg.batch_size, cfg.n_nodes, cfg.input_dim, device=dev,
                    dtype=torch.bfloat16)
    opt = FusedAdam(model.parameters(), lr=1e-3)

    def step():
        opt.zero_grad()
        loss = mse_loss(model(x, adjs), y)
        loss.backward()
        opt.step()
        return loss

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    acts = [torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]
    with torch.profiler.profile(activities=acts) as prof:
        loss = step()
        torch.cuda.synchronize()
    assert torch.isfinite(loss.float()).item()
    names = Counter()
    for e in prof.events():
        if (e.device_type == torch.autograd.DeviceType.CUDA
                and not e.name.startswith(("Memcpy", "Memset"))):
            names[e.name] += 1
    return names


@pytest.mark.gpu
def test_step_launch_count_does_not_grow():
    names = count_step_launches()
    total = sum(names.values())
    for n, c in sorted(names.items(), key=lambda kv: -kv[1]):
        print(f"{c:4d}  {n[:120]}")
    print("kernel launches per step:", total, "(was", PARENT_LAUNCHES, ")")
    assert total > 0, "profiler recorded no device events"
    assert total <= MEASURED_LAUNCHES, (total, MEASURED_LAUNCHES)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.getcwd())
    c = count_step_launches()
    for n, k in sorted(c.items(), key=lambda kv: -kv[1]):
        print(f"{k:4d}  {n[:120]}")
    print("TOTAL", sum(c.values()))
