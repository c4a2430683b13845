"""The contextual gate with its FC stages folded into the reduce kernels
(the last workgroup of a batch row runs them; the last row sums dw / db), and
its optional arguments: a passed-in x_seq, node-major output, no dobs.

Every run is held to the bound rule of _lowp_oracle (float64 oracle, floor of
the all-low-precision run) on the GATE_CASES, which include two reduce chunks
(several arrivers per row), B = 65 (many rows) and T = 1 and 16."""
import pytest
import torch

import _lowp_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda"
WRT = ("obs", "g", "w", "b")


def _run(case, dtype, pass_xs=False, node_major=False, obs_grad=True):
    from stmgcn_amd.ops.functional import require_hip
    from stmgcn_amd.ops.hip_ops import GateFn
    r = lo.gate_reference(case, dtype)
    t = {k: v.to(DEV, dtype).requires_grad_(k != "obs" or obs_grad)
         for k, v in r.inputs.items()}
    extra = ()
    if pass_xs or node_major:
        xs = require_hip().seqsum_permute(t["obs"].detach()) if pass_xs else None
        extra = (xs, node_major)
    out = GateFn.apply(t["obs"], t["g"], t["w"], t["b"], *extra)
    (out.float() ** 2).sum().backward()
    return r, {"out": out.detach(), "dobs": t["obs"].grad, "dg": t["g"].grad,
               "dw": t["w"].grad, "db": t["b"].grad}


@pytest.mark.parametrize("pass_xs", [False, True], ids=["own_xs", "given_xs"])
@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", lo.GATE_CASES, ids=str)
def test_gate_folded_fc_meets_the_bound(case, dtype, pass_xs):
    r, got = _run(case, dtype, pass_xs=pass_xs)
    r.check(got, f"gate {case} {lo.dtype_name(dtype)} xs={pass_xs}")


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", lo.GATE_CASES, ids=str)
def test_gate_given_xs_changes_nothing(case, dtype):
    """The passed x_seq is the one the op would compute: same forward bits."""
    _, a = _run(case, dtype)
    _, b = _run(case, dtype, pass_xs=True)
    assert torch.equal(a["out"], b["out"])
    assert torch.equal(a["dobs"], b["dobs"]) and torch.equal(a["dg"], b["dg"])


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", lo.GATE_CASES, ids=str)
def test_gate_node_major(case, dtype):
    """(B,N,T,C) output == the permuted default output, bit for bit; the
    loss sum(out^2) is layout-blind, so the gradients answer to the same
    oracle under the same bound."""
    _, base = _run(case, dtype)
    r, got = _run(case, dtype, node_major=True)
    B, T, N, C = case
    assert got["out"].shape == (B, N, T, C) and got["out"].is_contiguous()
    assert torch.equal(got["out"], base["out"].permute(0, 2, 1, 3))
    got["out"] = got["out"].permute(0, 2, 1, 3)
    r.check(got, f"gate node-major {case} {lo.dtype_name(dtype)}")


@pytest.mark.parametrize("node_major", [False, True], ids=["btnc", "bntc"])
@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", lo.GATE_CASES, ids=str)
def test_gate_without_dobs(case, dtype, node_major):
    """obs needs no gradient (training: it is input data): nothing else moves.
    dw / db pass through float atomics, so they answer to the bound instead."""
    _, base = _run(case, dtype, node_major=node_major)
    r, got = _run(case, dtype, node_major=node_major, obs_grad=False)
    assert got["dobs"] is None
    assert torch.equal(got["out"], base["out"])
    assert torch.equal(got["dg"], base["dg"])
    del got["dobs"]
    if node_major:
        got["out"] = got["out"].permute(0, 2, 1, 3)
    r.check(got, f"gate no-dobs {case} {lo.dtype_name(dtype)}", skip=("dobs",))
