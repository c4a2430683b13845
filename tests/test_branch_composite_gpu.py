"""One model branch on the GPU against float64: CG_LSTM (seqsum, temporal
gconv, node-major gate, fused RNN) and its GCN, composed as STMGCNBlock and
ST_MGCN compose them. The C = 64 cases are what every block of the deep
variant after the first runs: obs needs a gradient, which reaches it twice
(folded into dobs by the gate kernel, and through SeqsumPermuteFn.backward
from the temporal gconv's dX), the RNN reads cin = 64 and returns sequences,
and the post-RNN gconv runs over B*T batches.

The output, dobs and the gradient of every parameter of both modules are held,
each on its own, to the bound rule of _lowp_oracle with the references of
_branch_oracle. No op may leave the HIP path."""
import copy

import pytest
import torch

import _branch_oracle as bo
import _lowp_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gpu_branch(case, dtype):
    r = bo.branch_reference(case, dtype)
    rnn, gcn = (copy.deepcopy(m).to(DEV) for m in r.extra["modules"])
    assert all(p.dtype == dtype for p in rnn.parameters())
    return r, rnn, gcn, r.extra["csr"].to(DEV), r.inputs["obs"].to(DEV)


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", bo.BRANCH_CASES, ids=str)
def test_branch_meets_the_bound(case, dtype):
    from stmgcn_amd.ops import hip_ops
    r, rnn, gcn, csr, obs = _gpu_branch(case, dtype)
    hip_ops.reset_fallback_count()
    got = bo.fwd_bwd(rnn, gcn, csr, obs, case[6], want_dobs=case[3] > 1)
    assert hip_ops.fallback_count() == 0
    r.check(got, f"branch {case} {lo.dtype_name(dtype)}")


@pytest.mark.parametrize("dtype", lo.LOWP, ids=lo.dtype_name)
@pytest.mark.parametrize("case", bo.EVAL_CASES, ids=str)
def test_branch_eval_forward_is_the_training_forward(case, dtype):
    """eval() under no_grad skips saving the recurrence states, the gates and
    the gate's intermediates; the output bits must not depend on that."""
    _, rnn, gcn, csr, obs = _gpu_branch(case, dtype)
    train_out = bo.run_branch(rnn, gcn, csr, obs.clone().requires_grad_(True),
                              case[6]).detach()
    rnn.eval(), gcn.eval()
    with torch.no_grad():
        eval_out = bo.run_branch(rnn, gcn, csr, obs, case[6])
    assert torch.equal(eval_out, train_out)
