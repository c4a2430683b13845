"""CG_LSTM hands the gate the x_seq it already has, takes the gated sequence
node-major and leaves the zero initial states to the RNN op. On the CPU path
none of that may change a bit: the model is compared, in fp32 and exactly,
with the same computation written out against reference_impl — including the
explicit h0 / c0 zeros and the permute the model no longer spells out."""
import numpy as np
import pytest
import torch

from stmgcn_amd.data.synthetic import _random_sparse_sym_adj
from stmgcn_amd.graph import SupportGenerator
from stmgcn_amd.models import ST_MGCN, StackedSTMGCN
from stmgcn_amd.ops import reference_impl as ref

N, T, B, M = 12, 5, 2, 3


def _supports():
    rng = np.random.default_rng(0)
    gen = SupportGenerator("chebyshev", 2)
    return [gen.process(torch.from_numpy(
        _random_sparse_sym_adj(N, 4, rng, weighted=True))) for _ in range(M)]


def _branch_by_hand(cg, adj, obs, return_sequences):
    Bb, Tt, Nn, C = obs.shape
    x_seq = obs.sum(dim=-1).permute(0, 2, 1)
    gc = cg.gconv_temporal_feats
    g = ref.gconv_mix_dense(adj, x_seq, gc.W, gc.b, gc.activation)
    gated = ref.contextual_gate(obs, g, cg.fc.weight, cg.fc.bias)
    flat = gated.permute(0, 2, 1, 3).reshape(Bb * Nn, Tt, C)
    h0 = obs.new_zeros(cg.num_layers, Bb * Nn, cg.hidden_dim)
    ws = cg.lstm.flat_weights()
    if cg.cell == "lstm":
        out = ref.lstm_forward(flat, ws, h0, h0.clone(), return_sequences)
    else:
        out = ref.gru_forward(flat, ws, h0, return_sequences)
    if return_sequences:
        return out.reshape(Bb, Nn, Tt, cg.hidden_dim).permute(0, 2, 1, 3)
    return out.reshape(Bb, Nn, cg.hidden_dim)


def _grads(model, obs, y):
    model.zero_grad()
    obs.grad = None
    (y ** 2).sum().backward()
    return [obs.grad.clone()] + [p.grad.clone() for p in model.parameters()]


def _assert_same(model, obs, y_model, y_hand):
    assert torch.equal(y_model, y_hand)
    gm = _grads(model, obs, y_model)
    gh = _grads(model, obs, y_hand)
    names = ["obs"] + [n for n, _ in model.named_parameters()]
    for n, a, b in zip(names, gm, gh):
        assert torch.equal(a, b), n


def test_st_mgcn_matches_reference_impl_exactly():
    torch.manual_seed(0)
    model = ST_MGCN(M=M, seq_len=T, n_nodes=N, input_dim=1, lstm_hidden_dim=64,
                    lstm_num_layers=2, gcn_hidden_dim=16,
                    sta_kernel_config={"kernel_type": "chebyshev", "K": 2})
    adjs = _supports()
    obs = torch.randn(B, T, N, 1, requires_grad=True)
    feats = []
    for m in range(M):
        h = _branch_by_hand(model.rnn_list[m], adjs[m], obs, False)
        gc = model.gcn_list[m]
        feats.append(ref.gconv_mix_dense(adjs[m], h, gc.W, gc.b, gc.activation))
    y_hand = ref.branch_fuse_head(feats, model.fc.weight, model.fc.bias)
    _assert_same(model, obs, model(obs, adjs), y_hand)


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_cg_lstm_sequences_match_reference_impl_exactly(cell):
    """The sequence-returning form the stacked model uses, both cells, C > 1."""
    torch.manual_seed(1)
    model = StackedSTMGCN(M=1, seq_len=T, n_nodes=N, input_dim=3,
                          lstm_hidden_dim=64, lstm_num_layers=2,
                          gcn_hidden_dim=8, n_blocks=1, rnn_cell=cell,
                          sta_kernel_config={"kernel_type": "chebyshev", "K": 2})
    cg = model.blocks[0].rnn_list[0]
    adj = _supports()[0]
    obs = torch.randn(B, T, N, 3, requires_grad=True)
    y_model = cg(adj, obs, return_sequences=True)
    y_hand = _branch_by_hand(cg, adj, obs, True)
    assert torch.equal(y_model, y_hand)
    g_model = torch.autograd.grad((y_model ** 2).sum(), [obs] + list(cg.parameters()))
    g_hand = torch.autograd.grad((y_hand ** 2).sum(), [obs] + list(cg.parameters()))
    for a, b in zip(g_model, g_hand):
        assert torch.equal(a, b)
