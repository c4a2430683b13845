"""The host contract of the bindings: a tensor of the wrong dtype, size or
list length is a RuntimeError raised before anything is launched.

Per binding: one well-formed call, one call per malformed argument (each must
raise), the same well-formed call again. The two well-formed results are
bit-equal (every launch here is one workgroup per reduction or has no atomics),
and the state a binding updates in place is untouched by the refused calls.

Every malformed input is one an unchecked kernel would also survive: it is
larger than expected, of an equal or larger element size, a surplus list entry
the launcher refuses too, or -- where the fault is "too small" -- a leading
view of an allocation of the full size."""
import pytest
import torch

import _lowp_oracle as lo

DEV = "cuda"
BF16, F16, F32 = lo.BF16, lo.F16, lo.F32
S, TST, L, CIN = 33, 2, 2, 1      # two sequence tiles, the second with one live row
S_PAD = 64
B, N, G = 2, 5, 8
H = lo.H

pytestmark = pytest.mark.gpu


def _C():
    from stmgcn_amd.ops.functional import require_hip
    return require_hip()


def _flat(res):
    res = res if isinstance(res, (list, tuple)) else [res]
    return [t.cpu() for t in res if t is not None]


def _contract(good, bads):
    """good() before and after every refused bad(): bit-equal results."""
    want = _flat(good())
    for name, bad in bads.items():
        with pytest.raises(RuntimeError):
            bad()
            pytest.fail(f"{name}: the malformed call was accepted")
    got = _flat(good())
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"output {i} changed after the refused calls"


def _rnn_inputs():
    g = lo._gen("binding-contract-rnn")
    x = torch.randn(S, TST, CIN, generator=g).to(BF16).to(DEV)
    ws = [w.to(BF16).to(DEV) for w in lo.rnn_weights("lstm", L, CIN, g)]
    dout = torch.randn(S, H, generator=g).to(BF16).to(DEV)
    return x, ws, dout


def test_lstm_fwd_contract():
    C = _C()
    x, ws, _ = _rnn_inputs()
    w_ih, w_hh, b_ih, b_hh = ws[0::4], ws[1::4], ws[2::4], ws[3::4]
    _contract(
        lambda: C.lstm_fwd(x, w_ih, w_hh, b_ih, b_hh, False, True, False),
        {
            "w_hh one layer short": lambda: C.lstm_fwd(
                x, w_ih, w_hh[:-1], b_ih, b_hh, False, True, False),
            "fp32 bias": lambda: C.lstm_fwd(
                x, w_ih, w_hh, [b_ih[0].float(), b_ih[1]], b_hh, False, True, False),
        })


def test_lstm_bwd_contract():
    C = _C()
    x, ws, dout = _rnn_inputs()
    w_ih, w_hh = ws[0::4], ws[1::4]
    _, _, cseq, gates = C.lstm_fwd(x, w_ih, w_hh, ws[2::4], ws[3::4], False, True, False)
    wT = C.lstm_pack_bwd_weights(w_ih, w_hh)
    w_ihT, w_hhT = list(wT[:L]), list(wT[L:])
    # one more sequence tile of saved gates than (S, Tst, L) has
    gates_long = torch.zeros(L, TST, (S_PAD + 32) * 4 * H, dtype=BF16, device=DEV)
    # (64, 192): the leading part of a full-size (64, 256) allocation
    narrow = torch.zeros(H * 4 * H, dtype=BF16, device=DEV)[:H * 3 * H].view(H, 3 * H)
    nine_ih = [w_ihT[0]] + [w_ihT[1]] * 8
    nine_hh = [w_hhT[0]] * 9

    def call(dout=dout, cseq=cseq, gates=gates, w_ihT=w_ihT, w_hhT=w_hhT):
        return C.lstm_bwd(dout, x, cseq, gates, w_ihT, w_hhT, False, False)

    _contract(call, {
        "fp32 dout": lambda: call(dout=dout.float()),
        "gates of one extra tile": lambda: call(gates=gates_long),
        "f16 cseq": lambda: call(cseq=cseq.to(F16)),
        "(64, 192) transposed weight": lambda: call(w_ihT=[w_ihT[0], narrow]),
        "nine layers": lambda: call(w_ihT=nine_ih, w_hhT=nine_hh),
    })


def _head_inputs():
    g = lo._gen("binding-contract-head")
    feats = [torch.randn(B, N, G, generator=g).to(BF16).to(DEV) for _ in range(2)]
    w = torch.randn(G, generator=g).to(BF16).to(DEV)
    bias = torch.randn(1, generator=g).to(BF16).to(DEV)
    dy = torch.randn(B, N, 1, generator=g).to(BF16).to(DEV)
    return feats, w, bias, dy


def test_head_fwd_contract():
    C = _C()
    feats, w, bias, _ = _head_inputs()
    _contract(lambda: C.head_fwd(feats, w, bias), {
        "fp32 second feature map": lambda: C.head_fwd([feats[0], feats[1].float()], w, bias),
        "w of G + 8": lambda: C.head_fwd(feats, torch.cat([w, w]), bias),
        "bias of two": lambda: C.head_fwd(feats, w, torch.cat([bias, bias])),
    })


def test_head_bwd_contract():
    C = _C()
    _, w, _, dy = _head_inputs()
    _contract(lambda: C.head_bwd(dy, w, G),
              {"fp32 w": lambda: C.head_bwd(dy, w.float(), G)})


@pytest.mark.parametrize("form", ["head_wgrad", "head_wgrad_grads"])
def test_head_wgrad_contract(form):
    fn = getattr(_C(), form)
    feats, _, _, dy = _head_inputs()
    dy_long = torch.cat([dy.view(-1), dy.view(-1)[:1]]).view(1, B * N + 1, 1)
    _contract(lambda: fn(dy, feats[0]),
              {"dy with one extra row": lambda: fn(dy_long, feats[0])})


def test_mse_fwd_contract():
    C = _C()
    g = lo._gen("binding-contract-mse")
    pred = torch.randn(10, generator=g).to(BF16).to(DEV)
    tgt = torch.randn(10, generator=g).to(BF16).to(DEV)
    _contract(lambda: C.mse_fwd(pred, tgt), {
        "fp32 tgt": lambda: C.mse_fwd(pred, tgt.float()),
        "tgt with one extra element": lambda: C.mse_fwd(pred, torch.cat([tgt, tgt[:1]])),
    })


LENS = [4, 3, 5]      # three segments
OFS = [0, 4, 7]
NPAR = sum(LENS)


def test_adam_step_contract():
    C = _C()
    g = lo._gen("binding-contract-adam")
    master0 = torch.randn(NPAR, generator=g).to(DEV)
    grad = torch.randn(NPAR, generator=g).to(BF16).to(DEV)
    hyper0 = torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 1.0, 1.0], device=DEV)

    def state():
        return [master0.clone(), master0.to(BF16), grad, torch.zeros(NPAR, device=DEV),
                torch.zeros(NPAR, device=DEV), hyper0.clone()]

    def good():
        st = state()
        C.adam_step(*st)
        return st

    def bad(i, t):
        st = state()
        kept = [s.clone() for s in st]
        args = list(st)
        args[i] = t
        try:
            C.adam_step(*args)
        finally:   # a refused step leaves master, param, moments and hyper alone
            for s, k in zip(st, kept):
                assert torch.equal(s, k)

    _contract(good, {
        "m with one extra element": lambda: bad(3, torch.zeros(NPAR + 1, device=DEV)),
        "fp32 grad for a bf16 param": lambda: bad(2, grad.float()),
    })


def test_gather_grads_contract():
    C = _C()
    g = lo._gen("binding-contract-gather")
    grads = [torch.randn(n, generator=g).to(BF16).to(DEV) for n in LENS]
    full = torch.empty(NPAR, dtype=BF16, device=DEV)

    def call(grads=grads, ofs=OFS, lens=LENS, arena=None):
        arena = full if arena is None else arena
        full.fill_(-7.0)
        try:
            C.gather_grads(grads, ofs, lens, arena)
        except RuntimeError:   # a refused call wrote no segment
            assert bool((full == -7.0).all())
            raise
        return full.clone()

    long_grad = [grads[0], torch.cat([grads[1], grads[1][:1]]), grads[2]]
    _contract(call, {
        "lens one longer than ofs": lambda: call(lens=LENS + [1]),
        "a gradient longer than its len": lambda: call(grads=long_grad),
        # the arena is the leading part of the full-size allocation
        "last segment past the arena": lambda: call(arena=full[:NPAR - 1]),
    })
