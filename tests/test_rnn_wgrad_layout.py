"""The dA stream between lstm_bwd and lstm_wgrad is stored in wgrad-fragment
tile order (stmgcn_amd/csrc/common.h). These tests pin the layout from the
outside: a direct wgrad test that builds the tiled tensor with an independent
index helper, and a producer/consumer agreement test through FusedLSTMFn."""
import pytest
import torch

H = 64
TILE = 32


def rho(kp):
    """Reduction slot k' (0..31) of a dA tile -> row of the 32-row tile."""
    return 16 * ((kp >> 2) & 1) + 4 * (kp >> 3) + (kp & 3)


def tile_dA(dA):
    """Natural (L, T, S_pad, 4H) -> same shape/size in tile order: the block of
    tile (l, t, b) starts at element ((l*T + t)*S_pad + 32b)*4H and holds
    [gate g][k'] with element (g, k') = dA[row 32b + rho(k')][g]."""
    L, T, Sp, G = dA.shape
    assert Sp % TILE == 0
    rows = torch.tensor([rho(kp) for kp in range(TILE)], device=dA.device)
    tiles = dA.reshape(L, T, Sp // TILE, TILE, G)         # [.., row, g]
    blk = tiles.index_select(3, rows).transpose(3, 4)     # [.., g, k']
    return blk.contiguous().reshape(L, T, Sp, G)


def test_tile_helper_matches_literal_formula():
    """The vectorised helper against the spec written out element by element."""
    L, T, Sp, G = 2, 2, 64, 4 * H
    dA = torch.arange(L * T * Sp * G, dtype=torch.float32).reshape(L, T, Sp, G)
    flat = tile_dA(dA).reshape(-1)
    assert sorted(rho(k) for k in range(TILE)) == list(range(TILE))
    for (l, t, b, g, kp) in [(0, 0, 0, 0, 0), (0, 0, 0, 0, 4), (0, 1, 1, 255, 31),
                             (1, 0, 1, 77, 13), (1, 1, 0, 128, 22), (1, 1, 1, 3, 9)]:
        off = ((l * T + t) * Sp + TILE * b) * G + g * TILE + kp
        assert flat[off] == dA[l, t, TILE * b + rho(kp), g]


def _wgrad_reference(dA, hseq, x, S_pad):
    """fp32 references from the same rounded inputs. dA (L,T,S_pad,4H) natural,
    hseq (L,T,S_pad,H), x (S,T,cin); pad rows of x count as zero."""
    L, T = dA.shape[:2]
    S, _, cin = x.shape
    R = T * S_pad
    x_pad = torch.zeros(S_pad, T, cin, device=x.device)
    x_pad[:S] = x.float()
    x_rows = x_pad.transpose(0, 1).reshape(R, cin)         # row r = t*S_pad + s
    dwih = torch.zeros(L, 4 * H, H, device=x.device)
    dwhh = torch.zeros(L, 4 * H, H, device=x.device)
    db = torch.zeros(L, 4 * H, device=x.device)
    for l in range(L):
        a = dA[l].float().reshape(R, 4 * H)
        hp = torch.zeros(T, S_pad, H, device=x.device)
        hp[1:] = hseq[l, :-1].float()                      # h_{t-1}, zero at t == 0
        hx = x_rows if l == 0 else hseq[l - 1].float().reshape(R, H)
        dwhh[l] = a.T @ hp.reshape(R, H)
        dwih[l, :, :hx.shape[1]] = a.T @ hx
        db[l] = a.sum(dim=0)
    return dwih, dwhh, db


@pytest.mark.gpu
@pytest.mark.parametrize("T,S,S_pad,L,cin,dtype", [
    # two tiles, ragged S, the t == 0 guard, scalar layer-0 input + a layer >= 1
    (2, 40, 64, 2, 1, torch.bfloat16),
    # dense layer-0 input path
    (2, 64, 64, 2, 64, torch.bfloat16),
    # R = 1056: two chunks, ceil(R/2) = 528 is no multiple of 32, odd tile count
    (3, 352, 352, 1, 1, torch.bfloat16),
    (2, 40, 64, 2, 1, torch.float16),
])
def test_lstm_wgrad_on_tiled_stream(T, S, S_pad, L, cin, dtype):
    from stmgcn_amd.ops.functional import require_hip
    C = require_hip()
    torch.manual_seed(0)
    dev = torch.device("cuda")
    dA = (torch.randn(L, T, S_pad, 4 * H, device=dev) * 0.5).to(dtype)
    hseq = (torch.randn(L, T, S_pad, H, device=dev) * 0.5).to(dtype)
    x = (torch.randn(S, T, cin, device=dev) * 0.5).to(dtype)
    dwih, dwhh, db = C.lstm_wgrad(tile_dA(dA), hseq, x)
    r_ih, r_hh, r_db = _wgrad_reference(dA, hseq, x, S_pad)
    R = T * S_pad
    tol = dict(rtol=2e-2, atol=2e-2 * R ** 0.5)
    torch.testing.assert_close(dwhh, r_hh, **tol)
    torch.testing.assert_close(dwih[0, :, :cin], r_ih[0, :, :cin], **tol)
    if L > 1:
        torch.testing.assert_close(dwih[1:], r_ih[1:], **tol)
    torch.testing.assert_close(db, r_db, **tol)


def _lstm_weights(L, cin, seed=0):
    torch.manual_seed(seed)
    ws = []
    for l in range(L):
        in_l = cin if l == 0 else H
        ws += [torch.randn(4 * H, in_l) * 0.2, torch.randn(4 * H, H) * 0.2,
               torch.randn(4 * H) * 0.1, torch.randn(4 * H) * 0.1]
    return ws


def _gru_weights(L, cin, seed=3):
    torch.manual_seed(seed)
    ws = []
    for l in range(L):
        in_l = cin if l == 0 else H
        ws += [torch.randn(3 * H, in_l) * 0.2, torch.randn(3 * H, H) * 0.2,
               torch.randn(3 * H) * 0.1, torch.randn(3 * H) * 0.1]
    return ws


def _backward_rel_errors(cell, S=40, T=2, L=2, cin=1):
    """FusedLSTMFn backward vs the CPU fp32 oracle: {name: max-abs error
    relative to the oracle's max-abs}."""
    from stmgcn_amd.ops import reference_impl as ref
    from stmgcn_amd.ops.hip_ops import FusedLSTMFn
    ws = _lstm_weights(L, cin) if cell == "lstm" else _gru_weights(L, cin)
    x = torch.randn(S, T, cin)
    x_ref = x.clone().requires_grad_(True)
    ws_ref = [w.clone().requires_grad_(True) for w in ws]
    if cell == "lstm":
        out_ref = ref.lstm_forward(x_ref, ws_ref, torch.zeros(L, S, H),
                                   torch.zeros(L, S, H), False)
    else:
        out_ref, _ = torch._VF.gru(x_ref, torch.zeros(L, S, H), ws_ref, True, L,
                                   0.0, False, False, True)
        out_ref = out_ref[:, -1]
    (out_ref.float() ** 2).sum().backward()

    dev = torch.device("cuda")
    x_g = x.bfloat16().to(dev).requires_grad_(True)
    ws_g = [w.bfloat16().to(dev).requires_grad_(True) for w in ws]
    out = FusedLSTMFn.apply(x_g, cell, False, True, *ws_g)
    (out.float() ** 2).sum().backward()

    def relerr(a, b):
        return ((a.float().cpu() - b).abs().max() / (b.abs().max() + 1e-6)).item()

    errs = {"dx": relerr(x_g.grad, x_ref.grad)}
    for i, (wg, wr) in enumerate(zip(ws_g, ws_ref)):
        errs[f"w{i}"] = relerr(wg.grad, wr.grad)
    return errs


LAYOUT_SHAPES = {
    "": dict(S=40, T=2, L=2, cin=1),      # S_pad = 64: two dA tiles, 8 live rows in the last
    "-S70": dict(S=70, T=2, L=2, cin=1),  # S_pad = 96: three dA tiles, 6 live rows in the last
}


@pytest.mark.gpu
@pytest.mark.parametrize(
    "cell,shape",
    [(cell, shape) for shape in LAYOUT_SHAPES.values() for cell in ("lstm", "gru")],
    ids=[cell + tag for tag in LAYOUT_SHAPES for cell in ("lstm", "gru")])
def test_bwd_and_wgrad_agree_on_layout(cell, shape):
    errs = _backward_rel_errors(cell, **shape)
    print(errs)
    for name, e in errs.items():
        assert e < 0.08, f"{cell} {shape} {name} grad rel err {e}"
