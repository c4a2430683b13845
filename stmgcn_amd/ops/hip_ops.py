"""autograd.Function wrappers over the CDNA4 HIP kernels (stmgcn_amd._C).

Kernel coverage (all landed; SURVEY §2.4 op numbers in parentheses):
  - ChebGconvFn (K1/K2/K10; also the dual random-walk diffusion gconv over
    two generators, dual_gconv.hip): fully fused ChebConv — in-kernel CSR support
    recurrence with the mix GEMM + bias + act as an MFMA epilogue of each
    step; backward = Clenshaw over G^T with the U = dz W^T GEMM fused
    in-kernel + one multi-source atb_wgrad launch for every dW_k.
  - FusedLSTMFn / FusedRNNFn (K5/K6/K10): persistent multi-layer LSTM/GRU
    (fused_rnn.hip) + one batched wgrad launch for ALL layer weight grads
    (wgrad.hip). GRU rides the 4-slot packing documented on FusedLSTMFn.
  - SeqsumPermuteFn (K3), GateFn (K4), HeadFn (K7), FusedMSELossFn (K8);
    the K9 Adam kernel is driven by train/fused_adam.py.
  - HeadMultiFn (K7 with 2..32 output columns: the multi-step horizon) and
    MaskedLossFn (K8 over non-NaN targets: MSE / MAE / Huber).
The reduction kernels (wgrad, head wgrad, the gate's reduces) finish their own
outputs — the last workgroup to arrive rounds the fp32 sums to the parameter
dtype and writes the gradients in their final shapes — so the backward
methods below add no convert / fill / slice launches of their own when the
parameters have the activations' dtype.
Numerics tests compare every Function against the fp32 oracle in
reference_impl.py (tests/test_gpu_kernels.py).
"""
from __future__ import annotations

from typing import Optional

import torch

import os

from . import reference_impl as ref
from .functional import require_hip
from ..graph.preprocess import CSRSupport

# ---------------------------------------------------------------------------
# Fallback policy: the HIP kernels serve fixed shapes (H=64, T<=16, ...).
# Off-shape on the GPU hot path is a HARD ERROR unless the caller explicitly
# sets STMGCN_ALLOW_FALLBACK=1 — a silent torch fallback would bench stock
# PyTorch while reporting impl="hip" (fail-loud principle, functional.py).
# Every allowed fallback is counted so bench.py can surface impl="hip+fallback".
_fallback_count = 0


def fallback_count() -> int:
    return _fallback_count


def reset_fallback_count() -> None:
    global _fallback_count
    _fallback_count = 0


def _fallback(what: str) -> None:
    global _fallback_count
    if os.environ.get("STMGCN_ALLOW_FALLBACK", "0") != "1":
        raise RuntimeError(
            f"HIP kernel path cannot serve {what}; refusing a silent torch "
            "fallback on the GPU hot path. Set STMGCN_ALLOW_FALLBACK=1 to run "
            "the torch op anyway (reported as impl=hip+fallback), or "
            "STMGCN_IMPL=torch for the full stock-PyTorch path.")
    _fallback_count += 1


class ChebGconvFn(torch.autograd.Function):
    """y = act(concat_k(T_k(G) x) @ W + b) — fully fused ChebConv
    (reference GCN.py:34-42 materializes dense (K,N,N)
    stacks offline and a (B,N,K_s,C) feature concat per forward).

    Fused path (bf16/f16, C/Cout <= 64 and mult-of-8, K_s <= 4 — every
    BASELINE config): the K_s recurrence steps run in-kernel with the mix
    GEMM + bias + ReLU folded into each step's MFMA epilogue. Training keeps
    the recurrence states p_k (their HBM writes are mandatory anyway — the
    step dependency crosses workgroups) and the backward computes dX via
    Clenshaw over G^T with U_j = dz W_j^T fused in-kernel, plus ALL
    supports' dW_k in one atb_wgrad_multi launch over [x, p_1, ..]. Zero
    library GEMMs, zero (B,N,K_s,C) concat stacks in either direction.

    Stack path (fp32 parity / larger widths): cheb_apply support stack +
    rocBLAS mix, Clenshaw combine backward.

    csr.kind == "dual" (dual random-walk diffusion, 2K+1 supports
    [I, T_k(G_f).., T_k(G_b)..]): the fused path (same dtype/width limits,
    K <= 3) runs dual_gconv.hip — K forward launches and K+1 dX launches that
    advance both generators together — and two atb_wgrad_multi launches
    ([x, pf_1..pf_K] with db, then [pb_1..pb_K]). Its stack path runs
    cheb_apply / cheb_combine once per generator.
    """

    @staticmethod
    def forward(ctx, x: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor],
                csr: CSRSupport, activation: Optional[str],
                training: bool = True):
        C = require_hip()
        x = x.contiguous()
        Cin = x.shape[-1]
        Cout = W.shape[1]
        Wd = W.to(x.dtype).contiguous()
        fused = (x.dtype in (torch.bfloat16, torch.float16)
                 and Cin <= 64 and Cout <= 64
                 and Cin % 8 == 0 and Cout % 8 == 0
                 # atb_wgrad_multi: <= 4 sources ([x, pf_1..pf_K] for dual)
                 and (csr.K_supports <= 7 if csr.kind == "dual"
                      else csr.K_supports <= 4))
        ctx.fused = fused
        ctx.csr = csr
        ctx.act = activation
        ctx.has_b = b is not None
        ctx.cin = Cin
        if fused:
            bd = b.to(x.dtype).contiguous() if b is not None else None
            act = 1 if activation == "relu" else 0
            if csr.kind == "dual":
                gb = csr.dual
                outs = C.dual_gconv_fused_fwd(
                    x, csr.row_ptr, csr.col_idx, csr.vals,
                    gb.row_ptr, gb.col_idx, gb.vals, Wd, bd,
                    gb.K_supports - 1, act, training)
            else:
                outs = C.cheb_gconv_fused_fwd(
                    x, csr.row_ptr, csr.col_idx, csr.vals, Wd, bd,
                    csr.K_supports, csr.kind == "single", act, training)
            y = outs[0]
            # outs[1:] = the recurrence states, kept for the wgrad (their HBM
            # writes were mandatory regardless): p_1..p_{K_s-1} (p_0 == x), or
            # pf_1..pf_K, pb_1..pb_K for dual
            ctx.save_for_backward(x, Wd, W,
                                  y if activation == "relu" else None,
                                  *outs[1:])
            return y
        if csr.kind == "dual":
            S = torch.cat(
                [C.cheb_apply(x, g.row_ptr, g.col_idx, g.vals, g.K_supports,
                              False)[:, :, skip:]
                 for g, skip in zip(csr.directions(), (0, 1))], dim=2)
        else:
            S = C.cheb_apply(x, csr.row_ptr, csr.col_idx, csr.vals,
                             csr.K_supports, csr.kind == "single")
        B_, N, K, _ = S.shape
        feat = S.view(B_, N, K * Cin)
        if b is not None:
            y = torch.addmm(b.to(feat.dtype), feat.view(-1, K * Cin), Wd)
            y = y.view(B_, N, -1)
        else:
            y = feat @ Wd
        if activation == "relu":
            y = torch.relu_(y)
        ctx.save_for_backward(feat, W, y if activation == "relu" else None)
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        C = require_hip()
        csr: CSRSupport = ctx.csr
        if ctx.fused:
            x, Wd, W, y = ctx.saved_tensors[:4]
            ps = ctx.saved_tensors[4:]       # recurrence states from forward
            # parameters in the activations' dtype (the training setup): the
            # mask is one kernel and the wgrad kernel rounds dW / db itself
            fast = W.dtype == dy.dtype
            if ctx.act != "relu":
                dz = dy.contiguous()
            elif fast:
                dz = C.relu_bwd(dy, y)
            else:
                dz = (dy * (y > 0).to(dy.dtype)).contiguous()
            dual, single = csr.kind == "dual", csr.kind == "single"
            K_s = csr.K_supports
            Cin, Cout = ctx.cin, dz.shape[-1]
            if not ctx.needs_input_grad[0]:
                # x came from the input data (the temporal gconv in training)
                dX = None
            elif dual:
                gb = csr.dual
                dX = C.dual_gconv_fused_bwd_dx(
                    dz, Wd, csr.row_ptr_t, csr.col_idx_t, csr.vals_t,
                    gb.row_ptr_t, gb.col_idx_t, gb.vals_t, gb.K_supports - 1)
            else:
                dX = C.cheb_gconv_fused_bwd_dx(dz, Wd, csr.row_ptr_t,
                                               csr.col_idx_t, csr.vals_t, K_s,
                                               single)
            # ---- dW/db: multi-source MFMA reductions over the saved
            # recurrence states (no concat stack), <= 4 sources per launch
            dz2 = dz.reshape(-1, Cout)
            srcs = [p.reshape(-1, Cin)
                    for p in (ps if single else (x,) + tuple(ps))]
            # dual: rows [0,(K+1)Cin): x, pf_1..pf_K (+ db); rest: pb_1..pb_K
            split = csr.dual.K_supports if dual else len(srcs)
            if fast:
                outs = C.atb_wgrad_multi_grads(srcs, dz2, split, ctx.has_b)
                return (dX, outs[0], outs[1] if ctx.has_b else None,
                        None, None, None)
            dWf = torch.zeros(K_s * Cin, Cout, dtype=torch.float32,
                              device=dz.device)
            db_f = (torch.zeros(Cout, dtype=torch.float32, device=dz.device)
                    if ctx.has_b else None)
            if dual:
                C.atb_wgrad_multi(srcs[:split], dz2, dWf[:split * Cin], db_f)
                C.atb_wgrad_multi(srcs[split:], dz2, dWf[split * Cin:], None)
            else:
                C.atb_wgrad_multi(srcs, dz2, dWf, db_f)   # dz streamed once
            return (dX, dWf.to(W.dtype),
                    db_f.to(W.dtype) if ctx.has_b else None, None, None, None)

        feat, W, y = ctx.saved_tensors
        if ctx.act == "relu":
            dz = dy * (y > 0).to(dy.dtype)
        else:
            dz = dy
        dz = dz.contiguous()
        B_, N, KC = feat.shape
        Cout = dz.shape[-1]
        # tall-skinny reduction GEMM kernel (wgrad.hip): dW = feat^T dZ and
        # db = colsum(dZ) in one launch, fp32 accumulate. (bf16/f16 only —
        # the MFMA tile is 16x16x32_bf16/f16; fp32 parity runs rocBLAS.
        # M/N must be multiples of 8: the kernel issues 16-byte fragment
        # loads at column offsets cb*8 — a ragged tail would read OOB.)
        if (dz.dtype in (torch.bfloat16, torch.float16) and KC <= 256
                and Cout <= 64 and KC % 8 == 0 and Cout % 8 == 0):
            outs = C.atb_wgrad(feat.reshape(-1, KC), dz.reshape(-1, Cout), ctx.has_b)
            dW = outs[0].to(W.dtype)
            db = outs[1].to(W.dtype) if ctx.has_b else None
        else:
            dW = (feat.reshape(-1, KC).T @ dz.reshape(-1, Cout)).to(W.dtype)
            db = dz.sum(dim=(0, 1)).to(W.dtype) if ctx.has_b else None
        U = (dz @ W.to(dz.dtype).T).view(B_, N, csr.K_supports, ctx.cin).contiguous()
        if csr.kind == "dual":
            # one Clenshaw per transpose; U_0 counts once (zeroed 2nd time)
            gf, gb = csr.directions()
            K1 = gf.K_supports
            Ub = torch.cat([torch.zeros_like(U[:, :, :1]), U[:, :, K1:]], dim=2)
            dX = (C.cheb_combine(U[:, :, :K1].contiguous(), gf.row_ptr_t,
                                 gf.col_idx_t, gf.vals_t, False)
                  + C.cheb_combine(Ub, gb.row_ptr_t, gb.col_idx_t, gb.vals_t,
                                   False))
            return dX, dW, db, None, None, None
        dX = C.cheb_combine(U, csr.row_ptr_t, csr.col_idx_t, csr.vals_t,
                            csr.kind == "single")
        return dX, dW, db, None, None, None


def contextual_gate_hip(obs_seq, gconv_out, fc_weight, fc_bias, xs=None,
                        node_major=False):
    if obs_seq.shape[1] <= 16:
        return GateFn.apply(obs_seq, gconv_out, fc_weight, fc_bias, xs,
                            node_major)
    _fallback(f"contextual gate with T={obs_seq.shape[1]} > 16")
    out = ref.contextual_gate(obs_seq, gconv_out, fc_weight, fc_bias)
    return out.permute(0, 2, 1, 3) if node_major else out


def _vf_rnn(cell, x, h0, c0, return_sequences, weights):
    """torch native fused RNN (what nn.LSTM calls). Used for the stock floor
    (STMGCN_IMPL=torch) and as the interim path while fused_rnn.hip lands."""
    L = len(weights) // 4
    if cell == "lstm":
        out, _, _ = torch._VF.lstm(x, (h0, c0), list(weights), True, L, 0.0,
                                   torch.is_grad_enabled(), False, True)
    else:
        out, _ = torch._VF.gru(x, h0, list(weights), True, L, 0.0,
                               torch.is_grad_enabled(), False, True)
    return out if return_sequences else out[:, -1]


class FusedLSTMFn(torch.autograd.Function):
    """Persistent fused multi-layer LSTM/GRU: one kernel
    for all layers x timesteps (forward), one dgrad kernel for the BPTT, one
    batched reduction-GEMM kernel (wgrad.hip) for ALL weight gradients.

    GRU (the deep variant, BASELINE configs[3]) rides the same 4-slot MFMA
    kernels through weight packing — q-slots [r | z | n_input | n_hidden]:
      W_ih_packed = [Wr; Wz; Wn; 0],  W_hh_packed = [Ur; Uz; 0; Un]
      b_ih_packed = [bir; biz; bin; 0], b_hh_packed = [bhr; bhz; 0; bhn]
    and the packed dA stream [dr|dz|dn|dBn] flows through the shared dgrad
    GEMMs and wgrad kernel; grads are un-packed by slicing below.

    Constraints (checked): bf16/f16, H == 64, C_in in {1, 64}, T <= 16,
    L <= 8, zero initial states (the reference zero-inits every forward —
    STMGCN.py:93-98,109, quirk 8)."""

    @staticmethod
    def forward(ctx, x, cell, ret_seq, training, *weights):
        C = require_hip()
        L = len(weights) // 4
        gru = cell == "gru"
        if gru:
            H = weights[1].shape[1]
            w_ih, w_hh, b_ih, b_hh = [], [], [], []
            for l in range(L):
                wi, wh, bi, bh = weights[4 * l:4 * l + 4]
                wp = wi.new_zeros(4 * H, wi.shape[1])
                wp[:3 * H] = wi
                hp = wh.new_zeros(4 * H, H)
                hp[:2 * H] = wh[:2 * H]
                hp[3 * H:] = wh[2 * H:]
                bip = wi.new_zeros(4 * H)
                bhp = torch.zeros_like(bip)
                bip[:3 * H] = bi
                bhp[:2 * H] = bh[:2 * H]
                bhp[3 * H:] = bh[2 * H:]
                w_ih.append(wp.contiguous())
                w_hh.append(hp.contiguous())
                b_ih.append(bip)
                b_hh.append(bhp)
        else:
            w_ih = [weights[4 * l + 0].contiguous() for l in range(L)]
            w_hh = [weights[4 * l + 1].contiguous() for l in range(L)]
            b_ih = [weights[4 * l + 2].contiguous() for l in range(L)]
            b_hh = [weights[4 * l + 3].contiguous() for l in range(L)]
        outs = C.lstm_fwd(x.contiguous(), w_ih, w_hh, b_ih, b_hh, ret_seq,
                          training, gru)
        ctx.ret_seq = ret_seq
        ctx.L = L
        ctx.gru = gru
        if training:
            out, hseq, cseq, gates = outs
            ctx.save_for_backward(x, cseq, gates, hseq, *w_ih, *w_hh)
        else:
            out = outs[0]
        return out

    @staticmethod
    def backward(ctx, dout):
        C = require_hip()
        L = ctx.L
        x, cseq, gates, hseq = ctx.saved_tensors[:4]
        w_ih = ctx.saved_tensors[4:4 + L]        # packed for GRU
        w_hh = ctx.saved_tensors[4 + L:4 + 2 * L]
        x = x.contiguous()
        # parameters in the activations' dtype (the training setup): one pack
        # launch for every transposed weight, and lstm_wgrad rounds, slices
        # and un-packs its own outputs — backward is pack, lstm_bwd, one fill
        # + lstm_wgrad, nothing else
        fast = all(w.dtype == x.dtype for w in ctx.saved_tensors[4:])
        if fast:
            wT = C.lstm_pack_bwd_weights(list(w_ih), list(w_hh))
            w_ihT, w_hhT = wT[:L], wT[L:]
        else:
            w_ihT = [w.t().contiguous() for w in w_ih]
            w_hhT = [w.t().contiguous() for w in w_hh]
        dx, dA = C.lstm_bwd(dout, x, cseq, gates, w_ihT, w_hhT, ctx.ret_seq,
                            ctx.gru)
        S, Tst, cin = x.shape
        # ---- weight grads: ONE batched reduction-GEMM launch for all layers
        # (wgrad.hip; replaces 5 hipBLASLt GEMMs + 3 cat + 3 colsum per call
        # that measured 47.8% of step time — profiles/r01_*)
        if fast:
            return (dx, None, None, None,
                    *C.lstm_wgrad_grads(dA, hseq, x, ctx.gru))
        dwih, dwhh, dbf = C.lstm_wgrad(dA, hseq, x)
        grads = []
        H = 64
        for l in range(L):
            dt = w_ih[l].dtype
            cin_l = cin if l == 0 else H
            if ctx.gru:
                dw_ih = dwih[l, :3 * H, :cin_l].to(dt)
                dw_hh = torch.cat([dwhh[l, :2 * H], dwhh[l, 3 * H:]]).to(dt)
                db_ih = dbf[l, :3 * H].to(dt)
                db_hh = torch.cat([dbf[l, :2 * H], dbf[l, 3 * H:]]).to(dt)
            else:
                dw_ih = dwih[l, :, :cin_l].to(dt)
                dw_hh = dwhh[l].to(dt)
                db_ih = dbf[l].to(dt)
                db_hh = db_ih.clone()
            grads += [dw_ih, dw_hh, db_ih, db_hh]
        return (dx, None, None, None, *grads)


class FusedRNNFn:
    """Dispatch: LSTM/GRU -> fused HIP kernels (bf16/f16, H=64);
    fp32 or off-shape -> torch native fused RNN (the stock floor)."""

    @staticmethod
    def apply(cell, x, h0, c0, return_sequences, *weights):
        gmul = 4 if cell == "lstm" else 3
        if (cell in ("lstm", "gru")
                and x.dtype in (torch.bfloat16, torch.float16)
                and x.shape[-1] in (1, 64)
                and weights[1].shape == (gmul * 64, 64)
                and x.shape[1] <= 16):
            training = torch.is_grad_enabled() and (
                x.requires_grad or any(w.requires_grad for w in weights))
            return FusedLSTMFn.apply(x, cell, return_sequences, training, *weights)
        _fallback(
            f"fused {cell} with dtype={x.dtype}, C_in={x.shape[-1]}, "
            f"T={x.shape[1]}, hidden={tuple(weights[1].shape)} "
            "(served: bf16/f16, C_in in {1,64}, T<=16, H=64)")
        if h0 is None:   # the fused kernels start from zero and never read them
            h0 = x.new_zeros(len(weights) // 4, x.shape[0], weights[1].shape[1])
            c0 = torch.zeros_like(h0) if cell == "lstm" else None
        return _vf_rnn(cell, x, h0, c0, return_sequences, weights)


def branch_fuse_head_hip(branch_feats, fc_weight, fc_bias):
    if (fc_weight.shape[0] == 1 and fc_weight.shape[1] <= 64
            and len(branch_feats) <= 3):
        return HeadFn.apply(fc_weight, fc_bias, *branch_feats)
    _fallback(
        f"fused head with C_out={fc_weight.shape[0]}, G={fc_weight.shape[1]}, "
        f"M={len(branch_feats)} (served: C_out=1, G<=64, M<=3)")
    return ref.branch_fuse_head(branch_feats, fc_weight, fc_bias)


def branch_fuse_head_multi_hip(branch_feats, fc_weight, fc_bias):
    """The wide head (multi-step horizon, O = P*C >= 2 output columns) on the
    MFMA kernels. ops.branch_fuse_head routes here on fc_weight.shape[0] > 1;
    branch_fuse_head_hip stays the one-column entry with its own contract."""
    O, G = fc_weight.shape
    if (2 <= O <= 32 and G <= 64 and G % 8 == 0 and len(branch_feats) <= 3
            and branch_feats[0].dtype in (torch.bfloat16, torch.float16)):
        return HeadMultiFn.apply(fc_weight, fc_bias, *branch_feats)
    _fallback(
        f"fused wide head with C_out={O}, G={G}, M={len(branch_feats)}, "
        f"dtype={branch_feats[0].dtype} (served: 2<=C_out<=32, G<=64 with "
        "G%8==0, M<=3, bf16/f16)")
    return ref.branch_fuse_head(branch_feats, fc_weight, fc_bias)


class SeqsumPermuteFn(torch.autograd.Function):
    """K3: x_seq = obs.sum(-1).permute(0,2,1) as one kernel (reference
    STMGCN.py:36,39); backward broadcasts over T,C."""

    @staticmethod
    def forward(ctx, obs):
        C = require_hip()
        ctx.C = obs.shape[-1]
        return C.seqsum_permute(obs.contiguous())

    @staticmethod
    def backward(ctx, dxs):
        C = require_hip()
        return C.seqsum_permute_bwd(dxs, ctx.C)


class GateFn(torch.autograd.Function):
    """K4: fused contextual gate. The kernel folds the gradient of the
    residual x_seq path (x_seq = sum_c obs) directly into dobs, so the xs
    input gets no separate grad here; the gconv path (xs -> gconv -> g) flows
    through dg and the autograd graph of xs as usual.

    xs: the caller's already-computed seqsum_permute(obs) (the model has it as
    the gconv input), else it is computed here. node_major: the output is
    (B, N, T, C), the sequence layout the RNN reads, and the incoming gradient
    is taken in that layout, so no permute copy runs in either direction.
    dw / db come out of gate_bwd summed over the batch and rounded; dobs is
    neither computed nor stored when obs needs no gradient."""

    @staticmethod
    def forward(ctx, obs, g, fcw, fcb, xs=None, node_major=False):
        C = require_hip()
        obs = obs.contiguous()
        if xs is None:
            with torch.no_grad():
                xs = C.seqsum_permute(obs)
        out, z, u, s = C.gate_fwd(obs, g.contiguous(), xs.detach(),
                                  fcw.to(obs.dtype), fcb.to(obs.dtype),
                                  node_major)
        ctx.save_for_backward(obs, fcw, z, u, s)
        ctx.node_major = node_major
        return out

    @staticmethod
    def backward(ctx, dout):
        C = require_hip()
        obs, fcw, z, u, s = ctx.saved_tensors
        dobs, dg, dw, db, dw_f, db_f = C.gate_bwd(
            dout, obs, fcw.to(obs.dtype), z, u, s, ctx.node_major,
            ctx.needs_input_grad[0])
        if fcw.dtype != obs.dtype:
            dw, db = dw_f.to(fcw.dtype), db_f.to(fcw.dtype)
        return dobs, dg, dw, db, None, None


class HeadFn(torch.autograd.Function):
    """K7: y = (sum_m feats_m) @ w^T + b fused (reference STMGCN.py:116-118)."""

    @staticmethod
    def forward(ctx, fc_weight, fc_bias, *feats):
        C = require_hip()
        y, fsum = C.head_fwd(list(feats), fc_weight.view(-1).to(feats[0].dtype),
                             fc_bias.to(feats[0].dtype))
        ctx.save_for_backward(fc_weight, fsum)
        ctx.M = len(feats)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = require_hip()
        fc_weight, fsum = ctx.saved_tensors
        G = fsum.shape[-1]
        dfeat = C.head_bwd(dy, fc_weight.view(-1).to(dy.dtype), G)
        # dw = dy^T fsum, db = sum(dy) as one reduction kernel (the last
        # library GEMM on the step was exactly this 1xG tall-skinny)
        if fc_weight.dtype == dy.dtype:   # rounded by the kernel itself
            dw, db = C.head_wgrad_grads(dy, fsum)
            return (dw, db) + (dfeat,) * ctx.M
        dwf, dbf = C.head_wgrad(dy, fsum)
        dw = dwf.view(1, G).to(fc_weight.dtype)
        db = dbf.to(fc_weight.dtype)
        return (dw, db) + (dfeat,) * ctx.M


class FusedMSELossFn(torch.autograd.Function):
    """K8: mean((pred-target)^2) with the grad fused (diff saved once)."""

    @staticmethod
    def forward(ctx, pred, target):
        C = require_hip()
        loss, diff = C.mse_fwd(pred, target)
        ctx.save_for_backward(diff)
        return loss

    @staticmethod
    def backward(ctx, gout):
        C = require_hip()
        (diff,) = ctx.saved_tensors
        dpred = C.mse_bwd(diff, gout.detach().reshape(1).float().contiguous())
        return dpred, None


class HeadMultiFn(torch.autograd.Function):
    """K7 wide: y (B, N, O) = (sum_m feats_m) @ W^T + b for 2 <= O <= 32
    output columns (multi-step horizon: column o = p*C + c) on the MFMA
    kernels; fsum is rounded once and saved, the one dfeat tensor is handed to
    every branch and the wgrad kernel finishes dW / db itself, as in HeadFn."""

    @staticmethod
    def forward(ctx, fc_weight, fc_bias, *feats):
        C = require_hip()
        dt = feats[0].dtype
        y, fsum = C.head_multi_fwd(list(feats), fc_weight.to(dt),
                                   fc_bias.to(dt))
        ctx.save_for_backward(fc_weight, fsum)
        ctx.M = len(feats)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = require_hip()
        fc_weight, fsum = ctx.saved_tensors
        dy = dy.contiguous()
        dfeat = C.head_multi_bwd(dy, fc_weight.to(dy.dtype))
        if fc_weight.dtype == dy.dtype:   # rounded by the kernel itself
            dw, db = C.head_multi_wgrad_grads(dy, fsum)
        else:
            dwf, dbf = C.head_multi_wgrad(dy, fsum)
            dw, db = dwf.to(fc_weight.dtype), dbf.to(fc_weight.dtype)
        return (dw, db) + (dfeat,) * ctx.M


MASKED_LOSS_KINDS = {"mse": 0, "mae": 1, "huber": 2}


class MaskedLossFn(torch.autograd.Function):
    """K8 masked: mean of l(pred - target) over the non-NaN targets, l = MSE /
    MAE / Huber(delta = 1). The loss and 1 / max(count_valid, 1) stay on the
    device (no host read, capturable); diff is saved with 0 at masked elements,
    which is all the backward needs (l'(0) = 0 for every kind)."""

    @staticmethod
    def forward(ctx, pred, target, kind):
        C = require_hip()
        res, diff = C.masked_loss_fwd(pred, target, kind)
        ctx.save_for_backward(diff, res)
        ctx.kind = kind
        return res[0]

    @staticmethod
    def backward(ctx, gout):
        C = require_hip()
        diff, res = ctx.saved_tensors
        dpred = C.masked_loss_bwd(
            diff, res, gout.detach().reshape(1).float().contiguous(), ctx.kind)
        return dpred, None, None
