"""The graph-conv gather phases and atb_wgrad at the shapes where the
8-channel vector mapping, its 6-nnz blocks and the wgrad's prefetch can go
wrong: a CSR built by hand with every row degree 0..10, tile tails, one tile
that owns nearly all of the graph's nnz, two different generators for the dual
kernels, and reduction lengths of one to three K-steps with a ragged end.

The graph kernels are called through the raw bindings and judged by the rule
of _lowp_oracle: inputs rounded once to the dtype, oracle = the dense
recurrence in float64 on the CPU, bound(floor, dtype, cap) with the floor from
the same dense recurrence run in the dtype on the CPU. fp32 has no entry in
that rule; its bound is max(3 floor, n 2^-24) with n the number of roundings
on the longest path to one element (K_s C mix products plus, per recurrence
step, the widest row's nnz + 2), i.e. every rounding half an ulp the same way.
"""
import functools

import numpy as np
import pytest
import torch

import _lowp_oracle as lo

pytestmark = pytest.mark.gpu

DEV = "cuda"
K_S = 3   # T_0, T_1, T_2


# ---- hand-built graphs ------------------------------------------------------
def _csr_from_degrees(N, degs, seed, scale=0.5):
    """CSR with degs[r] entries in row r: sorted unique columns drawn over
    [0, N) (column N - 1 is forced into the widest row), random values.
    Returns int32 rowptr, int32 colidx, fp32 vals and the dense fp32 matrix."""
    rng = np.random.default_rng(seed)
    rowptr, cols, vals = [0], [], []
    widest = int(np.argmax(degs))
    for r in range(N):
        d = int(degs[r])
        c = np.sort(rng.choice(N, size=d, replace=False))
        if r == widest and d > 0 and N - 1 not in c:
            c[-1] = N - 1
        cols.extend(c.tolist())
        vals.extend(rng.uniform(-scale, scale, size=d).astype(np.float32).tolist())
        rowptr.append(len(cols))
    rp = torch.tensor(rowptr, dtype=torch.int32)
    ci = torch.tensor(cols, dtype=torch.int32)
    v = torch.tensor(vals, dtype=torch.float32)
    G = torch.zeros(N, N)
    for r in range(N):
        G[r, ci[rp[r]:rp[r + 1]].long()] = v[rp[r]:rp[r + 1]]
    return rp, ci, v, G


def _transpose_csr(G):
    """CSR arrays of G^T from the dense matrix (entries kept where G != 0)."""
    Gt = G.t().contiguous()
    N = Gt.shape[0]
    rowptr, cols, vals = [0], [], []
    for r in range(N):
        nz = torch.nonzero(Gt[r]).flatten()
        cols.extend(nz.tolist())
        vals.extend(Gt[r, nz].tolist())
        rowptr.append(len(cols))
    return (torch.tensor(rowptr, dtype=torch.int32),
            torch.tensor(cols, dtype=torch.int32),
            torch.tensor(vals, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def ladder(N, seed=0):
    """Row r has r % 11 entries: empty rows, every remainder of the 4-wide
    chunks and of the 6-wide blocks, a second full chunk."""
    degs = [min(r % 11, N) for r in range(N)]
    rp, ci, v, G = _csr_from_degrees(N, degs, 100 + seed)
    return {"fwd": (rp, ci, v), "bwd": _transpose_csr(G), "G": G, "maxdeg": max(degs)}


@functools.lru_cache(maxsize=None)
def heavy_tile():
    """N = 96: rows 0..31 dense, every other row one entry, so the first
    tile's CSR segment holds 3072 of the 3136 nnz."""
    N = 96
    degs = [N] * 32 + [1] * (N - 32)
    rp, ci, v, G = _csr_from_degrees(N, degs, 7, scale=0.1)
    return {"fwd": (rp, ci, v), "bwd": _transpose_csr(G), "G": G, "maxdeg": N}


# ---- oracle -----------------------------------------------------------------
def _states(G, x):
    """[x, G x, 2 G (G x) - x] in the dtype of x (the kernels' recurrence)."""
    p1 = torch.einsum("ij,bjc->bic", G, x)
    p2 = 2 * torch.einsum("ij,bjc->bic", G, p1) - x
    return [x, p1, p2]


def _fwd(G, x, W, b):
    ps = _states(G, x)
    y = torch.cat(ps, dim=-1) @ W + b
    return torch.relu(y), ps[1], ps[2]


def _bwd(G, dz, W, C):
    """dX = sum_k T_k(G)^T (dz W_k^T) by the Clenshaw recurrence."""
    U = [dz @ W[k * C:(k + 1) * C].t() for k in range(K_S)]
    Gt = G.t()
    b1 = U[1] + 2 * torch.einsum("ij,bjc->bic", Gt, U[2])
    return U[0] + torch.einsum("ij,bjc->bic", Gt, b1) - U[2]


@functools.lru_cache(maxsize=None)
def cheb_case(graph_key, B, C, Cout, dtype):
    """Rounded inputs, float64 results and low-precision floors, computed once
    per case on the CPU."""
    gr = heavy_tile() if graph_key == "heavy" else ladder(graph_key)
    G = gr["G"]
    N = G.shape[0]
    g = lo._gen("gconv-vector", graph_key, B, C, Cout)
    x = torch.randn(B, N, C, generator=g).to(dtype)
    W = (torch.randn(K_S * C, Cout, generator=g) * 0.15).to(dtype)
    b = (torch.randn(Cout, generator=g) * 0.1).to(dtype)
    dz = torch.randn(B, N, Cout, generator=g).to(dtype)

    def run(dt):
        y, p1, p2 = _fwd(G.to(dt), x.to(dt), W.to(dt), b.to(dt))
        return {"y": y, "p1": p1, "p2": p2,
                "dx": _bwd(G.to(dt), dz.to(dt), W.to(dt), C)}

    want, low = run(torch.float64), run(dtype)
    floor = {k: lo.relerr(low[k], want[k]) for k in want}
    if dtype == lo.F32:
        n = K_S * C + 2 * (gr["maxdeg"] + 2)
        tol = {k: max(3.0 * floor[k], n * 2.0 ** -24) for k in want}
    else:
        tol = {k: lo.bound(floor[k], dtype, lo.CAP_GRAD if k == "dx" else lo.CAP_OUT)
               for k in want}
    return {"graph": gr, "x": x, "W": W, "b": b, "dz": dz, "want": want,
            "floor": floor, "tol": tol}


def _check_cheb(graph_key, B, C, Cout, dtype):
    from stmgcn_amd.ops.functional import require_hip
    _C = require_hip()
    r = cheb_case(graph_key, B, C, Cout, dtype)
    fwd = [t.to(DEV) for t in r["graph"]["fwd"]]
    bwd = [t.to(DEV) for t in r["graph"]["bwd"]]
    y, p1, p2 = _C.cheb_gconv_fused_fwd(r["x"].to(DEV), *fwd, r["W"].to(DEV),
                                        r["b"].to(DEV), K_S, False, 1, True)
    dx = _C.cheb_gconv_fused_bwd_dx(r["dz"].to(DEV), r["W"].to(DEV), *bwd, K_S, False)
    got = {"y": y, "p1": p1, "p2": p2, "dx": dx}
    bad = []
    for k in sorted(got):
        e = lo.relerr(got[k], r["want"][k])
        print(f"{graph_key} C={C} Cout={Cout} {lo.dtype_name(dtype)} {k}: "
              f"err {e:.3e} floor {r['floor'][k]:.3e} tol {r['tol'][k]:.3e}")
        if not e <= r["tol"][k]:
            bad.append(f"{k}: err {e:.3e} > tol {r['tol'][k]:.3e}")
    assert not bad, "; ".join(bad)


# ---- 1. degree ladder -------------------------------------------------------
LADDER_CASES = [(C, Cout, dt) for C, Cout in ((8, 8), (24, 40), (40, 64), (64, 64), (64, 8))
                for dt in lo.LOWP] + [(24, 40, lo.F32)]


@pytest.mark.parametrize("C,Cout,dtype", LADDER_CASES,
                         ids=lambda v: lo.dtype_name(v) if isinstance(v, torch.dtype) else str(v))
def test_degree_ladder(C, Cout, dtype):
    """N = 37, degrees 0..10: y, p_1, p_2 of the K_s = 3 training forward and
    dX on the explicit transpose."""
    _check_cheb(37, 2, C, Cout, dtype)


# ---- 2. tile tails ----------------------------------------------------------
@pytest.mark.parametrize("N", [31, 32, 33, 65])
def test_tile_tails(N):
    """Last tile short, exact, one row over, three tiles."""
    _check_cheb(N, 2, 64, 64, lo.BF16)


# ---- 3. one tile owns nearly every nnz --------------------------------------
def test_large_csr_segment():
    r = cheb_case("heavy", 2, 64, 64, lo.BF16)
    for k, w in r["want"].items():
        assert torch.isfinite(w).all(), k
        cap = lo.CAP_GRAD if k == "dx" else lo.CAP_OUT
        assert 3.0 * r["floor"][k] < cap, (k, r["floor"][k])
    _check_cheb("heavy", 2, 64, 64, lo.BF16)


# ---- 4. dual gconv on two different ladders ---------------------------------
@functools.lru_cache(maxsize=None)
def dual_case(C, Cout, dtype):
    N, B, K = 37, 2, 2
    gf, gb = ladder(N, 1), ladder(N, 2)

    def stack(dt):
        Gf, Gb = gf["G"].to(dt), gb["G"].to(dt)
        eye = torch.eye(N, dtype=dt)
        return torch.stack([eye, Gf, 2 * Gf @ Gf - eye, Gb, 2 * Gb @ Gb - eye])

    g = lo._gen("gconv-vector-dual", C, Cout)
    inputs = {
        "x": torch.randn(B, N, C, generator=g).to(dtype),
        "W": (torch.randn((2 * K + 1) * C, Cout, generator=g) * 0.15).to(dtype),
        "b": (torch.randn(Cout, generator=g) * 0.1).to(dtype),
    }

    def fn(t):
        return lo.ref.gconv_mix_dense(stack(t["x"].dtype), t["x"], t["W"], t["b"], None)

    return lo.make_reference(fn, inputs, ("x",), dtype, extra={"gf": gf, "gb": gb})


@pytest.mark.parametrize("C,Cout", [(64, 64), (8, 8)])
def test_dual_two_ladders(C, Cout):
    """K = 2, forward and backward generators with different row degrees:
    y of the training forward, and dX from dz = d(sum y^2)/dy as the suite's
    oracle (_dual_oracle / make_reference) defines it."""
    from stmgcn_amd.ops.functional import require_hip
    _C = require_hip()
    r = dual_case(C, Cout, lo.BF16)
    gf, gb = r.extra["gf"], r.extra["gb"]
    dev = lambda ts: [t.to(DEV) for t in ts]
    W = r.inputs["W"].to(DEV)
    outs = _C.dual_gconv_fused_fwd(r.inputs["x"].to(DEV), *dev(gf["fwd"]),
                                   *dev(gb["fwd"]), W, r.inputs["b"].to(DEV), 2, 0, True)
    y = outs[0]
    assert len(outs) == 5
    dz = (2.0 * y.float()).to(y.dtype)
    dx = _C.dual_gconv_fused_bwd_dx(dz, W, *dev(gf["bwd"]), *dev(gb["bwd"]), 2)
    r.check({"out": y, "dx": dx}, f"dual ladders C={C} Cout={Cout}")


# ---- 5. atb_wgrad_multi and its finishing form ------------------------------
ATB_ROWS = (1, 31, 33, 64, 65, 129, 4097)
ATB_TOL = lambda rows: dict(rtol=2e-2, atol=2e-2 * rows ** 0.5)   # _check_atb_multi


def _atb_inputs(nsrc, CA, N, rows, dtype, tag):
    g = lo._gen("atb-vector", nsrc, CA, N, rows, lo.dtype_name(dtype), tag)
    As = [(torch.randn(rows, CA, generator=g) * 0.5).to(dtype) for _ in range(nsrc)]
    Bm = (torch.randn(rows, N, generator=g) * 0.5).to(dtype)
    want = torch.cat([a.double().T @ Bm.double() for a in As])
    return As, Bm, want, Bm.double().sum(dim=0)


def _check_atb(nsrc, CA, N, rows, dtype):
    from stmgcn_amd.ops.functional import require_hip
    _C = require_hip()
    tol = ATB_TOL(rows)
    As, Bm, want, db_want = _atb_inputs(nsrc, CA, N, rows, dtype, 0)
    As_d, B_d = [a.to(DEV) for a in As], Bm.to(DEV)
    Cg = torch.zeros(nsrc * CA, N, device=DEV)
    dbg = torch.zeros(N, device=DEV)
    _C.atb_wgrad_multi(As_d, B_d, Cg, dbg)
    torch.testing.assert_close(Cg.cpu().double(), want, **tol)
    torch.testing.assert_close(dbg.cpu().double(), db_want, **tol)
    # finishing form, twice back to back: the second call's workspace is the
    # block the first one's has just returned to the allocator
    dW1, db1 = _C.atb_wgrad_multi_grads(As_d, B_d, nsrc, True)
    As2, Bm2, want2, db_want2 = _atb_inputs(nsrc, CA, N, rows, dtype, 1)
    dW2, db2 = _C.atb_wgrad_multi_grads([a.to(DEV) for a in As2], Bm2.to(DEV), nsrc, True)
    assert dW1.dtype == dtype and dW1.shape == (nsrc * CA, N) and db1.shape == (N,)
    torch.testing.assert_close(dW1.cpu().double(), want, **tol)
    torch.testing.assert_close(db1.cpu().double(), db_want, **tol)
    torch.testing.assert_close(dW2.cpu().double(), want2, **tol)
    torch.testing.assert_close(db2.cpu().double(), db_want2, **tol)


def test_atb_wgrad_empty_chunk():
    """131073 rows: the 512-workgroup cap gives chunks of 257 rows, and the
    last workgroup starts past the end; it must add nothing and still arrive
    at the finishing form's ticket."""
    _check_atb(1, 8, 8, 131073, lo.BF16)


@pytest.mark.parametrize("N", [8, 40, 64])
@pytest.mark.parametrize("nsrc,CA", [(3, 64), (3, 8), (1, 24), (4, 40)])
def test_atb_wgrad_ksteps(nsrc, CA, N):
    """One, two and three K-steps per workgroup with a ragged last one, the
    accumulate-only form and the finishing form on a recycled workspace."""
    for rows in ATB_ROWS:
        _check_atb(nsrc, CA, N, rows, lo.BF16)
    _check_atb(nsrc, CA, N, 33, lo.F16)
