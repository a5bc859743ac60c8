"""Stochastic-depth compaction at its edges: the live counts where a tile ends (none / one / all samples kept, the T = 129 counts
whose 208-row tile stops short of the 64-row K-tile, multiples of 256, 64 k + 1), the 208-row tiles the hidden-width products take
at 128 x 129 token rows, and memory that holds NaN wherever nobody wrote (a poison context over torch.empty / torch.empty_like).

The unwritten-row contract these check (include/editor_hip.h, next to editor_gemm_h16_rows): a live-row PRODUCER writes every row
below roundup64(live) - rows [live, roundup64) from the zero rows of the compacted operand - and a live-row REDUCTION (the weight
gradients' whole 64-row K-tiles, the dgrad column sums, the compacted LayerNorm backward) reads nothing at or past roundup64(live)
(column sums and the LayerNorm backward: nothing at or past live).  Every kernel is compared with an fp64 reference on the live rows
- the L2 error AND the worst row of the tiles around live, roundup64(live) and the last row, where a wrong 16-row fragment would
not show in an L2 figure over 16 k rows - and, where the code claims it, bit for bit with its dense counterpart."""
import pytest
import torch

from conftest import rel_err
from edge_helpers import _NoCtx, _Poison, _boundary_rows, _check, _gelu64, _gelu_grad64, _gen, _randn, _up   # noqa: F401
from editor_amd import config, functional as fn, ops, synth

pytestmark = pytest.mark.gpu

T, B, D, HID = 129, 128, 768, 3072
M1 = B * T                      # 16 512 token rows: 208-row tiles on the (m, 3072) AND the (m, 768) products
M3 = 3 * B * T                  # 49 536: the headline's three modalities (208-row tiles on the (m, 768) products)
TOL16 = {torch.bfloat16: 4e-3, torch.float16: 5e-4}
TOL32, TOL_WG, TOL_CS = 1e-5, 2e-5, 1e-5
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def hazard_counts(b=B, t=T, th=208):
    """live sample counts nl whose nl * t rows end a th-row tile before their 64-row K-tile ends"""
    return [nl for nl in range(1, b + 1) if _up(nl * t, th) < _up(nl * t, 64)]


HZ = hazard_counts()


def _edge_counts(b):
    """live SAMPLE counts: none, one, the smallest / largest hazard count (the largest is 108), all"""
    assert HZ and 108 in HZ, HZ
    return sorted({0, 1, min(HZ), 108, max(HZ), b})


# live ROW counts of the kernel-level products: one sample (2 x 64 + 1), the hazard counts, an exact multiple of 256, all rows
LIVE_ROWS = sorted({T, min(HZ) * T, 108 * T, max(HZ) * T, 40 * 256, M1})


def _assert_short_tiles():
    # keeps these tests from going vacuous if the tile heuristic changes
    assert ops.gemm_tile_plan(M1, HID) == (208, False)
    assert ops.gemm_tile_rows(M1, HID) == 208
    assert ops.gemm_tile_plan(M1, D) == (208, False) and ops.gemm_tile_plan(M3, D) == (208, False)
    assert ops.gemm_tile_rows(M1, D) == 208 and ops.gemm_tile_rows(M3, D) == 208


def test_tile_plan_takes_short_tiles_at_these_shapes():
    assert HZ and min(HZ) < 108 and max(HZ) == 108       # (108 x 129 = 13 932: roundup208 13 936 < roundup64 13 952)
    _assert_short_tiles()
    for nl in (min(HZ), 108, max(HZ)):
        assert _up(nl * T, 208) < _up(nl * T, 64)


def _keep(b, nl, seed):
    """bool (b,): exactly nl samples kept, at random positions"""
    k = torch.zeros(b, dtype=torch.bool)
    k[torch.randperm(b, generator=torch.Generator().manual_seed(seed))[:nl]] = True
    return k


def _scales(keeps, t=T, rate=0.1):
    """keeps (L, 2, b) bool -> scales (L, 2, b*t) as the drop-path kernel writes them (kept: 1 / keep_prob, dropped: 0)"""
    s = keeps.float() / (1.0 - rate)
    return s.unsqueeze(-1).expand(*s.shape, t).reshape(s.shape[0], 2, -1).contiguous().cuda()


def _plan(b, nl, seed, t=T):
    """(rowscale, perm, inv, live (1,) int32) of one MLP branch with exactly nl of b samples kept"""
    keeps = torch.stack([_keep(b, b, 0), _keep(b, nl, seed)]).unsqueeze(0)
    sc = _scales(keeps, t)
    perm, inv, live = ops.droppath_plan(sc, 1, b, t)
    assert int(live[0, 1]) == nl * t
    return sc[0, 1].contiguous(), perm[0, 1].contiguous(), inv[0, 1].contiguous(), live[0, 1:2].contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# a. the plan
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [B, 3 * B])
def test_droppath_plan_at_edge_live_counts(b):
    pats = [_keep(b, nl, 31 + nl) for nl in _edge_counts(b)]
    first, last = torch.zeros(b, dtype=torch.bool), torch.zeros(b, dtype=torch.bool)
    first[0], last[-1] = True, True
    pats += [first, last]
    keeps = torch.stack([torch.stack([_keep(b, (3 * b) // 4, 7 + i), p]) for i, p in enumerate(pats)])     # (L, 2, b)
    sc = _scales(keeps)
    L = keeps.shape[0]
    perm, inv, live = ops.droppath_plan(sc, L, b, T)
    keep = keeps.cuda()
    assert torch.equal(live.long(), keep.sum(-1) * T)
    ar = torch.arange(b * T, device="cuda")
    tt = torch.arange(T, device="cuda")
    for l in range(L):
        for br in range(2):
            p, q, k = perm[l, br].long(), inv[l, br].long(), keep[l, br]
            assert torch.equal(q[p], ar) and torch.equal(p[q], ar)
            pos_live = torch.cumsum(k.long(), 0) - 1
            pos_dead = int(k.sum()) + torch.cumsum((~k).long(), 0) - 1
            slot = torch.where(k, pos_live, pos_dead)
            assert torch.equal(p, (slot[:, None] * T + tt[None]).reshape(-1))


# ---------------------------------------------------------------------------------------------------------------------------------
# b. LayerNorm-2 onto the compacted rows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "f16", "f16x2"])
@pytest.mark.parametrize("m", [M1, M3])
def test_layernorm_fwd_perm_at_edge_live_counts(mode, m, monkeypatch):
    b = m // T
    x = _randn((m, D), 1) * 2.0 + 0.5
    gam, bet = _randn((D,), 2) * 0.5 + 1.0, _randn((D,), 3) * 0.2
    x64 = x.double()
    mu = x64.mean(1, keepdim=True)
    ref = (x64 - mu) / torch.sqrt(((x64 - mu) ** 2).mean(1, keepdim=True) + 1e-6) * gam.double() + bet.double()
    split = mode == "f16x2"
    dt = torch.float16 if split else DTYPES[mode]
    if split:
        dhi, dlo, m0, r0 = ops.layernorm_fwd_split(x, gam, bet, 1e-6)
    else:
        dhi, m0, r0 = ops.layernorm_fwd(x, gam, bet, 1e-6, dt)
    for nl in _edge_counts(b):
        rs, p, q, lv = _plan(b, nl, 100 + nl)
        live = nl * T
        copy = torch.full_like(x, float("nan"))
        with _Poison(monkeypatch):
            if split:
                hi, lo, m1, r1 = ops.layernorm_fwd_split_perm(x, gam, bet, 1e-6, p, rs, copy)
            else:
                hi, m1, r1 = ops.layernorm_fwd_perm(x, gam, bet, 1e-6, dt, p, rs, copy)
        torch.cuda.synchronize()
        assert torch.equal(m0, m1) and torch.equal(r0, r1)
        kept, rows = rs != 0, q[:live].long()               # rows: token row of each live slot
        assert torch.equal(hi[:live], dhi[rows]), nl        # live rows: the dense LayerNorm's bits
        assert bool((hi[live:] == 0).all()), nl             # behind them: exact zeros (poisoned output)
        if split:
            assert torch.equal(lo[:live], dlo[rows]) and bool((lo[live:] == 0).all()), nl
            got = hi[:live].double() + lo[:live].double()
            _check(got, ref[rows], TOL32, m, ("f16x2 LN", nl))
        else:
            _check(hi[:live], ref[rows], TOL16[dt], m, (mode, "LN", nl))
        assert torch.equal(copy[~kept], x[~kept]) and bool(torch.isnan(copy[kept]).all()), nl


# ---------------------------------------------------------------------------------------------------------------------------------
# c. fc1 forward: GELU + gelu' (EPI_AUX_GRAD) on the live prefix
# ---------------------------------------------------------------------------------------------------------------------------------
def _compacted(live, m, n, seed):
    """(m, n) fp32: random rows below live, zero rows [live, m) - what LayerNorm-2 writes onto the compacted rows"""
    x = torch.zeros(m, n, device="cuda")
    x[:live] = _randn((live, n), seed)
    return x


@pytest.mark.parametrize("mode", ["bf16", "f16", "f16x2"])
@pytest.mark.parametrize("live", LIVE_ROWS)
def test_fc1_forward_writes_every_row_the_weight_gradient_reads(mode, live):
    _assert_short_tiles()
    m, r64 = M1, _up(live, 64)
    h32 = _compacted(live, m, D, 11)
    w32, b32 = _randn((HID, D), 12, 0.03), _randn((HID,), 13, 0.1)
    lv = torch.tensor([live], dtype=torch.int32, device="cuda")
    split = mode == "f16x2"
    dt = torch.float16 if split else DTYPES[mode]
    epi = ops.EPI_GELU | ops.EPI_AUX_GRAD

    def run(m_live):
        g = torch.full((m, HID), float("nan"), dtype=dt, device="cuda")
        a = torch.full_like(g, float("nan"))
        gl = torch.full_like(g, float("nan")) if split else None
        if split:
            ops.gemm_split(ops.split_f32(h32), ops.split_f32(w32, ops.SPLIT_WSCALE), g, gl, m, HID, D,
                           alpha=1.0 / ops.SPLIT_WSCALE, bias=b32, epilogue=epi, aux=a, m_live=m_live, live_dense=m_live is not None)
        else:
            ops.gemm(h32.to(dt), w32.to(dt), g, m, HID, D, D, D, HID, 0, 0, bias=b32, epilogue=epi, aux=a, m_live=m_live,
                     live_dense=m_live is not None)
        return g, a, gl
    g, a, gl = run(lv)
    gd, ad, gld = run(None)
    torch.cuda.synchronize()
    # the contract the weight gradients need: rows [live, roundup64(live)) of BOTH outputs are written (finite)
    assert bool(torch.isfinite(g[live:r64]).all()), ("g rows behind live", live, r64)
    assert bool(torch.isfinite(a[live:r64]).all()), ("gelu' rows behind live", live, r64)
    if split:
        assert bool(torch.isfinite(gl[live:r64]).all())
    # live rows: the dense product's bits, and fp64
    assert torch.equal(g[:live], gd[:live]) and torch.equal(a[:live], ad[:live])
    hq = h32[:live].double() if split else h32[:live].to(dt).double()
    wq = w32.double() if split else w32.to(dt).double()
    pre = hq @ wq.t() + b32.double()
    if split:
        assert torch.equal(gl[:live], gld[:live])
        _check(g[:live].double() + gl[:live].double(), _gelu64(pre), TOL32, m, ("f16x2 gelu", live))
    else:
        _check(g[:live], _gelu64(pre), TOL16[dt], m, (mode, "gelu", live))
    _check(a[:live], _gelu_grad64(pre), TOL16[dt], m, (mode, "gelu'", live))


# ---------------------------------------------------------------------------------------------------------------------------------
# d. fc2 dgrad (GELU' + column sums) and fc1 dgrad on the live prefix
# ---------------------------------------------------------------------------------------------------------------------------------
def _live_operand(live, m, n, seed, dt, std=1.0, tail=0.0):
    """(m, n) 16-bit: random below live, `tail` in [live, roundup64(live)), NaN from roundup64(live) on (not to be read)"""
    x = torch.full((m, n), float("nan"), device="cuda")
    r64 = _up(live, 64)
    x[:live] = _randn((live, n), seed, std)
    x[live:r64] = tail
    return x.to(dt)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("live", LIVE_ROWS)
def test_mlp_dgrads_on_the_live_prefix(dtype, live):
    _assert_short_tiles()
    dt, m, r64 = DTYPES[dtype], M1, _up(live, 64)
    lv = torch.tensor([live], dtype=torch.int32, device="cuda")
    dy = _live_operand(live, m, D, 21, dt)                                             # fc2's output gradient (compacted)
    a = torch.full((m, HID), float("nan"), device="cuda")
    a[:r64] = torch.rand(r64, HID, generator=_gen(22), device="cuda") * 1.2 - 0.1       # gelu'(pre-activation), from fc1
    a = a.to(dt)
    w2, w1 = _randn((D, HID), 23, 0.03).to(dt), _randn((HID, D), 24, 0.03).to(dt)
    w2t, w1t = w2.t().contiguous(), w1.t().contiguous()                                # the k-major copies the dgrads take

    def fc2_dgrad(dy_, a_, m_live):
        da = torch.full((m, HID), float("nan"), dtype=dt, device="cuda")
        cs = torch.full((HID,), float("nan"), device="cuda")
        ops.gemm(dy_, w2t, da, m, HID, D, D, D, HID, 0, 0, epilogue=ops.EPI_GELU_BWD | ops.EPI_AUX_GRAD, aux=a_, m_live=m_live,
                 colsum=cs, colsum_scale=1.0, live_dense=m_live is not None)
        return da, cs
    da, cs = fc2_dgrad(dy, a, lv)
    dyd, ad = dy.clone(), a.clone()                                                    # dense twin: finite everywhere
    dyd[live:] = 0
    ad[r64:] = 0.5
    dad, csd = fc2_dgrad(dyd, ad, None)
    torch.cuda.synchronize()
    assert torch.equal(da[:live], dad[:live])
    assert bool((da[live:r64] == 0).all()), ("da rows [live, roundup64)", live)
    assert torch.isfinite(cs).all() and torch.equal(cs, csd)
    ref = (dy[:live].double() @ w2.double()) * a[:live].double()
    _check(da[:live], ref, TOL16[dt], m, (dtype, "fc2 dgrad", live))
    if live:
        assert rel_err(cs, da[:live].double().sum(0)) < TOL_CS
    else:
        assert bool((cs == 0).all())
    # fc1 dgrad: dh2 = da W1 on the live prefix (its rows [live, roundup64) zero, NaN behind)
    dain = _live_operand(live, m, HID, 25, dt)
    dh2 = torch.full((m, D), float("nan"), dtype=dt, device="cuda")
    ops.gemm(dain, w1t, dh2, m, D, HID, HID, HID, D, 0, 0, m_live=lv, live_dense=True)
    daind = dain.clone()
    daind[live:] = 0
    dh2d = torch.empty(m, D, dtype=dt, device="cuda")
    ops.gemm(daind, w1t, dh2d, m, D, HID, HID, HID, D, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(dh2[:live], dh2d[:live])
    _check(dh2[:live], dain[:live].double() @ w1.double(), TOL16[dt], m, (dtype, "fc1 dgrad", live))


# ---------------------------------------------------------------------------------------------------------------------------------
# e. the grouped weight gradients with a live count per problem
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("lives", [(min(HZ) * T, 108 * T, 0), (T, max(HZ) * T, 40 * 256), (M1, 40 * 256 + 1, 0)])
def test_wgrad_group_live_counts_per_problem(dtype, lives):
    dt, m = DTYPES[dtype], M1
    shapes = [(D, D), (D, HID), (HID, D), (D, D)]                   # (n_i, k_i): one dense problem, three on live prefixes
    ops_ = []
    for i, (n, k) in enumerate(shapes):
        if i == 0:
            dy, x, live = _randn((m, n), 40, 0.5).to(dt), _randn((m, k), 41).to(dt), m
        else:
            live = lives[i - 1]
            dy = _live_operand(live, m, n, 42 + i, dt, 0.5)          # rows [live, roundup64): zero (the contract)
            x = _live_operand(live, m, k, 52 + i, dt, 1.0, tail=0.75)   # ... finite, not zero, in the other operand
        ops_.append((dy, x, live))

    def run():
        jobs = []
        for i, ((n, k), (dy, x, live)) in enumerate(zip(shapes, ops_)):
            dw = torch.full((n, k), float("nan"), device="cuda")
            jobs.append((dy, x, dw) if i == 0 else (dy, x, dw, torch.tensor([live], dtype=torch.int32, device="cuda")))
        ops.gemm_wgrad_group(jobs, m, 1.0)
        return [j[2] for j in jobs]
    dw1, dw2 = run(), run()
    torch.cuda.synchronize()
    for i, ((dy, x, live), a, b_) in enumerate(zip(ops_, dw1, dw2)):
        assert torch.equal(a, b_), ("not deterministic", i)
        if live == 0:
            assert bool((a == 0).all()), i
            continue
        ref = dy[:live].double().t() @ x[:live].double()
        assert rel_err(a, ref) < TOL_WG, (i, live, rel_err(a, ref))
        per = ((a.double() - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)).max().item()
        assert per < TOL_WG, (i, live, "worst row", per)


# ---------------------------------------------------------------------------------------------------------------------------------
# f. the compacted backward casts: cast_rows_colsum(perm=) and the LayerNorm backward on compacted dy
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_compacted_casts_and_layernorm_backward(dtype):
    dt, m, b = DTYPES[dtype], M1, B
    gs = 1.0 if dt == torch.bfloat16 else 1024.0
    dev = torch.device("cuda", 0)
    x1 = _randn((m, D), 61) * 1.5 + 0.2
    gam, bet = _randn((D,), 62) * 0.5 + 1.0, _randn((D,), 63) * 0.2
    _, mean, rstd = ops.layernorm_fwd(x1, gam, bet, 1e-6, dt)
    dx_in = _randn((m, D), 64, 0.5)
    xhat = (x1.double() - mean.double()[:, None]) * rstd.double()[:, None]
    for nl in _edge_counts(b):
        rs, p, q, lv = _plan(b, nl, 200 + nl)
        rs_c, p_c, _, _ = _plan(b, max(HZ), 300 + nl)               # the consumer branch of the cast (the block below's MLP)
        live = nl * T
        pl = p.long()
        # cast_rows_colsum onto the compacted rows vs its dense _parts form
        rq = ops.ReduceQueue(dev)
        out_p, cs_p = ops.cast_rows_colsum(dx_in, rs, dt, gs, rq=rq, perm=p)
        rq.flush()
        rq = ops.ReduceQueue(dev)
        out_d, cs_d = ops.cast_rows_colsum(dx_in, rs, dt, gs, rq=rq)
        rq.flush()
        torch.cuda.synchronize()
        assert torch.equal(out_p[pl], out_d) and bool((out_p[live:] == 0).all()) and torch.equal(cs_p, cs_d), nl
        kept = rs != 0
        _check(out_d[kept], (dx_in.double() * rs.double()[:, None] * gs)[kept], TOL16[dt], m, (dtype, "cast", nl))
        assert rel_err(cs_p, out_d.double().sum(0) / gs) < TOL_CS or (nl == 0 and bool((cs_p == 0).all())), nl
        # LayerNorm backward: dy on the compacted rows (slots >= live NaN: not read), the cast onto the consumer's rows
        dyc = torch.full((m, D), float("nan"), device="cuda")
        dyc[:live] = _randn((live, D), 70 + nl) * gs * 1e-2
        dyc = dyc.to(dt)
        dyd = torch.zeros(m, D, dtype=dt, device="cuda")
        dyd[kept] = dyc[pl[kept]]
        rq = ops.ReduceQueue(dev)
        res_p = ops.layernorm_bwd_cast(dyc, x1, gam, mean, rstd, dx_in, rs_c, gs, dy_scale=1.0 / gs, rq=rq, dy_perm=p, dy_live=lv,
                                       cast_perm=p_c)
        rq.flush()
        rq = ops.ReduceQueue(dev)
        res_d = ops.layernorm_bwd_cast(dyd, x1, gam, mean, rstd, dx_in, rs_c, gs, dy_scale=1.0 / gs, rq=rq)
        rq.flush()
        torch.cuda.synchronize()
        dx_p, dg_p, db_p, c16_p, cs16_p = res_p
        dx_d, dg_d, db_d, c16_d, cs16_d = res_d
        assert torch.equal(dx_p, dx_d) and torch.equal(dg_p, dg_d) and torch.equal(db_p, db_d), nl
        assert torch.equal(c16_p[p_c.long()], c16_d) and torch.equal(cs16_p, cs16_d), nl
        assert all(bool(torch.isfinite(t_).all()) for t_ in res_p), nl
        gdy = dyd.double() / gs * gam.double()
        dx_ref = dx_in.double() + rstd.double()[:, None] * (gdy - gdy.mean(1, keepdim=True)
                                                            - xhat * (gdy * xhat).mean(1, keepdim=True))
        _check(dx_p, dx_ref, TOL32, m, (dtype, "LN bwd dx", nl))
        if nl:
            assert rel_err(dg_p, (dyd.double() / gs * xhat).sum(0)) < TOL_CS, nl
            assert rel_err(db_p, (dyd.double() / gs).sum(0)) < TOL_CS, nl
        ref16 = dx_ref * rs_c.double()[:, None] * gs
        kc = rs_c != 0
        _check(c16_d[kc], ref16[kc], TOL16[dt], m, (dtype, "LN bwd cast", nl))
        assert rel_err(cs16_p, c16_d.double().sum(0) / gs) < TOL_CS, nl


# ---------------------------------------------------------------------------------------------------------------------------------
# g. fc2 forward with the row scatter, 208-row tiles
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "f16", "f16x2"])
@pytest.mark.parametrize("m", [M1, M3])
def test_fc2_row_scatter_at_edge_live_counts(mode, m):
    _assert_short_tiles()
    b = m // T
    split = mode == "f16x2"
    dt = torch.float16 if split else DTYPES[mode]
    x1 = _randn((m, D), 81)
    g32 = _randn((m, HID), 82)
    w32, bias = _randn((D, HID), 83, 0.02), _randn((D,), 84, 0.1)
    gp = ops.split_f32(g32) if split else None
    wp = ops.split_f32(w32, ops.SPLIT_WSCALE) if split else w32.to(dt)
    g16 = None if split else g32.to(dt)
    for nl in (1, min(HZ), 108, max(HZ), b):
        rs, p, q, lv = _plan(b, nl, 400 + nl)
        live, pl, dead = nl * T, p.long(), rs == 0
        dense = torch.empty_like(x1)
        out = torch.full_like(x1, float("nan"))
        out[dead] = x1[dead]                                       # what LayerNorm-2 leaves for the dropped rows
        if split:
            hi, lo = (torch.full_like(gp[0], float("nan")) for _ in range(2))
            hi[pl], lo[pl] = gp[0], gp[1]                          # compacted operand, NaN behind the live prefix
            hi[live:], lo[live:] = float("nan"), float("nan")
            ops.gemm_split(gp, wp, dense, None, m, D, HID, alpha=1.0 / ops.SPLIT_WSCALE, bias=bias, rowscale=rs,
                           epilogue=ops.EPI_RESIDUAL, aux=x1)
            ops.gemm_split((hi, lo), wp, out, None, m, D, HID, alpha=1.0 / ops.SPLIT_WSCALE, bias=bias, rowscale=rs,
                           epilogue=ops.EPI_RESIDUAL, aux=x1, m_live=lv, live_dense=True, rowmap=q)
        else:
            gc = torch.full_like(g16, float("nan"))
            gc[pl] = g16
            gc[live:] = float("nan")
            ops.gemm(g16, wp, dense, m, D, HID, HID, HID, D, 0, 0, bias=bias, rowscale=rs, epilogue=ops.EPI_RESIDUAL | ops.EPI_FORCE_PP,
                     aux=x1)
            ops.gemm(gc, wp, out, m, D, HID, HID, HID, D, 0, 0, bias=bias, rowscale=rs, epilogue=ops.EPI_RESIDUAL, aux=x1,
                     m_live=lv, live_dense=True, rowmap=q)
        torch.cuda.synchronize()
        assert torch.equal(out[~dead], dense[~dead]), nl           # live rows: the dense product's bits
        assert torch.equal(out[dead], x1[dead]), nl                # dropped rows: exactly x1
        gq = (gp[0].double() + gp[1].double()) if split else g16.double()
        wq = w32.double() if split else wp.double()
        rows = q[:live].long()
        ref = x1[rows].double() + rs[rows].double()[:, None] * (gq[rows] @ wq.t() + bias.double())
        _check(out[rows], ref, TOL32, m, (mode, "fc2 scatter", nl))


# ---------------------------------------------------------------------------------------------------------------------------------
# h. two chained blocks at 128 x 129 token rows, hazard live counts, poisoned memory
# ---------------------------------------------------------------------------------------------------------------------------------
def _grad_tolerances(name):
    if name.endswith("weight") and (".mlp.fc" in name or ".attn." in name):
        return TOL_WG
    return 1e-4                                                     # bias / LayerNorm gradients: partial-row folds regrouped


@pytest.mark.parametrize("mode", ["bf16", "f16", "f16x2"])
def test_two_blocks_with_hazard_live_counts(mode, monkeypatch):
    _assert_short_tiles()
    from editor_amd.modeling import make_model
    from editor_amd.modeling.make_model import _block_args
    cfg, c, cams = config.preset("RGBNT201", compute_dtype=mode, drop_path=0.1)
    model = make_model(cfg, c, cams)
    synth.fill_state_dict_(model.state_dict(), 13)
    model = model.cuda()
    base = model.BACKBONE.base
    blocks = list(base.blocks)[1:3]
    assert base.heads == 12 and blocks[0].norm1.weight.numel() == D
    act = model.fn_dtype
    keeps = torch.stack([torch.stack([_keep(B, 100, 501), _keep(B, 108, 502)]),
                         torch.stack([_keep(B, 90, 503), _keep(B, max(HZ), 504)])])
    sc = _scales(keeps)
    perm, inv, live = ops.droppath_plan(sc, 2, B, T)
    assert [int(live[i, 1]) for i in range(2)] == [108 * T, max(HZ) * T]
    x0 = _randn((B, T, D), 505)
    w_out = _randn((B, T, D), 506, 1e-3)
    names = ["%d.%s" % (i, n) for i, blk in enumerate(blocks) for n, _ in blk.named_parameters()]
    calls = [0]
    for nm in ("layernorm_fwd_perm", "layernorm_fwd_split_perm"):
        def counted(*a, _real=getattr(ops, nm), **k):
            calls[0] += 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, nm, counted)

    def run(skip, poison):
        for blk in blocks:
            for p_ in blk.parameters():
                p_.grad = None
        calls[0] = 0
        with _Poison(monkeypatch) if poison else _NoCtx():
            x = x0.clone().requires_grad_(True)
            h = x
            for i, blk in enumerate(blocks):
                plan = (perm[i, 1], inv[i, 1], live[i, 1:2]) if skip else None
                h = fn.TransformerBlockFn.apply(h, *_block_args(blk.norm1, blk.attn, blk.norm2, blk.mlp), None, None, base.heads,
                                                1e-6, act, sc[i, 0], sc[i, 1], None, None, None, base.qk_scale, None, None, None,
                                                False, False, plan)
            (h * w_out).sum().backward()
            torch.cuda.synchronize()
        assert calls[0] == (2 if skip else 0), ("compacted MLP branches that ran", calls[0])
        grads = [p_.grad.clone() for blk in blocks for p_ in blk.parameters()]
        return h.detach().clone(), x.grad.clone(), grads
    ref = run(False, False)
    got = run(True, False)
    poi = run(True, True)
    for what, t_ in [("out", poi[0]), ("dx", poi[1])] + list(zip(names, poi[2])):
        assert bool(torch.isfinite(t_).all()), (mode, what, "non-finite with poisoned memory")
    assert torch.equal(poi[0], got[0]) and torch.equal(poi[1], got[1])
    for n, a_, b_ in zip(names, poi[2], got[2]):
        assert torch.equal(a_, b_), (mode, n, "poisoned != unpoisoned")
    assert torch.equal(got[0], ref[0]), mode                        # forward: bit-identical to the dense blocks
    assert torch.equal(got[1], ref[1]), mode                        # input gradient: bit-identical
    for n, a_, b_ in zip(names, got[2], ref[2]):
        e = rel_err(a_, b_)
        assert e < _grad_tolerances(n), (mode, n, e)


# ---------------------------------------------------------------------------------------------------------------------------------
# i. the headline workload (RGBNT201, AL = 1, B = 128, drop_path 0.1), hand-picked live counts
# ---------------------------------------------------------------------------------------------------------------------------------
def _headline_keep(depth, nmod, seed):
    """(nmod, depth, 2, B) keep flags: MLP branch of block 1 keeps everyone, block 2 one sample, blocks 3-6 the T = 129 edge counts
    (smallest / largest hazard count, 108, 65: 65 x 129 = 131 x 64 + 1) over the stacked nmod * B samples; the rest drawn"""
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(depth, 2, nmod * B, generator=g) > 0.1
    keep[0] = True                                                  # block 0: rate 0, never dropped
    for blk, nl in ((1, nmod * B), (2, 1), (3, min(HZ)), (4, max(HZ)), (5, 108), (6, 65)):
        keep[blk, 1] = _keep(nmod * B, nl, seed + blk)
    return keep.view(depth, 2, nmod, B).permute(2, 0, 1, 3).contiguous(), keep


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_headline_step_with_edge_live_counts(dtype, monkeypatch):
    from editor_amd.modeling import make_model
    from editor_amd import losses
    seed, b = 17, B
    cfg, c, cams = config.preset("RGBNT201", compute_dtype=dtype, drop_path=0.1)
    assert cfg.MODEL.AL == 1
    h, w = cfg.INPUT.SIZE_TRAIN
    img, label, cam, view = synth.make_batch(seed + 1, b, h, w, cams, instances=16)
    nmod = len(img)
    depth = 12
    keep, flat = _headline_keep(depth, nmod, 77)

    class W:
        def add_scalar(self, *a, **k):
            pass

    def step(skip, poison):
        cfg.MODEL.DROP_SKIP = skip
        m = make_model(cfg, c, cams)
        synth.fill_state_dict_(m.state_dict(), seed)
        m = m.cuda().train()
        buckets = m.enable_grad_buckets()
        m.teacher_drop_keep = keep
        with _Poison(monkeypatch) if poison else _NoCtx():
            gimg = {k: v.cuda().requires_grad_(k == "RGB") for k, v in img.items()}
            out = m(gimg, label=label.cuda(), cam_label=cam.cuda(), view_label=view.cuda(), writer=W(), epoch=1)
            loss = losses.loss_pairs(out, label.cuda())
            loss.backward()
            buckets.finish()
            torch.cuda.synchronize()
            grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
            res = [o.detach().clone() for o in out], loss.detach().clone(), grads, m.last_drop_scales.clone()
        del m, buckets, gimg, out, loss
        torch.cuda.empty_cache()
        return res
    out0, loss0, g0, sc0 = step(False, False)
    out1, loss1, g1, sc1 = step(True, False)
    out2, loss2, g2, sc2 = step(True, True)
    live = (sc1.view(depth, 2, nmod * b, T)[:, 1, :, 0] != 0).sum(-1) * T
    assert [int(live[i]) for i in range(1, 7)] == [nmod * b * T, T, min(HZ) * T, max(HZ) * T, 108 * T, 65 * T]
    assert torch.equal(sc0, sc1) and torch.equal(sc1, sc2)
    # poisoned == unpoisoned, bit for bit: nothing reads a row nobody wrote
    for a_, b_ in zip(out2, out1):
        assert torch.equal(a_, b_)
    assert torch.equal(loss2, loss1) and set(g2) == set(g1)
    for k in g1:
        assert torch.equal(g2[k], g1[k]), k
        assert bool(torch.isfinite(g1[k]).all()), k
    # skipping vs dense: the existing step test's tolerances
    for a_, b_ in zip(out0, out1):
        assert torch.equal(a_, b_)
    assert torch.equal(loss0, loss1) and set(g0) == set(g1)
    for k in g0:
        if g0[k].dim() == 2 and (".mlp.fc" in k or ".attn." in k) and "BACKBONE" in k:
            assert rel_err(g1[k], g0[k]) < TOL_WG, k
        elif "BACKBONE" in k and ".norm" not in k and "bias" not in k:
            assert rel_err(g1[k], g0[k]) < TOL_WG, k
        else:
            assert rel_err(g1[k], g0[k]) < 1e-4, k
