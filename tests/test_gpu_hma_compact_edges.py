"""The compacted (variable-length) HMA head at its live-row and sequence-length edges (EDITOR._hma_compact): forced token selections
whose live row count live_a = sum_b L_b lands on every residue that matters - live % 64 in {0, 1, 63}, either side of a 256-row GEMM
tile, live == MA (no pad rows), one token per sample, 3 * live_a on another residue than live_a, the whole live extent inside the first
K-tile, the longest sequence next to length-2 ones (tests/hma_edges.py; every plan's target is asserted on the host in
tests/test_hma_edge_plans.py and again wherever a plan is built here).

The chain lives by the m_live contract of include/editor_hip.h: a producer writes every row below roundup64(live) - rows
[live, roundup64) zero / mask 0 - and nobody reads or writes a row at or past roundup64(live).  So every kernel runs on inputs whose
rows behind roundup64(live) are NaN, into outputs that hold NaN wherever nobody wrote (a poison context over torch.empty), and is
compared with an fp64 reference on the live rows: the L2 error AND the worst row of the tiles around live, roundup64(live) and the
last row.

Section e compares each HMA block, compact and dense-masked, with an fp64 restatement of the dense-masked block; the compact form may
err at most 1.5 x as much as the dense one.  Measured (MI355X; relative L2 on the kept rows, worst of the four blocks; "gradient" = the
worst of dx and the ten parameter gradients; last column = the worst single quantity's compact : dense ratio):

    mode   plan       B    output: dense / compact    worst gradient: dense / compact    worst compact : dense ratio
    bf16   all        8    1.37e-03 / 1.37e-03        5.14e-03 / 5.14e-03                1.000
    bf16   b1         8    1.38e-03 / 1.38e-03        5.14e-03 / 5.14e-03                1.005
    bf16   one_token  8    1.65e-03 / 1.65e-03        4.90e-03 / 4.90e-03                1.000
    bf16   r1         8    1.38e-03 / 1.38e-03        5.20e-03 / 5.19e-03                1.004
    bf16   skewed     8    1.41e-03 / 1.41e-03        5.15e-03 / 5.15e-03                1.000
    bf16   small      8    1.48e-03 / 1.48e-03        5.08e-03 / 5.08e-03                1.000
    bf16   t256p1     8    1.39e-03 / 1.39e-03        5.07e-03 / 5.02e-03                1.005
    bf16   typical    8    1.38e-03 / 1.38e-03        5.42e-03 / 5.43e-03                1.007
    bf16   skewed     64   1.48e-03 / 1.48e-03        5.19e-03 / 5.19e-03                1.000
    bf16   r1         128  1.38e-03 / 1.38e-03        5.22e-03 / 5.22e-03                1.002
    f16    all        8    1.68e-04 / 1.68e-04        6.65e-04 / 6.65e-04                1.000
    f16    b1         8    1.70e-04 / 1.70e-04        6.52e-04 / 6.48e-04                1.026
    f16    one_token  8    2.07e-04 / 2.07e-04        6.17e-04 / 6.17e-04                1.000
    f16    r1         8    1.70e-04 / 1.70e-04        6.92e-04 / 6.87e-04                1.009
    f16    skewed     8    1.72e-04 / 1.72e-04        6.35e-04 / 6.35e-04                1.001
    f16    small      8    1.81e-04 / 1.81e-04        6.18e-04 / 6.30e-04                1.020
    f16    t256p1     8    1.71e-04 / 1.71e-04        6.46e-04 / 6.43e-04                1.010
    f16    typical    8    1.70e-04 / 1.70e-04        6.83e-04 / 6.75e-04                1.008
    f16    skewed     64   1.82e-04 / 1.82e-04        6.58e-04 / 6.51e-04                1.002
    f16    r1         128  1.69e-04 / 1.69e-04        6.62e-04 / 6.52e-04                1.031
    f16x2  all        8    1.53e-07 / 1.53e-07        6.57e-04 / 6.57e-04                1.000
    f16x2  b1         8    1.54e-07 / 1.54e-07        6.26e-04 / 6.25e-04                1.005
    f16x2  one_token  8    1.73e-07 / 1.73e-07        5.75e-04 / 5.72e-04                1.002
    f16x2  r1         8    1.53e-07 / 1.53e-07        6.28e-04 / 6.17e-04                1.011
    f16x2  skewed     8    1.54e-07 / 1.54e-07        6.47e-04 / 6.34e-04                1.006
    f16x2  small      8    1.59e-07 / 1.58e-07        5.95e-04 / 5.94e-04                1.016
    f16x2  t256p1     8    1.54e-07 / 1.54e-07        6.11e-04 / 6.02e-04                1.005
    f16x2  typical    8    1.53e-07 / 1.53e-07        6.19e-04 / 6.25e-04                1.011
    f16x2  skewed     64   1.57e-07 / 1.57e-07        6.10e-04 / 6.01e-04                1.002
    f16x2  r1         128  1.53e-07 / 1.53e-07        6.30e-04 / 6.21e-04                1.010
"""
import pytest
import torch

import hma_edges as he
from conftest import rel_err
from edge_helpers import _NoCtx, _Poison, _boundary_rows, _check, _gelu64, _gelu_grad64, _gen, _randn, _up   # noqa: F401
from editor_amd import config, functional as fn, ops, synth   # noqa: F401

pytestmark = pytest.mark.gpu

T, HEADS, HD, D, HID = he.T, 12, 64, 768, 3072
NAN = float("nan")
TOL16 = {torch.bfloat16: 4e-3, torch.float16: 5e-4}          # as tests/test_gpu_dropskip_edges.py
TOL32, TOL_WG = 1e-5, 2e-5
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
CASE_IDS = ["%s-b%d" % c for c in he.CASES]


def _cases(names, bs=(8, 64, 128)):
    return [c for c in he.CASES if c[0] in names and c[1] in bs]


def _ids(cases):
    return ["%s-b%d" % c for c in cases]


def _plan(name, b, nmod=3):
    """-> (ops.CompactPlan on the device, host maps, live_a); the plan's target and its live count are asserted"""
    index, live = he.edge_plan(name, b)
    plan = ops.CompactPlan(index.cuda(), T, nmod)
    h = he.host_maps(index, nmod)
    assert plan.total == live == h["live"] and plan.ma == h["ma"] and plan.mb == h["mb"]
    assert int(plan.live_a.item()) == live and int(plan.live_b.item()) == nmod * live
    return plan, h, live


def _nan_mask(t):
    return torch.isnan(t.float()).all(dim=-1) if t.dim() > 1 else torch.isnan(t.float())


def _untouched(t, r0, what):
    """rows at or past r0 still hold the NaN sentinel in every element"""
    if r0 < t.shape[0]:
        assert bool(torch.isnan(t[r0:].float()).all()), (what, "rows at or past roundup64(live) were written")


def _finite(t, what):
    assert bool(torch.isfinite(t.float()).all()), (what, "non-finite")


# ---------------------------------------------------------------------------------------------------------------------------------
# a. plan, maps, row movement with live extents (csrc/compact.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nmod", [2, 3, 4])
@pytest.mark.parametrize("name,b", he.CASES, ids=CASE_IDS)
def test_plan_and_maps_equal_host_construction(name, b, nmod):
    index, live = he.edge_plan(name, b)
    h = he.host_maps(index, nmod)
    plan = ops.CompactPlan(index.cuda(), T, nmod)
    cu = torch.full((b + 1,), -7, dtype=torch.int32, device="cuda")
    tok = torch.full((b * T,), -7, dtype=torch.int32, device="cuda")
    ops.call("editor_compact_plan", index.cuda(), b, he.N, cu, tok)
    assert plan.total == live
    assert torch.equal(cu.cpu().long(), h["cu"]) and torch.equal(plan.cu.cpu().long(), h["cu"])
    assert torch.equal(tok[:live].cpu().long(), h["tok"]) and bool((tok[live:] == -7).all())
    assert torch.equal(plan.cu3.cpu().long(), h["cu3"])
    assert plan.ma == h["ma"] and plan.mb == h["mb"]
    for k in ("map_a", "map_b", "map_cls"):
        assert torch.equal(getattr(plan, k).cpu().long(), h[k]), k
    for k in ("mask_a", "mask_b"):
        assert torch.equal(getattr(plan, k).cpu(), h[k]), k
    # outside the live extent: -1 / 0 everywhere (restated, so that a host-construction slip cannot hide it)
    ma = plan.ma
    assert bool((plan.map_a.view(nmod, ma)[:, live:] == -1).all()) and bool((plan.map_b[nmod * live:] == -1).all())
    assert bool((plan.map_a.view(nmod, ma)[:, :live] >= 0).all()) and bool((plan.map_b[:nmod * live] >= 0).all())
    assert not bool(plan.mask_a[live:].any()) and not bool(plan.mask_b[nmod * live:].any())
    assert int(plan.live_a.item()) == live and int(plan.live_b.item()) == nmod * live


def test_compact_plan_batch_limits():
    """editor_compact_plan scans one workgroup of 1024 threads: B = 1024 works, B = 0 and B = 1025 are refused by return code"""
    n = 8
    index = (torch.rand(1025, n, generator=torch.Generator().manual_seed(3)) > 0.5).to(torch.uint8)
    dev = index.cuda()
    cu = torch.zeros(1026, dtype=torch.int32, device="cuda")
    tok = torch.zeros(1025 * (n + 1), dtype=torch.int32, device="cuda")
    for bad in (1025, 0):
        with pytest.raises(RuntimeError, match="editor_compact_plan failed"):
            ops.call("editor_compact_plan", dev, bad, n, cu, tok)
    torch.cuda.synchronize()
    assert not bool(cu.any())                                          # a refusal launches nothing
    ops.call("editor_compact_plan", dev, 1024, n, cu, tok)
    lens = 1 + index[:1024].long().sum(1)
    assert cu[:1025].cpu().long().tolist() == [0] + lens.cumsum(0).tolist()
    plan = ops.CompactPlan(dev[:1024].contiguous(), n + 1, 3)
    assert plan.total == int(lens.sum())


@pytest.mark.parametrize("nmod", [2, 3, 4])
@pytest.mark.parametrize("name,b", he.CASES, ids=CASE_IDS)
def test_gather_and_scatter_with_live_extents(name, b, nmod, monkeypatch):
    d = 32
    plan, h, live = _plan(name, b, nmod)
    ma, mb, r64a, r64b = plan.ma, plan.mb, _up(live, 64), min(_up(nmod * live, 64), plan.mb)
    dense = _randn((nmod * b * T, d), 5)
    with _Poison(monkeypatch):
        xa = ops.gather_rows(dense, plan.map_a, plan.live_a, 1, ma)                  # layout A, as GatherRowsFn calls it
        xb = ops.gather_rows(xa, plan.map_b, plan.live_a, nmod, mb)                   # layout B, as GatherPairFn calls it
        torch.cuda.synchronize()
    ma_l = h["map_a"].cuda()
    for m in range(nmod):
        seg = xa[m * ma:(m + 1) * ma]
        assert torch.equal(seg[:live], dense[ma_l[m * ma:m * ma + live]]), (m, "layout A live rows")
        assert bool((seg[live:r64a] == 0).all()), (m, "layout A pad rows")
        _untouched(seg, r64a, ("layout A", m))
    mb_l = h["map_b"].cuda()
    assert torch.equal(xb[:nmod * live], xa[mb_l[:nmod * live]]), "layout B live rows"
    assert bool((xb[nmod * live:r64b] == 0).all()), "layout B pad rows"
    _untouched(xb, r64b, "layout B")
    # the backwards: scatter is the exact adjoint on the rows the maps name
    dyb = torch.full((mb, d), NAN, device="cuda")
    dyb[:nmod * live] = _randn((nmod * live, d), 6)
    want = torch.zeros(nmod * ma, d, device="cuda")
    want[mb_l[:nmod * live]] = dyb[:nmod * live]
    named = torch.zeros(nmod * ma, dtype=torch.bool, device="cuda")
    named[mb_l[:nmod * live]] = True
    assert int(named.sum()) == nmod * live
    with _Poison(monkeypatch):
        full = ops.scatter_rows(dyb, plan.map_b, nmod * ma, fill="all")
        none = ops.scatter_rows(dyb, plan.map_b, nmod * ma, fill="none")
        tail = ops.scatter_rows(dyb, plan.map_b, nmod * ma, fill="tail", live=plan.live_a, seg_rows=ma)
        torch.cuda.synchronize()
    assert torch.equal(full, want)                                                    # "all": zero wherever no index points
    assert torch.equal(none[named], want[named]) and bool(torch.isnan(none[~named]).all())
    assert torch.equal(tail[named], want[named])
    for m in range(nmod):
        seg = tail[m * ma:(m + 1) * ma]
        assert bool((seg[live:r64a] == 0).all()), (m, "fill='tail': pad rows of every segment")
        _untouched(seg, r64a, ("fill='tail'", m))
    # layout A's own backward (fill "none" into the dense token tensor)
    dya = torch.full((nmod * ma, d), NAN, device="cuda")
    for m in range(nmod):
        dya[m * ma:m * ma + live] = _randn((live, d), 7 + m)
    with _Poison(monkeypatch):
        back = ops.scatter_rows(dya, plan.map_a, nmod * b * T, fill="none")
        back_all = ops.scatter_rows(dya, plan.map_a, nmod * b * T, fill="all")
        torch.cuda.synchronize()
    rows = torch.cat([ma_l[m * ma:m * ma + live] for m in range(nmod)])
    src = torch.cat([dya[m * ma:m * ma + live] for m in range(nmod)])
    want = torch.zeros(nmod * b * T, d, device="cuda")
    want[rows] = src
    assert torch.equal(back_all, want) and torch.equal(back[rows], src)
    rest = torch.ones(nmod * b * T, dtype=torch.bool, device="cuda")
    rest[rows] = False
    assert bool(torch.isnan(back[rest]).all())


def test_zero_tail_rows_edges():
    d = 24                                                                            # 96-byte rows (a multiple of 16)

    def run(rows, live, alloc):
        buf = torch.full((alloc, d), 7.0, device="cuda")
        ops.call("editor_zero_tail_rows", buf, d * 4, rows, torch.tensor([live], dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        return buf
    for rows, live in ((256, 128), (256, 0), (256, 256), (16512, 16512)):              # live % 64 == 0: nothing to write
        assert bool((run(rows, live, rows) == 7.0).all()), (rows, live)
    buf = run(100, 100, 128)                                                           # live == rows (not a multiple of 64)
    assert bool((buf == 7.0).all())
    buf = run(100, 70, 128)                                                            # roundup64(live) > rows: clamped to rows
    assert bool((buf[:70] == 7.0).all()) and bool((buf[70:100] == 0).all()) and bool((buf[100:] == 7.0).all())
    buf = run(256, 65, 256)
    assert bool((buf[:65] == 7.0).all()) and bool((buf[65:128] == 0).all()) and bool((buf[128:] == 7.0).all())
    buf = run(256, 127, 256)
    assert bool((buf[:127] == 7.0).all()) and bool((buf[127] == 0).all()) and bool((buf[128:] == 7.0).all())
    with pytest.raises(RuntimeError, match="editor_zero_tail_rows failed"):            # 24-byte rows: refused, not written
        ops.call("editor_zero_tail_rows", buf, 24, 256, torch.tensor([65], dtype=torch.int32, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------------------
# b. row kernels with m_live (csrc/norm.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def _contract_rows(live, m, n, seed, pad=0.0, std=1.0, shift=0.0):
    """(m, n) fp32 as the contract hands it to a live-row kernel: random rows below live, `pad` (0, or finite garbage when a float
    > 0 is given) in [live, roundup64(live)), NaN at and past roundup64(live)"""
    r64 = min(_up(live, 64), m)
    x = torch.full((m, n), NAN, device="cuda")
    x[:live] = _randn((live, n), seed, std) + shift
    if pad:
        x[live:r64] = _randn((r64 - live, n), seed + 1, pad) + 3.0 * pad
    else:
        x[live:r64] = 0
    return x


def _ln64(x64, gam, bet, eps):
    mu = x64.mean(1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x64 - mu) * rstd * gam.double() + bet.double(), (x64 - mu) * rstd, rstd


LN_TOL = {torch.float32: 1e-5, torch.bfloat16: 6e-3, torch.float16: 1e-3}            # test_layernorm_fwd_bwd's bounds


@pytest.mark.parametrize("pad", [0.0, 40.0], ids=["zero-pad", "garbage-pad"])
@pytest.mark.parametrize("name,b", he.CASES, ids=CASE_IDS)
def test_layernorm_and_cast_rows_with_m_live(name, b, pad, monkeypatch):
    eps = 1e-5
    plan, h, live_a = _plan(name, b, 3)
    shapes = [("A", plan.ma, plan.mask_a, plan.live_a, live_a, 768), ("B", plan.mb, plan.mask_b, plan.live_b, 3 * live_a, 768),
              ("A", plan.ma, plan.mask_a, plan.live_a, live_a, 1024), ("A", plan.ma, plan.mask_a, plan.live_a, live_a, 384)]
    dev = torch.device("cuda", 0)
    for lay, m, mask, lv, live, d in shapes:
        what = (name, b, lay, d, live)
        r64 = min(_up(live, 64), m)
        x = _contract_rows(live, m, d, 11, pad=pad, std=2.0, shift=0.3)
        gam, bet = _randn((d,), 12) * 0.5 + 1.0, _randn((d,), 13) * 0.2
        ref, xhat, rstd64 = _ln64(x[:live].double(), gam, bet, eps)
        stats = None
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            with _Poison(monkeypatch):
                y, mean, rstd = ops.layernorm_fwd(x, gam, bet, eps, dt, mask, 0, m_live=lv)
                torch.cuda.synchronize()
            _check(y[:live], ref, LN_TOL[dt], m, what + ("LN", dt))
            assert bool((y[live:r64] == 0).all()), what + ("LN pad rows not zero", dt)
            _untouched(y, r64, what + ("LN", dt))
            _finite(mean[:r64], what)
            _finite(rstd[:r64], what)
            _untouched(mean, r64, what)
            _untouched(rstd, r64, what)
            if stats is not None:
                assert torch.equal(stats[0][:r64], mean[:r64]) and torch.equal(stats[1][:r64], rstd[:r64])
            stats = (mean, rstd)
        with _Poison(monkeypatch):
            hi, lo, mean2, rstd2 = ops.layernorm_fwd_split(x, gam, bet, eps, mask, lv)
            torch.cuda.synchronize()
        _check(hi[:live].double() + lo[:live].double(), ref, TOL32, m, what + ("LN f16x2",))
        assert bool((hi[live:r64] == 0).all()) and bool((lo[live:r64] == 0).all()), what + ("LN f16x2 pad rows",)
        _untouched(hi, r64, what)
        _untouched(lo, r64, what)
        assert torch.equal(mean2[:r64], stats[0][:r64]) and torch.equal(rstd2[:r64], stats[1][:r64])
        mean, rstd = stats
        # backward: dy (16-bit and fp32) and dx_in by the same contract
        dx_in = _contract_rows(live, m, d, 21, pad=0.0, std=0.5)
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            dy = _contract_rows(live, m, d, 23, pad=pad).to(dt)
            dy64 = dy[:live].double()
            gdy = dy64 * gam.double()
            dx_ref = dx_in[:live].double() + rstd64 * (gdy - gdy.mean(1, keepdim=True) - xhat * (gdy * xhat).mean(1, keepdim=True))
            dg_ref, db_ref = (dy64 * xhat).sum(0), dy64.sum(0)
            with _Poison(monkeypatch):
                dx, dg, db = ops.layernorm_bwd(dy, x, gam, mean, rstd, mask, 0, dx_in=dx_in, m_live=lv)
                rq = ops.ReduceQueue(dev)
                dx2, dg2, db2 = ops.layernorm_bwd(dy, x, gam, mean, rstd, mask, 0, dx_in=dx_in, m_live=lv, rq=rq)
                rq.flush()
                torch.cuda.synchronize()
            for tag, dx_, dg_, db_ in (("bwd", dx, dg, db), ("bwd_queued", dx2, dg2, db2)):
                w2 = what + (tag, dt)
                _check(dx_[:live], dx_ref, 2e-5, m, w2)
                _finite(dx_[live:r64], w2 + ("dx pad rows",))
                _untouched(dx_, r64, w2)
                _finite(dg_, w2 + ("dgamma",))
                _finite(db_, w2 + ("dbeta",))
                assert rel_err(dg_, dg_ref) < 2e-5, w2 + ("dgamma", rel_err(dg_, dg_ref))
                assert rel_err(db_, db_ref) < 2e-5, w2 + ("dbeta", rel_err(db_, db_ref))
            assert torch.equal(dx[:r64], dx2[:r64])
        # the live-row cast (no row scale, a loss scale; with a row scale)
        rs = torch.full((m,), NAN, device="cuda")
        rs[:r64] = torch.rand(r64, generator=_gen(31), device="cuda") + 0.5
        src = _contract_rows(live, m, d, 33, pad=0.0, std=3.0)
        for dt in (torch.bfloat16, torch.float16):
            for rowscale, scale in ((None, 4.0), (rs, 1.0)):
                with _Poison(monkeypatch):
                    out = ops.cast_rows(src, rowscale, dt, lv, scale)
                    torch.cuda.synchronize()
                want = src[:live] * scale if rowscale is None else src[:live] * (rowscale[:live, None] * scale)
                assert torch.equal(out[:live], want.to(dt)), what + ("cast_rows", dt)          # test_cast_rows_colsum: the same bits
                assert bool((out[live:r64] == 0).all()), what + ("cast_rows pad rows", dt)
                _untouched(out, r64, what + ("cast_rows", dt))


# ---------------------------------------------------------------------------------------------------------------------------------
# c. live-row products (csrc/gemm_bf16.hip, 16-bit and split form), m_live WITHOUT live_dense: the compacted head's products
# ---------------------------------------------------------------------------------------------------------------------------------
GEMM_CASES = _cases(("small", "r1", "r63", "t256", "t256p1", "all", "typical"), bs=(8, 128))


def _lv(live):
    return torch.tensor([live], dtype=torch.int32, device="cuda")


def _gemm_shape(name, b):
    _, live = he.edge_plan(name, b)
    m = _up(b * T, 64)                                   # MA: 1 088 (B = 8), 16 512 (B = 128)
    assert m in (1088, 16512) and 0 < live <= m
    return live, m, min(_up(live, 64), m)


def _live_check(out, ref, live, m, tol, what):
    """live rows against fp64; rows [live, roundup64) finite; rows of wholly dead 256-row tiles untouched"""
    _check(out[:live], ref, tol, m, what)
    _finite(out[live:min(_up(live, 64), m)], what + ("rows [live, roundup64)",))
    _untouched(out, min(_up(live, 256), m), what)


def _nanfull(shape, dt=torch.float32):
    return torch.full(shape, NAN, dtype=dt, device="cuda")


def test_cases_of_the_products_cover_the_issue_list():
    assert {n for n, _ in GEMM_CASES} == {"small", "r1", "r63", "t256", "t256p1", "all", "typical"}
    assert {("r1", 128), ("t256p1", 128), ("all", 128), ("typical", 128), ("small", 8), ("r63", 8), ("t256", 8)} <= set(GEMM_CASES)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name,b", GEMM_CASES, ids=_ids(GEMM_CASES))
def test_live_row_forward_and_dgrad_products(name, b, dtype, monkeypatch):
    dt = DTYPES[dtype]
    live, m, r64 = _gemm_shape(name, b)
    lv = _lv(live)
    ops_in = {D: _contract_rows(live, m, D, 41).to(dt), HID: _contract_rows(live, m, HID, 42).to(dt)}
    res = _contract_rows(live, m, D, 43)
    with _Poison(monkeypatch):
        for i, (k, n) in enumerate(((D, 3 * D), (D, D), (D, HID), (HID, D))):
            what = (name, b, dtype, k, n, live)
            a = ops_in[k]
            w, bias = _randn((n, k), 50 + i, 0.03).to(dt), _randn((n,), 60 + i, 0.1)
            pre = a[:live].double() @ w.double().t() + bias.double()
            c = _nanfull((m, n), dt)
            ops.gemm(a, w, c, m, n, k, k, k, n, 0, 0, bias=bias, m_live=lv)
            _live_check(c, pre, live, m, TOL16[dt], what + ("plain",))
            if n == D:
                c32 = _nanfull((m, n))
                ops.gemm(a, w, c32, m, n, k, k, k, n, 0, 0, bias=bias, epilogue=ops.EPI_RESIDUAL, aux=res, m_live=lv)
                _live_check(c32, pre + res[:live].double(), live, m, TOL32, what + ("residual",))
            if n == HID:
                g, ax = _nanfull((m, n), dt), _nanfull((m, n), dt)
                ops.gemm(a, w, g, m, n, k, k, k, n, 0, 0, bias=bias, epilogue=ops.EPI_GELU | ops.EPI_AUX_GRAD, aux=ax, m_live=lv)
                _live_check(g, _gelu64(pre), live, m, TOL16[dt], what + ("gelu",))
                _live_check(ax, _gelu_grad64(pre), live, m, TOL16[dt], what + ("gelu'",))
        # fc2's dgrad: da = (dy W2) * gelu'(pre), gelu' from the forward above (written below roundup64(live), NaN behind)
        dy = ops_in[D]
        gp = _nanfull((m, HID))
        gp[:r64] = torch.rand(r64, HID, generator=_gen(71), device="cuda") * 1.2 - 0.1
        gp = gp.to(dt)
        w2 = _randn((D, HID), 72, 0.03).to(dt)
        da = _nanfull((m, HID), dt)
        ops.gemm(dy, w2.t().contiguous(), da, m, HID, D, D, D, HID, 0, 0, epilogue=ops.EPI_GELU_BWD | ops.EPI_AUX_GRAD, aux=gp, m_live=lv)
        torch.cuda.synchronize()
    _live_check(da, (dy[:live].double() @ w2.double()) * gp[:live].double(), live, m, TOL16[dt], (name, b, dtype, "fc2 dgrad", live))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name,b", GEMM_CASES, ids=_ids(GEMM_CASES))
def test_grouped_launch_equals_three_single_calls(name, b, dtype, monkeypatch):
    """editor_gemm_group (the three modality blocks' products as one launch, shared m_live): bit-identical to three editor_gemm calls,
    the rows it leaves unwritten included; below M = 2048 gemm_group_ok says no and the blocks launch one by one."""
    dt = DTYPES[dtype]
    live, m, r64 = _gemm_shape(name, b)
    lv = _lv(live)
    bits = {torch.float32: torch.int32, dt: torch.int16}
    for j, (n, cdt, epi) in enumerate(((3 * D, dt, 0), (D, torch.float32, ops.EPI_RESIDUAL), (HID, dt, ops.EPI_GELU | ops.EPI_AUX_GRAD))):
        reqs, singles = [], []
        for i in range(3):
            a = _contract_rows(live, m, D, 80 + 3 * j + i).to(dt)
            w, bias = _randn((n, D), 90 + 3 * j + i, 0.03).to(dt), _randn((n,), 100 + 3 * j + i, 0.1)
            kw = dict(bias=bias, m_live=lv, epilogue=epi)
            kw1 = dict(kw)
            if epi == ops.EPI_RESIDUAL:
                kw["aux"] = kw1["aux"] = _contract_rows(live, m, n, 110 + i)
            elif epi:
                kw["aux"], kw1["aux"] = _nanfull((m, n), dt), _nanfull((m, n), dt)
            reqs.append(((a, w, _nanfull((m, n), cdt), m, n, D, D, D, n), kw))
            singles.append(((a, w, _nanfull((m, n), cdt), m, n, D, D, D, n), kw1))
        assert ops.gemm_group_ok(reqs) == (m >= 2048), (name, b, n)
        if m < 2048:
            continue
        with _Poison(monkeypatch):
            ops.gemm_group(reqs)
            for args, kw in singles:
                ops.gemm(*args, **kw)
            torch.cuda.synchronize()
        for (ga, gk), (sa, sk) in zip(reqs, singles):
            outs = [(ga[2], sa[2])] + ([(gk["aux"], sk["aux"])] if (epi & 0xFF) == ops.EPI_GELU else [])
            for g_, s_ in outs:
                assert torch.equal(g_[:r64].view(bits[g_.dtype]), s_[:r64].view(bits[g_.dtype])), (name, b, dtype, n, "group != single")
                assert torch.equal(torch.isnan(g_), torch.isnan(s_)), (name, b, dtype, n, "different rows written")
                _finite(g_[:r64], (name, b, dtype, n))
                _untouched(g_, min(_up(live, 256), m), (name, b, dtype, n, "group"))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name,b", GEMM_CASES, ids=_ids(GEMM_CASES))
def test_live_row_weight_gradients(name, b, dtype, monkeypatch):
    dt = DTYPES[dtype]
    live, m, r64 = _gemm_shape(name, b)
    lv = _lv(live)
    shapes = [(3 * D, D), (D, D), (HID, D), (D, HID)]                    # (n, k) of a block's four dW = dy^T x
    jobs = []
    for i, (n, k) in enumerate(shapes):
        dy = _contract_rows(live, m, n, 120 + i, std=0.5).to(dt)          # rows [live, roundup64): zero (the contract) ...
        x = _contract_rows(live, m, k, 130 + i, pad=0.75).to(dt)          # ... finite, not zero, in the other operand; NaN behind both
        jobs.append((dy, x, _nanfull((n, k))))
    with _Poison(monkeypatch):
        ops.gemm_wgrad_group(jobs, m, 1.0, m_live=lv)
        single = []
        for (n, k), (dy, x, _) in zip(shapes, jobs):
            sk, skf = fn._splitk_for(n, k, m)
            assert sk > 1
            dw = _nanfull((n, k))
            ops.gemm(dy, x, dw, n, k, m, n, k, k, 1, 1, alpha=1.0, splitk=sk, epilogue=skf, m_live=lv)
            single.append(dw)
        torch.cuda.synchronize()
    for (n, k), (dy, x, dwg), dws in zip(shapes, jobs, single):
        ref = dy[:live].double().t() @ x[:live].double()
        for tag, dw in (("group", dwg), ("transA split-K", dws)):
            what = (name, b, dtype, n, k, live, tag)
            _finite(dw, what)
            e = rel_err(dw, ref)
            per = ((dw.double() - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)).max().item()
            assert e < TOL_WG and per < TOL_WG, what + (e, per)


@pytest.mark.parametrize("name,b", GEMM_CASES, ids=_ids(GEMM_CASES))
def test_live_row_products_f16x2(name, b, monkeypatch):
    live, m, r64 = _gemm_shape(name, b)
    lv = _lv(live)
    a32 = _contract_rows(live, m, D, 141)
    res = _contract_rows(live, m, D, 142)
    rows = sorted(set(r for r in edge_rows(live, m)) | set(range(min(live, 1024))))
    inv = 1.0 / ops.SPLIT_WSCALE
    for i, n in enumerate((3 * D, D)):
        what = (name, b, "f16x2", n, live)
        w32, bias = _randn((n, D), 150 + i, 0.02), _randn((n,), 160 + i, 0.1)
        ref = a32[:live].double() @ w32.double().t() + bias.double()
        # the bound of test_gemm_f16x2_vs_float64: fp32-class = within 2 x the error of torch's own fp32 CPU matmul on the same rows
        f32 = (a32[rows].cpu() @ w32.cpu().t() + bias.cpu()).double()
        r_ = ref[rows].cpu()
        f32_l2 = rel_err(f32, r_)
        f32_row = ((f32 - r_).norm(dim=1) / r_.norm(dim=1).clamp_min(1e-30)).max().item()
        tol, tol_row = max(3e-7, 2.0 * f32_l2), max(3e-7, 2.0 * f32_row)
        with _Poison(monkeypatch):
            ap, wp = ops.split_f32(a32), ops.split_f32(w32, ops.SPLIT_WSCALE)
            hi, lo = _nanfull((m, n), torch.float16), _nanfull((m, n), torch.float16)
            ops.gemm_split(ap, wp, hi, lo, m, n, D, alpha=inv, bias=bias, m_live=lv)
            outs = [("pair", hi.double() + lo.double(), ref)]
            if n == D:
                c = _nanfull((m, n))
                ops.gemm_split(ap, wp, c, None, m, n, D, alpha=inv, bias=bias, epilogue=ops.EPI_RESIDUAL, aux=res, m_live=lv)
                outs.append(("residual", c, ref + res[:live].double()))
            torch.cuda.synchronize()
        for tag, out, rf in outs:
            e = rel_err(out[:live], rf)
            er = [r for r in edge_rows(live, m)]
            per = ((out[er].double() - rf[er]).norm(dim=1) / rf[er].norm(dim=1).clamp_min(1e-30)).max().item()
            print("f16x2 live-row product", what, tag, "L2 %.2e (bound %.2e) worst boundary row %.2e (bound %.2e)" % (e, tol, per, tol_row))
            assert e < tol and per < tol_row, what + (tag, e, tol, per, tol_row)
            _finite(out[live:r64], what + (tag, "rows [live, roundup64)"))
            _untouched(out, min(_up(live, 256), m), what + (tag,))


def edge_rows(live, m):
    return [r for r in _boundary_rows(live, m) if r < live]


# ---------------------------------------------------------------------------------------------------------------------------------
# d. variable-length attention (csrc/attention_bf16.hip, csrc/attention_split.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
ATTN_CASES = _cases(("one_token", "skewed", "all", "r1", "b1", "typical"))


def _attn64(qkv, dout, cu):
    """per-sequence fp64 softmax attention and its autograd on the live rows -> out, dqkv"""
    x = qkv.double().requires_grad_(True)
    outs = []
    for s0, s1 in zip(cu[:-1], cu[1:]):
        n = s1 - s0
        q, k, v = (x[s0:s1, j * D:(j + 1) * D].view(n, HEADS, HD).transpose(0, 1) for j in range(3))
        p = torch.softmax(q @ k.transpose(1, 2) * HD ** -0.5, -1)
        outs.append((p @ v).transpose(0, 1).reshape(n, D))
    out = torch.cat(outs)
    if dout is None:
        return out.detach(), None
    out.backward(dout.double())
    return out.detach(), x.grad


def _seq_picks(cu):
    lens = [b_ - a_ for a_, b_ in zip(cu[:-1], cu[1:])]
    return sorted({0, len(lens) - 1, lens.index(min(lens)), lens.index(max(lens))})


def _layouts(name, b):
    """(tag, cu (device), cu (host list), T of the launch, rows, live) for layout A and for layout B with 3 and 4 modalities"""
    out = []
    for nmod in (1, 3, 4):
        plan, h, live_a = _plan(name, b, max(nmod, 2))
        if nmod == 1:
            out.append(("A", plan.cu, h["cu"].tolist(), T, plan.ma, live_a))
        else:
            assert nmod * T <= 608                                   # the 26- and 38-tile kernels (387 and 516 tokens)
            out.append(("B%d" % nmod, plan.cu3, h["cu3"].tolist(), nmod * T, plan.mb, nmod * live_a))
    return out


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name,b", ATTN_CASES, ids=_ids(ATTN_CASES))
def test_varlen_attention_at_edge_plans(name, b, dtype, monkeypatch):
    dt = DTYPES[dtype]
    eps16 = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    scale = HD ** -0.5
    for tag, cu, cul, t, rows, live in _layouts(name, b):
        what = (name, b, dtype, tag, live)
        r64 = min(_up(live, 64), rows)
        qkv = _contract_rows(live, rows, 3 * D, 171, std=1.2).to(dt)
        dout = _contract_rows(live, rows, D, 172).to(dt)
        with _Poison(monkeypatch):
            o, lse = ops.attention_fwd(qkv, b, t, HEADS, HD, None, None, cu=cu)
            dq = ops.attention_bwd(qkv, dout, b, t, HEADS, HD, None, lse, o, cu=cu)
            assert ops.attention_bwd_colsum_ok(qkv, t, HD)
            dq2 = ops._packed_alloc(rows, 3 * D, dt, qkv.device, cu)
            ws = torch.empty(HEADS * rows, dtype=torch.float32, device="cuda")
            parts = _nanfull((b, 3 * D))
            ops.call(ops._h16(qkv, "attention_bwd_colsum"), qkv, dout, o, lse, b, t, HEADS, HD, scale, None, dq2, ws, cu, rows, parts)
            cs = _nanfull((3 * D,))
            dq3 = ops.attention_bwd(qkv, dout, b, t, HEADS, HD, None, lse, o, cu=cu, colsum=cs, colsum_scale=0.5)
            torch.cuda.synchronize()
        ro, rdq = _attn64(qkv[:live], dout[:live], cul)
        # the bounds of test_attention_varlen_matches_dense_reference; per sequence too, so a wrong short one cannot hide
        eo, ed = rel_err(o[:live], ro), rel_err(dq[:live], rdq)
        assert eo < 1.5e-2 and ed < 2.5e-2, what + (eo, ed)
        for s in _seq_picks(cul):
            s0, s1 = cul[s], cul[s + 1]
            eo, ed = rel_err(o[s0:s1], ro[s0:s1]), rel_err(dq[s0:s1], rdq[s0:s1])
            assert eo < 1.5e-2 and ed < 2.5e-2, what + ("sequence", s, s1 - s0, eo, ed)
        for x_, nm in ((o, "out"), (dq, "dqkv"), (dq2, "dqkv (colsum form)")):
            assert bool((x_[live:r64] == 0).all()), what + (nm, "rows [live, roundup64) not zero")
            _untouched(x_, r64, what + (nm,))
        assert torch.equal(dq2[:r64].view(torch.int16), dq[:r64].view(torch.int16))
        assert torch.equal(dq3[:r64].view(torch.int16), dq[:r64].view(torch.int16))
        # a length-1 sequence: softmax of one score is 1 -> out = v up to the output rounding; ds = p (dp - delta) = 0 up to the fp32
        # rounding of the two 64-term dot products it subtracts (each within 64 * 2^-24 of sum |dout_i v_i|), so |dq|, |dk| stay
        # below 2^-17 * sum |dout_i v_i| * scale * |k|, |q| (plus their own 16-bit rounding)
        ones = [s for s in range(b) if cul[s + 1] - cul[s] == 1]
        if name == "one_token" and tag == "A":
            assert len(ones) == b
        if ones:
            r = torch.tensor([cul[s] for s in ones], device="cuda")
            v = qkv[r, 2 * D:].double()
            assert bool(((o[r].double() - v).abs() <= eps16 * v.abs()).all()), what + ("length-1: out != v",)
            dv = dq[r, 2 * D:].double()
            assert bool(((dv - dout[r].double()).abs() <= eps16 * dout[r].double().abs()).all()), what + ("length-1: dv != dout",)
            dp = (dout[r].double() * v).abs().view(-1, HEADS, HD).sum(-1, keepdim=True)            # (n, heads, 1)
            qk = qkv[r, :2 * D].double().abs().view(-1, 2, HEADS, HD)
            other = torch.stack([qk[:, 1], qk[:, 0]], 1)                                             # dq scales k, dk scales q
            lim = (2.0 ** -17 * scale * dp).unsqueeze(1) * other * (1.0 + eps16) + 1e-30
            got = dq[r, :2 * D].double().abs().view(-1, 2, HEADS, HD)
            assert bool((got <= lim).all()), what + ("length-1: dq / dk not zero", float((got / lim).max()))
        # column sums of dqkv from the kernel's own fp32 accumulators: every partial row written, folded within the rounding of the
        # stored entries (the bound of test_attention_bwd_column_sums)
        _finite(parts, what + ("colparts",))
        stored = dq[:live].double()
        bound = stored.abs().sum(0) * (0.5 * eps16 + 4e-6) + 1e-6
        for nm, got in (("parts", parts.double().sum(0)), ("ops", cs.double() * 2.0)):
            err = (got - stored.sum(0)).abs()
            assert bool((err <= bound).all()), what + ("colsum", nm, float((err / bound).max()))
    if dtype == "f16":                                                # the split-precision forward on the same sequences
        for tag, cu, cul, t, rows, live in _layouts(name, b):
            r64 = min(_up(live, 64), rows)
            q32 = _contract_rows(live, rows, 3 * D, 181, std=0.8)
            with _Poison(monkeypatch):
                (oh, ol), lse = ops.attention_fwd_split(ops.split_f32(q32), b, t, HEADS, HD, cu=cu)
                torch.cuda.synchronize()
            ro, _ = _attn64(q32[:live], None, cul)
            got = oh.double() + ol.double()
            e = rel_err(got[:live], ro)
            assert e < 5e-7, (name, b, "f16x2", tag, e)               # test_attention_f16x2_masked_and_varlen's bound
            for s in _seq_picks(cul):
                s0, s1 = cul[s], cul[s + 1]
                e = rel_err(got[s0:s1], ro[s0:s1])
                assert e < 5e-7, (name, b, "f16x2", tag, "sequence", s, s1 - s0, e)
            assert bool((oh[live:r64] == 0).all()) and bool((ol[live:r64] == 0).all())
            _untouched(oh, r64, (name, b, "f16x2", tag))
            _untouched(ol, r64, (name, b, "f16x2", tag))


def test_attention_refuses_packed_sequences_with_a_mask():
    cu = torch.tensor([0, 40, 64], dtype=torch.int32, device="cuda")
    qkv = torch.zeros(64, 3 * D, dtype=torch.bfloat16, device="cuda")
    mask = torch.ones(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="attention_fwd_bf16 failed"):
        ops.attention_fwd(qkv, 2, 40, HEADS, HD, mask, None, cu=cu)
    o, lse = ops.attention_fwd(qkv, 2, 40, HEADS, HD, None, None, cu=cu)
    with pytest.raises(RuntimeError, match="attention_bwd_bf16 failed"):
        ops.attention_bwd(qkv, o, 2, 40, HEADS, HD, mask, lse, o, cu=cu)
    with pytest.raises(RuntimeError, match="attention_bwd_colsum_bf16 failed"):
        ops.attention_bwd(qkv, o, 2, 40, HEADS, HD, mask, lse, o, cu=cu, colsum=torch.empty(3 * D, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------------------
# e. one block and the whole head, compact against dense
# ---------------------------------------------------------------------------------------------------------------------------------
MODES = ["bf16", "f16", "f16x2"]
# absolute caps: bf16 as test_hma_compact_equals_dense_bf16 (1.5e-2 outputs, 4e-2 gradients); f16 (and f16x2, whose backward is f16's)
# carries three more mantissa bits, asserted at 1/6 of the bf16 bound as tests/test_gpu_kernels.py does for every 16-bit kernel
CAPS = {"bf16": (1.5e-2, 4e-2), "f16": (1.5e-2 / 6, 4e-2 / 6), "f16x2": (1.5e-2 / 6, 4e-2 / 6)}
BLOCK_CASES = _cases(("one_token", "small", "r1", "b1", "t256p1", "skewed", "all", "typical"), bs=(8,)) + [("skewed", 64), ("r1", 128)]
_MODELS, _PRISTINE = {}, {}
_PNAMES = ("norm1.weight", "norm1.bias", "qkv.weight", None, "proj.weight", None, "norm2.weight", "norm2.bias", "fc1.weight", None,
           "fc2.weight", None)


def _hma_model(mode):
    if mode not in _MODELS:
        from editor_amd.modeling import make_model
        cfg, c, cams = config.preset("RGBNT201", compute_dtype=mode, drop_path=0.0)
        m = make_model(cfg, c, cams)
        synth.fill_state_dict_(m.state_dict(), 13)
        _MODELS[mode] = m.cuda()
    m = _MODELS[mode]
    fn.set_model_options(m.grad_scale_f16, m.act_light)
    return m


def _hma_blocks(model):
    """[(name, 12 parameters as TransformerBlockFn takes them)]: the three modality blocks, then the joint block"""
    from editor_amd.modeling.make_model import _block_args
    fb = model.FUSE_block
    out = []
    for m_ in model.modalities:
        tag = m_[2]
        out.append((tag, _block_args(getattr(fb, "norm" + tag), getattr(fb, "attn" + tag), getattr(fb, "norm" + tag + "_"),
                                     getattr(fb, "mlp" + tag))))
    out.append(("joint", _block_args(fb.norm1, fb.attn1, fb.norm2, fb.mlp)))
    return out


def _block64(x, mask, params, g):
    """The dense-masked block of BlockMask.forward in fp64 (oracle/editor_ref.py: x + AttentionMask(LN(x)), + MlpMasked(LN(.)), eps
    1e-5, no biases) and its autograd for the output gradient g -> out, dx, [parameter gradients]"""
    from oracle import editor_ref as ref
    sd = {}
    for nm, p in zip(_PNAMES, params):
        assert (nm is None) == (p is None)                  # the HMA linears have no bias
        if nm is not None:
            sd["b." + nm] = p.detach().double().requires_grad_(True)
    x = x.double().requires_grad_(True)
    m = mask.double()
    f = x + ref._masked_attention(ref._ln(x, {"w.weight": sd["b.norm1.weight"], "w.bias": sd["b.norm1.bias"]}, "w", 1e-5), m,
                                  {"a.qkv.weight": sd["b.qkv.weight"], "a.proj.weight": sd["b.proj.weight"]}, "a", HEADS)
    f = f + ref._masked_mlp(ref._ln(f, {"w.weight": sd["b.norm2.weight"], "w.bias": sd["b.norm2.bias"]}, "w", 1e-5), m,
                            {"m.fc1.weight": sd["b.fc1.weight"], "m.fc2.weight": sd["b.fc2.weight"]}, "m")
    f.backward(g.double())
    return f.detach(), x.grad, [None if nm is None else sd["b." + nm].grad for nm in _PNAMES]


def _run_block(params, x, g, tail, group=None):
    """TransformerBlockFn (or GroupedBlocksFn over `group` blocks) as EDITOR._hma / _hma_compact call it -> out, dx, parameter grads"""
    plist = params if group else [params]
    xs = x if group else [x]
    for ps in plist:
        for p in ps:
            if p is not None:
                p.grad = None
    xs = [x_.clone().requires_grad_(True) for x_ in xs]
    if group:
        outs = list(fn.GroupedBlocksFn.apply(len(xs), *[v for x_, ps, tl in zip(xs, plist, tail) for v in (x_, *ps, *tl)]))
        torch.autograd.backward(outs, g)
    else:
        outs = [fn.TransformerBlockFn.apply(xs[0], *plist[0], *tail)]
        outs[0].backward(g)
    torch.cuda.synchronize()
    res = [(o.detach(), x_.grad, [None if p is None else p.grad.clone() for p in ps]) for o, x_, ps in zip(outs, xs, plist)]
    return res if group else res[0]


def _errs(got, ref, rows_got=None, rows_ref=None):
    """relative errors of (out, dx, parameter gradients) against the fp64 block on the kept rows"""
    o, dx, gp = got
    ro, rdx, rgp = ref
    if rows_got is not None:
        o, dx = o[rows_got], dx[rows_got]
    if rows_ref is not None:
        ro, rdx = ro[rows_ref], rdx[rows_ref]
    e = {"out": rel_err(o, ro), "dx": rel_err(dx, rdx)}
    for nm, a, b_ in zip(_PNAMES, gp, rgp):
        if nm is not None:
            e["d" + nm] = rel_err(a, b_)
    return o, dx, gp, e


def _judge(mode, what, dense_e, comp_e, tensors):
    cap_o, cap_g = CAPS[mode]
    for t_ in tensors:
        _finite(t_, what)
    for k, ec in comp_e.items():
        ed = dense_e[k]
        print("hma block %s %-14s dense %.3e compact %.3e" % (what, k, ed, ec))
        assert ec <= 1.5 * ed, what + (k, "compact", ec, "dense", ed)
        assert ec <= (cap_o if k == "out" else cap_g), what + (k, ec)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,b", BLOCK_CASES, ids=_ids(BLOCK_CASES))
def test_hma_blocks_compact_against_dense_and_fp64(name, b, mode, monkeypatch):
    model = _hma_model(mode)
    act = {"bf16": torch.bfloat16, "f16": torch.float16, "f16x2": fn.F16X2}[mode]       # (f16x2: the head on half pairs, SPLIT_SCOPE 'all')
    assert model.hma_heads == HEADS
    blocks = _hma_blocks(model)
    nmod = 3
    index, live = he.edge_plan(name, b)
    plan, h, _ = _plan(name, b, nmod)
    ma, mb = plan.ma, plan.mb
    keep = torch.cat([torch.ones(b, 1, dtype=torch.uint8), index], 1).cuda()                  # (B, T): cls + selected patches
    feats = _randn((nmod, b, T, D), 201) * keep.view(1, b, T, 1)                               # what SFTS leaves: unkept rows zero
    map_a, map_b = h["map_a"].cuda(), h["map_b"].cuda()
    # ---- the three modality blocks: layout A -------------------------------------------------------------------------------------
    g_dense = _randn((nmod, b, T, D), 202, 1e-2) * keep.view(1, b, T, 1)
    xa, ga, rows_a = [], [], []
    for m in range(nmod):
        rows = map_a[m * ma:m * ma + live] - m * b * T                                          # dense row of every packed row
        rows_a.append(rows)
        x_ = _contract_rows(live, ma, D, 0)
        x_[:live] = feats[m].reshape(b * T, D)[rows]
        g_ = _contract_rows(live, ma, D, 0)
        g_[:live] = g_dense[m].reshape(b * T, D)[rows]
        xa.append(x_)
        ga.append(g_)
    tail_c = (plan.mask_a, None, HEADS, 1e-5, act, None, None, plan.cu, T, plan.live_a, None, None)
    tail_d = (keep, None, HEADS, 1e-5, act, None, None, None, None, None, None, None)
    refs = [_block64(feats[m], keep.view(b, T, 1), blocks[m][1], g_dense[m]) for m in range(nmod)]
    refs = [(o.reshape(b * T, D), dx.reshape(b * T, D), gp) for o, dx, gp in refs]
    with _Poison(monkeypatch, sync=True):                     # (blocks of >= 2048 rows run their weight gradients on a side stream)
        comp = [_run_block(blocks[m][1], xa[m], ga[m], tail_c) for m in range(nmod)]
        dense = [_run_block(blocks[m][1], feats[m], g_dense[m], tail_d) for m in range(nmod)]
        grouped = None
        if fn.GROUP_BLOCKS and act in ops.HALF_DTYPES:
            grouped = _run_block([blocks[m][1] for m in range(nmod)], xa, ga, [tail_c] * nmod, group=True)
    for m in range(nmod):
        what = (name, b, mode, blocks[m][0])
        d_ = (dense[m][0].reshape(b * T, D), dense[m][1].reshape(b * T, D), dense[m][2])
        *_, e_d = _errs(d_, refs[m], rows_a[m], rows_a[m])
        o, dx, gp, e_c = _errs(comp[m], refs[m], slice(0, live), rows_a[m])
        _judge(mode, what, e_d, e_c, [o, dx] + [g_ for g_ in gp if g_ is not None])
        if grouped is not None:                                                                # one node, grouped launches: the same bits
            for a_, b_ in zip([grouped[m][0][:live], grouped[m][1][:live]] + grouped[m][2], [comp[m][0][:live], comp[m][1][:live]] + comp[m][2]):
                assert (a_ is None and b_ is None) or torch.equal(a_, b_), what + ("GroupedBlocksFn != TransformerBlockFn",)
    # ---- the joint block: layout B (cu3, nmod * T tokens per sample, live_b rows) ------------------------------------------------------
    lb = nmod * live
    joint = feats.permute(1, 0, 2, 3).reshape(b, nmod * T, D).contiguous()                     # cat over the modalities, per sample
    gj = (_randn((b, nmod * T, D), 203, 1e-2) * keep.repeat(1, nmod).view(b, nmod * T, 1)).contiguous()
    da = map_a[map_b[:lb]]                                                                     # dense (nmod, B, T) row of each layout-B row
    mm, bb, tt = da // (b * T), (da // T) % b, da % T
    rows_b = bb * (nmod * T) + mm * T + tt
    xb, gb = _contract_rows(lb, mb, D, 0), _contract_rows(lb, mb, D, 0)
    xb[:lb] = joint.reshape(-1, D)[rows_b]
    gb[:lb] = gj.reshape(-1, D)[rows_b]
    keep3 = keep.repeat(1, nmod).contiguous()
    tail_c = (plan.mask_b, None, HEADS, 1e-5, act, None, None, plan.cu3, nmod * T, plan.live_b, None, None)
    tail_d = (keep3, None, HEADS, 1e-5, act, None, None, None, None, None, None, None)
    ro, rdx, rgp = _block64(joint, keep3.view(b, nmod * T, 1), blocks[3][1], gj)
    ref = (ro.reshape(-1, D), rdx.reshape(-1, D), rgp)
    with _Poison(monkeypatch, sync=True):                     # (blocks of >= 2048 rows run their weight gradients on a side stream)
        comp = _run_block(blocks[3][1], xb, gb, tail_c)
        dense = _run_block(blocks[3][1], joint, gj, tail_d)
    what = (name, b, mode, "joint")
    *_, e_d = _errs((dense[0].reshape(-1, D), dense[1].reshape(-1, D), dense[2]), ref, rows_b, rows_b)
    o, dx, gp, e_c = _errs(comp, ref, slice(0, lb), rows_b)
    _judge(mode, what, e_d, e_c, [o, dx] + [g_ for g_ in gp if g_ is not None])


def test_live_row_block_with_a_bias_is_refused():
    """functional._linear_bwd_gen: editor_colsum has no live-row form, so a bias gradient of a compacted product is an error, not a
    silent sum over rows nobody wrote"""
    model = _hma_model("bf16")
    params = list(_hma_blocks(model)[0][1])
    plan, h, live = _plan("r1", 8)
    x = _contract_rows(live, plan.ma, D, 211).requires_grad_(True)
    params[11] = torch.zeros(D, device="cuda", requires_grad=True)                            # an fc2 bias
    tail = (plan.mask_a, None, HEADS, 1e-5, torch.bfloat16, None, None, plan.cu, T, plan.live_a, None, None)
    out = fn.TransformerBlockFn.apply(x, *params, *tail)
    g = _contract_rows(live, plan.ma, D, 212, std=1e-2)
    with pytest.raises(RuntimeError, match="bias gradient of a live-row"):
        out.backward(g)


MODEL_CASES = [(n, b) for n in ("r1", "b1", "t256p1", "skewed", "all") for b in (8, 64)]
MODEL_GRADS = ("FUSE_block.attn1.qkv.weight", "FUSE_block.mlpN.fc2.weight", "FUSE_block.normR.weight", "FUSE_block.out_norm.bias",
               "BACKBONE.base.blocks.11.mlp.fc2.weight", "RGB_REDUCE.weight", "BACKBONE.base.cls_token")


class _Writer:
    def add_scalar(self, *a, **k):
        pass


def test_split_precision_mode_takes_the_compact_path_as_f16():
    """make_model.py: the f16x2 mode's HMA head runs as the f16 mode's (SPLIT_SCOPE 'selection', the preset) or on half pairs ('all');
    either way through _hma_compact - so the whole-model test below includes it"""
    m = _hma_model("f16x2")
    assert m.split_fwd and m.hma_compact and m.act_dtype == torch.float16 and not m.hma_attn_f32
    assert m.fn_dtype_hma == (torch.float16 if m.split_selection_only else fn.F16X2)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,b", MODEL_CASES, ids=_ids(MODEL_CASES))
def test_whole_model_compact_head_at_edge_plans(name, b, mode):
    """test_hma_compact_equals_dense_bf16 at forced edge selections: compact == dense within its bounds, and with every unwritten
    buffer poisoned the compact step stays finite and bit-identical."""
    import editor_amd.ops as ops_mod
    seed = 31
    counts = he.counts_for(name, b)
    live = he.check_plan(name, b, counts)
    assert min(counts) >= 1                                               # the pooling divides by the kept-patch count
    index = he.make_index(counts)
    img, label, cam, view = synth.make_batch(seed + 1, b, 256, 128, 4, instances=4)
    img, label, cam, view = {k: v.cuda() for k, v in img.items()}, label.cuda(), cam.cuda(), view.cuda()
    old = ops_mod.POISON_UNWRITTEN
    res = {}
    try:
        for tag, compact, poison in (("dense", False, False), ("compact", True, False), ("poison", True, True)):
            ops_mod.POISON_UNWRITTEN = poison
            m = _hma_model(mode)                           # one model per mode, put back to its initial state before every step
            if mode not in _PRISTINE:
                _PRISTINE[mode] = {k: v.detach().clone() for k, v in m.state_dict().items()}
            m.load_state_dict(_PRISTINE[mode])
            for p in m.parameters():
                p.grad = None
            m.train()
            m.hma_compact, m.teacher_index = compact, index
            out = m(img, label=label, cam_label=cam, view_label=view, writer=_Writer(), epoch=1)
            total = out[-1]
            for i, o in enumerate(out[:-1]):
                total = total + (o * synth.uniform(5, "proj/%d" % i, tuple(o.shape)).cuda()).mean()
            total.backward()
            torch.cuda.synchronize()
            assert ("plan" in m.last_aux) == compact
            if compact:
                assert m.last_aux["plan"].total == live == int(index.sum()) + b
            res[tag] = ([o.detach().float().cpu() for o in out],
                        {k: p.grad.detach().float().cpu() for k, p in m.named_parameters() if p.grad is not None},
                        m.last_aux["num"].cpu(), m.last_aux["index"].cpu())
            del out, total
    finally:
        ops_mod.POISON_UNWRITTEN = old
        m.hma_compact, m.teacher_index = True, None
        m.load_state_dict(_PRISTINE[mode])
        torch.cuda.empty_cache()
    dn, cp, po = res["dense"], res["compact"], res["poison"]
    assert torch.equal(dn[3], cp[3]) and torch.equal(cp[3], index) and torch.equal(dn[2], cp[2])
    assert torch.equal(cp[2], index.sum(1).float())
    cap_o, cap_g = 1.5e-2, 4e-2                                           # the existing test's bounds, in every mode
    for a_, b_ in zip(dn[0], cp[0]):
        assert rel_err(b_, a_) < cap_o, (name, b, mode, rel_err(b_, a_))
    for k in MODEL_GRADS:
        assert rel_err(cp[1][k], dn[1][k]) < cap_g, (name, b, mode, k, rel_err(cp[1][k], dn[1][k]))
    assert cp[1].keys() == po[1].keys() and len(po[1]) > 150
    for k, g in po[1].items():
        assert torch.isfinite(g).all(), (name, b, mode, k)
        assert torch.equal(g, cp[1][k]), (name, b, mode, k, "poisoned != unpoisoned")
    for a_, b_ in zip(cp[0], po[0]):
        assert torch.equal(a_, b_)
