"""The two-stage reductions' one protocol (include/editor_hip.h: a producer leaves partial rows and reports their count, the caller
folds): every producer once with rq=None (fold on the spot, editor_reduce_rows) and once through a ReduceQueue (one
editor_reduce_rows_multi launch at flush()).  Same partial rows, same summation order in both fold kernels: every output is
bit-identical.  The reduced vectors are also checked against an fp64 restatement on the CPU, with the tolerances the tests of the same
kernels in test_gpu_kernels.py use.  Shapes: the smallest that reach each branch (WS_ROWS = 1024 partial rows, four rows per
workgroup): fewer rows than one workgroup, and 4100 rows = 1025 workgroups capped to 1024, where the grid-stride tail runs."""
import pytest
import torch

from conftest import rel_err
from editor_amd import ops

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
TOL_LN = 2e-5        # test_gpu_kernels.test_layernorm_fwd_bwd: dgamma / dbeta
TOL_CS = 1e-5        # test_gpu_kernels: test_colsum_cast, test_cast_rows_colsum, test_layernorm_bwd_cast_fused, test_gemm_bf16_colsum_side_output
EPS = 1e-6


def _randn(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _both(run):
    """run(rq) -> tuple of tensors (None entries allowed): once unqueued, once through a fresh queue; asserts equal bits"""
    plain = run(None)
    rq = ops.ReduceQueue(torch.device("cuda", 0))
    queued = run(rq)
    assert rq.jobs, "the queued run left nothing in the queue"
    rq.flush()
    torch.cuda.synchronize()
    assert len(plain) == len(queued)
    for i, (a, b) in enumerate(zip(plain, queued)):
        assert (a is None) == (b is None), i
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a, b), ("output", i)
    return plain


def _ln_case(m, d, seed):
    x = _randn((m, d), seed, 2.0) + 0.3
    gam = _randn((d,), seed + 1, 0.5) + 1.0
    _, mean, rstd = ops.layernorm_fwd(x, gam, torch.zeros_like(gam), EPS, torch.float32)
    x64 = x.double().cpu()
    xhat = (x64 - x64.mean(1, keepdim=True)) / (x64.var(1, unbiased=False, keepdim=True) + EPS).sqrt()
    return x, gam, mean, rstd, xhat


def _plan(b, t, nl, seed):
    """(rowscale, perm, live (1,) int32) of one MLP branch with exactly nl of b samples kept (test_gpu_dropskip_edges._plan)"""
    def keep(n, s):
        k = torch.zeros(b, dtype=torch.bool)
        k[torch.randperm(b, generator=torch.Generator().manual_seed(s))[:n]] = True
        return k
    keeps = torch.stack([keep(b, 0), keep(nl, seed)]).unsqueeze(0)
    s = keeps.float() / 0.9
    sc = s.unsqueeze(-1).expand(*s.shape, t).reshape(1, 2, -1).contiguous().cuda()
    perm, _, live = ops.droppath_plan(sc, 1, b, t)
    assert int(live[0, 1]) == nl * t
    return sc[0, 1].contiguous(), perm[0, 1].contiguous(), live[0, 1:2].contiguous()


# rows as (samples, tokens): 3 rows, and 4100 = 1025 workgroups
ROWS = {3: (3, 1, 2), 4100: (100, 41, 60)}          # m: (b, t, live samples)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("m,d", [(3, 256), (4100, 256), (3, 384), (4100, 384)])
def test_layernorm_bwd(dtype, m, d):
    x, gam, mean, rstd, xhat = _ln_case(m, d, 10 + d)
    dy = _randn((m, d), 3).to(DT[dtype])
    dx, dg, db = _both(lambda rq: ops.layernorm_bwd(dy, x, gam, mean, rstd, dy_scale=0.5, rq=rq))
    dy64 = dy.double().cpu() * 0.5
    assert rel_err(dg.cpu(), (dy64 * xhat).sum(0)) < TOL_LN
    assert rel_err(db.cpu(), dy64.sum(0)) < TOL_LN
    # no parameter gradients: nothing to fold, queue or not - the same dx
    rq = ops.ReduceQueue(dx.device)
    for q in (None, rq):
        dx2, dg2, db2 = ops.layernorm_bwd(dy, x, gam, mean, rstd, want_param_grads=False, dy_scale=0.5, rq=q)
        assert dg2 is None and db2 is None and not rq.jobs and torch.equal(dx2, dx)


@pytest.mark.parametrize("want_colsum", [True, False])
@pytest.mark.parametrize("m,d", [(3, 256), (4100, 256), (3, 768), (4100, 768)])
def test_layernorm_bwd_cast(m, d, want_colsum):
    dt, gs = torch.bfloat16, 4.0
    x, gam, mean, rstd, xhat = _ln_case(m, d, 20 + d)
    dy = _randn((m, d), 4).to(dt)
    res = _randn((m, d), 5)
    rs = torch.rand(m, generator=torch.Generator().manual_seed(6)).cuda() + 0.5
    dx, dg, db, c16, cs = _both(lambda rq: ops.layernorm_bwd_cast(dy, x, gam, mean, rstd, res, rs, gs, dy_scale=0.5,
                                                                  want_colsum=want_colsum, rq=rq))
    dy64 = dy.double().cpu() * 0.5
    assert rel_err(dg.cpu(), (dy64 * xhat).sum(0)) < TOL_LN
    assert rel_err(db.cpu(), dy64.sum(0)) < TOL_LN
    assert (cs is not None) == want_colsum
    if want_colsum:
        assert rel_err(cs.cpu(), c16.double().sum(0).cpu() / gs) < TOL_CS

    # compacted rows (stochastic depth): dy on the rows of this branch's plan, the cast onto the consumer's - with and without a queue
    b, t, nl = ROWS[m]
    scale_p, p, lv = _plan(b, t, nl, 40 + m)
    rs_c, p_c, _ = _plan(b, t, max(nl - 1, 1), 50 + m)
    live, kept, pl = nl * t, (scale_p != 0), p.long()
    dyc = torch.full((m, d), float("nan"), device="cuda")               # slots >= live: not read
    dyc[:live] = _randn((live, d), 7)
    dyc = dyc.to(dt)
    dyd = torch.zeros(m, d, dtype=dt, device="cuda")
    dyd[kept] = dyc[pl[kept]]
    dx_p, dg_p, db_p, c16_p, cs_p = _both(lambda rq: ops.layernorm_bwd_cast(
        dyc, x, gam, mean, rstd, res, rs_c, gs, dy_scale=0.5, want_colsum=want_colsum, rq=rq, dy_perm=p, dy_live=lv, cast_perm=p_c))
    dx_d, dg_d, db_d, c16_d, cs_d = ops.layernorm_bwd_cast(dyd, x, gam, mean, rstd, res, rs_c, gs, dy_scale=0.5,
                                                           want_colsum=want_colsum)
    assert torch.equal(dx_p, dx_d) and torch.equal(dg_p, dg_d) and torch.equal(db_p, db_d)
    assert torch.equal(c16_p[p_c.long()], c16_d)
    dyd64 = dyd.double().cpu() * 0.5
    assert rel_err(dg_p.cpu(), (dyd64 * xhat).sum(0)) < TOL_LN
    assert rel_err(db_p.cpu(), dyd64.sum(0)) < TOL_LN
    if want_colsum:
        assert torch.equal(cs_p, cs_d)
        assert rel_err(cs_p.cpu(), c16_d.double().sum(0).cpu() / gs) < TOL_CS


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("m,n", [(65, 8), (70000, 8)])       # 70000 / 64 > 1024 partial rows: 128 rows per workgroup
def test_colsum(dtype, m, n):
    dy = _randn((m, n), 8).to(DT[dtype])
    out, = _both(lambda rq: (ops.colsum(dy, scale=0.25, rq=rq),))
    assert rel_err(out.cpu(), dy.double().sum(0).cpu() * 0.25) < TOL_CS


@pytest.mark.parametrize("m", [3, 4100])
def test_cast_rows_colsum(m):
    d, dt = 256, torch.bfloat16
    x = _randn((m, d), 9, 3.0)
    b, t, nl = ROWS[m]
    rs, p, _ = _plan(b, t, nl, 60 + m)
    out, cs = _both(lambda rq: ops.cast_rows_colsum(x, rs, dt, rq=rq))
    assert torch.equal(out.cpu(), (x.cpu() * rs.cpu().view(-1, 1)).to(dt))
    assert rel_err(cs.cpu(), out.double().sum(0).cpu()) < TOL_CS
    out_p, cs_p = _both(lambda rq: ops.cast_rows_colsum(x, rs, dt, 4.0, rq=rq, perm=p))
    out_d, cs_d = ops.cast_rows_colsum(x, rs, dt, 4.0)
    assert torch.equal(out_p[p.long()], out_d) and torch.equal(cs_p, cs_d)
    assert rel_err(cs_p.cpu(), out_d.double().sum(0).cpu() / 4.0) < TOL_CS


def test_gemm_colsum():
    m, n, k, dt = 2080, 512, 64, torch.bfloat16          # the smallest shape with a column-sum epilogue
    assert ops.gemm_colsum_ok(m, n, k, dt, 0, 1, None)
    a, w = _randn((m, k), 11).to(dt), _randn((n, k), 12, 0.1).to(dt)

    def run(rq):
        c = torch.empty(m, n, dtype=dt, device="cuda")
        cs = torch.empty(n, device="cuda")
        ops.gemm(a, w, c, m, n, k, k, k, n, 0, 0, colsum=cs, colsum_scale=0.5, rq=rq)
        return c, cs
    c, cs = _both(run)
    assert rel_err(cs.cpu(), c.double().sum(0).cpu() * 0.5) < TOL_CS


def test_attention_bwd_colsum():
    b, t, heads, hd, dt = 2, 17, 1, 64, torch.bfloat16
    qkv = _randn((b * t, 3 * hd), 13, 0.9).to(dt)
    do = _randn((b * t, hd), 14).to(dt)
    o, lse = ops.attention_fwd(qkv, b, t, heads, hd)
    assert ops.attention_bwd_colsum_ok(qkv, t, hd)

    def run(rq):
        cs = torch.full((3 * hd,), float("nan"), device="cuda")
        return ops.attention_bwd(qkv, do, b, t, heads, hd, None, lse, o, colsum=cs, colsum_scale=0.5, rq=rq), cs
    dqkv, cs = _both(run)
    # the bound of test_gpu_kernels._colsum_case: sums of the fp32 values the stored 16-bit entries were rounded from
    stored = dqkv.double()
    eps = 2.0 ** -8
    bound = stored.abs().sum(0) * (0.5 * eps + 4e-6) + 1e-6
    err = (cs.double() * 2.0 - stored.sum(0)).abs()
    assert torch.isfinite(cs).all() and bool((err <= bound).all()), float((err / bound).max())
    assert float(err.mean() / stored.abs().sum(0).mean()) < 0.1 * eps


def test_wgrad_group_ln_role():
    """ops.gemm_wgrad_group_ln at the shape of test_gpu_model's role test: a ViT-B block's four weight gradients over 64 x 129 rows"""
    m, d, dt, gs = 64 * 129, 768, torch.bfloat16, 2.0
    x, gam, mean, rstd, xhat = _ln_case(m, d, 70)
    dy = _randn((m, d), 15).to(dt)
    res = _randn((m, d), 16)
    rs = torch.rand(m, generator=torch.Generator().manual_seed(17)).cuda() + 0.5
    ops_ = [(_randn((m, n), 18 + i).to(dt), _randn((m, k), 28 + i).to(dt)) for i, (n, k) in
            enumerate([(2304, 768), (768, 768), (3072, 768), (768, 3072)])]

    def run(rq):
        jobs = [(gy, gx, torch.empty(gy.shape[1], gx.shape[1], device="cuda")) for gy, gx in ops_]
        r = ops.gemm_wgrad_group_ln(jobs, m, 1.0, dy, x, gam, mean, rstd, res, rs, gs, dy_scale=0.5, rq=rq)
        return tuple(r) + tuple(j[2] for j in jobs)
    dx, dg, db, c16, cs = _both(run)[:5]
    dy64 = dy.double().cpu() * 0.5
    assert rel_err(dg.cpu(), (dy64 * xhat).sum(0)) < TOL_LN
    assert rel_err(db.cpu(), dy64.sum(0)) < TOL_LN
    assert rel_err(cs.cpu(), c16.double().sum(0).cpu() / gs) < TOL_CS


def test_queue_overflow_and_oversized_request():
    dev = torch.device("cuda", 0)
    dys = [_randn((65, 8), 80 + i) for i in range(9)]
    want = [ops.colsum(dy) for dy in dys]
    rq = ops.ReduceQueue(dev)
    got = []
    for i, dy in enumerate(dys):                          # nine jobs through an eight-job queue: the seventh forces a flush
        got.append(ops.colsum(dy, rq=rq))
        assert len(rq.jobs) == (i % 7) + 1
    rq.flush()
    # a request larger than the queue's slot: no region, folded on the spot
    small = ops.ReduceQueue(dev, slot=0, nslots=4096)
    assert small.region(ops.WS_ROWS * 8) is None
    over = ops.colsum(dys[0], rq=small)
    assert not small.jobs
    torch.cuda.synchronize()
    for a, b in zip(want + [want[0]], got + [over]):
        assert torch.equal(a, b)
