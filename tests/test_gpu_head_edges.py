"""The small fp32 kernels behind the backbone - BatchNorm1d, OCFR, the loss head, SFTS apply / pooling, packed pooling, the
patch-embed assembly, mask_or - at the batch sizes and widths where they switch code paths (csrc/head.hip, loss.hip, norm.hip,
compact.hip, select.hip).  The whole-model tests reach them at a handful of sizes only.

Method, the same for every case:
  * reference = a plain PyTorch restatement of the documented formula (include/editor_hip.h, the comment above each kernel),
    evaluated on the CPU in float64 (`_*_ref(..., torch.float64)`); the oracle is compared too where it can express the case
    (it needs equal identity groups);
  * the kernels are called through editor_amd.ops, so the saved tensors are checked, and once per family through the autograd
    Function of editor_amd.functional;
  * every call runs inside _Poison (NaN in every floating-point torch.empty / empty_like): an element a kernel does not write
    fails the comparison.  Outputs documented as unwritten (pool_packed_bwd with `live`) are compared on their live rows only;
  * two error measures per tensor: the suite's L2 relative error (`rel_err`) and the worst single row (`_row_err`);
  * tolerances: L2 1e-5 (2e-5 for the triplet feature gradient), the project's figures for these kernels.  The worst-row bounds
    are 4 x the deviation of the SAME restatement evaluated in float32 on the CPU from its float64 value, maximum over the
    family's cases (the kernel and the CPU sum in different orders; 4 x covers that and no more).  `python
    tests/test_gpu_head_edges.py` prints those deviations (no GPU needed); they stand next to the constants in ROW_TOL.
"""
import itertools
import sys

import pytest
import torch

from conftest import rel_err
from test_gpu_dropskip_edges import _Poison

pytestmark = pytest.mark.gpu

L2 = 1e-5               # outputs, losses, BN / OCFR / SFTS / pool / embed gradients
L2_TRIPLET_DFEAT = 2e-5

# worst-row bounds: name -> (measured float32-CPU-vs-float64 worst-row deviation, maximum over the family's cases; bound = 4 x)
ROW_DEV = {
    # BatchNorm1d (rows = samples AND columns = features, whichever is worse), B >= 4
    "bn.y": 7.68e-6, "bn.dx": 4.51e-6,
    # B = 3: dx is a difference of nearly equal terms (three samples leave one degree of freedom per column besides the mean)
    "bn.dx.B3": 9.45e-5,
    "ocfr.fnorm": 1.55e-7, "ocfr.centers": 1.40e-7, "ocfr.dfeat": 9.85e-7,
    "ce.dlogits": 3.00e-7,
    # rows of identities with >= 2 samples / with one sample: a single-sample anchor's d_ap is the rounding noise of the expanded
    # form (~ sqrt(eps32 |f|^2) = 1e-2 at D = 2304), which enters its sigmoid(d_ap - d_an) and so its whole (tiny) gradient row
    "triplet.dfeat": 3.99e-6, "triplet.dfeat.single": 1.93e-2,
    "center.dx": 5.20e-8, "center.dc": 1.53e-7,
    "sfts.dfeat": 8.14e-8,
    "pool.out": 2.41e-8, "pool.dx": 2.88e-8,
    "embed.x": 5.83e-8, "embed.dpos": 1.59e-7, "embed.dsie": 3.60e-7,
}
# BatchNorm1d at B = 2: xhat = +-1 up to eps / var, so dx = k (2 dy_b - sum dy - xhat_b sum dy xhat) cancels to ~ eps / var of
# its terms.  float32 on the CPU deviates from float64 by 2.56e-5 in L2 (the 1e-5 does not fit: 4 x that instead) and by 4.5 in
# the worst column - no correct digit - so the worst-row measure is not taken for that one batch size.
BN_DX_B2_L2_DEV = 2.56e-5
ROW_TOL = {k: 4.0 * v for k, v in ROW_DEV.items()}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, std=1.0):
    return torch.randn(*shape, generator=_gen(seed)) * std


def _row_err(a, b):
    """worst single row: max over rows of |a_r - b_r| / |b_r| (a whole-tensor norm hides one wrong sample of 257)"""
    a = torch.as_tensor(a).double()
    b = torch.as_tensor(b).double()
    if a.dim() < 2:
        a, b = a.reshape(1, -1), b.reshape(1, -1)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    return ((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)).max().item()


def _check(what, got, ref, l2=L2, row=None, cols=False):
    """both measures against the float64 reference; prints each figure before it asserts"""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    e = rel_err(got, ref)
    r = _row_err(got, ref)
    if cols:
        r = max(r, _row_err(got.t(), ref.t()))
    print("%-40s l2 %.3e (< %.1e)  worst row %.3e%s" % (what, e, l2, r, "" if row is None else " (< %.1e)" % ROW_TOL[row]))
    assert e < l2, (what, "l2", e)
    if row is not None:
        assert r < ROW_TOL[row], (what, "worst row", r, ROW_TOL[row])


def _dev(acc, name, a32, a64, cols=False):
    """float32-CPU-vs-float64 deviation of one tensor in both measures (for the table printed by __main__)"""
    r = _row_err(a32, a64)
    if cols:
        r = max(r, _row_err(a32.t(), a64.t()))
    l, w = acc.get(name, (0.0, 0.0))
    acc[name] = (max(l, rel_err(a32, a64)), max(w, r))


def _ragged_sizes(b, lo=1, hi=9):
    """group sizes lo, lo+1, ..., hi, lo, ... until b samples are placed"""
    sizes, k = [], lo
    while sum(sizes) < b:
        sizes.append(min(k, b - sum(sizes)))
        k = lo if k == hi else k + 1
    return sizes


def _shuffled(labels, seed):
    return labels[torch.randperm(labels.numel(), generator=_gen(seed))]


# =================================================================================================================================
# BatchNorm1d
# =================================================================================================================================
BN_B = [1, 2, 3, 4, 5, 127, 128, 129, 255, 256, 257, 300]
BN_C = [768, 2304, 100, 65]
BN_MOM, BN_EPS = 0.1, 1e-5


def _bn_inputs(b, c):
    """every B takes the leading rows of ONE (300, C) matrix: 128 / 129 and 256 / 257 differ by the last row only"""
    return dict(x=(_randn((300, c), 11, 0.8) + 0.3)[:b].contiguous(), dy=_randn((300, c), 12)[:b].contiguous(),
                gamma=_randn((c,), 13, 0.3) + 1.0, beta=_randn((c,), 14, 0.2), rmean=_randn((c,), 15, 0.1),
                rvar=_randn((c,), 16, 0.1).abs() + 0.5)


def _bn_ref(i, dt, training=True):
    x, dy, gamma, beta, rmean, rvar = (i[k].to(dt) for k in ("x", "dy", "gamma", "beta", "rmean", "rvar"))
    b = x.shape[0]
    o = {}
    if training:
        mean = x.sum(0) / b
        q = ((x - mean) ** 2).sum(0)
        var = q / b                                                    # biased: normalisation
        invstd = (var + BN_EPS).rsqrt()
        o["rmean"] = (1 - BN_MOM) * rmean + BN_MOM * mean
        o["rvar"] = (1 - BN_MOM) * rvar + BN_MOM * (q / (b - 1) if b > 1 else var)      # unbiased; B == 1: the biased value (0)
        o["save_mean"], o["save_invstd"] = mean, invstd
    else:
        mean, invstd = rmean, (rvar + BN_EPS).rsqrt()
    o["y"] = (x - mean) * (gamma * invstd) + beta
    if training:
        xh = (x - mean) * invstd
        o["dbeta"] = dy.sum(0)
        o["dgamma"] = (dy * xh).sum(0)
        o["dx"] = gamma * invstd / b * (b * dy - o["dbeta"] - xh * o["dgamma"])
    return o


def _wide(x, pad=24, off=8, seed=99):
    """x as a column slice of a wider matrix (row stride > columns), as ops._rows_view allows"""
    w = _randn((x.shape[0], x.shape[1] + pad), seed)
    w[:, off:off + x.shape[1]] = x
    return w


@pytest.mark.parametrize("strided", [0, 1], ids=["contig", "ldx"])
@pytest.mark.parametrize("c", BN_C)
@pytest.mark.parametrize("b", BN_B)
def test_bn1d_training_fwd_bwd(monkeypatch, b, c, strided):
    """B <= 128: bn1d_*_reg_kernel<32>; 128 < B <= 256: <64>; B > 256: one thread per column.  C = 100, 65: partial last block."""
    from editor_amd import ops
    i = _bn_inputs(b, c)
    ref = _bn_ref(i, torch.float64)
    xw = _wide(i["x"]).cuda() if strided else None
    x = xw[:, 8:8 + c] if strided else i["x"].cuda()
    xw0 = xw.clone() if strided else None
    gamma, beta, rm, rv = i["gamma"].cuda(), i["beta"].cuda(), i["rmean"].cuda(), i["rvar"].cuda()
    with _Poison(monkeypatch):
        y, sm, si = ops.bn1d_fwd(x, gamma, beta, rm, rv, BN_MOM, BN_EPS, True)
        dx, dg, db = ops.bn1d_bwd(i["dy"].cuda(), x, gamma, sm, si)
        torch.cuda.synchronize()
    t = "bn B=%d C=%d %s " % (b, c, "ldx" if strided else "")
    _check(t + "y", y, ref["y"], row="bn.y", cols=True)
    _check(t + "save_mean", sm, ref["save_mean"])
    _check(t + "save_invstd", si, ref["save_invstd"])
    _check(t + "running_mean", rm, ref["rmean"])
    _check(t + "running_var", rv, ref["rvar"])
    if b == 1:                                                         # x - mean == 0 exactly: dx = 0, dgamma = 0
        assert not dx.any() and not dg.any()
    else:
        if b == 2:
            _check(t + "dx", dx, ref["dx"], l2=4 * BN_DX_B2_L2_DEV)
        else:
            _check(t + "dx", dx, ref["dx"], row="bn.dx.B3" if b == 3 else "bn.dx", cols=True)
        _check(t + "dgamma", dg, ref["dgamma"])
    _check(t + "dbeta", db, ref["dbeta"])
    if strided:
        assert torch.equal(xw, xw0)                                    # the input, and the columns beside it, bit for bit


@pytest.mark.parametrize("c", [768, 65])
@pytest.mark.parametrize("b", BN_B)
def test_bn1d_eval(monkeypatch, b, c):
    from editor_amd import ops
    i = _bn_inputs(b, c)
    ref = _bn_ref(i, torch.float64, training=False)
    rm, rv = i["rmean"].cuda(), i["rvar"].cuda()
    with _Poison(monkeypatch):
        y, sm, si = ops.bn1d_fwd(_wide(i["x"]).cuda()[:, 8:8 + c], i["gamma"].cuda(), i["beta"].cuda(), rm, rv, BN_MOM, BN_EPS, False)
        torch.cuda.synchronize()
    assert sm is None and si is None
    _check("bn eval B=%d C=%d y" % (b, c), y, ref["y"], row="bn.y", cols=True)
    assert torch.equal(rm.cpu(), i["rmean"]) and torch.equal(rv.cpu(), i["rvar"])      # eval: running statistics untouched


def test_bn1d_function_and_refusals(monkeypatch, oracle):
    from editor_amd import functional as fn, ops
    b, c = 129, 100
    i = _bn_inputs(b, c)
    ref = _bn_ref(i, torch.float64)
    x, gamma, beta = (i[k].cuda().requires_grad_(True) for k in ("x", "gamma", "beta"))
    rm, rv = i["rmean"].cuda(), i["rvar"].cuda()
    with _Poison(monkeypatch):
        y = fn.BatchNorm1dFn.apply(x, gamma, beta, rm, rv, BN_MOM, BN_EPS, True)
        y.backward(i["dy"].cuda())
        torch.cuda.synchronize()
    sd = {"p.running_mean": i["rmean"].clone(), "p.running_var": i["rvar"].clone(), "p.weight": i["gamma"], "p.bias": i["beta"]}
    yo = oracle._bn1d(i["x"], sd, "p", True, BN_MOM, BN_EPS)
    for name, got, want in [("y", y, ref["y"]), ("dx", x.grad, ref["dx"]), ("dgamma", gamma.grad, ref["dgamma"]),
                            ("dbeta", beta.grad, ref["dbeta"]), ("running_mean", rm, ref["rmean"]), ("running_var", rv, ref["rvar"]),
                            ("y vs oracle", y, yo.double()), ("running_var vs oracle", rv, sd["p.running_var"].double())]:
        _check("bn Function " + name, got, want)
    z = torch.zeros
    for bb, cc in [(0, 8), (4, 0)]:
        e = lambda *s: z(*s, device="cuda")                            # noqa: E731
        with pytest.raises(RuntimeError):
            ops.bn1d_fwd(e(bb, cc), e(cc), e(cc), e(cc), e(cc), BN_MOM, BN_EPS, True)
        with pytest.raises(RuntimeError):
            ops.bn1d_bwd(e(bb, cc), e(bb, cc), e(cc), e(cc), e(cc))


# =================================================================================================================================
# OCFR
# =================================================================================================================================
OCFR_SHAPES = [(128, 201, 768), (30, 7, 100), (257, 50, 1024), (4, 3, 36)]
OCFR_MOM = 0.8


def _ocfr_labels(b, c, seed):
    """ragged groups; class 0 appears exactly once, class c - 1 (and whatever the draw misses) never"""
    lab = torch.randint(1, max(c - 1, 2), (b,), generator=_gen(seed))
    lab[b // 2] = 0
    return lab


def _ocfr_inputs(b, c, d, seed):
    f = _randn((b, d), seed, 0.7)
    f[1] = 0.0                                                         # F.normalize's eps = 1e-12 clamp
    return dict(f=f, label=_ocfr_labels(b, c, seed + 1), centers=_randn((c, d), seed + 2, 0.05), dloss=torch.tensor([1.3]))


def _ocfr_ref(i, dt):
    f, c, dl = i["f"].to(dt), i["centers"].to(dt), i["dloss"].to(dt)
    lab = i["label"]
    b, d = f.shape
    inv = 1.0 / f.norm(dim=1).clamp_min(1e-12)
    fn_ = f * inv[:, None]
    c2 = c.clone()
    for u in lab.unique():
        c2[u] = OCFR_MOM * fn_[lab == u].mean(0) + (1 - OCFR_MOM) * c[u]
    loss = ((c2[lab] - fn_) ** 2).sum() / (b * d)
    g = dl * 2.0 / (b * d) * (fn_ - c2[lab])
    df = inv[:, None] * (g - fn_ * (fn_ * g).sum(1, keepdim=True))
    return dict(fnorm=fn_, inv_norm=inv, centers=c2, loss=loss.reshape(1), dfeat=df)


@pytest.mark.parametrize("nmod", [2, 4])
@pytest.mark.parametrize("b,c,d", OCFR_SHAPES)
def test_ocfr_fwd_bwd(monkeypatch, b, c, d, nmod):
    """ragged labels, absent classes, a class seen once, a zero feature row, strided features, loss accumulated over nmod tables"""
    from editor_amd import ops
    ins = [_ocfr_inputs(b, c, d, 100 * m + b) for m in range(nmod)]
    for i in ins[1:]:
        i["label"] = ins[0]["label"]
    refs = [_ocfr_ref(i, torch.float64) for i in ins]
    lab = ins[0]["label"]
    absent = torch.ones(c, dtype=torch.bool)
    absent[lab.unique()] = False
    assert absent[c - 1] and int((lab == 0).sum()) == 1
    with _Poison(monkeypatch):
        loss = torch.empty(1, dtype=torch.float32, device="cuda")      # poisoned: accumulate = 0 must overwrite it
        seven = torch.full((1,), 7.0, device="cuda")
        total = 0.0
        for m, (i, ref) in enumerate(zip(ins, refs)):
            feat = _wide(i["f"]).cuda()[:, 8:8 + d] if m % 2 == 0 else i["f"].cuda()
            cen = i["centers"].cuda()
            fn_, inv = ops.ocfr_fwd(feat, lab.cuda(), cen, OCFR_MOM, loss, accumulate=m > 0)
            df = ops.ocfr_bwd(fn_, inv, cen, lab.cuda(), i["dloss"].cuda())
            torch.cuda.synchronize()
            total = total + ref["loss"]
            t = "ocfr B=%d C=%d D=%d m=%d " % (b, c, d, m)
            _check(t + "fnorm", fn_, ref["fnorm"], row="ocfr.fnorm")
            _check(t + "inv_norm", inv, ref["inv_norm"])
            _check(t + "centers", cen, ref["centers"], row="ocfr.centers")
            assert torch.equal(cen.cpu()[absent], i["centers"][absent])             # classes without a sample: bit-identical
            _check(t + "loss (accumulated)", loss, total)
            _check(t + "dfeat", df, ref["dfeat"], row="ocfr.dfeat")
            assert not fn_[1].any()                                    # the zero row (its inv_norm = 1e12 is part of inv_norm above)
        i = ins[0]
        ops.ocfr_fwd(i["f"].cuda(), lab.cuda(), i["centers"].cuda(), OCFR_MOM, seven, accumulate=True)
        _check("ocfr accumulate onto 7", seven, 7.0 + refs[0]["loss"])


def test_ocfr_function_vs_oracle(monkeypatch, oracle):
    from editor_amd import functional as fn
    b, c, d, nmod = 128, 201, 768, 3
    lab = torch.arange(16).repeat_interleave(8) * 11                   # equal, contiguous groups: what the oracle expresses
    feats = [_randn((b, d), 40 + m, 0.7) for m in range(nmod)]
    cens = [_randn((c, d), 50 + m, 0.05) for m in range(nmod)]
    fr = [f.clone().requires_grad_(True) for f in feats]
    cr = [x.clone() for x in cens]
    lo = oracle.ocfr(fr, cr, lab, OCFR_MOM)
    (1.3 * lo).backward()
    ins = [dict(f=f, label=lab, centers=x, dloss=torch.tensor([1.3])) for f, x in zip(feats, cens)]
    refs = [_ocfr_ref(i, torch.float64) for i in ins]
    fg = [f.cuda().requires_grad_(True) for f in feats]
    cg = [x.cuda() for x in cens]
    with _Poison(monkeypatch):
        lg = fn.OCFRFn.apply(lab.cuda(), OCFR_MOM, nmod, *fg, *cg)
        (1.3 * lg).backward()
        torch.cuda.synchronize()
    _check("ocfr Function loss", lg.view(1), sum(r["loss"] for r in refs))
    _check("ocfr Function loss vs oracle", lg.view(1), lo.detach().double().view(1))
    for m in range(nmod):
        _check("ocfr Function dfeat %d" % m, fg[m].grad, refs[m]["dfeat"], row="ocfr.dfeat")
        _check("ocfr Function dfeat %d vs oracle" % m, fg[m].grad, fr[m].grad.double())
        _check("ocfr Function centers %d" % m, cg[m], refs[m]["centers"], row="ocfr.centers")
        _check("ocfr Function centers %d vs oracle" % m, cg[m], cr[m].double())


# =================================================================================================================================
# loss head: cross entropy with label smoothing
# =================================================================================================================================
CE_SHAPES = [(1, 5), (129, 171), (257, 1501), (1024, 255), (64, 257)]
CE_EPS = 0.1


def _ce_inputs(b, c):
    x = _randn((b, c), 7 * b + c, 3.0)
    x[0] = torch.linspace(-80.0, 80.0, c)[torch.randperm(c, generator=_gen(3))]       # the max-subtraction must hold
    t = torch.randint(0, c, (b,), generator=_gen(b + c))
    t[0], t[-1] = 0, c - 1
    if b > 2:
        t[1] = c - 1
    return dict(x=x, t=t, dloss=torch.tensor([0.37]))


def _ce_ref(i, dt):
    x, dl = i["x"].to(dt), i["dloss"].to(dt)
    b, c = x.shape
    logp = torch.log_softmax(x, dim=1)
    soft = torch.zeros_like(x).scatter_(1, i["t"][:, None], 1.0) * (1 - CE_EPS) + CE_EPS / c
    return dict(loss=(-(soft * logp).sum(1)).mean().reshape(1), dlogits=dl / b * (logp.exp() - soft))


@pytest.mark.parametrize("b,c", CE_SHAPES)
def test_ce_smooth(monkeypatch, oracle, b, c):
    from editor_amd import ops
    i = _ce_inputs(b, c)
    ref = _ce_ref(i, torch.float64)
    x, t = i["x"].cuda(), i["t"].cuda()
    with _Poison(monkeypatch):
        loss = torch.empty(1, dtype=torch.float32, device="cuda")
        ops.ce_smooth_fwd(x, t, CE_EPS, loss, accumulate=False)
        acc = torch.full((1,), -2.5, device="cuda")
        ops.ce_smooth_fwd(x, t, CE_EPS, acc, accumulate=True)
        d = ops.ce_smooth_bwd(x, t, CE_EPS, i["dloss"].cuda())
        torch.cuda.synchronize()
    n = "ce B=%d C=%d " % (b, c)
    _check(n + "loss", loss, ref["loss"])
    _check(n + "loss accumulated onto -2.5", acc, ref["loss"] - 2.5)
    _check(n + "dlogits", d, ref["dlogits"], row="ce.dlogits")
    _check(n + "loss vs oracle", loss, oracle.cross_entropy_label_smooth(i["x"], i["t"], CE_EPS).double().view(1))


# =================================================================================================================================
# loss head: batch-hard soft-margin triplet
# =================================================================================================================================
TRIPLET_SHAPES = [(2, 32), (63, 100), (64, 768), (65, 2304), (129, 2304), (257, 768), (1024, 2304), (300, 1152), (300, 1024)]
TRIPLET_EQUAL_K = {2: 1, 63: 3, 64: 4, 65: 5, 129: 3, 1024: 4, 300: 4}       # 257 is prime: ragged only
TRIPLET_CASES = [(b, d, "ragged") for b, d in TRIPLET_SHAPES] + [(b, d, "equal") for b, d in TRIPLET_SHAPES if b in TRIPLET_EQUAL_K]


def _triplet_inputs(b, d, groups, seed=2):
    if groups == "equal":
        k = TRIPLET_EQUAL_K[b]
        lab = torch.arange(b // k).repeat_interleave(k)
    else:
        sizes = _ragged_sizes(b) if b > 2 else [1, 1]                  # sizes 1 .. 9: single-sample identities included
        lab = torch.cat([torch.full((s,), n) for n, s in enumerate(sizes)])
    lab = _shuffled(lab * 3, seed + b)
    f = _randn((b, d), seed * 1000 + b + d, 0.7)
    if b == 2:
        # two single-sample identities: each anchor's positive distance is its own, i.e. the rounding noise of the expanded form,
        # and with only 32 columns that noise would be 1e-3 of the loss in ANY float32 evaluation.  Multiples of 1/4 make every
        # product and sum exact, so |f_i - f_i|^2 = 0 in float32 and float64 alike (the larger ragged cases keep the noisy form)
        f = (f * 4).round() / 4
    dup = None
    cnt = torch.bincount(lab)
    big = [int(u) for u in torch.nonzero(cnt >= 3).flatten()]
    if big:
        # two bit-identical rows in one identity, scaled so that they are the farthest positives of its other members: an exact
        # tie, which resolves to the lowest index
        m = torch.nonzero(lab == big[0]).flatten()
        j1, j2 = int(m[0]), int(m[1])
        f[j1] *= 4.0
        f[j2] = f[j1]
        dup = (j1, j2)
    return dict(f=f, label=lab, dup=dup, dloss=torch.tensor([0.37]))


def _first_arg(v, best):
    """lowest index among the exact maxima / minima (stated explicitly: argmax's choice among equals is not documented)"""
    return (v == best[:, None]).to(torch.uint8).argmax(1)


def _triplet_dist(i, dt):
    f = i["f"].to(dt)
    sq = (f * f).sum(1)
    q = sq[:, None] + sq[None, :] - 2.0 * (f @ f.t())                  # the expanded form, as the reference computes it
    if i["dup"] is not None:                                           # bit-identical rows have equal distances to everyone;
        j1, j2 = i["dup"]                                              # a BLAS may round their two Gram columns differently
        q[:, j2] = q[:, j1]
        q[j2, :] = q[j1, :]
    return f, q


def _triplet_ref(i, dt):
    f, q = _triplet_dist(i, dt)
    lab, dl = i["label"], i["dloss"].to(dt)
    b = f.shape[0]
    dist = q.clamp(min=1e-12).sqrt()
    same = lab[:, None] == lab[None, :]
    inf = torch.tensor(float("inf"), dtype=dt)
    dp, dn = torch.where(same, dist, -inf), torch.where(~same, dist, inf)
    ap, an = dp.max(1).values, dn.min(1).values
    ip, in_ = _first_arg(dp, ap), _first_arg(dn, an)
    z = ap - an
    loss = torch.nn.functional.softplus(z).mean()
    ar = torch.arange(b)
    s = torch.sigmoid(z)
    cp = torch.where(q[ar, ip] > 1e-12, 1.0 / ap, torch.zeros_like(ap))             # clamp(min) passes no gradient below the floor
    cn = torch.where(q[ar, in_] > 1e-12, 1.0 / an, torch.zeros_like(an))
    ep = (f - f[ip]) * (s * cp)[:, None]
    en = (f - f[in_]) * (s * cn)[:, None]
    df = ep - en
    df = df.index_add(0, ip, -ep).index_add(0, in_, en) * (dl / b)
    return dict(idx=torch.cat([ip, in_]), coef=torch.cat([s, cp, cn]), loss=loss.reshape(1), dfeat=df, dist=dist, same=same)


def _gap(best, runner):
    return ((best - runner).abs() / best.abs().clamp_min(1e-30))


def _triplet_precondition(i, ref):
    """The index comparison is exact, which is fair only without near-ties: for every anchor the relative gap between the best
    and the runner-up distance must exceed 4 x the float32-vs-float64 deviation of the expanded distance formula."""
    dist, same = ref["dist"].clone(), ref["same"]
    b = dist.shape[0]
    _, q32 = _triplet_dist(i, torch.float32)
    d32 = q32.clamp(min=1e-12).sqrt().double()
    off = ~torch.eye(b, dtype=torch.bool)
    if i["dup"] is not None:                                           # (their mutual distance is rounding noise, as on the diagonal)
        off[i["dup"][0], i["dup"][1]] = off[i["dup"][1], i["dup"][0]] = False
    dev = ((d32 - dist).abs() / dist)[off].max().item()
    if i["dup"] is not None:
        dist[:, i["dup"][1]] = float("nan")                            # the duplicate is the same candidate, not a runner-up
    ninf = torch.tensor(float("-inf"), dtype=torch.float64)
    dp = torch.where(same & ~torch.isnan(dist), dist, ninf)
    dn = torch.where(~same & ~torch.isnan(dist), -dist, ninf)
    worst = float("inf")
    for v in (dp, dn):
        top = v.topk(min(2, b), dim=1).values
        if top.shape[1] < 2:
            continue
        ok = torch.isfinite(top[:, 1])                                 # (a single-sample identity has no runner-up positive)
        if ok.any():
            worst = min(worst, _gap(top[ok, 0], top[ok, 1]).min().item())
    print("triplet precondition: distance deviation %.2e, smallest relative gap %.2e" % (dev, worst))
    assert worst > 4 * dev, ("near-tie in the reference: choose another seed", worst, dev)
    return dev


def _triplet_compare(name, i, ref, idx, coef, loss, df):
    b = i["f"].shape[0]
    idx, coef = idx.cpu().long(), coef.cpu()
    assert torch.equal(idx, ref["idx"]), (name, "mined indices", int((idx != ref["idx"]).sum()))
    if i["dup"] is not None:                                           # the tie went to the lower index
        j1, j2 = i["dup"]
        third = [int(k) for k in torch.nonzero(i["label"] == i["label"][j1]).flatten() if int(k) not in (j1, j2)]
        assert third and all(int(idx[k]) == j1 for k in third)
    selfpos = idx[:b] == torch.arange(b)
    assert torch.equal(selfpos, torch.bincount(i["label"])[i["label"]] == 1)
    # an identity with one sample is its own hardest positive: its distance is the rounding noise of the expanded form, so
    # 1 / d_ap is compared only where idx[i] != i; there it must be finite, which makes that anchor's positive term of dfeat
    # (f_i - f_i) * w exactly 0 - as in the reference dfeat compared below
    assert bool(torch.isfinite(coef[b:2 * b][selfpos]).all())
    _check(name + "coef sigmoid", coef[:b], ref["coef"][:b])
    _check(name + "coef 1/d_ap", coef[b:2 * b][~selfpos], ref["coef"][b:2 * b][~selfpos])
    _check(name + "coef 1/d_an", coef[2 * b:], ref["coef"][2 * b:])
    _check(name + "loss", loss, ref["loss"])
    _check(name + "dfeat", df, ref["dfeat"], l2=L2_TRIPLET_DFEAT)
    df = df.cpu()
    if bool((~selfpos).any()):
        _check(name + "dfeat rows, identities of >= 2", df[~selfpos], ref["dfeat"][~selfpos], l2=L2_TRIPLET_DFEAT, row="triplet.dfeat")
    if bool(selfpos.any()):
        _check(name + "dfeat rows, single-sample identities", df[selfpos], ref["dfeat"][selfpos], l2=1.0, row="triplet.dfeat.single")


@pytest.mark.parametrize("b,d,groups", TRIPLET_CASES)
def test_triplet(monkeypatch, oracle, b, d, groups):
    """D = 1024, 2304, 1152: split-K Gram product; 768, 100, 32: single product.  B = 1024: the whole LDS list of the backward."""
    from editor_amd import ops
    i = _triplet_inputs(b, d, groups)
    ref = _triplet_ref(i, torch.float64)
    _triplet_precondition(i, ref)
    feat = _wide(i["f"], pad=16).cuda()[:, 8:8 + d]                    # a strided column slice
    with _Poison(monkeypatch):
        loss = torch.empty(1, dtype=torch.float32, device="cuda")
        idx, coef = ops.triplet_fwd(feat, i["label"].cuda(), loss, accumulate=False)
        acc = torch.full((1,), 3.0, device="cuda")
        ops.triplet_fwd(feat, i["label"].cuda(), acc, accumulate=True)
        df = ops.triplet_bwd(feat, idx, coef, i["dloss"].cuda())
        torch.cuda.synchronize()
    name = "triplet B=%d D=%d %s " % (b, d, groups)
    _triplet_compare(name, i, ref, idx, coef, loss, df)
    _check(name + "loss accumulated onto 3", acc, ref["loss"] + 3.0)
    if groups == "equal" and b > 2:
        # (in float64: the oracle's log(1 + exp(d_ap - d_an)) overflows float32 for the scaled duplicates at D = 2304, d_ap - d_an = 91)
        _check(name + "loss vs oracle", loss, oracle.triplet_soft_margin(i["f"].double(), i["label"]).view(1))


def test_triplet_batch_limit(monkeypatch):
    """the backward lists an anchor's partners in 1024 LDS entries: B = 1025 is refused by the forward already"""
    from editor_amd import ops
    f = _randn((1025, 64), 5).cuda()
    lab = (torch.arange(1025) // 5).cuda()
    loss = torch.zeros(1, device="cuda")
    with pytest.raises(RuntimeError):
        ops.triplet_fwd(f, lab, loss, accumulate=False)
    torch.cuda.synchronize()
    assert float(loss) == 0.0
    with pytest.raises(RuntimeError):
        ops.triplet_bwd(f, torch.zeros(2050, dtype=torch.int32, device="cuda"), torch.zeros(3075, device="cuda"), loss)


def test_loss_functions_through_autograd(monkeypatch):
    from editor_amd import functional as fn
    i = _triplet_inputs(129, 768, "ragged", seed=3)
    ref = _triplet_ref(i, torch.float64)
    _triplet_precondition(i, ref)
    ce = _ce_inputs(129, 171)
    cref = _ce_ref(ce, torch.float64)
    cl = _center_inputs(129, 171, 768)
    lref = _center_ref(cl, torch.float64)
    with _Poison(monkeypatch):
        wide = _wide(i["f"], pad=16).cuda().requires_grad_(True)
        lt = fn.TripletSoftMarginFn.apply(wide[:, 8:8 + 768], i["label"].cuda())
        x = ce["x"].cuda().requires_grad_(True)
        lc = fn.CrossEntropyLabelSmoothFn.apply(x, ce["t"].cuda(), CE_EPS)
        cx, cc = cl["x"].cuda().requires_grad_(True), cl["centers"].cuda().requires_grad_(True)
        ll = fn.CenterLossFn.apply(cx, cc, cl["label"].cuda())
        (0.37 * (lt + lc) + 0.9 * ll).backward()
        torch.cuda.synchronize()
    _check("Function triplet loss", lt.view(1), ref["loss"])
    _check("Function triplet dfeat", wide.grad[:, 8:8 + 768], ref["dfeat"], l2=L2_TRIPLET_DFEAT)
    assert not wide.grad[:, :8].any() and not wide.grad[:, 8 + 768:].any()
    _check("Function ce loss", lc.view(1), cref["loss"])
    _check("Function ce dlogits", x.grad, cref["dlogits"], row="ce.dlogits")
    _check("Function center loss", ll.view(1), lref["loss"])
    _check("Function center dx", cx.grad, lref["dx"], row="center.dx")
    _check("Function center dc", cc.grad, lref["dc"], row="center.dc")


# =================================================================================================================================
# loss head: centre loss
# =================================================================================================================================
CENTER_SHAPES = [(129, 171, 2048), (7, 300, 36), (256, 5, 2304)]


def _center_inputs(b, c, d):
    lab = torch.randint(0, c, (b,), generator=_gen(b + d)) // 2 * 2 % c        # even classes only: the odd ones have no sample
    return dict(x=_randn((b, d), b + c, 1.0), centers=_randn((c, d), b + c + 1, 1.0), label=lab, dloss=torch.tensor([0.9]))


def _center_ref(i, dt):
    x, c, dl = i["x"].to(dt), i["centers"].to(dt), i["dloss"].to(dt)
    lab = i["label"]
    b, nc = x.shape[0], c.shape[0]
    cy = c[lab]
    dist = (x * x).sum(1) + (cy * cy).sum(1) - 2.0 * (x * cy).sum(1)
    # every entry of the (B, C) matrix is clamped: the B (C - 1) masked-out zeros contribute 1e-12 each
    loss = dist.clamp(1e-12, 1e12).sum() / b + (nc - 1) * 1e-12
    gate = ((dist >= 1e-12) & (dist <= 1e12)).to(dt)[:, None]
    dx = gate * 2.0 * dl / b * (x - cy)
    return dict(dist=dist, loss=loss.reshape(1), dx=dx, dc=torch.zeros_like(c).index_add(0, lab, -dx))


@pytest.mark.parametrize("b,c,d", CENTER_SHAPES)
def test_center_loss(monkeypatch, oracle, b, c, d):
    from editor_amd import ops
    i = _center_inputs(b, c, d)
    ref = _center_ref(i, torch.float64)
    absent = torch.ones(c, dtype=torch.bool)
    absent[i["label"].unique()] = False
    assert absent.any()
    x, cen, lab = i["x"].cuda(), i["centers"].cuda(), i["label"].cuda()
    with _Poison(monkeypatch):
        loss, dist = ops.center_loss_fwd(x, cen, lab)
        dx, dc = ops.center_loss_bwd(x, cen, lab, dist, i["dloss"].cuda())
        zx = torch.zeros(b, d, device="cuda")
        zloss, zdist = ops.center_loss_fwd(zx, torch.zeros(c, d, device="cuda"), lab)
        torch.cuda.synchronize()
    n = "center B=%d C=%d D=%d " % (b, c, d)
    _check(n + "loss", loss, ref["loss"])
    _check(n + "dist", dist, ref["dist"])
    _check(n + "dx", dx, ref["dx"], row="center.dx")
    _check(n + "dc", dc, ref["dc"], row="center.dc")
    assert not dc[absent.cuda()].any()                                 # classes without a sample: zero gradient rows
    xr, cr = i["x"].clone().requires_grad_(True), i["centers"].clone().requires_grad_(True)
    lo = oracle.center_loss(xr, cr, i["label"])
    (0.9 * lo).backward()
    _check(n + "loss vs oracle", loss, lo.detach().double().view(1))
    _check(n + "dx vs oracle", dx, xr.grad.double())
    _check(n + "dc vs oracle", dc, cr.grad.double())
    # all distances 0: every one of the B C entries sits on the 1e-12 floor -> loss = 1e-12 + (C - 1) 1e-12
    assert not zdist.any()
    _check(n + "clamp constant", zloss, torch.tensor([c * 1e-12], dtype=torch.float64))


# =================================================================================================================================
# non-finite features / logits (an overflowed f16 step): the loss value must say so, the indices must stay usable
# =================================================================================================================================
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_rows(monkeypatch, bad):
    from editor_amd import ops
    b, r = 129, 5
    i = _triplet_inputs(b, 768, "ragged", seed=3)
    i["f"][r, 17] = bad
    ce = _ce_inputs(b, 171)
    ce["x"][r, 3] = bad
    cl = _center_inputs(b, 171, 768)
    cl["x"][r, 17] = bad
    cl["centers"][cl["label"][r], 17] = -1.0                          # x . c = -inf for +inf: d = +inf, clamped to 1e12 (finite)
    ref_t, ref_c, ref_l = _triplet_ref(i, torch.float64), _ce_ref(ce, torch.float64), _center_ref(cl, torch.float64)
    with _Poison(monkeypatch):
        loss = torch.empty(1, dtype=torch.float32, device="cuda")
        feat = i["f"].cuda()
        idx, coef = ops.triplet_fwd(feat, i["label"].cuda(), loss, accumulate=False)
        torch.cuda.synchronize()
        idx_h = idx.cpu()
        assert bool((idx_h >= -1).all()) and bool((idx_h < b).all()) and bool((idx_h[:b] >= 0).all()), "mined indices out of range"
        df = ops.triplet_bwd(feat, idx, coef, i["dloss"].cuda())
        lce = torch.empty(1, dtype=torch.float32, device="cuda")
        ops.ce_smooth_fwd(ce["x"].cuda(), ce["t"].cuda(), CE_EPS, lce, accumulate=False)
        dce = ops.ce_smooth_bwd(ce["x"].cuda(), ce["t"].cuda(), CE_EPS, ce["dloss"].cuda())
        lcl, dist = ops.center_loss_fwd(cl["x"].cuda(), cl["centers"].cuda(), cl["label"].cuda())
        dxc, dcc = ops.center_loss_bwd(cl["x"].cuda(), cl["centers"].cuda(), cl["label"].cuda(), dist, cl["dloss"].cuda())
        torch.cuda.synchronize()
    for name, got, ref in [("triplet", loss, ref_t["loss"]), ("ce", lce, ref_c["loss"]), ("center", lcl, ref_l["loss"])]:
        print(name, "loss", float(got), "float64 reference", float(ref))
        assert bool(torch.isfinite(got).all()) == bool(torch.isfinite(ref).all()), (name, float(got), float(ref))
    assert not bool(torch.isfinite(ref_t["loss"]).all()) and not bool(torch.isfinite(ref_c["loss"]).all())
    # the affected gradient rows are non-finite, so the optimizer's gradient check skips the step
    for name, g in [("triplet", df), ("ce", dce), ("center", dxc)]:
        assert not bool(torch.isfinite(g[r]).all()), name


# =================================================================================================================================
# SFTS apply and pooling
# =================================================================================================================================
SP_NMOD = [2, 3, 4]
SP_D = [256, 384, 768, 1024, 196]                                      # 384 -> 96 threads, 196 -> 49: partial last wave
SP_BT = [(1, 2), (3, 17), (6, 33), (5, 129), (2, 193)]                 # B T % 8 = 2, 3, 6, 5, 2; B T < 8


def _index(b, n, kind, seed):
    """kind 0: every sample random; 1: sample 0 all selected, sample 1 (if any) none; 2: sample 0 none, sample 1 all"""
    idx = (torch.rand(b, n, generator=_gen(seed)) > 0.5).to(torch.uint8)
    if kind:
        idx[0] = 1 if kind == 1 else 0
        if b > 1:
            idx[1] = 0 if kind == 1 else 1
    return idx


def _sp_cases():
    out = []
    for n, (nmod, d) in enumerate(itertools.product(SP_NMOD, SP_D)):
        for k, (b, t) in enumerate(SP_BT):
            out.append((nmod, d, b, t, (n + k) % 3))
    return out


def _sfts_inputs(nmod, d, b, t, kind):
    return dict(feat=_randn((nmod, b, t, d), nmod + d + b, 1.0), index=_index(b, t - 1, kind, d + t),
                dout=_randn((nmod, b, t, d), nmod + d + b + 1, 1.0), dloss=torch.tensor([1.7]))


def _sfts_ref(i, dt, want_loss=True):
    f, dout, dl = i["feat"].to(dt), i["dout"].to(dt), i["dloss"].to(dt)
    nmod, b, t, d = f.shape
    sel = torch.cat([torch.ones(b, 1, dtype=torch.bool), i["index"].bool()], 1)[None, :, :, None]
    bg = f * (~sel)
    loss = sum(((bg[a] - bg[c]) ** 2).sum() for a in range(nmod) for c in range(a + 1, nmod)) / (b * (t - 1) * d)
    gs = dl * 2.0 / (b * (t - 1) * d) if want_loss else 0.0 * dl
    dfeat = torch.where(sel, dout, gs * (nmod * f - f.sum(0, keepdim=True)))
    return dict(out=f * sel, loss=loss.reshape(1), dfeat=dfeat)


@pytest.mark.parametrize("nmod,d,b,t,kind", _sp_cases())
def test_sfts_apply(monkeypatch, nmod, d, b, t, kind):
    from editor_amd import ops
    i = _sfts_inputs(nmod, d, b, t, kind)
    feat, index, dout = i["feat"].cuda(), i["index"].cuda(), i["dout"].cuda()
    n = "sfts nmod=%d D=%d B=%d T=%d kind=%d " % (nmod, d, b, t, kind)
    for want_loss in (True, False):
        ref = _sfts_ref(i, torch.float64, want_loss)
        with _Poison(monkeypatch):
            out, loss = ops.sfts_apply(feat, index, want_loss)
            dfeat = ops.sfts_apply_bwd(feat, index, dout, i["dloss"].cuda() if want_loss else None)
            torch.cuda.synchronize()
        assert torch.equal(out.cpu().double(), ref["out"])             # copies or zeros: bit-exact
        if want_loss:
            _check(n + "loss", loss, ref["loss"])
        else:
            assert loss is None
        _check(n + "dfeat" + ("" if want_loss else " (no loss)"), dfeat.view(nmod * b * t, d), ref["dfeat"].view(nmod * b * t, d),
               row="sfts.dfeat")


def test_sfts_refusals_and_function(monkeypatch, oracle):
    from editor_amd import functional as fn, ops
    for nmod, d in [(3, 1028), (5, 256)]:
        f = torch.zeros(nmod, 2, 5, d, device="cuda")
        with pytest.raises(RuntimeError):
            ops.sfts_apply(f, torch.ones(2, 4, dtype=torch.uint8, device="cuda"), True)
    with pytest.raises(RuntimeError):
        f = torch.zeros(5, 2, 5, 256, device="cuda")
        ops.sfts_apply_bwd(f, torch.ones(2, 4, dtype=torch.uint8, device="cuda"), f, None)
    i = _sfts_inputs(4, 384, 5, 129, 1)
    ref = _sfts_ref(i, torch.float64)
    fr = i["feat"].clone().requires_grad_(True)
    outs, lo = oracle.sfts_apply(list(fr.unbind(0)), i["index"].bool(), True)
    (sum((o * dd).sum() for o, dd in zip(outs, i["dout"])) + 1.7 * lo).backward()
    dcls = _randn((4, 5, 384), 77)
    fg = i["feat"].cuda().requires_grad_(True)
    with _Poison(monkeypatch):
        o, l, cls = fn.SFTSApplyFn.apply(fg, i["index"].cuda(), True)
        ((o * i["dout"].cuda()).sum() + 1.7 * l + (cls * dcls.cuda()).sum()).backward()
        torch.cuda.synchronize()
    want = ref["dfeat"].clone()
    want[:, :, 0] += dcls.double()
    assert torch.equal(o.detach().cpu().double(), ref["out"]) and torch.equal(cls.detach().cpu(), i["feat"][:, :, 0])
    _check("sfts Function loss", l.view(1), ref["loss"])
    _check("sfts Function loss vs oracle", l.view(1), lo.detach().double().view(1))
    _check("sfts Function dfeat", fg.grad.view(-1, 384), want.view(-1, 384), row="sfts.dfeat")
    _check("sfts Function dfeat vs oracle (without the cls term)", (fg.grad.cpu() - torch.nn.functional.pad(
        dcls[:, :, None], (0, 0, 0, 128))).view(-1, 384), fr.grad.double().view(-1, 384))


def _pool_inputs(nmod, d, b, t, kind):
    """the fused tokens after HMA: unselected patch rows are zero in every modality; sample 0 additionally has modality 0 zeroed
    (num = 0 with non-zero sums elsewhere: +-inf) and one column of modality 1 too (0 / 0: NaN) when kind == 2"""
    index = _index(b, t - 1, kind, d + t + 1)
    keep = torch.cat([torch.ones(b, 1, dtype=torch.bool), index.bool()], 1)
    x = _randn((b, nmod, t, d), nmod * d + b * t) * keep[:, None, :, None]
    if kind == 2:
        x[0, 1:, 1:] = _randn((nmod - 1, t - 1, d), 5)
        x[0, 1, 1:, 3] = 0.0
    return dict(x=x.reshape(b, nmod * t, d).contiguous(), dout=_randn((nmod, b, 2 * d), nmod + d + b * t), nmod=nmod, t=t)


def _pool_ref(i, dt):
    nmod, t = i["nmod"], i["t"]
    x, dout = i["x"].to(dt), i["dout"].to(dt)
    b, _, d = x.shape
    xm = x.view(b, nmod, t, d)
    num = (xm[:, 0, 1:].sum(2) != 0).sum(1).to(dt)                      # rows of modality 0 with a non-zero sum
    out = torch.cat([xm[:, :, 0], xm[:, :, 1:].sum(2) / num[:, None, None]], 2).permute(1, 0, 2)
    dx = torch.empty_like(xm)
    dx[:, :, 0] = dout[:, :, :d].permute(1, 0, 2)
    dx[:, :, 1:] = (dout[:, :, d:].permute(1, 0, 2) / num[:, None, None])[:, :, None, :]
    return dict(num=num, out=out.contiguous(), dx=dx.reshape(b, nmod * t, d))


def _check_with_pattern(what, got, ref, row):
    """inf / NaN (a sample with num = 0) at the reference's places and with its signs; everything else to tolerance"""
    got = got.detach().cpu().double()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), what
    assert torch.equal(torch.isinf(got), torch.isinf(ref)) and torch.equal(got[torch.isinf(ref)], ref[torch.isinf(ref)]), what
    fin = torch.isfinite(ref)
    _check(what, torch.where(fin, got, torch.zeros_like(got)), torch.where(fin, ref, torch.zeros_like(ref)), row=row)


@pytest.mark.parametrize("nmod,d,b,t,kind", _sp_cases())
def test_pool(monkeypatch, nmod, d, b, t, kind):
    from editor_amd import ops
    i = _pool_inputs(nmod, d, b, t, kind)
    ref = _pool_ref(i, torch.float64)
    with _Poison(monkeypatch):
        out, num = ops.pool_fwd(i["x"].cuda(), nmod, t)
        dx = ops.pool_bwd(i["dout"].cuda(), num, nmod, t)
        torch.cuda.synchronize()
    n = "pool nmod=%d D=%d B=%d T=%d kind=%d " % (nmod, d, b, t, kind)
    assert torch.equal(num.cpu().double(), ref["num"]), n
    if kind == 2:
        assert float(ref["num"][0]) == 0 and bool(torch.isinf(ref["out"]).any()) and bool(torch.isnan(ref["out"]).any())
    _check_with_pattern(n + "out", out.view(nmod * b, 2 * d), ref["out"].reshape(nmod * b, 2 * d), "pool.out")
    _check_with_pattern(n + "dx", dx.view(b * nmod * t, d), ref["dx"].reshape(b * nmod * t, d), "pool.dx")


def test_pool_function(monkeypatch):
    from editor_amd import functional as fn
    i = _pool_inputs(3, 384, 6, 33, 1)
    ref = _pool_ref(i, torch.float64)
    x = i["x"].cuda().requires_grad_(True)
    with _Poison(monkeypatch):
        out, num = fn.PoolFn.apply(x, 3, 33)
        out.backward(i["dout"].cuda())
        torch.cuda.synchronize()
    assert torch.equal(num.cpu().double(), ref["num"])
    _check_with_pattern("pool Function out", out.view(18, 768), ref["out"].reshape(18, 768), "pool.out")
    _check_with_pattern("pool Function dx", x.grad.view(-1, 384), ref["dx"].reshape(-1, 384), "pool.dx")


# =================================================================================================================================
# packed pooling and the row maps
# =================================================================================================================================
PACKED_COUNTS = [0, 1, 7, 8, 9, 128]                                   # len = 1, 2, 8, 9, 10, 129 against the 8-row unroll
PACKED_CASES = [(1, 3, 256), (1, 4, 100), (1, 3, 1024), (1, 4, 768), (7, 3, 768), (7, 4, 1024), (7, 3, 100), (7, 4, 256),
                (128, 3, 768), (128, 4, 100), (128, 3, 1024), (128, 4, 256)]


def _forced_index(b, n, counts, seed):
    idx = (torch.rand(b, n, generator=_gen(seed)) > 0.5).to(torch.uint8)
    for s, cnt in enumerate(counts[:b]):
        idx[s] = 0
        idx[s, torch.randperm(n, generator=_gen(seed + s))[:cnt]] = 1
    return idx


@pytest.mark.parametrize("b,nmod,d", PACKED_CASES)
def test_pool_packed_equals_dense(monkeypatch, b, nmod, d):
    """Packed pooling of the gathered rows = dense pool_fwd of the masked dense tensor (itself checked against float64 above):
    both are float32 sums of the same rows in row order (the dense one adds the zero rows in between), so the dense family's
    bounds apply.  The backward, scattered back through the two row maps, equals the dense backward on the kept rows."""
    from editor_amd import ops
    t = 129
    plans = [[c] for c in PACKED_COUNTS] if b == 1 else [PACKED_COUNTS]
    for counts in plans:
        index = _forced_index(b, t - 1, counts, 31 * b + d)
        keep = torch.cat([torch.ones(b, 1, dtype=torch.bool), index.bool()], 1).cuda()
        feat = torch.randn(nmod, b, t, d, generator=torch.Generator(device="cuda").manual_seed(d + b), device="cuda")
        feat = feat * keep[None, :, :, None]
        dout = torch.randn(nmod, b, 2 * d, generator=torch.Generator(device="cuda").manual_seed(d + b + 1), device="cuda")
        n = "packed B=%d nmod=%d D=%d counts=%s " % (b, nmod, d, counts[:b])
        with _Poison(monkeypatch):
            plan = ops.CompactPlan(index.cuda(), t, nmod)
            lens = 1 + index.sum(1)
            assert plan.cu.cpu().tolist() == [0] + lens.cumsum(0).tolist()
            xb = ops.gather_rows(ops.gather_rows(feat.view(-1, d), plan.map_a), plan.map_b)      # layout A, then layout B
            out, num = ops.pool_packed_fwd(xb, plan.cu, b, nmod)
            dense = feat.permute(1, 0, 2, 3).reshape(b, nmod * t, d).contiguous()
            out_d, num_d = ops.pool_fwd(dense, nmod, t)
            dxb = ops.pool_packed_bwd(dout, num, plan.cu, b, nmod, plan.mb)                     # zero-filled form
            dxb_live = ops.pool_packed_bwd(dout, num, plan.cu, b, nmod, plan.mb, live=plan.live_b)
            dx_d = ops.pool_bwd(dout, num_d, nmod, t).view(b, nmod, t, d).permute(1, 0, 2, 3)
            back = ops.scatter_rows(ops.scatter_rows(dxb, plan.map_b, nmod * plan.ma), plan.map_a, nmod * b * t).view(nmod, b, t, d)
            torch.cuda.synchronize()
        assert torch.equal(num, num_d) and torch.equal(num.cpu().long(), index.sum(1)), n
        _check_with_pattern(n + "out", out.view(nmod * b, 2 * d), out_d.cpu().double().view(nmod * b, 2 * d), "pool.out")
        km = keep[None, :, :, None].expand(nmod, b, t, d)
        zero = torch.zeros((), device="cuda")
        _check_with_pattern(n + "dx on kept rows", torch.where(km, back, zero).reshape(-1, d),
                            torch.where(km, dx_d, zero).cpu().double().reshape(-1, d), "pool.dx")
        assert not back[~km].any()                                     # rows no index names: the zero fill
        # the form without the fill writes the live rows [0, nmod * total) only and zeroes the pad rows up to the next multiple of
        # 64; everything behind is documented as unwritten and not compared
        live = nmod * plan.total
        a, c = dxb_live[:live], dxb[:live]
        assert torch.equal(torch.isnan(a), torch.isnan(c)) and torch.equal(a[~torch.isnan(a)], c[~torch.isnan(c)]), n
        assert not dxb_live[live:min(plan.mb, (live + 63) // 64 * 64)].any() and not dxb[live:].any(), n


# =================================================================================================================================
# patch-embed assembly
# =================================================================================================================================
EMBED_BN = [(1, 1), (5, 1), (3, 3), (23, 3), (128, 3)]                 # Btot = 1, 5, 9, 69, 384
EMBED_D = [256, 768, 1024, 1280, 100]
EMBED_DT = [torch.float32, torch.bfloat16, torch.float16]
EMBED_COEF = 3.0


def _embed_cases():
    out = []
    for n, ((bcam, nmod), d) in enumerate(itertools.product(EMBED_BN, EMBED_D)):
        t = 9 if (n % 2 or (bcam * nmod > 100 and d >= 1024)) else 129
        out.append((bcam, nmod, t, d, n % 3, n % 6 != 5, n % 4 == 1))
    return out


def _embed_inputs(bcam, nmod, t, d, dti, sie, one_cam):
    btot, ncam, dt = bcam * nmod, 6, EMBED_DT[dti]
    cam = torch.randint(0, ncam - 1, (bcam,), generator=_gen(bcam + d))        # camera ncam - 1 is never used
    if one_cam:
        cam[:] = 2
    return dict(patch=_randn((btot * (t - 1), d), d + btot, 1.0).to(dt), cls=_randn((d,), 1, 0.5), pos=_randn((t, d), 2, 0.5),
                sie=_randn((ncam, d), 3, 0.5) if sie else None, cam=cam if sie else None, ncam=ncam if sie else 0,
                dx=_randn((btot, t, d), d + btot + 1, 1.0), btot=btot, bcam=bcam, dt=dt)


def _embed_ref(i, dt):
    btot, bcam = i["btot"], i["bcam"]
    patch, cls, pos, dx = i["patch"].to(dt), i["cls"].to(dt), i["pos"].to(dt), i["dx"].to(dt)
    t, d = pos.shape
    x = torch.cat([cls.expand(btot, 1, d), patch.view(btot, t - 1, d)], 1) + pos
    o = dict(dpos=dx.sum(0), dpatch=dx[:, 1:].reshape(btot * (t - 1), d))
    if i["sie"] is not None:
        camb = i["cam"][torch.arange(btot) % bcam]                     # the modality copies share the camera labels
        x = x + EMBED_COEF * i["sie"].to(dt)[camb][:, None, :]
        o["dsie"] = EMBED_COEF * torch.zeros(i["ncam"], d, dtype=dt).index_add(0, camb, dx.sum(1))
    o["x"] = x
    return o


def _ulps(a, b):
    """distance in units in the last place between two tensors of one dtype (sign-magnitude integers made monotonic)"""
    it = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}[a.dtype]
    top = {torch.int32: 0x7fffffff, torch.int16: 0x7fff}[it]

    def key(v):
        k = v.contiguous().view(it).long()
        return torch.where(k < 0, -(k & top), k)
    return (key(a) - key(b)).abs().max().item()


@pytest.mark.parametrize("bcam,nmod,t,d,dti,sie,one_cam", _embed_cases())
def test_embed_assemble(monkeypatch, bcam, nmod, t, d, dti, sie, one_cam):
    """Btot = 1, 5: fewer partial rows than EDITOR_EMBED_POS_SPLITS; 9, 69, 384: one, two and six trips of the 8 S sample stride;
    D = 1280: two 1024-column blocks; D = 100: partial 64-column block of the camera sum"""
    from editor_amd import ops
    i = _embed_inputs(bcam, nmod, t, d, dti, sie, one_cam)
    ref = _embed_ref(i, torch.float64)
    cam = i["cam"].cuda() if sie else None
    with _Poison(monkeypatch):
        x = ops.embed_assemble(i["patch"].cuda(), i["cls"].cuda(), i["pos"].cuda(), i["sie"].cuda() if sie else None, cam,
                               EMBED_COEF, i["btot"], t, d)
        dpatch, dpos, dsie = ops.embed_assemble_bwd(i["dx"].cuda(), cam, i["ncam"], EMBED_COEF, i["dt"], 1.0)
        torch.cuda.synchronize()
    n = "embed Btot=%d(%dx%d) T=%d D=%d %s sie=%d " % (i["btot"], bcam, nmod, t, d, str(i["dt"])[6:], sie)
    _check(n + "x", x.view(-1, d), ref["x"].view(-1, d), row="embed.x")
    assert dpatch.dtype == i["dt"]
    u = _ulps(dpatch.cpu(), ref["dpatch"].to(i["dt"]))                 # the float64 value rounded to the activation dtype
    print(n + "dpatch: %d ulp" % u)
    assert u <= 1, (n, u)
    _check(n + "dpos", dpos, ref["dpos"], row="embed.dpos")
    if sie:
        _check(n + "dsie", dsie, ref["dsie"], row="embed.dsie")
        unused = torch.ones(i["ncam"], dtype=torch.bool)
        unused[i["cam"].unique()] = False
        assert unused[-1] and not dsie.cpu()[unused].any()            # a camera without a sample: exactly 0
    else:
        assert dsie is None


# =================================================================================================================================
# mask_or
# =================================================================================================================================
@pytest.mark.parametrize("n", [1, 255, 256, 257, 128 * 128 * 3])
@pytest.mark.parametrize("nops", [2, 3, 4])
def test_mask_or(n, nops):
    from editor_amd import ops
    ms = [(torch.rand(n, generator=_gen(n + k)) > 0.7).to(torch.uint8) * (1 + k) for k in range(nops)]     # any non-zero counts
    out = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    real_like = torch.empty_like
    torch.empty_like = lambda *a, **k: out
    try:
        got = ops.mask_or(*[m.cuda() for m in ms])
    finally:
        torch.empty_like = real_like
    want = torch.stack(ms).bool().any(0).to(torch.uint8)
    assert got is out and torch.equal(got.cpu(), want)


# =================================================================================================================================
# the float32-CPU-vs-float64 deviations behind ROW_DEV
# =================================================================================================================================
def cpu_deviations():
    acc = {}
    for b, c in itertools.product(BN_B, BN_C):
        i = _bn_inputs(b, c)
        r32, r64 = _bn_ref(i, torch.float32), _bn_ref(i, torch.float64)
        _dev(acc, "bn.y", r32["y"], r64["y"], cols=True)
        for k in ("save_mean", "save_invstd", "rmean", "rvar", "dgamma", "dbeta"):
            if b > 1 or k not in ("dgamma",):
                _dev(acc, "bn." + k + " (l2 only)", r32[k], r64[k])
        if b > 1:
            _dev(acc, "bn.dx.B%d" % b if b < 4 else "bn.dx", r32["dx"], r64["dx"], cols=True)
    for (b, c, d), m in itertools.product(OCFR_SHAPES, range(4)):
        i = _ocfr_inputs(b, c, d, 100 * m + b)
        r32, r64 = _ocfr_ref(i, torch.float32), _ocfr_ref(i, torch.float64)
        for k in ("fnorm", "centers", "dfeat", "loss", "inv_norm"):
            _dev(acc, "ocfr." + k, r32[k], r64[k])
    for b, c in CE_SHAPES:
        i = _ce_inputs(b, c)
        r32, r64 = _ce_ref(i, torch.float32), _ce_ref(i, torch.float64)
        _dev(acc, "ce.dlogits", r32["dlogits"], r64["dlogits"])
        _dev(acc, "ce.loss", r32["loss"], r64["loss"])
    for b, d, g in TRIPLET_CASES + [(129, 768, "ragged2")]:
        i = _triplet_inputs(b, d, "ragged", seed=3) if g == "ragged2" else _triplet_inputs(b, d, g)
        r32, r64 = _triplet_ref(i, torch.float32), _triplet_ref(i, torch.float64)
        dev = _triplet_precondition(i, r64)
        acc["triplet.distance deviation"] = (max(acc.get("triplet.distance deviation", (0, 0))[0], dev), 0.0)
        assert torch.equal(r32["idx"], r64["idx"])
        single = torch.bincount(i["label"])[i["label"]] == 1
        for k, m in (("triplet.dfeat", ~single), ("triplet.dfeat.single", single)):
            if m.any():
                _dev(acc, k, r32["dfeat"][m], r64["dfeat"][m])
        _dev(acc, "triplet.dfeat (whole)", r32["dfeat"], r64["dfeat"])
        _dev(acc, "triplet.loss", r32["loss"], r64["loss"])
    for b, c, d in CENTER_SHAPES + [(129, 171, 768)]:
        i = _center_inputs(b, c, d)
        r32, r64 = _center_ref(i, torch.float32), _center_ref(i, torch.float64)
        for k in ("dx", "dc", "loss", "dist"):
            _dev(acc, "center." + k, r32[k], r64[k])
    for nmod, d, b, t, kind in _sp_cases():
        i = _sfts_inputs(nmod, d, b, t, kind)
        r32, r64 = _sfts_ref(i, torch.float32), _sfts_ref(i, torch.float64)
        _dev(acc, "sfts.dfeat", r32["dfeat"].view(-1, d), r64["dfeat"].view(-1, d))
        _dev(acc, "sfts.loss", r32["loss"], r64["loss"])
        i = _pool_inputs(nmod, d, b, t, kind)
        r32, r64 = _pool_ref(i, torch.float32), _pool_ref(i, torch.float64)
        for k, w in (("out", 2 * d), ("dx", d)):
            fin = torch.isfinite(r64[k])
            z32, z64 = torch.zeros_like(r32[k]), torch.zeros_like(r64[k])
            _dev(acc, "pool." + k, torch.where(fin, r32[k], z32).reshape(-1, w), torch.where(fin, r64[k], z64).reshape(-1, w))
    for case in _embed_cases():
        i = _embed_inputs(*case)
        r32, r64 = _embed_ref(i, torch.float32), _embed_ref(i, torch.float64)
        d = case[3]
        _dev(acc, "embed.x", r32["x"].view(-1, d), r64["x"].view(-1, d))
        _dev(acc, "embed.dpos", r32["dpos"], r64["dpos"])
        if i["sie"] is not None:
            _dev(acc, "embed.dsie", r32["dsie"], r64["dsie"])
    return acc


if __name__ == "__main__":
    for name, (l2, row) in sorted(cpu_deviations().items()):
        print("%-32s l2 %.2e   worst row %.2e" % (name, l2, row))
    sys.exit(0)
