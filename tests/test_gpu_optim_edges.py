"""The training-step kernels of csrc/train.hip per element at chunk, tail and alignment edges (optim_edge_helpers.py).

Every array lives in a sentinel-guarded arena at a chosen offset from a 16-byte boundary; after every launch the sentinels, the
gradient arena and every array of the tensor without a gradient must hold their bits.  SGD runs on operands for which fp32 is exact
and is compared bit for bit with the float64 closed form; AdamW is held, one step from the device's own state, to the bound derived
in the helper; the overflow check is probed one non-finite element at a time at the positions its index map makes special; scaler,
split pairs and transposes are compared bit for bit with their one-rounding definitions.  Most launches go to the C ABI directly:
the Python classes only ever hand the kernels fresh, aligned allocations."""
import functools

import numpy as np
import pytest
import torch

import optim_edge_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F16 = H.F32, H.BF16, H.F16
C = H.chunk_elems()
TABLE = H.size_table(C)
NOGRAD = H.index_of(TABLE, "nograd")
POISONS = H.poison_positions(TABLE, C)
POISON_VALUES = H.POISON_VALUES
_dt = lambda d: "noshadow" if d is None else str(d).split(".")[-1]
_sc = lambda s: "unscaled" if s is None else "inv_scale"


def call(name, *args):
    from editor_amd import _lib
    _lib.call(name, *args)


def flag(v=0):
    return torch.full((1,), v, dtype=torch.int32, device=DEV)


def scalar(x):
    return None if x is None else torch.full((1,), float(x), dtype=F32, device=DEV)


def sgd_launch(st, mu, inv=None, nonfinite=None, skip=None):
    call("editor_sgd_multi", st.p_ptrs, st.g_ptrs, st.m_ptrs, st.chunk_t, st.chunk_o, st.numel, st.lr, st.wd, float(mu), st.nchunks,
         st.h_ptrs, st.shadow_code, nonfinite, inv, skip)


def adamw_launch(st, step, inv=None, nonfinite=None, skip=None):
    call("editor_adamw_multi", st.p_ptrs, st.g_ptrs, st.m_ptrs, st.v_ptrs, st.chunk_t, st.chunk_o, st.numel, st.lr, st.wd,
         H.BETAS[0], H.BETAS[1], H.EPS, step, st.nchunks, st.h_ptrs, st.shadow_code, nonfinite, inv, skip)


def check_launch(st, found, sticky):
    call("editor_grad_check_multi", st.g_ptrs, st.chunk_t, st.chunk_o, st.numel, st.nchunks, found, sticky)


def freeze(st):
    """Bits of everything a launch must not touch: the gradient arena and all arrays of the tensor without a gradient."""
    return st.g.snapshot(), {k: a.raw_view(NOGRAD).clone() for k, a in st.arenas.items() if k != "g"}


def assert_untouched(st, frozen):
    torch.cuda.synchronize()
    g_snap, nograd = frozen
    st.assert_guards()
    assert st.g.unchanged(g_snap), "the kernel wrote the gradient arena"
    for k, bits in nograd.items():
        assert torch.equal(st.arenas[k].raw_view(NOGRAD), bits), "%s of the tensor without a gradient changed" % k


def assert_same(got, want, what):
    """Element for element; names the first element that differs."""
    if not torch.equal(got, want):
        i = int(torch.nonzero(got != want).flatten()[0])
        raise AssertionError("%s: element %d of %d is %r, expected %r (%d differ)"
                             % (what, i, got.numel(), got[i].item(), want[i].item(), int((got != want).sum())))


def assert_shadow(h, p, dtype, what):
    assert_same(h.view(torch.int16), p.to(dtype).view(torch.int16), what + " shadow")


@functools.lru_cache(None)
def _sgd_ops():
    return H.sgd_operands(TABLE)


@functools.lru_cache(None)
def _sgd_ref(mu, s):
    p0, grads = _sgd_ops()
    return H.sgd_reference(TABLE, p0, grads, mu, s)


def _nograd_state(st, seed=5):
    """The tensor without a gradient holds non-trivial momentum (and exp_avg_sq): 'unchanged' must mean something."""
    gen = torch.Generator().manual_seed(seed)
    n = H.numel(TABLE[NOGRAD])
    for k in ("m", "v"):
        if k in st.arenas:
            st.arenas[k].set(NOGRAD, (torch.randint(1, 64, (n,), generator=gen).float() / 8).to(DEV))


# ---------------------------------------------------------------------------------------------------------------------------
# SGD
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shadow", [None, BF16, F16], ids=_dt)
@pytest.mark.parametrize("inv_scale", list(H.INV_SCALES), ids=_sc)
@pytest.mark.parametrize("align", list(H.ALIGN))
def test_sgd_three_steps_bit_for_bit(align, inv_scale, shadow):
    mu = H.MOMENTA[0] if inv_scale is None else H.MOMENTA[1]
    p0, grads = _sgd_ops()
    ref = _sgd_ref(mu, inv_scale)
    st = H.State(TABLE, align, DEV, C, shadow_dtype=shadow)
    st.load("p", p0)
    st.load("m", [torch.zeros_like(x) for x in p0])
    _nograd_state(st)
    inv = scalar(inv_scale)
    for k in range(H.SGD_STEPS):
        st.load("g", [g if e.grad else None for g, e in zip(grads[k], TABLE)])
        frozen = freeze(st)
        sgd_launch(st, mu, inv)
        assert_untouched(st, frozen)
        P, M = st.p.host(), st.m.host()
        Hh = st.h.host() if shadow is not None else None
        for i, e in enumerate(TABLE):
            if not e.grad:
                continue
            what = "%s %s step %d" % (align, e.name, k + 1)
            assert_same(P[i].double(), ref[k][0][i], what + " p")
            assert_same(M[i].double(), ref[k][1][i], what + " m")
            if shadow is not None and e.shadow:
                assert_shadow(Hh[i], P[i], shadow, what)


@pytest.mark.parametrize("shadow", [BF16, F16], ids=_dt)
@pytest.mark.parametrize("align", list(H.ALIGN))
def test_sgd_shadows_round_ties_as_torch(align, shadow):
    """Every tensor gets a shadow; parameters where 16-bit rounding matters, a quarter of them exact ties that the update (weight
    decay 0, zero momentum, zero gradient there) leaves in place: only shadow == cast(p) is asserted, bit for bit."""
    st = H.State(TABLE, align, DEV, C, shadow_dtype=shadow, shadow_all=True)
    st.wd.zero_()
    ps, gs = H.tie_operands(TABLE, shadow)
    st.load("p", ps)
    st.load("g", [g if e.grad else None for g, e in zip(gs, TABLE)])
    st.load("m", [torch.zeros_like(x) for x in ps])
    _nograd_state(st)
    frozen = freeze(st)
    sgd_launch(st, 0.5, scalar(2.0 ** -3))
    assert_untouched(st, frozen)
    P, Hh = st.p.host(), st.h.host()
    for i, e in enumerate(TABLE):
        if e.grad:
            k = -(-H.numel(e) // 4)
            assert H.is_tie(P[i][:k], shadow).all(), "%s: the ties moved" % e.name
            assert_shadow(Hh[i], P[i], shadow, "%s %s" % (align, e.name))


@pytest.mark.parametrize("kernel", ["sgd", "adamw"])
@pytest.mark.parametrize("align", list(H.ALIGN))
def test_skip_flag_freezes_everything(align, kernel):
    """skip pointing at a non-zero flag: parameters, momentum, exp_avg_sq, shadows and AdamW's step count keep their bits; the
    same launch with the flag cleared applies."""
    adam = kernel == "adamw"
    st = H.State(TABLE, align, DEV, C, shadow_dtype=F16, adam=adam)
    p, g, m, v = H.adam_operands(TABLE, seed=1, state=True)
    st.load("p", p); st.load("g", [x if e.grad else None for x, e in zip(g, TABLE)]); st.load("m", m)
    if adam:
        st.load("v", v)
    snaps = {k: a.snapshot() for k, a in st.arenas.items()}
    step, nonfinite = scalar(5.0), flag(0)
    for skip_value in (1, -7):
        skip = flag(skip_value)
        adamw_launch(st, step, scalar(0.5), nonfinite, skip) if adam else sgd_launch(st, 0.5, scalar(0.5), nonfinite, skip)
        torch.cuda.synchronize()
        for k, a in st.arenas.items():
            assert a.unchanged(snaps[k]), "%s changed in a skipped step" % k
        assert step.item() == 5.0 and skip.item() == skip_value
    frozen = freeze(st)
    adamw_launch(st, step, scalar(0.5), nonfinite, flag(0)) if adam else sgd_launch(st, 0.5, scalar(0.5), nonfinite, flag(0))
    assert_untouched(st, frozen)
    P, Hh = st.p.host(), st.h.host()
    for i, e in enumerate(TABLE):
        if e.grad:
            assert (P[i] != p[i]).float().mean() > 0.9, e.name
            if e.shadow:
                assert_shadow(Hh[i], P[i], F16, e.name)
    assert nonfinite.item() == 0 and (not adam or step.item() == 6.0)


# ---------------------------------------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shadow", [BF16, F16], ids=_dt)
@pytest.mark.parametrize("inv_scale", [None, H.ADAM_INV_SCALE], ids=_sc)
@pytest.mark.parametrize("t", list(H.ADAM_T))
@pytest.mark.parametrize("align", list(H.ALIGN))
def test_adamw_one_step_from_device_state(align, t, inv_scale, shadow):
    """t = 1: zero state; t = 2: the step after it; t = 1001: the step scalar set to 1000 over non-zero m, v.  Each step is
    compared with the float64 step from the state the device itself held before it."""
    st = H.State(TABLE, align, DEV, C, shadow_dtype=shadow, adam=True)
    lr, wd = H.adam_hyper(TABLE)
    st.lr.copy_(lr); st.wd.copy_(wd)
    p, g, m, v = H.adam_operands(TABLE, seed=t, state=True)
    if t < 1000:
        m, v = [torch.zeros_like(x) for x in m], [torch.zeros_like(x) for x in v]
    if inv_scale is not None:
        g = [(x.double() / inv_scale).float() for x in g]                      # (a power of two: exact)
    st.load("p", p); st.load("m", m); st.load("v", v)
    st.load("g", [x if e.grad else None for x, e in zip(g, TABLE)])
    _nograd_state(st)
    step = scalar(float(t - 1 if t > 1000 else 0))
    inv = scalar(inv_scale)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for now in ((1, 2) if t == 2 else (t,)):
        P0, M0, V0 = st.p.host(), st.m.host(), st.v.host()
        frozen = freeze(st)
        adamw_launch(st, step, inv)
        assert_untouched(st, frozen)
        assert step.item() == float(now)
        P1, M1, V1, Hh = st.p.host(), st.m.host(), st.v.host(), st.h.host()
        for i, e in enumerate(TABLE):
            if not e.grad:
                continue
            r = H.adam_ref_step(P0[i], g[i], M0[i], V0[i], float(lr[i]), float(wd[i]), now, inv_scale)
            got = {"p": H.worst_ratio(P1[i], r.p, r.tol_p), "m": H.worst_ratio(M1[i], r.m, r.tol_m), "v": H.worst_ratio(V1[i], r.v, r.tol_v)}
            for k in got:
                worst[k] = max(worst[k], got[k])
            assert max(got.values()) <= 1.0, "%s %s t=%d: error / bound %r" % (align, e.name, now, got)
            if e.shadow:
                assert_shadow(Hh[i], P1[i], shadow, "%s %s t=%d" % (align, e.name, now))
    print("adamw %s t=%d: worst error / bound p %.3f m %.3f v %.3f" % (align, t, worst["p"], worst["m"], worst["v"]))


# ---------------------------------------------------------------------------------------------------------------------------
# overflow detection by position
# ---------------------------------------------------------------------------------------------------------------------------
def _finite_state(st, adam):
    p0, grads = _sgd_ops()
    st.load("p", p0)
    st.load("g", [g if e.grad else None for g, e in zip(grads[0], TABLE)])
    st.load("m", [torch.zeros_like(x) for x in p0])
    if adam:
        st.load("v", [torch.ones_like(x) for x in p0])


@pytest.mark.parametrize("kernel", ["check", "sgd", "adamw"])
@pytest.mark.parametrize("align", list(H.POISON_ALIGN))
def test_poisoned_gradient_is_found_at_every_position(align, kernel):
    """One non-finite value per launch, everything else finite: editor_grad_check_multi sets found and sticky; the update kernels
    (nonfinite given, no skip) raise their flag.  A clean launch before and after raises nothing."""
    st = H.State(TABLE, align, DEV, C, adam=kernel == "adamw")
    _finite_state(st, kernel == "adamw")
    frozen = freeze(st)
    cases = [(pos, name, bits) for pos in POISONS for name, bits in POISON_VALUES.items()]
    flags = torch.zeros(len(cases) + 2, 2, dtype=torch.int32, device=DEV)
    step = scalar(0.0)

    def launch(k):
        if kernel == "check":
            check_launch(st, flags[k, 0:1], flags[k, 1:2])
        elif kernel == "sgd":
            sgd_launch(st, 0.5, None, flags[k, 0:1], None)
        else:
            adamw_launch(st, step, None, flags[k, 0:1], None)

    launch(len(cases))
    for k, (pos, name, bits) in enumerate(cases):
        idx = st.g.offs[pos.tensor] + pos.element
        keep = st.g.raw[idx].clone()
        st.g.raw[idx] = bits
        launch(k)
        st.g.raw[idx] = keep
    launch(len(cases) + 1)
    assert_untouched(st, frozen)
    f = flags.cpu()
    assert f[len(cases):].eq(0).all(), "a finite gradient raised the flag"
    missed = [(pos.label, name) for k, (pos, name, _) in enumerate(cases) if f[k, 0] != 1 or (kernel == "check" and f[k, 1] != 1)]
    assert not missed, "%s, %s gradient: missed %r" % (kernel, align, missed)


@pytest.mark.parametrize("align", list(H.POISON_ALIGN))
def test_finite_extremes_raise_nothing(align):
    """+-FLT_MAX, denormals and -0.0 everywhere: neither the check nor the update kernels' own detection fires.  (The tensor
    without a gradient has a NULL entry in g_ptrs in every launch of this file: it is never read.)"""
    st = H.State(TABLE, align, DEV, C, adam=True)
    _finite_state(st, True)
    sets = H.clean_gradient_sets(TABLE)
    flags = torch.zeros(len(sets), 4, dtype=torch.int32, device=DEV)
    step = scalar(0.0)
    for k, (name, gs) in enumerate(sets.items()):
        st.load("g", [g if e.grad else None for g, e in zip(gs, TABLE)])
        frozen = freeze(st)
        check_launch(st, flags[k, 0:1], flags[k, 1:2])
        sgd_launch(st, 0.5, None, flags[k, 2:3], None)
        adamw_launch(st, step, None, flags[k, 3:4], None)
        assert_untouched(st, frozen)
    assert flags.cpu().eq(0).all(), dict(zip(sets, flags.cpu().tolist()))


# ---------------------------------------------------------------------------------------------------------------------------
# loss scaler
# ---------------------------------------------------------------------------------------------------------------------------
def _scaler_arena(scale):
    a = H.Arena([1, 1, 1, 1], 0, F32, DEV, fill=0)                 # scale, inv_scale (fp32); tracker, found (int32 bit patterns)
    a.view(0).fill_(scale)
    a.view(1).fill_(1.0 / scale)
    return a


def _bits(x):
    return int(np.float32(x).view(np.int32))


@pytest.mark.parametrize("case", list(H.SCALER_CASES))
def test_scaler_update_follows_the_restatement(case):
    founds, growth, backoff, interval, scale = H.SCALER_CASES[case]
    a = _scaler_arena(scale)
    s, tr = np.float32(scale), 0
    for n, f in enumerate(founds):
        a.raw_view(3).fill_(f)
        call("editor_scaler_update", a.view(0), a.view(1), a.raw_view(2), a.raw_view(3), growth, backoff, interval)
        s, inv, tr, cleared = H.scaler_ref(s, tr, f, growth, backoff, interval)
        got =[int(x.view(torch.int32)[0]) for x in a.host()]
        assert got == [_bits(s), _bits(inv), tr, cleared], "%s call %d (found %d): %r" % (case, n, f, got)
        assert not a.broken_sentinels()


def test_scaler_update_refuses_invalid_arguments():
    a = _scaler_arena(1024.0)
    a.raw_view(3).fill_(1)
    snap = a.snapshot()
    ok = [a.view(0), a.view(1), a.raw_view(2), a.raw_view(3)]
    for bad in range(4):
        args = [None if i == bad else x for i, x in enumerate(ok)]
        with pytest.raises(RuntimeError, match="editor_scaler_update failed"):
            call("editor_scaler_update", *args, 2.0, 0.5, 3)
    for interval in (0, -1):
        with pytest.raises(RuntimeError, match="editor_scaler_update failed"):
            call("editor_scaler_update", *ok, 2.0, 0.5, interval)
    torch.cuda.synchronize()
    assert a.unchanged(snap)


def test_device_grad_scaler_checkpoint_round_trip():
    from editor_amd.optim import DeviceGradScaler
    a = DeviceGradScaler(DEV, init_scale=2.0 ** 10, growth_interval=3)
    s, tr = np.float32(2.0 ** 10), 0
    state = lambda sc: (_bits(sc._scale.item()), _bits(sc._inv_scale.item()), int(sc._tracker.item()), int(sc._found.item()))
    for f in (0, 0, 1, 0):
        a._found.fill_(f)
        a.update()
        s, inv, tr, _ = H.scaler_ref(s, tr, f, 2.0, 0.5, 3)
        assert state(a) == (_bits(s), _bits(inv), tr, 0)
    assert tr == 1
    b = DeviceGradScaler(DEV, init_scale=7.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=11)
    b.load_state_dict(a.state_dict())
    assert state(b) == state(a) and (b.growth_factor, b.backoff_factor, b.growth_interval) == (2.0, 0.5, 3)
    for f in (0, 0, 0, 1, 0, 0, 0):
        for sc in (a, b):
            sc._found.fill_(f)
            sc.update()
        s, inv, tr, _ = H.scaler_ref(s, tr, f, 2.0, 0.5, 3)
        assert state(a) == state(b) == (_bits(s), _bits(inv), tr, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# split pairs and transposes
# ---------------------------------------------------------------------------------------------------------------------------
def test_split_pairs_bit_for_bit():
    """hi = half(p * 256), lo = half(p * 256 - hi): two single roundings, equal to torch's on the CPU; the tensor whose hi_ptrs
    entry is NULL keeps its (never written) pair."""
    st = H.State(TABLE, "aligned", DEV, C, pairs=True)
    ps = H.split_operands(TABLE)
    st.load("p", ps)
    p_snap = st.p.snapshot()
    call("editor_split_multi", st.p_ptrs, st.hi_ptrs, st.lo_ptrs, st.chunk_t, st.chunk_o, st.numel, st.nchunks, H.SPLIT_SCALE)
    torch.cuda.synchronize()
    st.assert_guards()
    assert st.p.unchanged(p_snap)
    HI, LO = st.hi.host(), st.lo.host()
    for i, e in enumerate(TABLE):
        if e.name == "nograd":
            assert (HI[i].view(torch.int16) == H.UNWRITTEN16).all() and (LO[i].view(torch.int16) == H.UNWRITTEN16).all()
            continue
        hi, lo = H.split_ref(ps[i])
        assert_same(HI[i].view(torch.int16), hi.view(torch.int16), e.name + " hi")
        assert_same(LO[i].view(torch.int16), lo.view(torch.int16), e.name + " lo")


def test_transpose_multi_bit_for_bit():
    """One launch over four shapes, tile table shuffled, all 65536 bit patterns: every dst equals src.t(), sentinels intact."""
    xs = H.transpose_operands()
    sizes = [x.numel() for x in xs]
    src, dst = H.Arena(sizes, 0, F16, DEV), H.Arena(sizes, 0, F16, DEV, fill=H.UNWRITTEN16)
    for i, x in enumerate(xs):
        src.raw_view(i).copy_(x.reshape(-1))
    snap = src.snapshot()
    tiles = H.tile_table(H.TRANSPOSE_SHAPES)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)
    call("editor_transpose_multi", i64(src.ptrs()), i64(dst.ptrs()), i32([r for r, _ in H.TRANSPOSE_SHAPES]),
         i32([c for _, c in H.TRANSPOSE_SHAPES]), i32([t for t, _, _ in tiles]), i32([a for _, a, _ in tiles]),
         i32([b for _, _, b in tiles]), len(tiles))
    torch.cuda.synchronize()
    assert not dst.broken_sentinels() and not src.broken_sentinels() and src.unchanged(snap)
    out = dst.host()
    for x, y, (r, c) in zip(xs, out, H.TRANSPOSE_SHAPES):
        assert_same(y.view(torch.int16), x.t().contiguous().reshape(-1), "transpose of (%d, %d)" % (r, c))


# ---------------------------------------------------------------------------------------------------------------------------
# through the Python classes
# ---------------------------------------------------------------------------------------------------------------------------
EXTRA = (("big.weight", (512, 512)), ("ragged.weight", (520, 512)), ("small.weight", (256, 256)))


def _class_params(seed):
    """The table's tensors plus three 2-D weights, parameters on exact-recipe values; gradients are consecutive views into one
    flat buffer (GradBuckets' layout: a view behind a tensor of odd size is 4-byte aligned only)."""
    gen = torch.Generator().manual_seed(seed)
    names, shapes, grad = [], [], []
    for i, e in enumerate(TABLE):
        names.append("t%d.%s" % (i, "weight" if len(e.shape) >= 2 else ("bias" if i % 2 else "scale")))
        shapes.append(e.shape)
        grad.append(e.grad)
    for n, s in EXTRA:
        names.append(n); shapes.append(s); grad.append(True)
    ps = [torch.nn.Parameter((torch.randint(-32, 33, s, generator=gen).float() / 8).to(DEV)) for s in shapes]
    total = sum(p.numel() for p, g in zip(ps, grad) if g)
    flat = torch.zeros(total, dtype=F32, device=DEV)
    views, off = [], 0
    for p, g in zip(ps, grad):
        views.append(flat[off:off + p.numel()].view_as(p) if g else None)
        off += p.numel() if g else 0
    assert any(v is not None and v.data_ptr() % 16 for v in views) and any(v is not None and v.data_ptr() % 16 == 0 for v in views)
    return names, ps, flat, views


class _Twin:
    """The same update through the C ABI: own copies of parameters, state and shadows, own chunk tables (helper-built), the
    optimizer's lr / wd tables and gradient views."""

    def __init__(self, opt, ps, views, adam):
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)
        self.p = [p.detach().clone() for p in ps]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.h = [None if h is None else torch.full_like(h, float("nan")) for h in opt.shadows]
        n = [p.numel() for p in ps]
        ct, co = H.chunk_tables(n, C)
        self.args = dict(p=i64([x.data_ptr() for x in self.p]), m=i64([x.data_ptr() for x in self.m]), v=i64([x.data_ptr() for x in self.v]),
                         h=i64([0 if x is None else x.data_ptr() for x in self.h]), g=i64([0 if x is None else x.data_ptr() for x in views]),
                         ct=torch.tensor(ct, dtype=torch.int32, device=DEV), co=i64(co), n=i64(n), nch=len(ct))
        self.opt, self.adam, self.step, self.sticky = opt, adam, scalar(0.0), flag(0)

    def run(self):
        a, found = self.args, flag(0)
        call("editor_grad_check_multi", a["g"], a["ct"], a["co"], a["n"], a["nch"], found, self.sticky)
        if self.adam:
            call("editor_adamw_multi", a["p"], a["g"], a["m"], a["v"], a["ct"], a["co"], a["n"], self.opt.lr, self.opt.wd, H.BETAS[0],
                 H.BETAS[1], H.EPS, self.step, a["nch"], a["h"], 2, None, None, found)
        else:
            call("editor_sgd_multi", a["p"], a["g"], a["m"], a["ct"], a["co"], a["n"], self.opt.lr, self.opt.wd, 0.5, a["nch"], a["h"], 2,
                 None, None, found)


@pytest.mark.parametrize("cls", ["sgd", "adamw"])
def test_fused_optimizers_equal_the_direct_launch_on_bucket_views(cls):
    from editor_amd.optim import FusedAdamW, FusedSGD
    adam = cls == "adamw"
    names, ps, flat, views = _class_params(21)
    if adam:
        opt = FusedAdamW(list(zip(names, ps)), base_lr=2e-3, weight_decay=5e-2, bias_lr_factor=2.0, weight_decay_bias=1e-3,
                         shadow_dtype=F16, check_overflow=True)
    else:
        opt = FusedSGD(list(zip(names, ps)), base_lr=2.0 ** -3, weight_decay=2.0 ** -2, bias_lr_factor=2.0, weight_decay_bias=2.0 ** -3,
                       momentum=0.5, shadow_dtype=F16, check_overflow=True)
    assert opt.check_overflow and len({g["lr"] for g in opt.param_groups}) == 2
    # k-major copies: only for 2-D weights with both extents multiples of 64 and at least 2^18 elements
    by_name = dict(zip(names, opt.shadows_t))
    assert by_name["big.weight"] is not None and by_name["ragged.weight"] is None and by_name["small.weight"] is None
    assert sum(h is not None for h in opt.shadows_t) == 1
    twin = _Twin(opt, ps, views, adam)
    p64 = [p.detach().cpu().double() for p in ps]
    m64 = [torch.zeros_like(x) for x in p64]
    gen = torch.Generator().manual_seed(22)

    def compare(step):
        torch.cuda.synchronize()
        state = [("p", [p.detach() for p in ps], twin.p), ("m", opt.bufs, twin.m)]
        if adam:
            state.append(("v", opt.bufs_sq, twin.v))
            assert opt.step_count.item() == twin.step.item()
        for kind, mine, theirs in state:
            for name, x, y in zip(names, mine, theirs):
                assert_same(x.reshape(-1), y.reshape(-1), "%s %s step %d" % (name, kind, step))
        for name, p, h, hh, v in zip(names, ps, opt.shadows, twin.h, views):
            if h is not None and v is not None:
                assert_same(h.view(torch.int16).reshape(-1), hh.view(torch.int16).reshape(-1), "%s shadow step %d" % (name, step))
                assert_shadow(h.reshape(-1), p.detach().reshape(-1), F16, name)

    for step in range(1, 4):
        flat.copy_(torch.randint(-8, 9, (flat.numel(),), generator=gen).float())
        for p, v in zip(ps, views):
            p.grad = v
        opt.step()
        twin.run()
        compare(step)
        if not adam:                                             # exact operands: the float64 closed form as well
            for i, (p, v, g) in enumerate(zip(ps, views, opt.param_groups)):
                if v is not None:
                    p64[i], m64[i], _ = H.sgd_ref_step(p64[i], v.detach().cpu().double(), m64[i], g["lr"], g["weight_decay"], 0.5)
                assert_same(p.detach().cpu().double().reshape(-1), p64[i].reshape(-1), "%s vs closed form, step %d" % (names[i], step))
    assert not opt.found_inf()
    big = names.index("big.weight")
    assert torch.equal(opt.shadows_t[big], ps[big].detach().half().t())
    # a poisoned last element of the last tensor: the step is skipped, and reported once
    before = [(p.detach().clone(), b.clone(), None if h is None else h.clone()) for p, b, h in zip(ps, opt.bufs, opt.shadows)]
    t0 = opt.step_count.item() if adam else None
    flat[-1] = float("inf")
    assert views[-1].reshape(-1)[-1].item() == float("inf")
    opt.step()
    twin.run()
    compare(4)
    for name, p, b, h, (p0, b0, h0) in zip(names, ps, opt.bufs, opt.shadows, before):
        assert torch.equal(p.detach(), p0) and torch.equal(b, b0), name
        assert h is None or torch.equal(h.view(torch.int16), h0.view(torch.int16)), name     # (bits: a never-written shadow may hold NaNs)
    assert not adam or opt.step_count.item() == t0
    assert opt.found_inf() and not opt.found_inf()
    assert twin.sticky.item() == 1


def test_fused_adamw_first_step_under_capture_replays_like_eager_steps():
    """The device-resident step count: the FIRST step() is the captured one; three replays equal three eager steps of a twin
    optimizer bit for bit (p, exp_avg, exp_avg_sq, step_count), and a learning rate set to 0 between replays is honoured."""
    from editor_amd.optim import FusedAdamW
    gen = torch.Generator().manual_seed(31)
    names = ["a.weight", "a.bias", "b.weight", "cls_token", "c.bias"]
    shapes = [(64, 48), (64,), (33, 64), (1, 1, 48), (C + 5,)]
    ps = [torch.randn(s, generator=gen).to(DEV).requires_grad_(True) for s in shapes]
    ps2 = [p.detach().clone().requires_grad_(True) for p in ps]
    grads = [torch.randn(s, generator=gen).to(DEV) for s in shapes]
    kw = dict(base_lr=3e-3, weight_decay=5e-2, bias_lr_factor=2.0, weight_decay_bias=1e-3)
    eager = FusedAdamW(list(zip(names, ps2)), **kw)
    for _ in range(3):
        for q, gr in zip(ps2, grads):
            q.grad = gr
        eager.step()
    cap = FusedAdamW(list(zip(names, ps)), **kw)
    for p, gr in zip(ps, grads):
        p.grad = gr
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            cap.step()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert cap.step_count.item() == 3.0 == eager.step_count.item()
    for name, p, q, m, m2, v, v2 in zip(names, ps, ps2, cap.bufs, eager.bufs, cap.bufs_sq, eager.bufs_sq):
        assert_same(p.detach().reshape(-1), q.detach().reshape(-1), name + " p")
        assert_same(m.reshape(-1), m2.reshape(-1), name + " exp_avg")
        assert_same(v.reshape(-1), v2.reshape(-1), name + " exp_avg_sq")
    for g in cap.param_groups:
        g["weight_decay"] = 0.0
    cap.set_lr(0.0)
    before = [p.detach().clone() for p in ps]
    graph.replay()
    torch.cuda.synchronize()
    assert cap.step_count.item() == 4.0
    for p, b in zip(ps, before):
        assert torch.equal(p.detach(), b)
