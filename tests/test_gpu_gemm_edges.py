"""The dense GEMM kernels (gemm_bf16.hip, gemm_f32.hip) bit for bit at tile, dispatch and split-K edges.

Operands are small integers and every epilogue constant is dyadic (gemm_edge_helpers.py), so each output element is ONE rounding of a
number known exactly in float64: the plain, residual, beta and split-K cases compare bits, element by element, and every buffer is NaN
wherever the kernel has no business (operand padding, guard rows and columns, unwritten outputs).  GELU outputs are held to a per-element
bound.  Kernels are pinned through EPI_FORCE_PP / EPI_PIPE128 / EPI_TILE_ROWS(208) only; leading dimensions differ from the contiguous
extent everywhere, which is why most calls go to the C entry directly (ops.gemm always passes ldaux = n)."""
import pytest
import torch
import torch.nn.functional as F

import gemm_edge_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = H.BF16, H.F16, H.F32
_dt = lambda d: str(d).split(".")[-1]
_cid = lambda c: "%s-%dx%dx%d-%d" % (c.family, c.m, c.n, c.k, c.ldc_pad)


@pytest.fixture
def ops(monkeypatch):
    from editor_amd import ops
    monkeypatch.setattr(ops, "SHORT_TILES", False)           # the kernel is pinned by the flags each case passes
    return ops


def _vec(x):
    return None if x is None else x.to(F32).to(DEV)


def _nan_workspace(ops, nfloats):
    ws = ops.workspace(torch.device(DEV, torch.cuda.current_device()), nfloats)
    ws.fill_(H.NAN)                                          # a slab nobody wrote must not hold the previous call's partial sums
    return ws


def run_h16(ops, dtype, a, b, m, n, k, ta=0, tb=0, c_dtype=None, alpha=1.0, beta=0.0, bias=None, rs=None, splitk=1, epi=0, aux=None,
            aux_dtype=None, c_pad=H.PAD, aux_pad=H.PAD, old=None, keep=None, over=None, a_shift=0):
    """editor_gemm_bf16 / _f16 on padded, NaN-guarded buffers.  a (>= m, k), b (>= n, k) float64; aux: 'out' (a NaN-filled buffer the
    epilogue writes), a float64 matrix (an epilogue input) or None.  over / a_shift: raw argument overrides (refusal cases: the buffers
    are built for m, n, k, ta, tb; the call says otherwise).  -> (C, aux) buffers"""
    c_dtype = c_dtype or dtype
    A, lda, ao = H.padded(a[:m, :k].t() if ta else a[:m, :k], dtype, DEV)
    B, ldb, bo = H.padded(b[:n, :k].t() if tb else b[:n, :k], dtype, DEV)
    C, ldc, co = H.out_buffer(m, n, c_dtype, DEV, c_pad, old)
    X, ldaux, xo = None, n + aux_pad, 0
    if isinstance(aux, str):
        X, ldaux, xo = H.out_buffer(m, n, aux_dtype or dtype, DEV, aux_pad)
    elif aux is not None:
        X, ldaux, xo = H.padded(aux, aux_dtype or dtype, DEV, aux_pad)
    if keep is not None:
        keep.append(C)
    ws = _nan_workspace(ops, splitk * m * n) if splitk > 1 else None
    g = dict(A=ops._ptr(A, ao + a_shift), B=ops._ptr(B, bo), m=m, n=n, k=k, lda=lda, ldb=ldb, ldc=ldc, ta=ta, tb=tb)
    g.update(over or {})
    ops.call(ops._h16(A, "gemm"), g["A"], g["B"], ops._ptr(C, co), 1 if c_dtype == F32 else 0, g["m"], g["n"], g["k"], g["lda"], g["ldb"],
             g["ldc"], int(g["ta"]), int(g["tb"]), float(alpha), float(beta), _vec(bias), _vec(rs), int(splitk), int(epi),
             None if X is None else ops._ptr(X, xo), ldaux, ws, None)
    return C, X


def _same_bits(x, y):
    return torch.equal(H._bits(x.cpu()), H._bits(y.cpu()))


# ---------------------------------------------------------------------------------------------------------------------------
# plain epilogue: every family, all four layouts, 16-bit and fp32 C
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", H.HALF, ids=_dt)
@pytest.mark.parametrize("c", H.PLAIN_CASES, ids=_cid)
def test_plain_epilogue_every_layout_exact(ops, c, dtype):
    d = H.exact_operands(c.m, c.n, c.k)
    ran = 0
    for ta, tb in H.LAYOUTS:
        m, n = H.layout_shape(c.m, c.n, ta, tb)
        if min(m, n) == 0:
            continue
        for cdt in (dtype, F32):
            ref = H.exact_ref(d, cdt, rows=m, cols=n)
            H.check_preconditions(ref, cdt, c.k)
            C, _ = run_h16(ops, dtype, d["a"], d["b"], m, n, c.k, ta, tb, cdt, alpha=0.5, bias=H.bias_for(d, cdt)[:n], rs=d["rs"][:m],
                           epi=H.flag_bits(c.flags), c_pad=c.ldc_pad)
            H.check_exact(C, ref, m, n, "%s %dx%dx%d ta=%d tb=%d C %s" % (c.family, m, n, c.k, ta, tb, _dt(cdt)))
            ran += 1
    assert ran >= 2


# ---------------------------------------------------------------------------------------------------------------------------
# fused epilogues and beta at each family's most ragged shapes (k-major operands)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", H.HALF, ids=_dt)
@pytest.mark.parametrize("name", H.EPILOGUES)
@pytest.mark.parametrize("c", H.EPILOGUE_CASES, ids=_cid)
def test_fused_epilogues(ops, c, name, dtype):
    m, n, k = c.m, c.n, c.k
    d = H.exact_operands(m, n, k)
    fl = H.flag_bits(c.flags)
    what = "%s %dx%dx%d %s %s" % (c.family, m, n, k, name, _dt(dtype))
    kw = dict(alpha=0.5, rs=d["rs"], c_pad=c.ldc_pad)
    if name == "residual_f32":
        ref = H.exact_ref(d, F32, residual=True)
        C, _ = run_h16(ops, dtype, d["a"], d["b"], m, n, k, c_dtype=F32, bias=d["ibias"], epi=fl | ops.EPI_RESIDUAL, aux=d["res"], aux_dtype=F32, **kw)
        H.check_exact(C, ref, m, n, what)
    elif name in ("beta_f32", "beta_h16"):
        cdt = F32 if name == "beta_f32" else dtype
        ref = H.exact_ref(d, cdt, beta=0.5)
        H.check_preconditions(ref, cdt, k)
        if c.family == "pp208":                               # short tiles have no beta path: refused before any launch, C keeps its bits
            keep = []
            with pytest.raises(RuntimeError, match="hipError 1"):
                run_h16(ops, dtype, d["a"], d["b"], m, n, k, c_dtype=cdt, beta=0.5, bias=H.bias_for(d, cdt), epi=fl, old=d["cold"], keep=keep, **kw)
            return H.check_exact(keep[0], d["cold"], m, n, what + " refused")
        C, _ = run_h16(ops, dtype, d["a"], d["b"], m, n, k, c_dtype=cdt, beta=0.5, bias=H.bias_for(d, cdt), epi=fl, old=d["cold"], **kw)
        H.check_exact(C, ref, m, n, what)
    elif name == "gelu_bwd_auxgrad":                          # C = value * saved gelu' (dyadic here: exact)
        ref = H.exact_ref(d, dtype) * d["sel"]
        C, X = run_h16(ops, dtype, d["a"], d["b"], m, n, k, bias=H.bias_for(d, dtype), epi=fl | ops.EPI_GELU_BWD | ops.EPI_AUX_GRAD, aux=d["sel"], **kw)
        H.check_exact(C, ref, m, n, what)
        H.check_exact(X, d["sel"], m, n, what + " (aux is an input)")
    elif name == "gelu_bwd":                                  # C = value * gelu'(saved pre-activation), sixteenths in [-4, 4]
        x = d["res"] / 16.0
        v = H.exact_ref(d, dtype)
        C, _ = run_h16(ops, dtype, d["a"], d["b"], m, n, k, bias=H.bias_for(d, dtype), epi=fl | ops.EPI_GELU_BWD, aux=x, **kw)
        H.check_guards(C, m, n, what)
        H.check_gelu_bound(H.window(C.cpu(), m, n), v * H.gelu_grad64(x), x, dtype, what, scale=v)
    else:
        pre = H.exact_ref(d, dtype)                           # fractional: the saved pre-activation is itself a rounding under test
        x = pre.to(F32).to(dtype).double()
        flags = fl | ops.EPI_GELU | (ops.EPI_AUX_GRAD if name == "gelu_auxgrad" else 0)
        C, X = run_h16(ops, dtype, d["a"], d["b"], m, n, k, bias=H.bias_for(d, dtype), epi=flags, aux=None if name == "gelu_noaux" else "out", **kw)
        H.check_guards(C, m, n, what)
        H.check_gelu_bound(H.window(C.cpu(), m, n), H.gelu64(x), x, dtype, what + " C")
        if name == "gelu":
            H.check_exact(X, pre, m, n, what + " saved pre-activation")
        elif name == "gelu_auxgrad":
            H.check_guards(X, m, n, what + " aux")
            H.check_gelu_bound(H.window(X.cpu(), m, n), H.gelu_grad64(x), x, dtype, what + " saved gelu'")
        else:                                                 # no-grad forward: same activation bits as with the pre-activation saved
            C2, _ = run_h16(ops, dtype, d["a"], d["b"], m, n, k, bias=H.bias_for(d, dtype), epi=fl | ops.EPI_GELU, aux="out", **kw)
            assert _same_bits(C, C2), what


# ---------------------------------------------------------------------------------------------------------------------------
# 208-row tiles
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", H.HALF, ids=_dt)
@pytest.mark.parametrize("c", H.T208, ids=_cid)
def test_short_tiles_exact_and_equal_to_full_tiles(ops, c, dtype):
    m, n, k = c.m, c.n, c.k
    d = H.exact_operands(m, n, k)
    for cdt in (dtype, F32):
        what = "208-row tiles %dx%dx%d C %s" % (m, n, k, _dt(cdt))
        kw = dict(c_dtype=cdt, alpha=0.5, bias=H.bias_for(d, cdt), rs=d["rs"])
        if m < 256:
            # fewer than 256 rows are outside the pipelined kernels: gemm_h16 refuses short tiles there before any launch
            keep = []
            with pytest.raises(RuntimeError, match="hipError 1"):
                run_h16(ops, dtype, d["a"], d["b"], m, n, k, epi=H.flag_bits(c.flags), keep=keep, **kw)
            H.check_untouched(keep[0], what)
            continue
        ref = H.exact_ref(d, cdt)
        C, _ = run_h16(ops, dtype, d["a"], d["b"], m, n, k, epi=H.flag_bits(c.flags), **kw)
        H.check_exact(C, ref, m, n, what)
        full, _ = run_h16(ops, dtype, d["a"], d["b"], m, n, k, epi=ops.EPI_FORCE_PP, **kw)
        assert _same_bits(C, full), what + ": differs from full tiles"


# ---------------------------------------------------------------------------------------------------------------------------
# auto dispatch: the 2047 / 2048-row and 504 / 512-column thresholds, with and without the wrapper's tile plan
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", H.HALF, ids=_dt)
@pytest.mark.parametrize("plan", [False, True], ids=["thresholds", "tile-plan"])
@pytest.mark.parametrize("c", H.AUTO, ids=_cid)
def test_auto_dispatch_exact(ops, monkeypatch, c, plan, dtype):
    monkeypatch.setattr(ops, "SHORT_TILES", plan)
    m, n, k = c.m, c.n, c.k
    d = H.exact_operands(m, n, k)
    for cdt in (dtype, F32):
        A, lda, ao = H.padded(d["a"], dtype, DEV)
        B, ldb, bo = H.padded(d["b"], dtype, DEV)
        C, ldc, co = H.out_buffer(m, n, cdt, DEV)
        ops.gemm(A, B, C, m, n, k, lda, ldb, ldc, alpha=0.5, bias=_vec(H.bias_for(d, cdt)), rowscale=_vec(d["rs"]), a_off=ao, b_off=bo, c_off=co)
        H.check_exact(C, H.exact_ref(d, cdt), m, n, "auto %dx%dx%d C %s plan=%s" % (m, n, k, _dt(cdt), plan))


# ---------------------------------------------------------------------------------------------------------------------------
# split-K into fp32 C: slabs (transposed operands) and atomics (k-major), empty and clamped splits, beta
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", H.HALF, ids=_dt)
@pytest.mark.parametrize("s", H.SPLITK_CASES, ids=lambda s: "%dx%dx%d-%s-t%d-s%d" % (s.m, s.n, s.k, "".join(s.flags) or "none", s.ta, s.splitk))
def test_splitk_exact_and_repeatable(ops, s, dtype):
    m, n, k = s.m, s.n, s.k
    d = H.exact_operands(m, n, k)
    c_pad = 0 if (s.ta or s.tb) else H.PAD                    # slabs need a contiguous C; the guard rows stay
    for beta in (0.0, 1.0, 0.5):
        what = "split-K %d of %dx%dx%d t=%d beta=%g %s" % (s.splitk, m, n, k, s.ta, beta, _dt(dtype))
        ref = H.exact_ref(d, F32, beta=beta)                  # the bias once, whatever the split count
        old = None if beta == 0.0 else d["cold"]
        runs = []
        for _ in range(2):
            if s.wrapper:                                     # whole K-tiles as slabs + the tail as a second product (ops.gemm)
                A, lda, ao = H.padded(d["a"].t(), dtype, DEV)
                B, ldb, bo = H.padded(d["b"].t(), dtype, DEV)
                C, ldc, co = H.out_buffer(m, n, F32, DEV, c_pad, old)
                _nan_workspace(ops, s.splitk * m * n)
                ops.gemm(A, B, C, m, n, k, lda, ldb, ldc, 1, 1, alpha=0.5, beta=beta, bias=_vec(d["ibias"]), rowscale=_vec(d["rs"]),
                         splitk=s.splitk, a_off=ao, b_off=bo, c_off=co, epilogue=H.flag_bits(s.flags))
            else:
                C, _ = run_h16(ops, dtype, d["a"], d["b"], m, n, k, s.ta, s.tb, F32, alpha=0.5, beta=beta, bias=d["ibias"], rs=d["rs"],
                               splitk=s.splitk, epi=H.flag_bits(s.flags), c_pad=c_pad, old=old)
            H.check_exact(C, ref, m, n, what)
            runs.append(C)
        assert _same_bits(*runs), what + ": two runs differ"


# ---------------------------------------------------------------------------------------------------------------------------
# the bf16 GELU table of the one-pass epilogue against its arithmetic fallback
# ---------------------------------------------------------------------------------------------------------------------------
def test_gelu_table_returns_the_bits_of_the_arithmetic(ops):
    m, n, k = H.GELU_TABLE_SHAPE
    assert H.dispatch(m, n, k, flags=("pp",), epi=ops.EPI_GELU, ldc=n + H.PAD, ldaux=n + H.PAD).epilogue == "onepass"
    seen = {"C": [], "gelu'": []}
    for kind in H.GELU_SETS:
        a, b, bias, pre = H.gelu_operands(kind, m, n, k)
        x = pre.to(BF16).double()
        C, X = run_h16(ops, BF16, a, b, m, n, k, bias=bias, epi=ops.EPI_FORCE_PP | ops.EPI_GELU, aux="out")
        H.check_exact(X, pre, m, n, "GELU %s set: saved pre-activation" % kind)
        H.check_guards(C, m, n, kind)
        H.check_gelu_bound(H.window(C.cpu(), m, n), H.gelu64(x), x, BF16, "GELU table, %s set, C" % kind)
        C2, D = run_h16(ops, BF16, a, b, m, n, k, bias=bias, epi=ops.EPI_FORCE_PP | ops.EPI_GELU | ops.EPI_AUX_GRAD, aux="out")
        H.check_guards(D, m, n, kind)
        H.check_gelu_bound(H.window(D.cpu(), m, n), H.gelu_grad64(x), x, BF16, "GELU table, %s set, saved gelu'" % kind)
        assert _same_bits(C, C2), "GELU %s set: the activation depends on what is saved" % kind
        key = (H._bits(pre.to(BF16)).long() & 0xFFFF) << 16
        seen["C"].append(torch.stack([key, H._bits(H.window(C.cpu(), m, n)).long() & 0xFFFF]).flatten(1))
        seen["gelu'"].append(torch.stack([key, H._bits(H.window(D.cpu(), m, n)).long() & 0xFFFF]).flatten(1))
    # C and gelu' are functions of the pre-activation's 16 bits alone, whichever path (table or arithmetic) a chunk took
    for name, parts in seen.items():
        kv = torch.cat(parts, 1)
        pairs, inputs = torch.unique(kv[0] | kv[1]), torch.unique(kv[0])
        if pairs.numel() != inputs.numel():
            ks, counts = torch.unique(torch.unique(kv[0] | kv[1]) >> 16, return_counts=True)
            bad = int(ks[counts > 1][0])
            raise AssertionError("%s: pre-activation bits 0x%04x map to %d different outputs" % (name, bad, int(counts.max())))


# ---------------------------------------------------------------------------------------------------------------------------
# split mode (editor_gemm_f16x2): always the 256x256 kernel, any M
# ---------------------------------------------------------------------------------------------------------------------------
def _run_split(ops, d, m, n, k, c_f32, flags, bias=None, rs=None, epi=0, aux=None):
    bufs = [H.padded(d[name], F16, DEV) for name in ("a_hi", "a_lo", "b_hi", "b_lo")]
    lda, ldb = bufs[0][1], bufs[2][1]
    C, ldc, co = H.out_buffer(m, n, F32 if c_f32 else F16, DEV)
    L = None if c_f32 else H.out_buffer(m, n, F16, DEV)[0]
    X, ldaux, xo = None, n + H.PAD, 0
    if isinstance(aux, str):
        X, ldaux, xo = H.out_buffer(m, n, F16, DEV)
    elif aux is not None:
        X, ldaux, xo = H.padded(aux, F32, DEV)
    ops.call("editor_gemm_f16x2", *[ops._ptr(t, off) for t, _, off in bufs], ops._ptr(C, co), None if L is None else ops._ptr(L, co),
             1 if c_f32 else 0, m, n, k, lda, ldb, ldc, 1.0, _vec(bias), _vec(rs), int(epi) | H.flag_bits(flags),
             None if X is None else ops._ptr(X, xo), ldaux, None)
    return C, L, X


@pytest.mark.parametrize("m,n,k,flags", H.SPLIT_MODE_CASES)
def test_split_mode_pairs_exact(ops, m, n, k, flags):
    d = H.pair_operands(m, n, k)
    what = "f16x2 %dx%dx%d %s" % (m, n, k, "".join(flags))
    plain = (d["prod"] + d["ibias"]) * d["rs"][:, None]
    H.check_preconditions(plain, F32, k)
    # pair output: hi = half(ref), lo = half(ref - hi), bit for bit
    C, L, _ = _run_split(ops, d, m, n, k, False, flags, bias=d["ibias"], rs=d["rs"])
    hi, lo = H.pair_of(plain)
    H.check_exact(C, plain, m, n, what + " pair hi")
    H.check_exact(L, plain - hi.double(), m, n, what + " pair lo")
    # fp32 output, plain and with the residual
    C, _, _ = _run_split(ops, d, m, n, k, True, flags, bias=d["ibias"], rs=d["rs"])
    H.check_exact(C, plain, m, n, what + " fp32")
    C, _, _ = _run_split(ops, d, m, n, k, True, flags, bias=d["ibias"], rs=d["rs"], epi=ops.EPI_RESIDUAL, aux=d["res"])
    H.check_exact(C, plain + d["res"], m, n, what + " fp32 residual")
    # GELU of the unrounded pre-activation as a pair, gelu' saved as half
    C, L, X = _run_split(ops, d, m, n, k, False, flags, bias=d["ibias"], rs=d["rs"], epi=ops.EPI_GELU | ops.EPI_AUX_GRAD, aux="out")
    for buf in (C, L, X):
        H.check_guards(buf, m, n, what + " GELU")
    got = H.window(C.cpu(), m, n).double() + H.window(L.cpu(), m, n).double()
    ref = H.gelu64(plain)
    H.check_erff_bound(got, ref, what + " GELU pair")
    torch32 = F.gelu(plain.to(F32)).double()                  # the bar of test_gemm_f16x2_vs_float64, per row
    row = lambda v: (v - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)
    worst = (row(got) / torch.maximum(2.0 * row(torch32), torch.full((m,), 3e-7, dtype=torch.float64))).max().item()
    assert worst <= 1.0, (what, "GELU pair row error over the bar", worst)
    H.check_gelu_bound(H.window(X.cpu(), m, n), H.gelu_grad64(plain), plain, F16, what + " saved gelu'")


# ---------------------------------------------------------------------------------------------------------------------------
# grouped weight gradients
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", H.HALF, ids=_dt)
@pytest.mark.parametrize("m", H.WGRAD_M)
def test_wgrad_group_exact_and_repeatable(ops, m, dtype):
    rows = lambda buf, r: buf[H.GUARD:H.GUARD + r]            # (contiguous: these buffers have no padding columns)
    data, refs = [], []
    for n, k in H.WGRAD_PROBLEMS:
        d = H.exact_operands(n, k, m)                         # dW (n, k) = dy^T x over m token rows
        data.append((H.padded(d["a"].t(), dtype, DEV, 0)[0], H.padded(d["b"].t(), dtype, DEV, 0)[0]))
        refs.append(0.5 * d["prod"])
    runs = []
    for _ in range(2):
        outs = [H.out_buffer(n, k, F32, DEV, 0)[0] for n, k in H.WGRAD_PROBLEMS]
        _nan_workspace(ops, 1 << 22)
        ops.gemm_wgrad_group([(rows(dy, m), rows(x, m), rows(o, n)) for (dy, x), o, (n, k) in zip(data, outs, H.WGRAD_PROBLEMS)], m, alpha=0.5)
        for o, ref, (n, k) in zip(outs, refs, H.WGRAD_PROBLEMS):
            H.check_exact(o, ref, n, k, "grouped wgrad M=%d problem %dx%d %s" % (m, n, k, _dt(dtype)))
        runs.append(outs)
    assert all(_same_bits(p, q) for p, q in zip(*runs))


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 kernel
# ---------------------------------------------------------------------------------------------------------------------------
def run_f32(ops, a, b, m, n, k, ta=0, tb=0, pad=1, alpha=0.5, beta=0.0, bias=None, rs=None, splitk=1, epi=0, aux=None, old=None, keep=None):
    A, lda, ao = H.padded(a.t() if ta else a, F32, DEV, pad)
    B, ldb, bo = H.padded(b.t() if tb else b, F32, DEV, pad)
    C, ldc, co = H.out_buffer(m, n, F32, DEV, pad, old)
    X, ldaux, xo = None, n + pad, 0
    if isinstance(aux, str):
        X, ldaux, xo = H.out_buffer(m, n, F32, DEV, pad)
    elif aux is not None:
        X, ldaux, xo = H.padded(aux, F32, DEV, pad)
    if keep is not None:
        keep.append(C)
    ops.call("editor_gemm_f32", ops._ptr(A, ao), ops._ptr(B, bo), ops._ptr(C, co), m, n, k, lda, ldb, ldc, int(ta), int(tb), 1, 0, 0, 0,
             1, 0, 0, 0, float(alpha), float(beta), _vec(bias), _vec(rs), int(splitk), int(epi), None if X is None else ops._ptr(X, xo), ldaux)
    return C, X


@pytest.mark.parametrize("pad", H.F32_PADS)
@pytest.mark.parametrize("m,n,k", H.F32_SHAPES)
def test_f32_kernel_exact(ops, m, n, k, pad):
    d = H.exact_operands(m, n, k)
    a, b = d["a"], d["b"]
    for ta, tb in H.LAYOUTS:
        what = "f32 %dx%dx%d ta=%d tb=%d pad %d" % (m, n, k, ta, tb, pad)
        C, _ = run_f32(ops, a, b, m, n, k, ta, tb, pad, bias=d["ibias"], rs=d["rs"])
        H.check_exact(C, H.exact_ref(d, F32), m, n, what)
        C, _ = run_f32(ops, a, b, m, n, k, ta, tb, pad, beta=0.5, bias=d["ibias"], rs=d["rs"], old=d["cold"])
        H.check_exact(C, H.exact_ref(d, F32, beta=0.5), m, n, what + " beta")
        for sk in H.F32_SPLITK:
            C, _ = run_f32(ops, a, b, m, n, k, ta, tb, pad, bias=d["ibias"], splitk=sk)
            H.check_exact(C, H.exact_ref(d, F32, rowscale=False), m, n, what + " split-K %d" % sk)
            C, _ = run_f32(ops, a, b, m, n, k, ta, tb, pad, beta=0.5, bias=d["ibias"], splitk=sk, old=d["cold"])
            H.check_exact(C, H.exact_ref(d, F32, rowscale=False, beta=0.5), m, n, what + " split-K %d beta" % sk)
    what = "f32 %dx%dx%d pad %d" % (m, n, k, pad)
    C, _ = run_f32(ops, a, b, m, n, k, 0, 0, pad, bias=d["ibias"], rs=d["rs"], epi=ops.EPI_RESIDUAL, aux=d["res"])
    H.check_exact(C, H.exact_ref(d, F32, residual=True), m, n, what + " residual")
    pre = H.exact_ref(d, F32)
    C, X = run_f32(ops, a, b, m, n, k, 0, 0, pad, bias=d["ibias"], rs=d["rs"], epi=ops.EPI_GELU, aux="out")
    H.check_exact(X, pre, m, n, what + " saved pre-activation")
    H.check_guards(C, m, n, what)
    H.check_erff_bound(H.window(C.cpu(), m, n), H.gelu64(pre), what + " GELU")
    # C = value * gelu'(saved): the bound is absolute (1e-6) around the zero of gelu', so the multiplier is kept O(1) - alpha 2^-6, no
    # bias, no row scale: |value| <= 2.5 against erff's ~1.5e-7 on gelu'
    x = d["res"] / 16.0
    C, _ = run_f32(ops, a, b, m, n, k, 0, 0, pad, alpha=2.0 ** -6, epi=ops.EPI_GELU_BWD, aux=x)
    H.check_guards(C, m, n, what)
    H.check_erff_bound(H.window(C.cpu(), m, n), 2.0 ** -6 * d["prod"] * H.gelu_grad64(x), what + " GELU_BWD")


def test_f32_two_level_batch_leaves_the_gaps_alone(ops):
    m, n, k, b1, b2 = 63, 65, 17, 2, 3
    d = H.exact_operands(b1 * b2 * m, b1 * b2 * n, k)
    sA2, sB2, sC2 = m * k + 5, n * k + 9, m * n + 3
    sA1, sB1, sC1 = b2 * sA2 + 7, b2 * sB2 + 2, b2 * sC2 + 11
    A = torch.full((b1 * sA1 + 16,), H.NAN, dtype=F32)
    B = torch.full((b1 * sB1 + 16,), H.NAN, dtype=F32)
    refs = {}
    for i in range(b1):
        for j in range(b2):
            s = i * b2 + j
            ai, bi = d["a"][s * m:(s + 1) * m], d["b"][s * n:(s + 1) * n]
            A[8 + i * sA1 + j * sA2:][:m * k] = ai.to(F32).flatten()
            B[8 + i * sB1 + j * sB2:][:n * k] = bi.to(F32).flatten()
            refs[i, j] = 0.5 * ai @ bi.t() + d["ibias"][:n]
    C = torch.full((b1 * sC1 + 16,), H.NAN, dtype=F32, device=DEV)
    Ag, Bg = A.to(DEV), B.to(DEV)
    ops.call("editor_gemm_f32", ops._ptr(Ag, 8), ops._ptr(Bg, 8), ops._ptr(C, 8), m, n, k, k, k, n, 0, 0, b1, sA1, sB1, sC1, b2, sA2, sB2, sC2,
             0.5, 0.0, _vec(d["ibias"][:n]), None, 1, 0, None, n)
    got = C.cpu()
    written = torch.zeros(got.shape, dtype=torch.bool)
    for (i, j), ref in refs.items():
        o = 8 + i * sC1 + j * sC2
        buf = torch.full((m + 2 * H.GUARD, n), H.NAN, dtype=F32)
        buf[H.GUARD:H.GUARD + m] = got[o:o + m * n].view(m, n)
        H.check_exact(buf, ref, m, n, "f32 batch slice (%d, %d)" % (i, j))
        written[o:o + m * n] = True
    assert bool(torch.isnan(got[~written]).all()), "the gaps between the batch slices were written"


def test_f32_chunked_reduction_wrapper_exact(ops):
    m, n, k = H.F32_CHUNKED
    d = H.exact_operands(m, n, k)
    C = torch.full((m, n), H.NAN, dtype=F32, device=DEV)
    _nan_workspace(ops, 7 * m * n)
    ops.gemm(d["a"].to(F32).to(DEV), d["b"].to(F32).to(DEV), C, m, n, k, k, k, n, alpha=0.5, bias=_vec(d["ibias"]))
    buf = torch.full((m + 2 * H.GUARD, n), H.NAN, dtype=F32)
    buf[H.GUARD:H.GUARD + m] = C.cpu()
    H.check_exact(buf, H.exact_ref(d, F32, rowscale=False), m, n, "f32 eight-chunk path")


# ---------------------------------------------------------------------------------------------------------------------------
# refusals: an error before any launch, C untouched.  (Each is rejected by gemm_h16 / editor_gemm_f32 ahead of their first launch; every
# argument set stays inside its buffers, so nothing out of contract could run even if a check were missing.)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", H.HALF, ids=_dt)
@pytest.mark.parametrize("name", H.REFUSALS)
def test_refusals_write_nothing(ops, name, dtype):
    m, n, k = 256, 256, 128
    d = H.exact_operands(m, n, k)
    keep = []
    kw, over = dict(alpha=0.5, bias=d["ibias"], rs=d["rs"]), {}
    if name == "f32_rowscale_splitk":
        with pytest.raises(RuntimeError, match="hipError 1"):
            run_f32(ops, d["a"], d["b"], m, n, k, splitk=2, bias=d["ibias"], rs=d["rs"], keep=keep)
        return H.check_untouched(keep[0], name)
    if name in ("lda", "ldb"):
        over[name] = k + 4
    elif name == "n_mod4":
        over["n"] = n - 2
    elif name == "k_mod8":
        over["k"] = k - 4
    elif name == "ta_m_mod8":
        over.update(ta=1, m=m - 4, lda=m)                     # (the same bytes read as a (K, M) operand: in bounds)
        over["k"] = k // 2
    elif name == "tb_n_mod8":
        over.update(tb=1, n=n - 4, ldb=n, k=k // 2)
    elif name == "pointer":
        kw.update(a_shift=1)                                  # one element: 2 bytes off the 16-byte alignment
    elif name == "splitk_h16_c":
        kw.update(splitk=2)
    elif name == "splitk_epilogue":
        kw.update(splitk=2, c_dtype=F32, epi=ops.EPI_RESIDUAL, aux=d["res"], aux_dtype=F32)
    elif name == "auxgrad_plain":
        kw.update(epi=ops.EPI_AUX_GRAD, aux="out")
    elif name == "t208_transposed":
        kw.update(epi=ops.EPI_TILE_ROWS(208), tb=1)
    elif name == "t208_narrow":
        kw.update(epi=ops.EPI_TILE_ROWS(208))
        over["n"] = 128
    elif name == "t208_few_rows":
        kw.update(epi=ops.EPI_TILE_ROWS(208))
        over["m"] = 208
    elif name == "tile_rows_240":
        kw.update(epi=ops.EPI_TILE_ROWS(240))
    with pytest.raises(RuntimeError, match="hipError 1"):
        run_h16(ops, dtype, d["a"], d["b"], m, n, k, keep=keep, over=over, **kw)
    H.check_untouched(keep[0], name)
