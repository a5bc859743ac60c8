"""Data, case tables and checks of the dense-GEMM edge suite (test_gemm_edges_host.py, test_gpu_gemm_edges.py).

The products are tested EXACTLY: operands are small integers, so every partial sum is an integer below 2^24 and fp32 accumulation is
exact in any order; alpha, bias, row scale, beta and the residual are dyadic, so the whole plain epilogue is exact in fp32 as well and a
16-bit output is ONE round-to-nearest-even of a number known in float64.  Every buffer a kernel sees is NaN wherever it has no business:
operand padding, guard rows, guard columns, unwritten outputs.  Nothing here runs GPU code at import."""
import functools
from collections import namedtuple

import torch

from editor_amd import ops as O                     # (flag constants and the tile-plan heuristic only)

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
HALF = (BF16, F16)
NAN = float("nan")
GUARD, PAD = 2, 8                                   # guard rows on each side of a window, padding columns behind it
BK = 64                                             # K-tile of the 16-bit kernels
UNIT = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -23}      # one unit of the output type, relative
MIN_NORMAL = {BF16: 2.0 ** -126, F16: 2.0 ** -14, F32: 2.0 ** -126}   # below it the spacing is absolute: UNIT * MIN_NORMAL is half of it
GELU_FLOOR = 2 * 8e-7                               # twice the documented fp32 error of the erfc form (gemm_bf16.hip, above phi2)
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))          # (transposed A, transposed B)

# ---------------------------------------------------------------------------------------------------------------------------
# case tables: (M, N, K) per kernel family, with the flags that pin the kernel
# ---------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "family m n k flags ldc_pad")
Case.__new__.__defaults__ = ((), PAD)


def _cases(family, shapes, flags=()):
    return [Case(family, m, n, k, tuple(flags)) for m, n, k in shapes]


SMALL_REG = _cases("small_reg", [(1, 4, 8), (7, 8, 64), (9, 12, 72), (129, 132, 200), (128, 128, 8), (300, 124, 136)])
SMALL_GLDS = _cases("small_glds", [(8, 8, 64), (9, 8, 128), (127, 128, 64), (255, 260, 192), (1100, 124, 64), (1000, 120, 128)])
PIPE128 = _cases("pipe128", [(256, 128, 64), (257, 132, 128), (511, 136, 192), (513, 260, 256), (770, 384, 320)]) + \
    _cases("pipe128", [(2049, 512, 64)], ("pipe128",))
PP256 = _cases("pp256", [(256, 256, 64), (257, 264, 128), (513, 520, 320), (511, 260, 192)], ("pp",)) + \
    [Case("pp256", 513, 520, 320, ("pp",), 4), Case("pp256", 264, 256, 256, ("pp",))]      # (the last: the missing K-tile count, 4)
T208 = _cases("pp208", [(207, 256, 64), (209, 264, 128), (417, 520, 192), (625, 256, 64)], ("t208",))
AUTO = _cases("auto", [(2047, 512, 64), (2048, 512, 64), (2048, 504, 64)])
PLAIN_CASES = SMALL_REG + SMALL_GLDS + PIPE128 + PP256
# the most ragged shapes of each family: every fused epilogue and beta run here (k-major operands)
# (208-row tiles take beta 0 only: there the two beta cases assert the refusal)
EPILOGUE_CASES = [SMALL_REG[3], SMALL_REG[5], SMALL_GLDS[3], SMALL_GLDS[4], PIPE128[1], PIPE128[3], PIPE128[5], PP256[2], PP256[3], PP256[4],
                  T208[2]]
EPILOGUES = ("residual_f32", "gelu", "gelu_auxgrad", "gelu_noaux", "gelu_bwd", "gelu_bwd_auxgrad", "beta_f32", "beta_h16")

SplitCase = namedtuple("SplitCase", "m n k flags ta tb splitk wrapper")
SPLITK_CASES = [SplitCase(m, n, 320, fl, t, t, s, False)
                for (m, n, fl) in ((256, 128, ()), (256, 256, ("pp",))) for t in (1, 0) for s in (2, 4, 7)] + \
    [SplitCase(129, 132, 200, (), 0, 0, 3, False),
     SplitCase(256, 128, 200, (), 1, 1, 2, True), SplitCase(256, 128, 248, (), 1, 1, 2, True)]
GELU_TABLE_SHAPE = (513, 520, 64)
GELU_SETS = ("table", "fallback", "mixed")
SPLIT_MODE_CASES = [(1, 8, 64, ()), (255, 264, 128, ()), (257, 520, 192, ()), (209, 256, 64, ("t208",))]
WGRAD_M = (64, 128, 320)
WGRAD_PROBLEMS = ((256, 256), (512, 256), (256, 768))          # (N_i, K_i) of dW_i = dy_i^T x_i
F32_SHAPES = [(1, 1, 1), (64, 64, 16), (63, 65, 17), (65, 63, 33), (129, 130, 100)]
F32_PADS = (1, 4)
F32_SPLITK = (2, 9)
F32_CHUNKED = (64, 64, 1024)
REFUSALS = ("lda", "ldb", "n_mod4", "k_mod8", "ta_m_mod8", "tb_n_mod8", "pointer", "splitk_h16_c", "splitk_epilogue", "auxgrad_plain",
            "t208_transposed", "t208_narrow", "t208_few_rows", "tile_rows_240", "f32_rowscale_splitk")


def flag_bits(flags):
    bits = 0
    for f in flags:
        bits |= {"pp": O.EPI_FORCE_PP, "pipe128": O.EPI_PIPE128, "t208": O.EPI_TILE_ROWS(208)}[f]
    return bits


def layout_shape(m, n, ta, tb):
    """A transposed operand's contiguous extent (M or N) must be a multiple of 8: round it down (0: the layout does not exist)."""
    return (m // 8 * 8 if ta else m), (n // 8 * 8 if tb else n)


# ---------------------------------------------------------------------------------------------------------------------------
# the host dispatch of gemm_h16 / launch_pipe / pp_body, restated from their documented thresholds
# ---------------------------------------------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "family epilogue split glds")


def dispatch(m, n, k, ta=0, tb=0, c_f32=False, flags=(), splitk=1, beta=0.0, ldc=None, ldaux=None, epi=O.EPI_NONE, ws=True):
    """-> Plan(kernel family, epilogue path, split-K form, LDS-DMA staging) that editor_gemm_bf16 / _f16 takes for these arguments."""
    ldc = n if ldc is None else ldc
    ldaux = n if ldaux is None else ldaux
    ktiles = -(-k // BK)
    splitk = max(1, min(splitk, ktiles))
    glds = k % BK == 0 and m >= 8 and n >= 8
    pipe = glds and m >= 256 and n >= 128
    short = "t208" in flags
    force = "pp" in flags or short
    prefer_pipe = "pipe128" in flags and not force
    slabs = splitk > 1 and pipe and bool(ta or tb) and ws and ldc == n and (m * n) % 4 == 0
    split = "none" if splitk == 1 else ("slabs" if slabs else "atomics")
    staged_ok = beta == 0.0 and (splitk == 1 or slabs) and n % 8 == 0 and ldc % 8 == 0 and ldaux % 8 == 0
    if not pipe:
        return Plan("small_glds" if glds else "small_reg", "direct", split, glds)
    pp_auto = m >= 2048 and splitk == 1 and not ta and n >= 512 and not prefer_pipe
    if n >= 256 and (force or pp_auto):
        if staged_ok and not c_f32 and epi in (O.EPI_NONE, O.EPI_GELU, O.EPI_GELU_BWD):
            path = "onepass"
        else:
            path = "staged" if staged_ok else "direct"
        return Plan("pp208" if short else "pp256", path, split, True)
    k_staged = bool(ta or tb)                               # forward layouts measured faster with the direct epilogue
    return Plan("pipe128", "staged" if k_staged and staged_ok else "direct", split, True)


def wrapper_flags(m, n, k, ldc, short_tiles=True):
    """the kernel-selection flags ops.gemm adds on its own for a plain forward product (k-major operands, split-K 1, beta 0)"""
    if short_tiles and m >= 2048 and n >= 512 and n % 8 == 0 and ldc % 8 == 0 and k % BK == 0:
        th, narrow = O.gemm_tile_plan(m, n)
        if narrow:
            return ("pipe128",)
        if th != 256:
            return ("t208",)
    return ()


# ---------------------------------------------------------------------------------------------------------------------------
# exact operands
# ---------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


@functools.lru_cache(maxsize=None)
def exact_operands(m, n, k):
    """float64 tensors: a (m, k) and b (n, k) integers in [-3, 3], prod = a b^T, rs in {0.5, 1, 2}, odd (n) odd integers (the fractional
    bias's numerator), ibias (n) integers, res and cold (m, n) integers in [-64, 64], sel (m, n) in {+-0.5, +-1, +-2}."""
    g = _gen(m, n, k)
    a, b = _ints(g, -3, 3, m, k), _ints(g, -3, 3, n, k)
    d = dict(a=a, b=b, prod=a @ b.t())
    d["rs"] = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (m,), generator=g)]
    d["odd"] = 2 * _ints(g, -32, 31, n) + 1
    d["ibias"] = _ints(g, -8, 8, n)
    d["res"], d["cold"] = _ints(g, -64, 64, m, n), _ints(g, -64, 64, m, n)
    d["sel"] = torch.tensor([0.5, 1.0, 2.0, -0.5, -1.0, -2.0], dtype=torch.float64)[torch.randint(0, 6, (m, n), generator=g)]
    return d


def bias_for(d, out_dtype):
    """odd multiples of 2^-6 (bf16 outputs) / 2^-9 (f16 outputs): almost every output of magnitude >= 4 is then inexact in the output
    type, ties included; integers for fp32 outputs"""
    if out_dtype == F32:
        return d["ibias"]
    return d["odd"] * (2.0 ** -6 if out_dtype == BF16 else 2.0 ** -9)


def exact_ref(d, out_dtype, alpha=0.5, bias=True, rowscale=True, residual=False, beta=0.0, rows=None, cols=None):
    """float64 reference ((alpha * a b^T + bias) * rowscale + residual + beta * old C) over the first `rows` x `cols` window"""
    m, n = d["prod"].shape
    rows, cols = (m if rows is None else rows), (n if cols is None else cols)
    v = alpha * d["prod"][:rows, :cols]
    if bias:
        v = v + bias_for(d, out_dtype)[:cols]
    if rowscale:
        v = v * d["rs"][:rows, None]
    if residual:
        v = v + d["res"][:rows, :cols]
    if beta != 0.0:
        v = v + beta * d["cold"][:rows, :cols]
    return v


def rounded_share(ref, out_dtype):
    return (ref.to(F32).to(out_dtype).double() != ref).double().mean().item()


def check_preconditions(ref, out_dtype, k, fractional=True):
    """what makes the bit comparison meaningful: the reference is exact in fp32 (so a 16-bit output is ONE rounding of it), inside the
    f16 range, and - for 16-bit outputs of a fractional bias with K >= 128 - at least a quarter of the entries really round"""
    assert torch.equal(ref.to(F32).double(), ref), "reference is not exact in fp32"
    if out_dtype == F16:
        assert ref.abs().max().item() < 60000
    if out_dtype in HALF and fractional and k >= 128:
        share = rounded_share(ref, out_dtype)
        assert share >= 0.25, ("rounded share", share)


# ---------------------------------------------------------------------------------------------------------------------------
# GELU operand sets (bf16 table of the one-pass epilogue)
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gelu_operands(kind, m, n, k):
    """-> a (m, k), b (n, k), bias (n), pre (m, n) float64.  'table': rows of at most 7 non-zeros of +-1 against b in [-2, 2] and bias 0.5 -
    every pre-activation a non-zero half-integer with 0.5 <= |x| <= 14.5, so every wave chunk takes the table.  'fallback': integer
    pre-activations, zeros and |x| >= 16 among them - every chunk takes the arithmetic.  'mixed': the table set's rows alternating with
    dense rows under the same bias, so that one chunk (two tile rows) holds both and in-range values go through the arithmetic."""
    g = _gen(m, n, k, GELU_SETS.index(kind))

    def sparse():
        a = torch.zeros(m, k, dtype=torch.float64)
        idx = torch.randint(0, k, (m, 7), generator=g)               # (repeats allowed: at most 7 non-zeros)
        a.scatter_(1, idx, _ints(g, 0, 1, m, 7) * 2 - 1)
        return a
    if kind == "table":
        a, b, bias = sparse(), _ints(g, -2, 2, n, k), torch.full((n,), 0.5, dtype=torch.float64)
    elif kind == "fallback":
        a, b, bias = _ints(g, -3, 3, m, k), _ints(g, -3, 3, n, k), torch.zeros(n, dtype=torch.float64)
    else:
        a, b, bias = sparse(), _ints(g, -2, 2, n, k), torch.full((n,), 0.5, dtype=torch.float64)
        a[1::2] = _ints(g, -3, 3, m, k)[1::2]
    return a, b, bias, a @ b.t() + bias


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x * 0.5 ** 0.5)) + x * torch.exp(-0.5 * x * x) * (2.0 * torch.pi) ** -0.5


def gelu_bound_ratio(got, ref64, x64, out_dtype, scale=None):
    """worst |got - ref| / (u |ref| + floor) and its position; floor = 2 * 8e-7 * max(1, |x|) (times |scale|: the error of gelu' in a
    GELU' product value * gelu'(x) is multiplied by |value|).  u |ref| is the output rounding, so below the type's smallest normal number
    (f16: 2^-14, reached by those products) it stays at u * 2^-14 = half the subnormal spacing."""
    floor = GELU_FLOOR * x64.abs().clamp_min(1.0)
    if scale is not None:
        floor = floor * scale.abs()
    ratio = (got.double() - ref64).abs() / (UNIT[out_dtype] * ref64.abs().clamp_min(MIN_NORMAL[out_dtype]) + floor)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    pos = int(ratio.argmax())
    return ratio.flatten()[pos].item(), (pos // ratio.shape[1], pos % ratio.shape[1])


def check_gelu_bound(got, ref64, x64, out_dtype, what, scale=None):
    worst, (r, c) = gelu_bound_ratio(got, ref64, x64, out_dtype, scale)
    print("%s: worst element %.3f of its bound at (%d, %d), x = %r" % (what, worst, r, c, x64[r, c].item()))
    assert worst <= 1.0, "%s: |got - ref| is %.3f of the bound at %s, x = %r, got %r, ref %r" % (
        what, worst, tile_of(r, c), x64[r, c].item(), got[r, c].item(), ref64[r, c].item())
    return worst


def check_erff_bound(got, ref64, what):
    """the fp32 kernel and the split mode evaluate GELU with erff: per element 1e-6 * max(1, |ref|)"""
    ratio = (got.double() - ref64).abs() / (1e-6 * ref64.abs().clamp_min(1.0))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    pos = int(ratio.argmax())
    r, c = pos // ratio.shape[1], pos % ratio.shape[1]
    assert ratio[r, c].item() <= 1.0, "%s: %.3f of the bound at %s, got %r, ref %r" % (what, ratio[r, c].item(), tile_of(r, c),
                                                                                    got[r, c].item(), ref64[r, c].item())


# ---------------------------------------------------------------------------------------------------------------------------
# pair operands of the split mode
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_operands(m, n, k):
    """x = s + t * 2^-13, s = +-1, t in {-1, 0, 1}: hi = half(x) = s and lo = half(x - hi) = t * 2^-13, built directly.  The reference is
    hi.hi + hi.lo + lo.hi in float64 (the kernel drops lo.lo by design)."""
    g = _gen(m, n, k, 13)
    d = {}
    for name, rows in (("a", m), ("b", n)):
        d[name + "_hi"] = _ints(g, 0, 1, rows, k) * 2 - 1
        d[name + "_lo"] = _ints(g, -1, 1, rows, k) * 2.0 ** -13
    d["prod"] = d["a_hi"] @ d["b_hi"].t() + d["a_hi"] @ d["b_lo"].t() + d["a_lo"] @ d["b_hi"].t()
    d["rs"] = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (m,), generator=g)]
    d["ibias"] = _ints(g, -4, 4, n)
    d["res"] = _ints(g, -64, 64, m, n)
    return d


def pair_of(ref):
    """the pair a split-mode product leaves for the exactly known value ref: half(ref), half(ref - half(ref))"""
    hi = ref.to(F32).to(F16)
    return hi, (ref - hi.double()).to(F32).to(F16)


# ---------------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------------
def padded(x2d, dtype, device, pad=PAD):
    """-> (buffer, ld, element offset of the window): x2d inside GUARD rows above and below and `pad` columns behind, all NaN"""
    rows, cols = x2d.shape
    buf = torch.full((rows + 2 * GUARD, cols + pad), NAN, dtype=dtype)
    buf[GUARD:GUARD + rows, :cols] = x2d.to(dtype)
    return buf.to(device), cols + pad, GUARD * (cols + pad)


def out_buffer(m, n, dtype, device, pad=PAD, old=None):
    """a NaN-filled output with guard rows and `pad` guard columns; old: the M x N window's previous contents (beta != 0)"""
    return padded(torch.full((m, n), NAN, dtype=torch.float64) if old is None else old, dtype, device, pad)


def window(buf, m, n):
    return buf[GUARD:GUARD + m, :n]


def tile_of(r, c):
    return ("row %d col %d: 16-row fragment %d, 128x128 tile (%d, %d), 256x128 tile (%d, %d), 208x256 tile (%d, %d), 256x256 tile (%d, %d)"
            % (r, c, r // 16, r // 128, c // 128, r // 256, c // 128, r // 208, c // 256, r // 256, c // 256))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def check_exact(got_buffer, ref, m, n, what=""):
    """The M x N window of the buffer equals the float64 reference rounded once to the buffer's type, bit for bit (+0 / -0 count as
    equal only where the reference is 0), and every guard element is still NaN."""
    buf = got_buffer.detach().cpu()
    assert buf.shape[0] == m + 2 * GUARD and buf.shape[1] >= n and tuple(ref.shape) == (m, n), (what, buf.shape, ref.shape, m, n)
    win = window(buf, m, n)
    want = ref.to(F32).to(buf.dtype)
    bad = _bits(win) != _bits(want)
    bad &= ~((ref == 0) & (win == 0))
    if bad.any():
        pos = bad.flatten().nonzero()[0].item()
        r, c = pos // n, pos % n
        mask = 0xFFFFFFFF if buf.dtype == F32 else 0xFFFF
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r (0x%x), want %r (0x%x)" % (
            what, int(bad.sum()), m * n, tile_of(r, c), win[r, c].item(), _bits(win)[r, c].item() & mask,
            want[r, c].item(), _bits(want)[r, c].item() & mask))
    check_guards(buf, m, n, what)


def check_guards(buf, m, n, what=""):
    buf = buf.detach().cpu()
    touched = ~torch.isnan(buf)
    touched[GUARD:GUARD + m, :n] = False
    if touched.any():
        pos = touched.flatten().nonzero()[0].item()
        r, c = pos // buf.shape[1] - GUARD, pos % buf.shape[1]
        raise AssertionError("%s: %d guard elements were written; first at window row %d col %d (window %d x %d): %s" % (
            what, int(touched.sum()), r, c, m, n, tile_of(max(r, 0), c)))


def check_untouched(buf, what=""):
    assert bool(torch.isnan(buf.detach().cpu()).all()), what + ": a refused call wrote to C"
