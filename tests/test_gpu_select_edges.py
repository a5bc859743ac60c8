"""The token-selection kernels of csrc/select.hip at branch, launch and tie edges (select_edge_helpers.py), through the C ABI.

Top-k: every case of the shared table - every selector, the depth-limit fallback from both directions and with ties at the k-th
value, rows around a wave, around the four-rows-to-one workgroup switch and at the limit - bit for bit against the oracle, into a
mask the test dirtied beforehand with a guard behind it.  Rollout: every launch geometry, padded rows and gapped layers poisoned
with NaN, against float64 within the bound derived in the helper.  Frequency counts: every instantiation the launcher can take,
the 4x4-pixels-per-lane and the 2x2 form bit for bit against the oracle and against each other.  Every refusal leaves its output
as it was."""
import pytest
import torch

import select_edge_helpers as H
from select_edge_helpers import FREQ_KINDS, ROLLOUT_BH, ROLLOUT_GAP, ROLLOUT_L, cases_for, rollout_ldps

pytestmark = pytest.mark.gpu
DEV = "cuda"
TABLE = H.topk_table()
GUARD = 256
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from editor_amd import ops
    return ops


def guarded(numel, dtype, fill):
    """-> (view of `numel` elements filled with `fill`, whole buffer): GUARD bytes of 0xA5 lie behind the view"""
    es = torch.empty((), dtype=dtype).element_size()
    assert GUARD % es == 0
    buf = torch.empty(numel * es + GUARD, dtype=torch.uint8, device=DEV)
    buf[numel * es:] = H.GUARD_BYTE
    view = buf[:numel * es].view(dtype)
    view.fill_(fill)
    return view, buf


def guard_intact(buf):
    return bool((buf[-GUARD:] == H.GUARD_BYTE).all())


def refused(ops, name, *args):
    with pytest.raises(RuntimeError, match=r"hipError 1$"):
        ops.call(name, *args)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# top-k
# ---------------------------------------------------------------------------------------------------------------------------
def _entry(dtype):
    return "editor_topk_mask_i32" if dtype == H.I32 else "editor_topk_mask_f32"


@pytest.mark.parametrize("n", H.table_n())
def test_topk_table_case_masks_bit_for_bit(ops, oracle, n):
    for c in cases_for(n):
        want = oracle.topk_mask(c.values, c.k).reshape(c.rows // c.group, c.group, n).any(1)
        x = c.values.to(DEV)
        # the entry point clears the mask itself: 0xFF everywhere before the call
        mask, buf = guarded((c.rows // c.group) * n, torch.uint8, 0xFF)
        ops.call(_entry(c.dtype), x, c.rows, n, c.k, c.group, mask)
        got = mask.cpu().view(c.rows // c.group, n)
        assert guard_intact(buf), c.name
        assert torch.equal(got, want.to(torch.uint8)), c.name
        if c.group == 1:
            assert (got.sum(1) == c.k).all(), c.name
        via_ops = ops.topk_mask(x, c.k, group=c.group)
        assert via_ops.dtype == torch.uint8 and torch.equal(via_ops.cpu(), got), c.name


def test_topk_refusals_leave_mask_and_guard_alone(ops):
    for dtype in (H.I32, H.F32):
        for rows, n, k, group in ((4, 128, 0, 1), (4, 128, 129, 1), (2, 4097, 2, 1), (4, 128, 2, 0), (4, 128, 2, 3), (4, 128, -1, 1),
                                  (4, 128, 2, -2)):
            x = torch.ones(rows, n, device=DEV).to(dtype)
            mask, buf = guarded(rows * n, torch.uint8, 0xFF)
            refused(ops, _entry(dtype), x, rows, n, k, group, mask)
            assert bool((mask == 0xFF).all()) and guard_intact(buf), (dtype, rows, n, k, group)
    x = torch.rand(1, 4096, device=DEV)                                        # the limit itself is served
    assert int(ops.topk_mask(x, 4096).sum()) == 4096


# ---------------------------------------------------------------------------------------------------------------------------
# rollout
# ---------------------------------------------------------------------------------------------------------------------------
def _rollout_buffer(probs, layers, bh, ldp, gap):
    """probs (>= layers, >= bh, t, t) on the device -> (flat buffer with NaN in the padding columns [t, ldp) and in the gap behind
    every layer's slab, layer stride in floats)"""
    t = probs.shape[-1]
    slab = bh * t * ldp
    stride = slab + gap
    buf = torch.full((layers * stride,), NAN, device=DEV)
    for l in range(layers):
        buf[l * stride:l * stride + slab].view(bh, t, ldp)[:, :, :t] = probs[l, :bh]
    return buf, stride


@pytest.mark.parametrize("t", H.ROLLOUT_T)
def test_rollout_at_every_launch_geometry(ops, t):
    probs = H.rollout_probs(t)
    refs = {layers: H.rollout_reference(probs, layers) for layers in ROLLOUT_L}
    assert min(float(r.min()) for r in refs.values()) > H.ROLLOUT_MIN_SCORE    # nothing near the denormal range: the bound is relative
    dprobs = probs.to(DEV)
    worst = 0.0
    for layers in ROLLOUT_L:
        for bh in ROLLOUT_BH:
            ref = refs[layers][:bh]
            bound = H.rollout_bound(ref, layers, t)
            for ldp in rollout_ldps(t):
                for gap in ROLLOUT_GAP:
                    buf, stride = _rollout_buffer(dprobs, layers, bh, ldp, gap)
                    assert stride == bh * t * ldp + gap
                    scores, sbuf = guarded(bh * (t - 1), torch.float32, NAN)
                    ops.call("editor_attn_rollout_f32", buf, layers, bh, t, ldp, stride, scores)
                    got = scores.cpu().double().view(bh, t - 1)
                    what = (t, layers, bh, ldp, gap)
                    assert guard_intact(sbuf), what
                    assert torch.isfinite(got).all(), what                     # no padding column, no gap was read
                    err = (got - ref).abs()
                    if layers > 1:
                        worst = max(worst, float((err / bound).max()))
                    assert (err <= bound).all(), (what, float((err / bound).max()))
                    if layers == 1:
                        assert torch.equal(got, ref), what                     # no product: the probabilities themselves
    print("rollout T = %d (threads, G, remainder trips) = %s: worst error / bound %.3f" % (t, H.rollout_geometry(t), worst))


def test_rollout_refusals_leave_scores_alone(ops):
    t = 8
    probs = torch.full((2 * 2 * 1025 * 1025,), 0.125, device=DEV)
    for layers, tt, ldp in ((2, 1, 1), (2, 1025, 1025), (2, t, t - 1), (0, t, t), (-1, t, t), (2, 0, 4)):
        scores, sbuf = guarded(2 * 1025, torch.float32, NAN)
        refused(ops, "editor_attn_rollout_f32", probs, layers, 2, tt, ldp, 2 * tt * ldp, scores)
        assert bool(torch.isnan(scores).all()) and guard_intact(sbuf), (layers, tt, ldp)


# ---------------------------------------------------------------------------------------------------------------------------
# frequency counts
# ---------------------------------------------------------------------------------------------------------------------------
def _place(x, offset):
    """device copy of x whose address is `offset` bytes past a 16-byte boundary"""
    assert offset % 4 == 0
    buf = torch.empty(x.numel() + 4, device=DEV)
    v = buf[offset // 4:offset // 4 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == offset and v.is_contiguous()
    return v


def _freq_call(ops, mods, b, c, h, w, entry="nmod"):
    counts, buf = guarded(H.freq_tiles(b, h, w), torch.int32, -1)
    if entry == "nmod":
        ptrs = list(mods) + [None] * (4 - len(mods))
        ops.call("editor_freq_counts_nmod_f32", *ptrs, len(mods), b, c, h, w, counts)
    else:
        ops.call("editor_freq_counts_f32", mods[0], mods[1], mods[2] if len(mods) > 2 else None, b, c, h, w, counts)
    got = counts.cpu().view(b, -1)
    assert guard_intact(buf)
    return got


@pytest.mark.parametrize("form", H.FREQ_FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("geom", H.FREQ_GEOM, ids=lambda g: "%dx%dx%d" % g)
def test_frequency_counts_every_instantiation(ops, oracle, geom, form):
    b, h, w = geom
    name, c, offset, nmods = form
    for nmod in nmods:
        for kind in FREQ_KINDS:
            mods = H.freq_operands(kind, nmod, c, b, h, w)
            ref = H.freq_reference(oracle, mods)
            what = (H.freq_kernel(nmod, c, offset == 0), geom, kind)
            dm = [_place(m, offset) for m in mods]
            got = _freq_call(ops, dm, b, c, h, w)
            assert torch.equal(got, ref), what
            if nmod <= 3:                                                      # the (rgb, nir, tir) entry point takes the same route
                assert torch.equal(_freq_call(ops, dm, b, c, h, w, "rgb_nir_tir"), ref), what
            if kind in ("zero", "cancel", "nan"):
                assert got[-1, -1] == 0, what


@pytest.mark.parametrize("geom", H.FREQ_GEOM, ids=lambda g: "%dx%dx%d" % g)
@pytest.mark.parametrize("nmod", (3, 4))
def test_frequency_4x4_and_2x2_forms_count_alike(ops, nmod, geom):
    """freq_counts4_kernel<nmod,3> (16-byte aligned images) and freq_counts_kernel<nmod,3> (the same pixels 8 bytes further on)"""
    b, h, w = geom
    for kind in FREQ_KINDS:
        mods = H.freq_operands(kind, nmod, 3, b, h, w)
        aligned = _freq_call(ops, [_place(m, 0) for m in mods], b, 3, h, w)
        shifted = _freq_call(ops, [_place(m, 8) for m in mods], b, 3, h, w)
        assert torch.equal(aligned, shifted), (geom, kind)


def test_frequency_refusals_leave_counts_alone(ops):
    x = torch.zeros(2 * 4 * 48 * 48, device=DEV)
    cases = [("H = 24", (x, x, x, None, 3, 1, 3, 24, 32)), ("W = 40", (x, x, x, None, 3, 1, 3, 32, 40)), ("B = 0", (x, x, x, None, 3, 0, 3, 32, 32)),
             ("C = 0", (x, x, x, None, 3, 1, 0, 32, 32)), ("nmod = 1", (x, None, None, None, 1, 1, 3, 32, 32)),
             ("nmod = 5", (x, x, x, x, 5, 1, 3, 32, 32)), ("null third pointer", (x, x, None, None, 3, 1, 3, 32, 32)),
             ("null fourth pointer", (x, x, x, None, 4, 1, 3, 32, 32))]
    for what, args in cases:
        counts, buf = guarded(16, torch.int32, -1)
        refused(ops, "editor_freq_counts_nmod_f32", *args, counts)
        assert bool((counts == -1).all()) and guard_intact(buf), what
    for what, (bb, cc, hh, ww) in (("H = 24", (1, 3, 24, 32)), ("W = 40", (1, 3, 32, 40)), ("B = 0", (0, 3, 32, 32)), ("C = 0", (1, 0, 32, 32))):
        counts, buf = guarded(16, torch.int32, -1)
        refused(ops, "editor_freq_counts_f32", x, x, x, bb, cc, hh, ww, counts)
        assert bool((counts == -1).all()) and guard_intact(buf), what
