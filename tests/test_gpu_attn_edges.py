"""Fused 16-bit attention (csrc/attention_bf16.hip) per row at its dispatch, tile and mask edges, against the float64 reference and
the per-element bounds of attn_edge_helpers.py.  One test function per dispatch family, so that a single family can be rerun alone:
short non-FULL, FULL, 26 / 38 tiles, long (chunked), packed, masked - plus the column-sum form of the backward.

Every case: forward through the raw entry point into guarded buffers (out, lse, probabilities with ldp = roundup4(T) and + 8 where
the form has them), the backward from the reference's own out / lse into guarded buffers (dqkv, delta workspace), both twice
(same bits), and every sample alone through ops.attention_fwd / ops.attention_bwd (same bits as inside the batch)."""
import pytest
import torch

import attn_edge_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = H.GUARD


@pytest.fixture(scope="module")
def ops():
    from editor_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------------------------------------------------------
def _guard16(rows, cols, dtype):
    big = torch.full((rows + 2 * G, cols), H.SENT16, dtype=torch.int16, device=DEV)
    return big, big[G:G + rows].view(dtype)


def _guard32(n):
    big = torch.full((n + 2 * G,), H.SENT32, dtype=torch.int32, device=DEV)
    return big, big[G:G + n].view(torch.float32)


def _intact16(big, rows, outside, what):
    """Guard rows before and behind the slice, and the slice's rows outside every sequence, still hold the sentinel."""
    h = big.cpu()
    assert bool((h[:G] == H.SENT16).all()), what + ": guard rows before the buffer were written"
    assert bool((h[G + rows:] == H.SENT16).all()), what + ": guard rows behind the buffer were written"
    assert bool((h[G:G + rows][outside] == H.SENT16).all()), what + ": rows outside every sequence were written"


def _intact32(big, n, what, heads=None, outside=None):
    h = big.cpu()
    assert bool((h[:G] == H.SENT32).all()), what + ": guard elements before the buffer were written"
    assert bool((h[G + n:] == H.SENT32).all()), what + ": guard elements behind the buffer were written"
    if outside is not None:
        assert bool((h[G:G + n].view(heads, -1)[:, outside] == H.SENT32).all()), what + ": entries of rows outside every sequence were written"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# one launch: forward, backward, guards, exact checks
# ---------------------------------------------------------------------------------------------------------------------------
def _run_launch(ops, case, op, ref, form, what):
    sfx = "f16" if op.dtype == H.F16 else "bf16"
    heads, hd, rows, t = op.heads, op.hd, op.rows, case.T
    d = heads * hd
    nb = len(op.seqs)
    packed, masked = case.form == "packed", case.form == "masked"
    disp = H.dispatch(hd, t, masked, packed)
    qkv = op.qkv.to(DEV)[:rows]
    do = op.do.to(DEV)
    mask = H.mask_of(op).to(DEV) if masked else None
    cu = H.cu_of(op).to(DEV) if packed else None
    outside = ref.row_seq < 0
    dead = torch.isinf(ref.lse) & ~outside[None, :]                       # (heads, rows): masked queries / rows without a valid key

    # ---- forward, twice: with the two probability strides where the form has the output, else plainly -----------------------
    r4 = (t + 3) // 4 * 4
    ldps = (0, 0) if (disp.long or packed) else (r4, r4 + 8)
    first = None
    for ldp in ldps:
        out_big, out = _guard16(rows, d, op.dtype)
        lse_big, lse = _guard32(heads * rows)
        probs_big = probs = None
        if ldp:
            probs_big, probs = _guard32(nb * heads * t * ldp)
        ops.call("editor_attention_fwd_" + sfx, qkv, nb, t, heads, hd, op.scale, mask, out, probs, ldp, lse, cu, rows)
        torch.cuda.synchronize()
        tag = "%s fwd ldp %d" % (what, ldp)
        _intact16(out_big, rows, outside, tag + " out")
        _intact32(lse_big, heads * rows, tag + " lse", heads, outside)
        got_out, got_lse = out.cpu(), lse.cpu().view(heads, rows)
        got_p = None
        if ldp:
            _intact32(probs_big, nb * heads * t * ldp, tag + " probs")
            got_p = probs.cpu().view(nb, heads, t, ldp)
            pad = got_p[..., t:]
            assert bool(((_bits(pad) == H.SENT32) | (pad == 0)).all()), tag + ": probability padding holds neither the sentinel nor 0"
        res = H.check(op, ref, out=got_out, lse=got_lse, probs=got_p)
        H.record(form, res)
        H.assert_ok(res, tag)
        assert bool((_bits(got_out).view(rows, heads, hd)[dead.t()] == 0).all()), tag + ": output bits of a masked query row"
        if first is None:
            first = (out, lse)
        else:
            assert torch.equal(_bits(out), _bits(first[0])) and torch.equal(_bits(lse), _bits(first[1])), tag + ": not deterministic"
    out, lse = first

    # ---- backward from the reference's out / lse, twice ------------------------------------------------------------------------
    out_in, lse_in = ref.out16.to(DEV), ref.lse32.contiguous().to(DEV)
    firstb = None
    for rep in range(2):
        dq_big, dqkv = _guard16(rows, 3 * d, op.dtype)
        ws_big, ws = _guard32(heads * rows)
        ops.call("editor_attention_bwd_" + sfx, qkv, do, out_in, lse_in, nb, t, heads, hd, op.scale, mask, dqkv, ws, cu, rows)
        torch.cuda.synchronize()
        tag = what + " bwd"
        _intact16(dq_big, rows, outside, tag + " dqkv")
        _intact32(ws_big, heads * rows, tag + " workspace", heads, outside)
        if firstb is None:
            res = H.check(op, ref, dqkv=dqkv.cpu(), delta=ws.cpu().view(heads, rows))
            H.record(form, res)
            H.assert_ok(res, tag)
            firstb = dqkv
        else:
            assert torch.equal(_bits(dqkv), _bits(firstb)), tag + ": not deterministic"
    dqkv = firstb

    # ---- every sample alone gives the bits it has inside the batch -----------------------------------------------------------
    lse2 = lse.view(heads, rows)
    for b, (row0, n, _) in enumerate(op.seqs):
        sl = slice(row0, row0 + n)
        m1 = mask[b:b + 1] if masked else None
        cu1 = torch.tensor([0, n], dtype=torch.int32, device=DEV) if packed else None
        o1, l1 = ops.attention_fwd(qkv[sl], 1, t, heads, hd, m1, None, cu=cu1)
        tag = "%s sample %d alone" % (what, b)
        assert torch.equal(_bits(o1), _bits(out[sl])), tag + ": forward output differs from the batch's"
        assert torch.equal(_bits(l1.view(heads, n)), _bits(lse2[:, sl])), tag + ": lse differs from the batch's"
        g1 = ops.attention_bwd(qkv[sl], do[sl], 1, t, heads, hd, m1, lse_in[:, sl].contiguous().flatten(), out_in[sl], cu=cu1)
        assert torch.equal(_bits(g1), _bits(dqkv[sl])), tag + ": dqkv differs from the batch's"


def _run_case(ops, case, dtype):
    form = H.family(case)
    nbatch = len(H.mask_batches(case.T)) if case.form == "masked" else 1
    for recipe in H.RECIPES:
        for batch in range(nbatch):
            op = H.case_operands(case, dtype, recipe, batch)
            ref = H.case_reference(case, dtype, recipe, batch)
            _run_launch(ops, case, op, ref, form, "%s %s %s launch %d" % (H.case_id(case), str(dtype)[6:], recipe, batch))


def _family(name):
    cs = [c for c in H.all_cases() if H.family(c) == name]
    return pytest.mark.parametrize("case", cs, ids=[H.case_id(c) for c in cs])


_dtypes = pytest.mark.parametrize("dtype", H.DTYPES, ids=["bf16", "f16"])


@_dtypes
@_family("short")
def test_short_forms(ops, case, dtype):
    """10- and 14-tile kernels with a run-time tile count (T < 129, 161..192): scores in registers, rolled loops."""
    _run_case(ops, case, dtype)


@_dtypes
@_family("full")
def test_full_forms(ops, case, dtype):
    """The unrolled dense forms (T = 129..160, 193..224): compile-time trip counts, validity checked on the last tile pair only."""
    _run_case(ops, case, dtype)


@_dtypes
@_family("tiles26_38")
def test_26_and_38_tile_forms(ops, case, dtype):
    """225..416 and 417..608 tokens: the streaming two-sweep forward; 608 tokens of 64-wide heads leave no LDS for staged stores."""
    _run_case(ops, case, dtype)


@_dtypes
@_family("long")
def test_long_forms(ops, case, dtype):
    """Beyond 608 tokens (416 at hd = 96): 64 own rows per workgroup, 256-row chunks; 640 / 641 and 768 / 769 straddle both."""
    _run_case(ops, case, dtype)


@_dtypes
@_family("packed")
def test_packed_forms(ops, case, dtype):
    """Variable-length sequences behind one another: a sequence's neighbours are its first invalid keys; pad rows stay untouched."""
    _run_case(ops, case, dtype)


@_dtypes
@_family("masked")
def test_masked_forms(ops, case, dtype):
    """Dense-masked form, one pattern per sample: the three-word key bitmap, dead key tiles, masked queries (+inf, exact zeros)."""
    _run_case(ops, case, dtype)


FAMILY_TESTS = {"short": test_short_forms, "full": test_full_forms, "tiles26_38": test_26_and_38_tile_forms,
                "long": test_long_forms, "packed": test_packed_forms, "masked": test_masked_forms}


# ---------------------------------------------------------------------------------------------------------------------------
# column sums from the backward's accumulators
# ---------------------------------------------------------------------------------------------------------------------------
COLSUM_CASES = ([H.Case("dense", hd, t, None) for hd in (64, 32, 96) for t in H.COLSUM_DENSE_T[hd]]
                + [H.Case("masked", hd, t, None) for hd in (64, 32, 96) for t in H.COLSUM_MASKED_T[hd]])


@_dtypes
@pytest.mark.parametrize("case", COLSUM_CASES, ids=[H.case_id(c) for c in COLSUM_CASES])
def test_colsum_form(ops, case, dtype):
    """attention_bwd(colsum=...) at the tile-count edges and on the masked 14- / 38-tile forms (10-tile at hd = 96, the only one it
    has): the dqkv bits of the plain backward, and column sums that are the sums of the fp32 values the stored entries were rounded
    from (the rule of test_gpu_kernels._colsum_case)."""
    masked = case.form == "masked"
    op = H.case_operands(case, dtype, "peaked", 0)
    ref = H.case_reference(case, dtype, "peaked", 0)
    heads, hd, t, nb = op.heads, op.hd, case.T, len(op.seqs)
    qkv, do = op.qkv.to(DEV)[:op.rows], op.do.to(DEV)
    mask = H.mask_of(op).to(DEV) if masked else None
    out_in, lse_in = ref.out16.to(DEV), ref.lse32.contiguous().to(DEV).flatten()
    assert ops.attention_bwd_colsum_ok(qkv, t, hd)
    plain = ops.attention_bwd(qkv, do, nb, t, heads, hd, mask, lse_in, out_in)
    cs = torch.full((3 * heads * hd,), float("nan"), device=DEV)
    got = ops.attention_bwd(qkv, do, nb, t, heads, hd, mask, lse_in, out_in, colsum=cs, colsum_scale=0.5)
    assert torch.equal(_bits(got), _bits(plain))
    H.assert_ok(H.check(op, ref, dqkv=plain.cpu()), H.case_id(case))
    stored = plain.double()
    want = stored.sum(0)
    eps = H.unit(dtype)
    bound = stored.abs().sum(0) * (0.5 * eps + 4e-6) + 1e-6               # every entry within half an ulp of its fp32 value
    err = (cs.double() * 2.0 - want).abs()
    assert bool(torch.isfinite(cs).all())
    assert bool((err <= bound).all()), (float((err / bound).max()), H.case_id(case))
    assert float(err.mean() / stored.abs().sum(0).mean()) < 0.1 * eps         # sums of the unrounded values, not garbage that fits
    cs2 = torch.empty_like(cs)
    ops.attention_bwd(qkv, do, nb, t, heads, hd, mask, lse_in, out_in, colsum=cs2, colsum_scale=0.5)
    assert torch.equal(cs, cs2)


def test_colsum_is_refused_where_it_is_not_built(ops):
    x = torch.empty(1, 3 * 2 * 96, dtype=H.BF16, device=DEV)
    assert ops.attention_bwd_colsum_ok(x, 160, 96) and not ops.attention_bwd_colsum_ok(x, 161, 96)
    assert ops.attention_bwd_colsum_ok(x, 608, 64) and not ops.attention_bwd_colsum_ok(x, 609, 64)
