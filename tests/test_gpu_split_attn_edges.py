"""Split-precision attention (csrc/attention_split.hip) per row at its dispatch, chunk and mask edges, against the float64 reference
and the per-element bounds of split_attn_edge_helpers.py.  One test function per form, so that a single one can be rerun alone:
reg10, reg14, whole, chunked, packed, masked - and the rollout step.

Every forward launch: the raw entry point into guarded buffers (out_hi, out_lo, lse; dense and masked launches: probabilities with
ldp = roundup4(T) and + 8), twice (same bits), and every sample alone through ops.attention_fwd_split (the bits it has inside the
batch).  Every rollout launch: lse from the reference, r_in NULL or a positive random vector, both output layouts, once with +inf
on the rows of a mask pattern, into a guarded buffer, twice."""
import pytest
import torch

import split_attn_edge_helpers as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = S.GUARD
FWD, ROLL = "editor_attention_fwd_f16x2", "editor_attn_rollout_step_f16x2"


@pytest.fixture(scope="module")
def ops():
    from editor_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------------------------------------------------------
def _guard16(rows, cols):
    big = torch.full((rows + 2 * G, cols), S.SENT16, dtype=torch.int16, device=DEV)
    return big, big[G:G + rows].view(torch.float16)


def _guard32(n):
    big = torch.full((n + 2 * G,), S.SENT32, dtype=torch.int32, device=DEV)
    return big, big[G:G + n].view(torch.float32)


def _intact16(big, rows, outside, what):
    """Guard rows before and behind the slice, and the slice's rows outside every sequence, still hold the sentinel."""
    h = big.cpu()
    assert bool((h[:G] == S.SENT16).all()), what + ": guard rows before the buffer were written"
    assert bool((h[G + rows:] == S.SENT16).all()), what + ": guard rows behind the buffer were written"
    assert bool((h[G:G + rows][outside] == S.SENT16).all()), what + ": rows outside every sequence were written"


def _intact32(big, n, what, heads=None, outside=None):
    h = big.cpu()
    assert bool((h[:G] == S.SENT32).all()), what + ": guard elements before the buffer were written"
    assert bool((h[G + n:] == S.SENT32).all()), what + ": guard elements behind the buffer were written"
    if outside is not None:
        assert bool((h[G:G + n].view(heads, -1)[:, outside] == S.SENT32).all()), what + ": entries of rows outside every sequence were written"


def _untouched(big, what):
    assert bool((big.cpu() == (S.SENT16 if big.dtype == torch.int16 else S.SENT32)).all()), what + ": a refused call wrote"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# one forward launch
# ---------------------------------------------------------------------------------------------------------------------------
def _run_launch(ops, case, op, ref, form, what):
    heads, hd, rows, t = op.heads, op.hd, op.rows, case.T
    d = heads * hd
    nb = len(op.seqs)
    packed, masked = case.form == "packed", case.form == "masked"
    hi, lo = op.hi.to(DEV)[:rows], op.lo.to(DEV)[:rows]
    mask = S.mask_of(op).to(DEV) if masked else None
    cu = S.cu_of(op).to(DEV) if packed else None
    outside = ref.row_seq < 0
    dead = torch.isinf(ref.lse) & ~outside[None, :]                       # (heads, rows): masked queries / rows without a valid key

    r4 = (t + 3) // 4 * 4
    first = None
    for ldp in ((0, 0) if packed else (r4, r4 + 8)):
        hi_big, out_hi = _guard16(rows, d)
        lo_big, out_lo = _guard16(rows, d)
        lse_big, lse = _guard32(heads * rows)
        probs_big = probs = None
        if ldp:
            probs_big, probs = _guard32(nb * heads * t * ldp)
        ops.call(FWD, hi, lo, nb, t, heads, hd, op.scale, mask, out_hi, out_lo, probs, ldp, lse, cu, rows)
        torch.cuda.synchronize()
        tag = "%s %s ldp %d" % (form, what, ldp)
        _intact16(hi_big, rows, outside, tag + " out_hi")
        _intact16(lo_big, rows, outside, tag + " out_lo")
        _intact32(lse_big, heads * rows, tag + " lse", heads, outside)
        got_hi, got_lo, got_lse = out_hi.cpu(), out_lo.cpu(), lse.cpu().view(heads, rows)
        got_p = None
        if ldp:
            _intact32(probs_big, nb * heads * t * ldp, tag + " probs")
            got_p = probs.cpu().view(nb, heads, t, ldp)
            pad = got_p[..., t:]
            assert bool(((_bits(pad) == S.SENT32) | (pad == 0)).all()), tag + ": probability padding holds neither the sentinel nor 0"
        res = S.check(op, ref, out=got_hi.double() + got_lo.double(), lse=got_lse, probs=got_p)
        S.record("f16x2 " + form, res)
        S.assert_ok(res, tag)
        for half, name in ((got_hi, "hi"), (got_lo, "lo")):
            assert bool((half.view(rows, heads, hd)[dead.t()] == 0).all()), tag + ": %s half of a masked query row is not zero" % name
        if first is None:
            first = (out_hi, out_lo, lse)
        else:
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((out_hi, out_lo, lse), first)), tag + ": not deterministic"
    out_hi, out_lo, lse = first

    # ---- every sample alone gives the bits it has inside the batch -----------------------------------------------------------
    lse2 = lse.view(heads, rows)
    for b, (row0, n, _) in enumerate(op.seqs):
        sl = slice(row0, row0 + n)
        m1 = mask[b:b + 1] if masked else None
        cu1 = torch.tensor([0, n], dtype=torch.int32, device=DEV) if packed else None
        (h1, l1), s1 = ops.attention_fwd_split((hi[sl], lo[sl]), 1, t, heads, hd, m1, None, cu=cu1)
        tag = "%s %s sample %d alone" % (form, what, b)
        assert torch.equal(_bits(h1), _bits(out_hi[sl])) and torch.equal(_bits(l1), _bits(out_lo[sl])), tag + ": output differs from the batch's"
        assert torch.equal(_bits(s1.view(heads, n)), _bits(lse2[:, sl])), tag + ": lse differs from the batch's"


def _run_case(ops, case):
    form = S.family(case)
    for recipe in S.RECIPES:
        for batch in range(S.launches(case)):
            op = S.case_operands(case, recipe, batch)
            ref = S.case_reference(case, recipe, batch)
            _run_launch(ops, case, op, ref, form, "%s %s launch %d" % (S.case_id(case), recipe, batch))


def _family(name):
    cs = [c for c in S.forward_cases() + S.rollout_cases() if S.family(c) == name]
    return pytest.mark.parametrize("case", cs, ids=[S.case_id(c) for c in cs])


@_family("reg10")
def test_reg10_form(ops, case):
    """T <= 160: the scores of a 16-query tile in registers, ten key tiles, a run-time count of populated ones."""
    _run_case(ops, case)


@_family("reg14")
def test_reg14_form(ops, case):
    """161 .. 224 tokens at hd = 32 / 64: fourteen key tiles in registers."""
    _run_case(ops, case)


@_family("whole")
def test_whole_form(ops, case):
    """The whole sequence in LDS, two sweeps: 225 .. 288 tokens at hd = 32 / 64, 161 .. 192 at hd = 96."""
    _run_case(ops, case)


@_family("chunked")
def test_chunked_form(ops, case):
    """64-query workgroups that stream 128-key chunks twice: last chunks of one key, last query blocks of one query."""
    _run_case(ops, case)


@_family("packed")
def test_packed_form(ops, case):
    """Variable-length sequences behind one another, the form chosen from the longest: a sequence's neighbours are its first invalid
    keys; pad rows stay untouched."""
    _run_case(ops, case)


@_family("masked")
def test_masked_form(ops, case):
    """Dense-masked launches of every form, one pattern per sample: dead key tiles, masked queries (+inf, exact zeros in both halves)."""
    _run_case(ops, case)


def test_forward_refusals(ops):
    """Probabilities with cu, cu with a mask, ldp < T, ldp % 4, T = 0: an error, and nothing written."""
    hd, heads, t, nb = 64, 3, 33, 2
    d = heads * hd
    rows = 128
    hi = torch.zeros(rows, 3 * d, dtype=torch.float16, device=DEV)
    cu = torch.tensor([0, 33, 66], dtype=torch.int32, device=DEV)
    mask = torch.ones(nb, t, dtype=torch.uint8, device=DEV)
    hi_big, out_hi = _guard16(rows, d)
    lo_big, out_lo = _guard16(rows, d)
    lse_big, lse = _guard32(heads * rows)
    probs_big, probs = _guard32(nb * heads * t * 40)
    for what, tt, m, p, ldp, c in (("probabilities with cu", t, None, probs, 36, cu), ("cu with a mask", t, mask, None, 0, cu),
                                   ("ldp < T", t, None, probs, 32, None), ("ldp % 4", t, None, probs, 34, None),
                                   ("T = 0", 0, None, None, 0, None)):
        with pytest.raises(RuntimeError, match=FWD + " failed"):
            ops.call(FWD, hi, hi, nb, tt, heads, hd, hd ** -0.5, m, out_hi, out_lo, p, ldp, lse, c, rows)
        torch.cuda.synchronize()
        for big in (hi_big, lo_big, lse_big, probs_big):
            _untouched(big, what)
    ops.call(FWD, hi, hi, nb, t, heads, hd, hd ** -0.5, None, out_hi, out_lo, probs, 36, lse, None, nb * t)      # the same call, allowed
    torch.cuda.synchronize()
    p = probs[:nb * heads * t * 36].view(-1, 36)[:, :t]
    assert bool((out_hi[:nb * t] == 0).all()) and float((p - 1.0 / t).abs().max()) < 1e-7


# ---------------------------------------------------------------------------------------------------------------------------
# the rollout step
# ---------------------------------------------------------------------------------------------------------------------------
@_family("rollout")
def test_rollout_step(ops, case):
    """r_out[k] = sum_q r_in[q] P[q, k] with P recomputed from the q / k pairs and the given lse: 10 / 14 / 26 / 38 key tiles, both
    thread counts, rows with lse = +inf, r_in NULL (the class-token row), both output layouts."""
    hd, t = case.hd, case.T
    form = "f16x2 rollout"
    for recipe in S.RECIPES:
        op = S.case_operands(case, recipe)
        ref = S.case_reference(case, recipe)
        heads, nb = op.heads, len(op.seqs)
        hi, lo = op.hi.to(DEV)[:op.rows], op.lo.to(DEV)[:op.rows]
        w = S.rollout_weights(op, t)
        w_dev = w.to(DEV).contiguous()
        for dead in (None, S.inf_rows(t)):
            lse = S.rollout_lse(ref, t, dead).contiguous().to(DEV)
            for r_in, r_dev in ((None, None), (w, w_dev)):
                want, base = S.rollout_reference(op, ref, r_in, dead)
                for final in (0, 1):
                    n = t - 1 if final else t
                    first = None
                    for rep in range(2):
                        big, r_out = _guard32(nb * heads * n)
                        ops.call(ROLL, hi, lo, lse, r_dev, nb, t, heads, hd, op.scale, r_out, final)
                        torch.cuda.synchronize()
                        tag = "%s %s inf rows %s r_in %s final %d" % (S.case_id(case), recipe, dead is not None, r_in is not None, final)
                        _intact32(big, nb * heads * n, tag)
                        if first is None:
                            first = r_out
                            got = r_out.cpu().view(nb, heads, n).double()
                            res = S.check_rollout(want[..., final:], base[..., final:], got)
                            S.record(form, res)
                            S.assert_ok(res, tag)
                        else:
                            assert torch.equal(_bits(r_out), _bits(first)), tag + ": not deterministic"


ROLLOUT_REFUSALS = [(hd, t) for hd in S.WIDTHS for t in S.ROLLOUT_REFUSED_T[hd]]


@pytest.mark.parametrize("hd,t", ROLLOUT_REFUSALS)
def test_rollout_refusals(ops, hd, t):
    """One token, more than 608, and 96-wide heads beyond 416 (two 608-row images do not fit the LDS): an error, nothing written."""
    assert S.rollout_dispatch(hd, t).refused
    heads, nb = S.heads_of(hd), 2
    hi = torch.zeros(nb * t, 3 * heads * hd, dtype=torch.float16, device=DEV)
    lse = torch.zeros(heads * nb * t, device=DEV)
    for final in (0, 1):
        big, r_out = _guard32(nb * heads * t)
        with pytest.raises(RuntimeError, match=ROLL + " failed"):
            ops.call(ROLL, hi, hi, lse, None, nb, t, heads, hd, hd ** -0.5, r_out, final)
        torch.cuda.synchronize()
        _untouched(big, "rollout hd %d T %d" % (hd, t))


FAMILY_TESTS = {"reg10": test_reg10_form, "reg14": test_reg14_form, "whole": test_whole_form, "chunked": test_chunked_form,
                "packed": test_packed_form, "masked": test_masked_form, "rollout": test_rollout_step}
