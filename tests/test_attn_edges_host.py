"""Grounds attn_edge_helpers.py on the CPU: the case table reaches both sides of every dispatch switch of csrc/attention_bf16.hip,
the rounding model of the kernels stays inside the bounds, the fp32 constants hold their margin, the designated keys carry weight in
every row, the checker rejects each kind of damage, and the GPU tests walk the whole table."""
import math

import pytest
import torch

import attn_edge_helpers as H

WIDTHS = (32, 64, 96)


# ---------------------------------------------------------------------------------------------------------------------------
# switch coverage
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", WIDTHS)
def test_dense_table_is_on_both_sides_of_every_switch(hd):
    ts = H.DENSE_T[hd]
    d = {t: H.dispatch(hd, t) for t in ts}
    assert {x.nt for x in d.values()} == ({10, 14, 26, 38, 0} if hd <= 64 else {10, 14, 26, 0})
    # the tile-count thresholds themselves
    assert {160, 161, 416, 417} <= set(ts) and (d[160].nt, d[161].nt, d[416].nt, d[417].nt) == (10, 14, 26, 38 if hd <= 64 else 0)
    if hd <= 64:
        assert (d[608].nt, d[609].nt) == (38, 0)
    if hd == 64:
        assert (d[224].nt, d[225].nt) == (14, 26)
        assert not d[128].full and d[129].full and not d[192].full and d[193].full            # FULL begins at 129 and at 193
        assert d[640].qblocks + 1 == d[641].qblocks and d[768].chunks + 1 == d[769].chunks    # 64-row workgroups, 256-row chunks
        assert d[256].nt == d[257].nt == 26 and d[512].nt == d[513].nt == 38
    for nt in (10, 14):                                                                      # unrolled and rolled form of both
        assert {x.full for x in d.values() if x.nt == nt} == {True, False}
    assert not any(x.full for x in d.values() if x.nt not in (10, 14))
    assert {x.threads for x in d.values() if not x.long} == {192, 256}
    assert {x.staged_bwd for x in d.values() if not x.long} == ({True} if hd == 32 else {True, False})
    longs = [x for x in d.values() if x.long]
    assert len({x.chunks for x in longs}) >= 2 and len({x.last_chunk_tiles for x in longs}) >= 2
    assert {x.colsum for x in d.values() if not x.long} == ({True} if hd <= 64 else {True, False})
    assert 1 in ts and 17 in ts                                                              # one token; one key in the second tile


@pytest.mark.parametrize("hd", WIDTHS)
def test_masked_and_packed_tables_reach_every_form(hd):
    d = {t: H.dispatch(hd, t, masked=True) for t in H.MASKED_T[hd]}
    assert {x.nt for x in d.values()} == ({10, 14, 26, 38, 0} if hd <= 64 else {10, 14, 26, 0})      # the masked backward of each
    assert {x.words for x in d.values() if not x.long} == ({1, 2, 3} if hd <= 64 else {1, 2})        # every bitmap word
    assert not any(x.full for x in d.values())
    for t in H.MASKED_T[hd]:
        names = [n for ns, _ in H.mask_batches(t) for n in ns]
        assert len(names) == len(set(names)) and (t < 48 or names == list(H.PATTERNS))
        masks = torch.cat([m for _, m in H.mask_batches(t)])
        assert len({tuple(m.tolist()) for m in masks}) == masks.shape[0]                            # deduplicated
    p = [H.dispatch(hd, max(lens), packed=True) for lens in H.PACKED_LENS]
    assert [(x.nt, x.full) for x in p] == [(14, False), (0, False)]
    assert H.PACKED_LENS == ((1, 160, 161, 17, 129, 16), (609, 64, 1, 257, 256))


def test_dispatch_restatement_agrees_with_the_package():
    from editor_amd import ops
    for hd in WIDTHS:
        x = torch.empty(1, 3 * H.heads_of(hd) * hd, dtype=H.BF16)
        for t in H.DENSE_T[hd]:
            d = H.dispatch(hd, t)
            assert bool(ops.attention_bwd_colsum_ok(x, t, hd)) == (d.colsum and not d.long)
        for t in H.COLSUM_DENSE_T[hd] + H.COLSUM_MASKED_T[hd]:
            assert ops.attention_bwd_colsum_ok(x, t, hd)
        assert set(H.COLSUM_DENSE_T[hd]) <= set(H.DENSE_T[hd]) and set(H.COLSUM_MASKED_T[hd]) <= set(H.MASKED_T[hd])
    assert {H.dispatch(hd, t, masked=True).nt for hd in (32, 64) for t in H.COLSUM_MASKED_T[hd]} == {14, 38}
    # row strides: 16-byte accesses stay aligned with the head counts used
    assert all((3 * H.heads_of(hd) * hd) % 8 == 0 and (H.heads_of(hd) * hd) % 8 == 0 for hd in WIDTHS)


# ---------------------------------------------------------------------------------------------------------------------------
# one sweep over the whole table: rounding model, fp32 constants, designated keys
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    worst16, worst32 = {}, {"lse": 0.0, "delta": 0.0, "probs": 0.0}
    cond = []
    for c in H.all_cases():
        nbatch = len(H.mask_batches(c.T)) if c.form == "masked" else 1
        for dtype in H.DTYPES:
            for recipe in H.RECIPES:
                for batch in range(nbatch):
                    op = H.case_operands(c, dtype, recipe, batch)
                    ref = H.reference(op)
                    if recipe == "designated":
                        cond.append((H.case_id(c), dtype, batch) + H.designated_condition(op, ref))
                    m = H.restate(op, ref, True)
                    for k, w in H.check(op, ref, out=m["out"], dqkv=m["dqkv"]).items():
                        if w.ratio > worst16.get(k, (0.0,))[0]:
                            worst16[k] = (w.ratio, H.case_id(c), dtype, recipe, batch)
                    f = H.restate(op, ref, False)
                    res = H.check(op, ref, lse=f["lse"], delta=f["delta"])
                    worst32["lse"] = max(worst32["lse"], res["lse"].ratio * H.LSE_TOL)
                    worst32["delta"] = max(worst32["delta"], res["delta"].ratio * H.DELTA_TOL)
                    for p, want in zip(f["probs"], ref.probs):
                        nz = want > 1e-36
                        if bool(nz.any()):
                            worst32["probs"] = max(worst32["probs"], float(((p - want).abs()[nz] / want[nz]).max()))
                        assert bool((p[want == 0] == 0).all())
    return worst16, worst32, cond


def test_rounding_model_stays_below_half_of_every_bound(sweep):
    worst16 = sweep[0]
    assert set(worst16) == {"out", "dq", "dk", "dv"}
    assert all(v[0] < 0.5 for v in worst16.values()), worst16
    assert all(v[0] > 0.05 for v in worst16.values()), worst16                 # ... and the bounds are not loose by orders


def test_fp32_constants_hold_their_margin(sweep):
    """LSE_TOL, PROB_TOL and DELTA_TOL are 8 x the fp32 restatement's worst error over the table (within the rounding of the constants)."""
    worst32 = sweep[1]
    for name, const in (("lse", H.LSE_TOL), ("probs", H.PROB_TOL), ("delta", H.DELTA_TOL)):
        assert 7.5 * worst32[name] <= const <= 8.5 * worst32[name], (name, worst32[name], const)


def test_designated_keys_hold_weight_in_every_live_row(sweep):
    cond = sweep[2]
    assert len(cond) >= len(H.all_cases()) * 2
    for name, dtype, batch, lo, hi in cond:
        assert lo >= 0.005 and hi <= 0.7, (name, dtype, batch, lo, hi)
    assert any(math.isfinite(hi) for *_, hi in cond)


# ---------------------------------------------------------------------------------------------------------------------------
# the checker rejects damage
# ---------------------------------------------------------------------------------------------------------------------------
MUT_DENSE = [H.Case("dense", 64, 161, None), H.Case("dense", 32, 609, None), H.Case("dense", 96, 17, None),
             H.Case("packed", 64, 161, H.PACKED_LENS[0])]
MUT_MASKED = [H.Case("masked", 64, 513, None), H.Case("masked", 96, 161, None)]


def _bad(op, ref, mut):
    return {w.section for w in H.failures(H.check(op, ref, out=mut.out, lse=mut.lse, dqkv=mut.dqkv, delta=mut.delta))}


def _every_row_moves(ref, mut):
    """The damaged lse differs from the reference's in EVERY live row: by at least 0.018 (log2 units - a key that held 1.2 % of the
    row), more than 100 x the lse bound (a one-token sequence that lost its key: +inf)."""
    live = torch.isfinite(ref.lse)
    shift = (mut.lse - ref.lse).abs()[live]
    return bool((shift >= 0.018).all()) and bool((shift > 100 * H.LSE_TOL * ref.lse.abs().clamp_min(1.0)[live]).all())


@pytest.mark.parametrize("dtype", H.DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", MUT_DENSE, ids=[H.case_id(c) for c in MUT_DENSE])
def test_checker_rejects_a_dropped_or_leaked_key_in_every_row(case, dtype):
    op = H.case_operands(case, dtype, "designated")
    ref = H.reference(op)
    assert not H.failures(H.check(op, ref, out=ref.out, lse=ref.lse, dqkv=ref.dqkv, delta=ref.delta))
    for kw in (dict(drop_last=True), dict(leak_next=True)):
        mut = H.reference(op, **kw)
        assert {"out", "lse", "dq"} <= _bad(op, ref, mut), kw
        assert _every_row_moves(ref, mut), kw
    # the same damage on the sharp-rowed recipe is still caught (in some rows)
    op2 = H.case_operands(case, dtype, "peaked")
    ref2 = H.reference(op2)
    assert _bad(op2, ref2, H.reference(op2, drop_last=True)) and _bad(op2, ref2, H.reference(op2, leak_next=True))


@pytest.mark.parametrize("dtype", H.DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", MUT_MASKED, ids=[H.case_id(c) for c in MUT_MASKED])
def test_checker_rejects_mask_damage(case, dtype):
    for batch in range(2):
        op = H.case_operands(case, dtype, "designated", batch)
        ref = H.reference(op)
        assert {"out", "lse", "dq"} <= _bad(op, ref, H.reference(op, leak_dead=True)), batch          # one masked key leaked
        assert {"out", "lse"} <= _bad(op, ref, H.reference(op, drop_last=True)), batch
    op = H.case_operands(case, dtype, "designated", 0)
    ref = H.reference(op)
    bad = _bad(op, ref, H.reference(op, mask_from=[0, 0, 2]))                                      # sample 1 under sample 0's mask
    assert {"out", "lse", "dq", "dk", "dv"} <= bad
    w = H.check(op, ref, out=H.reference(op, mask_from=[0, 0, 2]).out)["out"]
    assert w.sample == 1 and w.ratio > 1


@pytest.mark.parametrize("dtype", H.DTYPES, ids=["bf16", "f16"])
def test_checker_rejects_swapped_heads_shifted_lse_and_dirt_in_masked_rows(dtype):
    case = H.Case("masked", 64, 161, None)
    for recipe in H.RECIPES:
        op = H.case_operands(case, dtype, recipe, 0)
        ref = H.reference(op)
        hd = op.hd
        out = ref.out.clone()
        out[:, :hd], out[:, hd:2 * hd] = ref.out[:, hd:2 * hd], ref.out[:, :hd]
        assert H.failures(H.check(op, ref, out=out))
        dq = ref.dqkv.clone()
        dq[:, :hd], dq[:, hd:2 * hd] = ref.dqkv[:, hd:2 * hd], ref.dqkv[:, :hd]
        assert H.failures(H.check(op, ref, dqkv=dq))
        assert H.failures(H.check(op, ref, lse=torch.roll(ref.lse, 1, 1)))
        # a masked query row (sample 0, class token only: rows 1.. are masked) must be exact: the smallest dirt fails, -0.0 passes
        out = ref.out.clone()
        out[5, 3] = -0.0
        assert not H.failures(H.check(op, ref, out=out))
        out[5, 3] = 1e-30
        w = H.check(op, ref, out=out)["out"]
        assert w.ratio == math.inf and (w.sample, w.head, w.row) == (0, 0, 5)
        lse = ref.lse.clone()
        lse[1, 7] = 1e30                                                       # a masked query's lse must be +inf itself
        w = H.check(op, ref, lse=lse)["lse"]
        assert w.ratio == math.inf and (w.sample, w.head, w.row) == (0, 1, 7)
        dq = ref.dqkv.clone()
        dq[9, 3 * op.heads * hd - 1] = float("nan")    # dV of a masked key
        assert H.failures(H.check(op, ref, dqkv=dq))


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU tests use the table
# ---------------------------------------------------------------------------------------------------------------------------
def _params(fn, name):
    for mark in getattr(fn, "pytestmark", []):
        if mark.name == "parametrize" and mark.args[0] == name:
            return list(mark.args[1])
    raise AssertionError("%s is not parametrized over %s" % (fn.__name__, name))


def test_gpu_tests_walk_every_table_entry_with_both_dtypes():
    import test_gpu_attn_edges as GT
    assert GT.pytestmark.name == "gpu"
    seen = []
    for fam, fn in GT.FAMILY_TESTS.items():
        cases = _params(fn, "case")
        assert cases and all(H.family(c) == fam for c in cases)
        assert _params(fn, "dtype") == list(H.DTYPES)
        seen += cases
    assert sorted(seen) == sorted(H.all_cases()) and len(set(seen)) == len(seen)
    assert set(GT.FAMILY_TESTS) == {"short", "full", "tiles26_38", "long", "packed", "masked"}
    cs = _params(GT.test_colsum_form, "case")
    want = [(c.form, c.hd, c.T) for c in cs]
    assert sorted(want) == sorted([("dense", hd, t) for hd in WIDTHS for t in H.COLSUM_DENSE_T[hd]]
                                  + [("masked", hd, t) for hd in WIDTHS for t in H.COLSUM_MASKED_T[hd]])
    assert _params(GT.test_colsum_form, "dtype") == list(H.DTYPES)
