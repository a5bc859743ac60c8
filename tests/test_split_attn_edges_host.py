"""Grounds split_attn_edge_helpers.py on the CPU: the case tables reach both sides of every host switch of csrc/attention_split.hip,
the fp32 restatement of the kernels stays inside the bounds, the measured constants obey the rule they were set by, the designated
keys carry weight in every row, the checker rejects each kind of damage on every case, and the GPU tests walk the whole table."""
import math

import pytest
import torch

import split_attn_edge_helpers as S

FORMS = {64: {"reg10", "reg14", "whole", "chunked"}, 32: {"reg10", "reg14", "whole", "chunked"}, 96: {"reg10", "whole", "chunked"}}


# ---------------------------------------------------------------------------------------------------------------------------
# switch coverage
# ---------------------------------------------------------------------------------------------------------------------------
def test_dispatch_restates_the_lds_limits():
    """Four K / V images: 288 rows of 64-wide heads fit, 224 rows of 96-wide ones do not (so no reg14 there) and the whole form
    ends at 192 tokens; the rollout's two Q images and row vectors: 38 tiles of 96-wide heads do not fit, 26 do."""
    assert [S.split_dispatch(64, t).form for t in (160, 161, 224, 225, 288, 289)] == ["reg10", "reg14", "reg14", "whole", "whole", "chunked"]
    assert [S.split_dispatch(32, t).form for t in (160, 161, 224, 225, 288, 289)] == ["reg10", "reg14", "reg14", "whole", "whole", "chunked"]
    assert [S.split_dispatch(96, t).form for t in (160, 161, 192, 193, 224, 225)] == ["reg10", "whole", "whole", "chunked", "chunked", "chunked"]
    assert 4 * 224 * 192 > S.LDS_MAX >= 4 * 192 * 192 and 4 * 288 * 128 <= S.LDS_MAX
    assert S.split_dispatch(64, 385) == ("chunked", 256, 26, 4, 7, 2) and S.split_dispatch(64, 384) == ("chunked", 256, 24, 3, 6, 8)
    assert S.split_dispatch(64, 144).threads == 192 and S.split_dispatch(64, 145).threads == 256
    assert [S.rollout_dispatch(64, t).nt for t in (2, 160, 161, 224, 225, 416, 417, 608)] == [10, 10, 14, 14, 26, 26, 38, 38]
    assert S.rollout_dispatch(96, 416).nt == 26 and S.rollout_dispatch(96, 417).refused and not S.rollout_dispatch(32, 608).refused
    assert all(S.rollout_dispatch(hd, t).refused for hd in S.WIDTHS for t in (0, 1, 609))
    # row strides: 16-byte accesses stay aligned with the head counts used
    assert all((3 * S.heads_of(hd) * hd) % 8 == 0 and (S.heads_of(hd) * hd) % 8 == 0 for hd in S.WIDTHS)


@pytest.mark.parametrize("hd", S.WIDTHS)
def test_tables_are_on_both_sides_of_every_switch(hd):
    ts = S.DENSE_T[hd]
    d = {t: S.split_dispatch(hd, t) for t in ts}
    dm = {t: S.split_dispatch(hd, t, masked=True) for t in S.MASKED_T[hd]}
    dp = [S.split_dispatch(hd, max(lens), packed=True) for lens in S.PACKED_LENS]
    # every form x {dense, masked, packed} the dispatch allows at this width
    assert {x.form for x in d.values()} == FORMS[hd]
    assert {x.form for x in dm.values()} == FORMS[hd]
    assert {x.form for x in dp} == FORMS[hd]
    # the switches themselves, each with both neighbours in the table
    edges = ((160, 161), (192, 193)) if hd == 96 else ((160, 161), (224, 225), (288, 289))
    for a, b in edges:
        assert a in ts and b in ts and d[a].form != d[b].form
    if hd == 96:
        assert d[161].form == d[192].form == "whole" and d[193].form == "chunked"
    # both thread counts in every form that has the choice
    both = list(d.values()) + list(dm.values())
    for form in FORMS[hd] - {"chunked"}:
        assert {x.threads for x in both if x.form == form} == {192, 256}, form
    # tile counts: one token, one key in the second tile, a pair of tiles half populated (odd number of 16-key tiles)
    assert 1 in ts and 17 in ts and any(((t + 15) // 16) % 2 == 1 for t in ts)
    # chunked: last chunk of one key and of 128, last query block of one query and of 64 (the full ones: the 64-wide build)
    ch = [t for t in ts if d[t].form == "chunked"]
    assert any(t % 128 == 1 for t in ch) and any(t % 64 == 1 for t in ch)
    assert len({d[t].chunks for t in ch}) >= 2 and len({d[t].last_chunk_tiles for t in ch}) >= 2
    if hd == 64:
        assert any(t % 128 == 0 for t in ch) and any(t % 64 == 0 for t in ch)
        assert d[384].qblocks + 1 == d[385].qblocks and d[384].chunks + 1 == d[385].chunks and d[385].last_chunk_tiles == 2
    if hd == 96:
        assert 257 in ch and 385 in ch
    # packed: the form is chosen by a sequence longer than most members of the launch, some of which alone would take another form
    for form in FORMS[hd] - {"reg10"}:
        assert any(x.form == form and sum(n < max(lens) for n in lens) * 2 > len(lens)
                   and any(S.split_dispatch(hd, n).form != form for n in lens) for x, lens in zip(dp, S.PACKED_LENS)), form
    # masked launches: the six patterns, deduplicated
    for t in S.MASKED_T[hd]:
        names = [n for ns, _ in S.mask_batches(t) for n in ns]
        assert len(names) == len(set(names)) and (t < 48 or names == list(S.PATTERNS))
    # rollout: every tile count the width has, 192 threads at the larger ones, each refusal
    r = {t: S.rollout_dispatch(hd, t) for t in S.ROLLOUT_T[hd]}
    assert not any(x.refused for x in r.values())
    assert {x.nt for x in r.values()} == ({10, 14, 26, 38} if hd <= 64 else {10, 14, 26})
    assert all(S.rollout_dispatch(hd, t).refused for t in S.ROLLOUT_REFUSED_T[hd])
    assert {1, 609} <= set(S.ROLLOUT_REFUSED_T[hd]) and (hd != 96 or 417 in S.ROLLOUT_REFUSED_T[hd])
    if hd == 64:
        assert {x.nt for x in r.values() if x.threads == 192} >= {10, 26, 38}
        for a, b in ((160, 161), (224, 225), (416, 417)):
            assert r[a].nt != r[b].nt
        assert 608 in r


def test_issue_tables_are_kept():
    """The issue's lengths are all there; the additions are 192 (dense, hd 32 / 64: reg14 with 192 threads) and the fourth packed
    launch (no longer than 160: the packed reg10 form)."""
    assert set(S.DENSE_T[64]) - {192} == {1, 2, 16, 17, 32, 33, 48, 129, 144, 160, 161, 193, 224, 225, 257, 288, 289, 321, 384, 385, 513, 641}
    assert set(S.DENSE_T[32]) - {192} == {1, 17, 129, 160, 161, 224, 225, 288, 289, 385}
    assert S.DENSE_T[96] == (1, 17, 129, 160, 161, 192, 193, 257, 385)
    assert S.MASKED_T == {64: (1, 17, 33, 129, 161, 225, 257, 289, 385), 32: (17, 161, 257, 289), 96: (17, 129, 161, 192, 193)}
    assert S.PACKED_LENS[:3] == ((1, 160, 161, 17, 129, 16), (288, 64, 1, 257, 225), (385, 64, 1, 129, 289))
    assert S.ROLLOUT_T == {64: (2, 17, 129, 160, 161, 224, 225, 416, 417, 608), 32: (2, 160, 161, 416, 417, 608), 96: (2, 129, 161, 225, 416)}


def test_operands_are_the_pair_and_the_reference_reads_the_pair():
    op = S.case_operands(S.Case("packed", 64, 161, S.PACKED_LENS[0]), "designated")
    assert op.hi.dtype == op.lo.dtype == torch.float16 and op.hi.shape == (op.rows + S.TRAIL, 3 * 3 * 64) and op.rows % 64 == 0
    x = op.hi.double() + op.lo.double()
    assert bool((op.lo != 0).any()) and float((op.lo.double().abs() / op.hi.double().abs().clamp_min(1e-30)).max()) <= 2.0 ** -11
    ref = S.reference(op)
    row0, n, _ = op.seqs[2]
    q, k = x[row0 + 5, :64], x[row0:row0 + n, 192:256]
    want = torch.logsumexp((k @ q) * op.scale, 0) * S.LOG2E
    assert abs(float(ref.lse[0, row0 + 5]) - float(want)) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# one sweep over the whole table: restatement against the bounds, the constants, the designated keys, the damage
# ---------------------------------------------------------------------------------------------------------------------------
def _worst_of(res):
    return max(w.ratio for w in res.values())


@pytest.fixture(scope="module")
def sweep():
    worst = dict(out=0.0, lse=0.0, probs=0.0, exp=0.0)
    cond = []
    damage = {}                                           # name -> list of (ratio of the worst section, case id, recipe, launch)

    def note(name, c, recipe, batch, op, ref, **got):
        damage.setdefault(name, []).append((_worst_of(S.check(op, ref, **got)), S.case_id(c), recipe, batch))
    for c in S.forward_cases():
        for recipe in S.RECIPES:
            for batch in range(S.launches(c)):
                op = S.case_operands(c, recipe, batch)
                ref = S.reference(op)
                m = S.restate(op)
                res = S.check(op, ref, out=m["out"], lse=m["lse"], probs=m["probs"])
                worst["out"] = max(worst["out"], res["out"].ratio)
                worst["lse"] = max(worst["lse"], res["lse"].ratio * S.LSE_TOL)
                worst["exp"] = max(worst["exp"], m["exp_err"])
                for p, want in zip(m["probs"], ref.probs):
                    nz = want > 1e-36
                    if bool(nz.any()):
                        worst["probs"] = max(worst["probs"], float(((p - want).abs()[nz] / want[nz]).max()))
                    assert bool((p[want == 0] == 0).all())
                # this family's own damage, on every launch of both recipes
                for name, kw in (("hi_only", dict(hi_only=True)), ("drop_cross", dict(drop_cross=True))):
                    mut = S.reference(op, **kw)
                    note(name, c, recipe, batch, op, ref, out=mut.out, lse=mut.lse, probs=mut.probs)
                note("out_lo_zeroed", c, recipe, batch, op, ref, out=S.half_rounded(ref.out))
                if recipe != "designated":
                    continue
                cond.append((S.case_id(c), batch) + S.designated_condition(op, ref))
                # the 16-bit suite's four, where the damage exists
                nb = len(op.seqs)
                kws = [("drop_last", dict(drop_last=True)), ("leak_next", dict(leak_next=True))]
                if any(bool(live.any()) and any(not live[j] for j in op.designated[b][1]) for b, (_, _, live) in enumerate(op.seqs)):
                    kws.append(("leak_dead", dict(leak_dead=True)))
                if c.form == "masked" and nb > 1:
                    kws.append(("mask_from", dict(mask_from=[(b + 1) % nb for b in range(nb)])))
                for name, kw in kws:
                    mut = S.reference(op, **kw)
                    note(name, c, recipe, batch, op, ref, out=mut.out, lse=mut.lse, probs=mut.probs)
    roll = 0.0
    for c in S.rollout_cases():
        for recipe in S.RECIPES:
            op = S.case_operands(c, recipe)
            ref = S.reference(op)
            for dead in (None, S.inf_rows(c.T)):
                for w in (None, S.rollout_weights(op, c.T)):
                    m = S.restate(op, S.rollout_lse(ref, c.T, dead), w)
                    want, base = S.rollout_reference(op, ref, w, dead)
                    assert bool((m["rollout"][base == 0] == 0).all())
                    roll = max(roll, S.check_rollout(want, base, m["rollout"])["rollout"].ratio * S.ROLL_TOL)
    worst["roll"] = roll
    return worst, cond, damage


def test_restatement_stays_below_half_of_the_out_bound_and_C_is_the_smallest_power_of_two(sweep):
    worst = sweep[0]
    assert worst["out"] < 0.5, worst
    assert 2.0 * worst["out"] >= 0.5, worst                                   # half of C would not hold the margin
    assert math.log2(S.C_BOUND) == round(math.log2(S.C_BOUND))


def test_fp32_constants_are_eight_times_the_restatement_error(sweep):
    """C_EXP (units of 2^-24), LSE_TOL, PROB_TOL, ROLL_TOL: 8 x the restatement's worst error (within the rounding of the constants),
    so the restatement stays below 1/8 of each."""
    worst = sweep[0]
    for name, const in (("exp", S.C_EXP * 2.0 ** -24), ("lse", S.LSE_TOL), ("probs", S.PROB_TOL), ("roll", S.ROLL_TOL)):
        assert 7.5 * worst[name] <= const <= 8.5 * worst[name], (name, worst[name], const)


def test_designated_keys_hold_weight_in_every_live_row(sweep):
    cond = sweep[1]
    assert len(cond) >= len(S.forward_cases())
    for name, batch, lo, hi in cond:
        assert lo >= 0.005 and hi <= 0.7, (name, batch, lo, hi)
    assert any(math.isfinite(hi) for *_, hi in cond)


def test_every_damaged_reference_exceeds_the_bound_on_every_case(sweep):
    damage = sweep[2]
    assert set(damage) == {"hi_only", "drop_cross", "out_lo_zeroed", "drop_last", "leak_next", "leak_dead", "mask_from"}
    nlaunch = sum(S.launches(c) for c in S.forward_cases())
    for name in ("hi_only", "drop_cross", "out_lo_zeroed"):
        assert len(damage[name]) == 2 * nlaunch
    assert len(damage["drop_last"]) == len(damage["leak_next"]) == nlaunch
    assert len(damage["mask_from"]) == sum(S.launches(c) for c in S.masked_cases())
    for name, seen in damage.items():
        low = min(seen)
        print("damage %-14s smallest ratio to the bound %.3g at %s" % (name, low[0], low[1:]))
        assert low[0] > 1.0, (name, low)


def test_checker_rejects_swapped_heads_shifted_lse_and_dirt_in_masked_rows():
    case = S.Case("masked", 64, 161, None)
    for recipe in S.RECIPES:
        op = S.case_operands(case, recipe, 0)
        ref = S.reference(op)
        assert not S.failures(S.check(op, ref, out=ref.out, lse=ref.lse, probs=ref.probs))
        hd = op.hd
        out = ref.out.clone()
        out[:, :hd], out[:, hd:2 * hd] = ref.out[:, hd:2 * hd], ref.out[:, :hd]
        assert S.failures(S.check(op, ref, out=out))
        assert S.failures(S.check(op, ref, lse=torch.roll(ref.lse, 1, 1)))
        # a masked query row (sample 0, class token only: rows 1.. are masked) must be exact: the smallest dirt fails, -0.0 passes
        out = ref.out.clone()
        out[5, 3] = -0.0
        assert not S.failures(S.check(op, ref, out=out))
        out[5, 3] = 1e-30
        w = S.check(op, ref, out=out)["out"]
        assert w.ratio == math.inf and (w.sample, w.head, w.row) == (0, 0, 5)
        lse = ref.lse.clone()
        lse[1, 7] = 1e30                                                       # a masked query's lse must be +inf itself
        w = S.check(op, ref, lse=lse)["lse"]
        assert w.ratio == math.inf and (w.sample, w.head, w.row) == (0, 1, 7)
        probs = [p.clone() for p in ref.probs]
        probs[1][2, 9, 160] *= 1.0 + 3 * S.PROB_TOL
        w = S.check(op, ref, probs=probs)["probs"]
        assert w.ratio > 1 and (w.sample, w.head, w.row) == (1, 2, 9)
    # rollout: a key of another head, and dirt where nothing may arrive
    c = S.Case("rollout", 64, 17, None)
    op = S.case_operands(c, "peaked")
    ref = S.reference(op)
    dead = torch.ones(S.B, 17, dtype=torch.bool)
    dead[:2, 0] = False
    want, base = S.rollout_reference(op, ref, None, dead)
    assert bool((base[2] == 0).all()) and S.check_rollout(want, base, want)["rollout"].ratio == 0
    got = want.clone()
    got[2, 1, 4] = 1e-30
    w = S.check_rollout(want, base, got)["rollout"]
    assert w.ratio == math.inf and (w.sample, w.head, w.row) == (2, 1, 4)
    assert S.check_rollout(want, base, torch.roll(want, 1, 1))["rollout"].ratio > 1


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU tests use the tables
# ---------------------------------------------------------------------------------------------------------------------------
def _params(fn, name):
    for mark in getattr(fn, "pytestmark", []):
        if mark.name == "parametrize" and mark.args[0] == name:
            return list(mark.args[1])
    raise AssertionError("%s is not parametrized over %s" % (fn.__name__, name))


def test_gpu_tests_walk_every_table_entry():
    import test_gpu_split_attn_edges as GT
    assert GT.pytestmark.name == "gpu"
    assert set(GT.FAMILY_TESTS) == {"reg10", "reg14", "whole", "chunked", "packed", "masked", "rollout"}
    seen = []
    for fam, fn in GT.FAMILY_TESTS.items():
        cases = _params(fn, "case")
        assert cases and all(S.family(c) == fam for c in cases)
        seen += cases
    want = S.forward_cases() + S.rollout_cases()
    assert sorted(seen) == sorted(want) and len(set(seen)) == len(seen)
    assert sorted(_params(GT.test_rollout_refusals, "hd,t")) == sorted((hd, t) for hd in S.WIDTHS for t in S.ROLLOUT_REFUSED_T[hd])
