"""The token-selection edge suite's own ground (select_edge_helpers.py), on the CPU: the plain-Python port of topk_mask_kernel's walk
selects what torch.topk and the oracle select on every case of the shared table, the table reaches every path of the walk - asserted
from the statistics the port records - the adversary's rows replay the comparisons they were built from, the rollout reference
and the frequency operands are what the GPU module takes them for, and every table is used by the GPU tests."""
import math

import pytest
import torch

import select_edge_helpers as H

TABLE = H.topk_table()


@pytest.fixture(scope="module")
def walked():
    """{case name: (mask of the port, [Path per row])}, computed once"""
    return {c.name: H.walk_rows(c.values, c.k) for c in TABLE}


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
def test_table_holds_the_listed_shapes_and_value_families():
    plain = [c for c in TABLE if c.group == 1 and not c.name.startswith("adversary")]
    assert sorted({c.n for c in plain}) == list(H.N_VALUES)
    assert H.N_VALUES == (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 210, 1023, 1024, 1025, 4096)
    for n in H.N_VALUES:
        want = {k for k in (1, 2, 3, n // 64, n // 64 + 1, n // 2, n - 1, n) if 1 <= k <= n}
        for fam in H.FAMILIES:
            assert {c.k for c in plain if c.n == n and c.name.startswith(fam)} == want, (n, fam)
        assert {c.rows for c in plain if c.n == n} <= set(H.ROWS)
    assert {c.rows for c in plain} == {1, 3, 5, 7}
    assert {c.rows for c in plain if c.n > 1024} >= {1, 3} and {c.rows for c in plain if c.n <= 1024} >= {1, 3, 5, 7}
    grouped = [c for c in TABLE if c.group > 1]
    assert {(c.rows, c.group, c.n) for c in grouped} == {(r, g, n) for r, g in ((6, 3), (36, 12)) for n in (129, 210, 1025)}
    adv = [c for c in TABLE if c.name.startswith("adversary")]
    assert {c.n for c in adv} == {128, 210, 512, 2048} and {c.dtype for c in adv} == {H.I32, H.F32}
    for c in TABLE:
        assert c.values.shape == (c.rows, c.n) and c.values.dtype == c.dtype and c.dtype in (H.I32, H.F32), c.name
        assert 1 <= c.k <= c.n <= 4096 and c.rows % c.group == 0, c.name
    assert H.topk_table() is TABLE                      # built once: the GPU module sees the same values


def test_value_families_are_what_their_names_say():
    by = lambda fam: [c for c in TABLE if c.name.startswith(fam)]
    assert all(c.dtype == H.I32 and 90 <= int(c.values.min()) and int(c.values.max()) < 110 for c in by("tie_i32"))
    assert all(c.dtype == H.F32 and set(c.values.flatten().tolist()) <= {0.0, 1.0, 2.0, 3.0} for c in by("tie_f32"))
    assert all(torch.unique(c.values).numel() == 1 for c in by("equal")) and {c.dtype for c in by("equal")} == {H.I32, H.F32}
    assert all(c.dtype == H.F32 and torch.unique(c.values).numel() == c.values.numel() for c in by("uniform") if c.n <= 210)
    sp = torch.cat([c.values.flatten() for c in by("special")])
    bits = sp.view(torch.int32)
    assert torch.isnan(sp).any() and (sp == float("inf")).any() and (sp == -float("inf")).any()
    assert (bits == 0).any() and (bits == -(1 << 31)).any()                     # +0.0 and -0.0
    wide = [c for c in by("special") if c.n >= 63]
    assert all(torch.isnan(c.values).any() and torch.isinf(c.values).any() and (c.values.view(torch.int32) == -(1 << 31)).any()
               for c in wide)


def test_quantiser_is_floor_division():
    assert H.quantise([0, 1, 2, 3, 7, 8, 9], 4) == [0, 0, 0, 0, 1, 2, 2]
    assert H.quantise([5, 3], 1) == [5, 3]


# ---------------------------------------------------------------------------------------------------------------------------
# the port selects what torch.topk and the oracle select
# ---------------------------------------------------------------------------------------------------------------------------
def test_port_equals_torch_topk_and_the_oracle_on_every_case(walked, oracle):
    for c in TABLE:
        mask, _ = walked[c.name]
        want = torch.zeros(c.values.shape, dtype=torch.bool).scatter_(1, torch.topk(c.values, c.k).indices, True)
        assert torch.equal(mask, want), "torch.topk: " + c.name
        assert torch.equal(mask, oracle.topk_mask(c.values, c.k)), "oracle: " + c.name
        assert (mask.sum(1) == c.k).all()


def test_port_orders_nan_first_and_signed_zeros_as_equal():
    assert H.before_float(float("nan"), float("inf")) and not H.before_float(float("inf"), float("nan"))
    assert not H.before_float(float("nan"), float("nan"))
    assert not H.before_float(0.0, -0.0) and not H.before_float(-0.0, 0.0)
    assert H.kth_is_tied([1.0, float("nan"), float("nan"), 0.0], 1) and not H.kth_is_tied([1.0, float("nan"), 0.0], 1)
    assert H.kth_is_tied([3, 5, 5, 1], 1) and not H.kth_is_tied([3, 5, 5, 1], 2) and not H.kth_is_tied([3, 5], 2)


# ---------------------------------------------------------------------------------------------------------------------------
# every path of the walk is reached - from the recorded statistics
# ---------------------------------------------------------------------------------------------------------------------------
def _paths(walked):
    return [(c, i, p) for c in TABLE for i, p in enumerate(walked[c.name][1])]


def test_table_reaches_both_selectors_on_both_sides_of_the_dispatch_boundary(walked):
    sel = {}
    for c, _, p in _paths(walked):
        assert p.selector == ("heap_select" if c.k * 64 <= c.n else "introselect")
        sel.setdefault(c.n, {}).setdefault(p.selector, set()).add(c.k)
    for n in (64, 65, 127, 128, 129, 210, 1023, 1024, 1025, 4096):
        heap, intro = sel[n]["heap_select"], sel[n]["introselect"]
        assert max(heap) == n // 64 and min(intro) == n // 64 + 1, n           # k * 64 <= n and the first k beyond it, at the same n
    assert (128 // 64) * 64 == 128 and (1024 // 64) * 64 == 1024 and 4096 // 64 * 64 == 4096     # ... with equality at three of them
    assert all("heap_select" not in sel[n] for n in (1, 2, 3, 4, 63))


def test_table_reaches_the_insertion_sort_alone(walked):
    only = {c.n for c, _, p in _paths(walked) if p.insertion_only}
    assert only == {1, 2, 3}
    assert all(p.levels >= 1 for c, _, p in _paths(walked) if c.n >= 4 and p.selector == "introselect")


def test_table_reaches_the_depth_limit_fallback_from_both_directions_and_with_ties(walked):
    hits = [(c, i, p) for c, i, p in _paths(walked) if p.fallback is not None]
    for c, _, p in hits:
        first, nth, last = p.fallback
        assert p.levels == p.depth_limit == 2 * int(math.log2(c.n)) and first <= nth == c.k - 1 < last and last - first > 3
    assert any(p.fallback[0] == 0 and p.fallback[2] < c.n for c, _, p in hits)               # `last` crept down
    assert any(p.fallback[0] > 0 and p.fallback[2] == c.n for c, _, p in hits)               # `first` crept up
    assert {c.n for c, _, _ in hits} == {128, 210, 512, 2048} and {c.dtype for c, _, _ in hits} == {H.I32, H.F32}
    tied = {(c.n, c.k, c.name[9], H.QUANTA[i]) for c, i, p in hits if H.kth_is_tied(c.values[i].tolist(), c.k)}
    print("fallback rows with a tie at the k-th value (n, k, sign, quantum):", sorted(tied))
    assert len(tied) >= 2
    assert any(p.fallback[0] == 0 for c, i, p in hits if H.kth_is_tied(c.values[i].tolist(), c.k))
    assert any(p.fallback[0] > 0 for c, i, p in hits if H.kth_is_tied(c.values[i].tolist(), c.k))
    # only the adversary gets there
    assert all(c.name.startswith("adversary") for c, _, _ in hits)


def test_table_scans_lengths_that_are_and_are_not_multiples_of_eight(walked):
    scans = {p.scan for _, _, p in _paths(walked) if p.selector == "heap_select"}
    assert any(s % 8 == 0 for s in scans) and any(s % 8 for s in scans)
    assert {s % 8 for s in scans} >= {0, 1, 7} and min(scans) == 63            # n = 64, k = 1: shorter than the eight-wide stride never
    fb = {p.fallback[2] - p.fallback[1] - 1 for _, _, p in _paths(walked) if p.fallback}     # the fallback's own scans
    assert any(s % 8 for s in fb)


def test_adversary_rows_replay_the_lazy_run():
    for n, k in H.ADVERSARY:
        for sign in (1, -1):
            row, lazy = H.adversary_row(n, k, sign)
            assert sorted(row) == list(range(n))                               # distinct int32 values
            assert row == H.adversary_rows()[(n, k, sign)]
            _, replay = H.walk(row, k, H.before_int)
            assert replay.key() == lazy.key(), (n, k, sign)
            _, as_float = H.walk([float(v) for v in row], k, H.before_float)
            assert as_float.key() == lazy.key()
    key = lambda n, k, s: H.adversary_row(n, k, s)[1].fallback
    assert key(128, 10, 1) == (0, 9, 101) and key(210, 105, -1) == (28, 104, 210) and key(512, 256, -1) == (36, 255, 512)
    assert H.adversary_row(2048, 1024, 1)[1].levels == 22 and H.adversary_row(512, 256, 1)[1].levels == 18


def test_sorted_and_organ_pipe_rows_stay_clear_of_the_depth_limit():
    """The rows of test_gpu_select.py::test_topk_wide_rows_and_nan: 18 levels allowed at n = 512, none of them needs more than 16."""
    used = {}
    for name, row in H.wide_test_rows().items():
        for k in H.WIDE_TEST_K:
            _, p = H.walk(row, k, H.before_int)
            assert p.selector == "introselect" and p.depth_limit == 18 and p.fallback is None, (name, k)
            used.setdefault(name, set()).add(p.levels)
    assert used == {"ascending": {8}, "descending": {10}, "organ_pipe": {15, 16}, "all_zero": {8}}


def test_a_fallback_row_with_a_tied_kth_value_has_equals_on_both_sides_of_the_cut():
    """On such a row elements equal to the k-th value lie inside AND outside the selection: an equally large set exists, and
    only the fallback's tie order picks the right one."""
    row = H.quantise(H.adversary_rows()[(210, 105, 1)], 2)
    idx, p = H.walk(row, 105, H.before_int)
    assert p.fallback == (0, 104, 183) and H.kth_is_tied(row, 105)
    tie = sorted(row, reverse=True)[104]
    inside = [i for i in idx if row[i] == tie]
    outside = [i for i in range(210) if row[i] == tie and i not in idx]
    assert inside and outside                           # an equally large selection exists: only the tie order decides


# ---------------------------------------------------------------------------------------------------------------------------
# rollout: geometry, reference and bound
# ---------------------------------------------------------------------------------------------------------------------------
def test_rollout_cases_cover_the_launch_geometries():
    assert H.ROLLOUT_T == (2, 3, 5, 63, 64, 65, 129, 211, 256, 257, 511, 512, 513, 1024)
    geo = {t: H.rollout_geometry(t) for t in H.ROLLOUT_T}
    assert geo[2][:2] == (512, 256) and geo[256][:2] == (512, 2) and geo[257][:2] == (257, 1) and geo[512][:2] == (512, 1)
    assert geo[513][:2] == (512, 1) and geo[1024][:2] == (512, 1)              # columns strided over 512 threads
    assert geo[3][:2] == (510, 170) and geo[129][:2] == (387, 3)
    assert {g[2] for g in geo.values()} >= {0, 1, 2, 3}                        # every remainder of the four-way unrolled row loop
    assert all(64 <= thr <= 512 or thr == t for t, (thr, _, _) in geo.items())
    for t in H.ROLLOUT_T:
        assert H.rollout_ldps(t) == sorted({t, (t + 3) // 4 * 4, t + 5})
    assert any(len(H.rollout_ldps(t)) == 2 for t in H.ROLLOUT_T) and any(len(H.rollout_ldps(t)) == 3 for t in H.ROLLOUT_T)


@pytest.mark.parametrize("t", (2, 5, 65, 257))
def test_rollout_reference_is_the_matrix_product_and_scores_stay_normal(t, oracle):
    probs = H.rollout_probs(t)
    assert probs.dtype == H.F32 and probs.shape == (3, 3, t, t)
    for layers in H.ROLLOUT_L:
        ref = H.rollout_reference(probs, layers)
        assert ref.dtype == torch.float64 and ref.shape == (3, t - 1)
        full = oracle.rollout_scores([probs[i].double()[None] for i in range(layers)])[0]
        assert torch.allclose(ref, full, rtol=1e-12, atol=0.0)
        assert ref.min() > H.ROLLOUT_MIN_SCORE
        bound = H.rollout_bound(ref, layers, t)
        assert torch.equal(bound, layers * (t + 2) * 2.0 ** -24 * ref)
        if layers == 1:
            assert torch.equal(ref, probs[0][:, 0, 1:].double())               # no product at all: the fp32 values themselves
        elif layers == 2:                                      # one dropped row of the product: scores of every (sample, head) leave the bound
            short = torch.einsum("bi,bij->bj", probs[1].double()[:, 0, :t - 1], probs[0].double()[:, :t - 1, :])
            assert ((short[:, 1:] - ref).abs() > bound).any(1).all()


# ---------------------------------------------------------------------------------------------------------------------------
# frequency counts: launch shapes, operands, what the oracle accepts
# ---------------------------------------------------------------------------------------------------------------------------
def test_frequency_geometries_have_the_tile_bookkeeping_they_are_chosen_for():
    shape = {g: H.freq_launch_shape(*g) for g in H.FREQ_GEOM}
    assert shape[(1, 16, 16)] == (1, 1, 1, 15, 1)      # one tile: three clamped tile slots in its wave, three waves wholly clamped
    assert shape[(1, 16, 80)][0] == 5 and shape[(1, 48, 16)][0] == 3 and shape[(3, 32, 48)][0] == 18
    assert shape[(17, 16, 16)][:3] == (17, 2, 5)
    assert all(s[3] > 0 for s in shape.values())       # every geometry leaves clamped slots behind the last tile
    assert {s[0] % 4 for s in shape.values()} >= {1, 2, 3}                     # the 2x2 form's last block is partly empty too


def test_frequency_forms_name_every_instantiation_the_launcher_can_take():
    got = {H.freq_kernel(nm, c, off == 0) for _, c, off, nmods in H.FREQ_FORMS for nm in nmods}
    assert got == {"freq_counts4_kernel<2,3>", "freq_counts4_kernel<3,3>", "freq_counts4_kernel<4,3>", "freq_counts_kernel<3,3>",
                   "freq_counts_kernel<4,3>", "freq_counts_kernel<0,0>"}
    assert {f[0]: {H.freq_kernel(nm, f[1], f[2] == 0) for nm in f[3]} for f in H.FREQ_FORMS}["2x2"] == {
        "freq_counts_kernel<3,3>", "freq_counts_kernel<4,3>"}


@pytest.mark.parametrize("c", (1, 3, 4))
@pytest.mark.parametrize("nmod", (2, 3, 4))
def test_oracle_accepts_every_channel_count_and_special_pixel(nmod, c, oracle):
    """C = 1, C = 4 and a NaN pixel included: no case of the GPU module had to be dropped."""
    b, h, w = 3, 32, 48
    last = -1
    noise = H.freq_reference(oracle, H.freq_operands("noise", nmod, c, b, h, w))
    assert noise.shape == (b, 6) and noise.dtype == torch.int32 and 0 < noise.min() and noise.max() < 256
    for kind in H.FREQ_KINDS:
        mods = H.freq_operands(kind, nmod, c, b, h, w)
        assert len(mods) == nmod and all(m.shape == (b, c, h, w) and m.is_contiguous() for m in mods)
        ref = H.freq_reference(oracle, mods)
        tile = torch.stack(mods)[:, -1, :, h - 16:, w - 16:]
        if kind in ("zero", "cancel", "nan"):
            assert ref[last, last] == 0, kind          # an exact zero is not positive; a NaN poisons its whole tile
        if kind == "cancel":
            assert (tile != 0).any() and tile.sum(0).eq(0).all()
        if kind == "denormal":
            assert (tile.abs() < 2.0 ** -126).all() and (tile != 0).any() and 0 < ref[last, last] < 256
        if kind == "inf":
            assert torch.isinf(tile).sum() == 1
        if kind == "nan":
            assert torch.isnan(tile).sum() == 1
        assert (ref.flatten()[:-1] > 0).all()                                  # every other tile is plain noise


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU tests use every table
# ---------------------------------------------------------------------------------------------------------------------------
def _params(fn, name):
    for mark in getattr(fn, "pytestmark", []):
        if mark.name == "parametrize" and mark.args[0] == name:
            return list(mark.args[1])
    raise AssertionError("%s is not parametrized over %s" % (fn.__name__, name))


def test_gpu_tests_walk_every_case_and_table():
    import test_gpu_select_edges as G
    assert G.pytestmark.name == "gpu" and G.TABLE is TABLE
    ns = _params(G.test_topk_table_case_masks_bit_for_bit, "n")
    assert ns == H.table_n() and sum(len(H.cases_for(n)) for n in ns) == len(TABLE)
    assert G.cases_for is H.cases_for
    assert _params(G.test_rollout_at_every_launch_geometry, "t") == list(H.ROLLOUT_T)
    assert (G.ROLLOUT_L, G.ROLLOUT_BH, G.ROLLOUT_GAP) == (H.ROLLOUT_L, H.ROLLOUT_BH, H.ROLLOUT_GAP) and G.rollout_ldps is H.rollout_ldps
    assert _params(G.test_frequency_counts_every_instantiation, "geom") == list(H.FREQ_GEOM)
    assert _params(G.test_frequency_counts_every_instantiation, "form") == list(H.FREQ_FORMS)
    assert G.FREQ_KINDS == H.FREQ_KINDS == ("noise", "zero", "cancel", "denormal", "inf", "nan")
