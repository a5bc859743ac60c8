"""The optimizer edge suite's own ground (optim_edge_helpers.py), on the CPU: the SGD recipe is exact in fp32, the AdamW bound is
anchored on torch's CPU AdamW and rejects a skipped update, the poison positions sit where the kernels' index maps say, the scaler
restatement equals torch._amp_update_scale_, and every table is used by the GPU tests."""

import numpy as np
import pytest
import torch

import optim_edge_helpers as H

F32 = torch.float32
C = H.chunk_elems()
TABLE = H.size_table(C)


# ---------------------------------------------------------------------------------------------------------------------------
# table and arenas
# ---------------------------------------------------------------------------------------------------------------------------
def test_size_table_holds_the_listed_sizes_in_mixed_order():
    n = [H.numel(e) for e in TABLE]
    assert set(n) >= {1, 3, 4, 5, 1023, 1024, 1027, C - 1, C, C + 1, 2 * C + 7}
    shadowed = [e for e in TABLE if e.shadow and e.grad]
    assert len(shadowed) >= 2 and all(len(e.shape) >= 2 for e in shadowed) and any(H.numel(e) % 4 for e in shadowed)
    assert sum(not e.grad for e in TABLE) == 1 and TABLE[H.index_of(TABLE, "nograd")].shadow
    assert n != sorted(n) and n != sorted(n, reverse=True)
    # every updated tensor has its own (lr, wd) pair
    live = [(e.lr, e.wd) for e in TABLE if e.grad]
    assert len(set(live)) == len(live)
    assert all(2.0 ** -4 <= x <= 0.5 for pair in live for x in pair)
    assert len(TABLE) <= C                                       # (a table index is never a valid chunk offset by accident)


def test_chunk_tables_match_fused_sgd():
    """The helper builds chunk_tensor / chunk_off as FusedSGD.__init__ does: every element of every tensor in exactly one chunk."""
    n = [H.numel(e) for e in TABLE]
    ct, co = H.chunk_tables(n, C)
    seen = [np.zeros(k, dtype=np.int32) for k in n]
    for t, o in zip(ct, co):
        assert o % C == 0 and o < n[t]
        seen[t][o:min(o + C, n[t])] += 1
    assert all((s == 1).all() for s in seen)
    assert ct == sorted(ct) and len(ct) == sum(-(-k // C) for k in n)


@pytest.mark.parametrize("align", list(H.ALIGN))
def test_arena_slices_have_the_alignment_of_their_class(align):
    st = H.State(TABLE, align, "cpu", C, shadow_dtype=H.BF16, adam=True, pairs=True)
    sp, sg, sm = H.ALIGN[align]
    for kind, shift in (("p", sp), ("g", sg), ("m", sm), ("v", sm), ("h", sp), ("hi", 0), ("lo", 0)):
        a = st.arenas[kind]
        es = a.buf.element_size()
        assert a.total % H.SLOT == 0
        for i, (o, k) in enumerate(zip(a.offs, a.sizes)):
            assert (o - shift) % H.SLOT == 0 and (o * es) % 16 == (shift * es) % 16
            lo = a.offs[i - 1] + a.sizes[i - 1] if i else 0
            assert o - lo >= H.GUARD and a.total - (o + k) >= H.GUARD              # sentinels on both sides of every slice
            assert not a.inside[o - H.GUARD:o].any() and a.inside[o:o + k].all()
        assert not a.broken_sentinels()
    assert (sp | sg | sm) % 4 == 0 or align != "aligned"
    assert st.g_ptrs[H.index_of(TABLE, "nograd")].item() == 0 and (st.g_ptrs != 0).sum().item() == len(TABLE) - 1
    assert [bool(x) for x in (st.h_ptrs != 0).tolist()] == [e.shadow for e in TABLE]
    assert st.hi_ptrs[H.index_of(TABLE, "nograd")].item() == 0


def test_alignment_classes_cover_the_kernels_switches():
    """p | g | m decides the update's path, g alone the check's: all aligned; only g off by 1, 2, 3 (a GradBuckets slice behind
    a tensor of odd size); only p off; everything off."""
    shifts = set(H.ALIGN.values())
    assert (0, 0, 0) in shifts and {(0, 1, 0), (0, 2, 0), (0, 3, 0)} <= shifts
    assert any(p and not g and not m for p, g, m in shifts) and any(p and g and m for p, g, m in shifts)
    assert [H.ALIGN[a][1] % 4 == 0 for a in H.POISON_ALIGN] == [True, False]


def test_sentinel_check_sees_a_write_next_to_a_slice():
    st = H.State(TABLE, "g+1", "cpu", C)
    i = H.index_of(TABLE, "three")
    st.p.raw[st.p.offs[i] + 3] = 0
    with pytest.raises(AssertionError, match=r"three\[3\]"):
        st.assert_guards()
    st.p.raw[st.p.offs[i] + 3] = H.SENT32
    st.m.raw[st.m.offs[i] - 1] = 0
    with pytest.raises(AssertionError, match=r"three\[-1\]"):
        st.assert_guards()


# ---------------------------------------------------------------------------------------------------------------------------
# SGD: the recipe is exact
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", H.INV_SCALES, ids=lambda s: "unscaled" if s is None else "inv_scale")
@pytest.mark.parametrize("mu", H.MOMENTA)
def test_sgd_recipe_is_exact_in_fp32_and_equals_torch_sgd(mu, s):
    """Every table case, three steps: the fp32 restatement (one rounding per operation) equals the float64 closed form at every
    operation - so an fma changes nothing either - and torch.optim.SGD on the CPU produces the same bits."""
    p0, grads = H.sgd_operands(TABLE)
    assert all(((x * 8) == (x * 8).round()).all() and x.abs().max() <= 4 for x in p0)
    assert all((g == g.round()).all() and g.abs().max() <= 8 for gs in grads for g in gs) and len(grads) == H.SGD_STEPS
    ref = H.sgd_reference(TABLE, p0, grads, mu, s)
    tp = [torch.nn.Parameter(x.float()) for x in p0]
    topt = torch.optim.SGD([{"params": [q], "lr": e.lr, "weight_decay": e.wd} for q, e in zip(tp, TABLE)], lr=1.0, momentum=mu)
    for i, e in enumerate(TABLE):
        p64, m64 = p0[i].clone(), torch.zeros_like(p0[i])
        p32, m32 = p0[i].float(), torch.zeros(H.numel(e))
        for k in range(H.SGD_STEPS):
            if not e.grad:
                assert torch.equal(ref[k][0][i], p0[i]) and not ref[k][1][i].any()
                continue
            p64, m64, d64 = H.sgd_ref_step(p64, grads[k][i], m64, e.lr, e.wd, mu, s)
            p32, m32, d32 = H.sgd_f32_step(p32, grads[k][i].float(), m32, e.lr, e.wd, mu, s)
            lr_m = torch.tensor(e.lr, dtype=F32) * m32
            assert torch.equal(d32.double(), d64) and torch.equal(m32.double(), m64) and torch.equal(p32.double(), p64), (e.name, k)
            assert torch.equal(lr_m.double(), e.lr * m64) and torch.equal((torch.tensor(e.wd, dtype=F32) * p32).double(), e.wd * p64)
            assert torch.equal(ref[k][0][i], p64) and torch.equal(ref[k][1][i], m64)
    for k in range(H.SGD_STEPS):
        for q, g, e in zip(tp, grads[k], TABLE):
            q.grad = (g * (1.0 if s is None else s)).float() if e.grad else None
        topt.step()
        for i, (q, e) in enumerate(zip(tp, TABLE)):
            assert torch.equal(q.detach().double(), ref[k][0][i]), (e.name, k)
            if e.grad:
                assert torch.equal(topt.state[q]["momentum_buffer"].double(), ref[k][1][i]), (e.name, k)


def test_sgd_reference_depends_on_each_tensors_own_hyper_parameters():
    """Reading a neighbour's (or tensor 0's) lr or wd changes bits of every updated tensor after one step."""
    p0, grads = H.sgd_operands(TABLE)
    live = [i for i, e in enumerate(TABLE) if e.grad]
    for i in live:
        e = TABLE[i]
        want, _, _ = H.sgd_ref_step(p0[i], grads[0][i], torch.zeros_like(p0[i]), e.lr, e.wd, 0.5)
        for j in {live[0], live[live.index(i) - 1]} - {i}:
            o = TABLE[j]
            for lr, wd in ((o.lr, e.wd), (e.lr, o.wd)):
                if (lr, wd) != (e.lr, e.wd):
                    got, _, _ = H.sgd_ref_step(p0[i], grads[0][i], torch.zeros_like(p0[i]), lr, wd, 0.5)
                    assert not torch.equal(got, want) or H.numel(e) < 4, (e.name, o.name)


@pytest.mark.parametrize("dtype", (H.BF16, H.F16), ids=("bf16", "f16"))
def test_tie_operands_hold_exact_ties_that_an_update_does_not_move(dtype):
    ps, gs = H.tie_operands(TABLE, dtype)
    for e, p, g in zip(TABLE, ps, gs):
        k = -(-H.numel(e) // 4)
        assert H.is_tie(p[:k], dtype).all() and torch.isfinite(p.to(dtype)).all()
        # with wd = 0, m = 0, g = 0 the update leaves the tie in place
        p1, m1, _ = H.sgd_f32_step(p[:k], g[:k], torch.zeros(k), e.lr, 0.0, 0.5, 2.0 ** -3)
        assert torch.equal(p1.view(torch.int32) & 0x7FFFFFFF, p[:k].view(torch.int32) & 0x7FFFFFFF)
        assert (p.to(dtype).float() != p).float().mean() > 0.5 or H.numel(e) < 8      # rounding matters for most elements
    allp = torch.cat([p[:-(-p.numel() // 4)] for p in ps])
    r = allp.to(dtype).double()
    assert (r.abs() > allp.double().abs()).any() and (r.abs() < allp.double().abs()).any()       # ties resolved in both directions


# ---------------------------------------------------------------------------------------------------------------------------
# AdamW: the bound is anchored on torch's CPU AdamW
# ---------------------------------------------------------------------------------------------------------------------------
def _torch_adamw_step(p, g, m, v, lr, wd, t):
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([q], lr=lr, weight_decay=wd, betas=H.BETAS, eps=H.EPS, foreach=False)
    if t > 1:
        opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    q.grad = g.clone()
    opt.step()
    assert float(opt.state[q]["step"]) == t
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]


@pytest.mark.parametrize("t", H.ADAM_T)
def test_adamw_bound_holds_torch_cpu_adamw_and_rejects_a_skipped_update(t):
    """torch.optim.AdamW (fp32, single-tensor path) lies within the derived bound of the float64 step for every table tensor
    (gradient scales 1e-4, 1, 2^10 by tensor); leaving p, m or v as it was lies more than 1000 x outside."""
    p, g, m, v = H.adam_operands(TABLE, state=True)
    lr, wd = H.adam_hyper(TABLE)
    assert {H.GRAD_SCALES[i % 3] for i in range(len(TABLE))} == set(H.GRAD_SCALES)
    worst = 0.0
    for i, e in enumerate(TABLE):
        if t == 1:
            m[i], v[i] = torch.zeros_like(m[i]), torch.zeros_like(v[i])
        elif t == 2:                                             # the state one step from zero leaves behind
            g0 = m[i].double() / 0.3
            m[i], v[i] = (0.1 * g0).float(), (0.001 * g0 * g0).float()
        lri, wdi = float(lr[i]), float(wd[i])
        ref = H.adam_ref_step(p[i], g[i], m[i], v[i], lri, wdi, t)
        tp, tm, tv = _torch_adamw_step(p[i], g[i], m[i], v[i], lri, wdi, t)
        rs = (H.worst_ratio(tp, ref.p, ref.tol_p), H.worst_ratio(tm, ref.m, ref.tol_m), H.worst_ratio(tv, ref.v, ref.tol_v))
        assert max(rs) <= 1.0, (e.name, rs)
        worst = max(worst, *rs)
        # sensitivity: a parameter that was not updated is far outside (from zero state: at EVERY element); stale m and v at the typical one (an
        # element with g = m is rightly not moved)
        for old, new, tol in ((m[i], ref.m, ref.tol_m), (v[i], ref.v, ref.tol_v)):
            ratio = (old.double() - new).abs() / tol
            assert ratio.median() > 1000.0, (e.name, float(ratio.median()))
        ratio = (p[i].double() - ref.p).abs() / ref.tol_p
        if t == 1:                                               # |u| = lr at every element
            assert ratio.min() > 1000.0, (e.name, float(ratio.min()))
        else:                                                    # (m' crosses zero somewhere: there u is rightly tiny)
            assert (ratio > 1000.0).float().mean() > 0.9 or H.numel(e) < 8, (e.name, float((ratio > 1000.0).float().mean()))
            assert ratio.median() > 1000.0, (e.name, float(ratio.median()))
    print("torch CPU AdamW at t = %d: worst ratio to the bound %.3f" % (t, worst))
    assert worst > 0.05                                          # the bound is not slack by orders of magnitude


def test_adamw_bound_with_the_loss_scale_is_the_unscaled_one():
    """A power-of-two 1 / scale is exact: the step from g / s with s equals the step from g."""
    p, g, m, v = H.adam_operands(TABLE, state=True)
    i = H.index_of(TABLE, "k1027")
    big = (g[i].double() / H.ADAM_INV_SCALE).float()
    assert torch.equal(big.double() * H.ADAM_INV_SCALE, g[i].double())
    a = H.adam_ref_step(p[i], big, m[i], v[i], 1e-3, 1e-2, 7, H.ADAM_INV_SCALE)
    b = H.adam_ref_step(p[i], g[i], m[i], v[i], 1e-3, 1e-2, 7)
    assert torch.equal(a.p, b.p) and torch.equal(a.tol_p, b.tol_p)


def test_worst_ratio_requires_equality_where_the_tolerance_is_zero():
    z = torch.zeros(3, dtype=torch.float64)
    assert H.worst_ratio(torch.zeros(3), z, z) == 0.0
    assert H.worst_ratio(torch.tensor([0.0, 1e-30, 0.0]), z, z) == float("inf")
    assert H.worst_ratio(torch.tensor([1.0]), torch.tensor([1.5], dtype=torch.float64), torch.tensor([0.25], dtype=torch.float64)) == 2.0


# ---------------------------------------------------------------------------------------------------------------------------
# overflow detection: index maps and poison positions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", (True, False), ids=("aligned", "unaligned"))
@pytest.mark.parametrize("n", (1, 3, 4, 5, 7, 1023, 1024, 1027, C - 1, C))
def test_check_map_is_the_inverse_of_the_kernels_loops(n, aligned):
    """check_visits restates grad_check_multi_kernel's loops; every element of a chunk is read exactly once, by the lane that
    check_map names."""
    visits = H.check_visits(n, aligned)
    assert sorted(v[0] for v in visits) == list(range(n))
    for e, tid, outer, j in visits[::37] + visits[-8:]:
        w = H.check_map(n, e, aligned, C)
        assert (w.thread, w.iteration, w.load) == (tid, outer, j), (e, w)


def test_poison_positions_sit_at_the_edges_of_the_index_maps():
    pos = {p.label: p for p in H.poison_positions(TABLE, C)}
    big = H.index_of(TABLE, "two_c7")
    n = 2 * C + 7
    cm = lambda label, aligned=True: H.check_map(n, pos[label].element, aligned, C)
    um = lambda label: H.update_map(n, pos[label].element, True, C)
    assert all(pos[k].tensor == big for k in pos if not k.startswith(("only", "three", "later")))
    assert cm("first") == H.Where(0, "body", 0, 0, 0, 0)
    assert um("last_thread_first_pass_end") == H.Where(0, "body", H.THREADS - 1, 0, 0, 3)
    assert H.update_map(n, pos["last_thread_first_pass_end"].element + 1, True, C) == H.Where(0, "body", 0, 1, 0, 0)
    assert cm("unroll_outer0_end")[:5] == (0, "body", H.THREADS - 1, 0, H.UNROLL - 1)
    assert pos["unroll_outer0_end"].element == 4 * 2047 and pos["unroll_outer1_start"].element == 4 * 2048
    assert cm("unroll_outer1_start") == H.Where(0, "body", 0, 1, 0, 0)
    assert cm("chunk0_last").chunk == 0 and cm("chunk0_last").lane == 3 and cm("chunk1_first") == H.Where(1, "body", 0, 0, 0, 0)
    assert pos["chunk0_last"].element == C - 1 and pos["chunk1_first"].element == C
    assert cm("last_chunk_body_end") == H.Where(2, "body", 0, 0, 0, 3)
    assert cm("last_chunk_tail_first") == H.Where(2, "tail", 0, 0, 0, 0) and cm("last_chunk_tail_last") == H.Where(2, "tail", 2, 0, 0, 0)
    assert pos["last_chunk_tail_last"].element == n - 1
    # unaligned: the same elements sit in other lanes (the scalar path is a different loop)
    assert cm("last_chunk_tail_last", False) == H.Where(2, "scalar", 6, 0, 0, 0)
    assert cm("chunk0_last", False) == H.Where(0, "scalar", H.THREADS - 1, C // H.THREADS - 1, 0, 0)
    # the small tensors: tail only; the later tensor follows others in the table
    assert H.check_map(1, pos["only_element"].element, True, C).path == "tail" and H.numel(TABLE[pos["only_element"].tensor]) == 1
    assert H.check_map(3, pos["three_last"].element, True, C) == H.Where(0, "tail", 2, 0, 0, 0)
    late = pos["later_tensor_first"].tensor
    assert late == pos["later_tensor_last"].tensor and late > big and TABLE[late].grad
    assert pos["later_tensor_last"].element == H.numel(TABLE[late]) - 1 and pos["later_tensor_first"].element == 0
    for p in pos.values():
        assert TABLE[p.tensor].grad and 0 <= p.element < H.numel(TABLE[p.tensor])


def test_poison_values_are_the_four_non_finite_kinds():
    v = torch.tensor(list(H.POISON_VALUES.values()), dtype=torch.int32).view(F32)
    assert v[0] == float("inf") and v[1] == -float("inf") and torch.isnan(v[2:]).all()
    assert (v.view(torch.int32)[3].item() & 0xFFFFFFFF) == 0x7F800001
    for name, gs in H.clean_gradient_sets(TABLE).items():
        assert all(torch.isfinite(g).all() and g.numel() == H.numel(e) for g, e in zip(gs, TABLE)), name
    sets = H.clean_gradient_sets(TABLE)
    assert sets["flt_max"][4].abs().min() == H.FLT_MAX and (sets["denormal"][4].abs() < 2.0 ** -126).all()
    assert (sets["neg_zero"][4].view(torch.int32) == -(1 << 31)).all()


# ---------------------------------------------------------------------------------------------------------------------------
# loss scaler
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(H.SCALER_CASES))
def test_scaler_restatement_equals_torch_amp_update_scale(case):
    founds, growth, backoff, interval, scale = H.SCALER_CASES[case]
    s_t, tr_t = torch.full((1,), scale, dtype=F32), torch.zeros(1, dtype=torch.int32)
    s, tr = np.float32(scale), 0
    anchored = True
    for f in founds:
        s, inv, tr, cleared = H.scaler_ref(s, tr, f, growth, backoff, interval)
        assert inv == np.float32(1.0) / s and cleared == 0 and np.isfinite(s)
        if anchored:
            try:
                torch._amp_update_scale_(s_t, tr_t, torch.tensor([float(f != 0)]), growth, backoff, interval)
            except (RuntimeError, NotImplementedError):
                anchored = False                       # this torch has no CPU kernel for it: only the torch anchor is skipped
                continue
            assert s_t.item() == float(s) and tr_t.item() == tr, (case, f)
    if not anchored:
        pytest.skip("torch._amp_update_scale_ refuses CPU tensors here: the restatement stands unanchored")


def test_scaler_cases_reach_backoff_growth_interval_one_and_the_overflow_guard():
    founds, growth, backoff, interval, scale = H.SCALER_CASES["growth_would_overflow"]
    s, tr, kept = np.float32(scale), 0, 0
    for f in founds:
        s2, _, tr2, _ = H.scaler_ref(s, tr, f, growth, backoff, interval)
        kept += int(not f and tr + 1 == interval and s2 == s)
        assert not kept or tr2 == 0 or f or tr2 == tr + 1
        s, tr = s2, tr2
    with np.errstate(over="ignore"):
        assert kept >= 1 and not np.isfinite(np.float32(scale) * np.float32(growth))
    assert H.SCALER_CASES["interval_one"][3] == 1
    assert any(f not in (0, 1) for f in H.SCALER_CASES["found_other_than_one"][0])


# ---------------------------------------------------------------------------------------------------------------------------
# split pairs, transposes
# ---------------------------------------------------------------------------------------------------------------------------
def test_split_operands_reach_subnormal_lo_zeros_and_negatives():
    ps = H.split_operands(TABLE)
    allp = torch.cat(ps)
    hi, lo = H.split_ref(allp)
    sub = (lo.float().abs() > 0) & (lo.float().abs() < 2.0 ** -14)
    assert sub.sum() > 100 and (allp == 0).sum() > 100 and (allp < 0).sum() > 100 and torch.isfinite(hi.float()).all()
    assert (allp.view(torch.int32) == -(1 << 31)).any()                                  # -0.0
    assert any(p.numel() % 4 for p in ps)
    # hi + lo carries p * 256 to about 2^-22 relative where lo is normal: the pair is worth asserting bit for bit
    v = allp.double() * H.SPLIT_SCALE
    ok = lo.float().abs() >= 2.0 ** -14
    assert ((hi.double() + lo.double() - v).abs()[ok] <= v.abs()[ok] * 2.0 ** -21).all()
    assert H.SPLIT_SCALE == 256.0 and np.log2(H.SPLIT_SCALE) % 1 == 0


def test_transpose_operands_cover_every_16_bit_pattern_and_the_tiles_are_shuffled():
    xs = H.transpose_operands()
    assert [tuple(x.shape) for x in xs] == list(H.TRANSPOSE_SHAPES) and max(max(s) for s in H.TRANSPOSE_SHAPES) == 512
    assert torch.unique(xs[-1]).numel() == 65536
    assert all(torch.unique(x).numel() == min(x.numel(), 65536) for x in xs)
    tiles = H.tile_table(H.TRANSPOSE_SHAPES)
    want = sorted((t, a, b) for t, (r, c) in enumerate(H.TRANSPOSE_SHAPES) for a in range(r // 64) for b in range(c // 64))
    order = [t for t, _, _ in tiles]
    assert sorted(tiles) == want and tiles != want and order != sorted(order) and order != sorted(order, reverse=True)


# ---------------------------------------------------------------------------------------------------------------------------
# the GPU tests use every table
# ---------------------------------------------------------------------------------------------------------------------------
def _params(fn, name):
    for mark in getattr(fn, "pytestmark", []):
        if mark.name == "parametrize" and mark.args[0] == name:
            return list(mark.args[1])
    raise AssertionError("%s is not parametrized over %s" % (fn.__name__, name))


def test_gpu_tests_walk_every_alignment_class_poison_position_and_case():
    import test_gpu_optim_edges as G
    for fn in (G.test_sgd_three_steps_bit_for_bit, G.test_adamw_one_step_from_device_state, G.test_sgd_shadows_round_ties_as_torch,
               G.test_skip_flag_freezes_everything):
        assert _params(fn, "align") == list(H.ALIGN), fn.__name__
    assert _params(G.test_poisoned_gradient_is_found_at_every_position, "align") == list(H.POISON_ALIGN)
    assert G.POISONS == H.poison_positions(TABLE, C) and G.POISON_VALUES == H.POISON_VALUES
    assert _params(G.test_poisoned_gradient_is_found_at_every_position, "kernel") == ["check", "sgd", "adamw"]
    assert _params(G.test_sgd_three_steps_bit_for_bit, "inv_scale") == list(H.INV_SCALES)
    assert _params(G.test_sgd_three_steps_bit_for_bit, "shadow") == [None, H.BF16, H.F16]
    assert _params(G.test_adamw_one_step_from_device_state, "t") == list(H.ADAM_T)
    assert _params(G.test_scaler_update_follows_the_restatement, "case") == list(H.SCALER_CASES)
    assert all(m.name == "gpu" for m in [G.pytestmark]) and G.TABLE == TABLE
