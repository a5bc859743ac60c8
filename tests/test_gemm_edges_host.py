"""Host side of the dense-GEMM edge suite (no GPU): the exact-operand recipe's preconditions hold for every case of the tables in
gemm_edge_helpers.py, and the tables reach the dispatch branches of gemm_h16 / launch_pipe / pp_body they are there for.  The dispatch is
restated in Python (gemm_edge_helpers.dispatch) from the documented thresholds; the .hip file is not parsed."""
import pytest
import torch

import gemm_edge_helpers as H
from editor_amd import ops

BF16, F16, F32 = H.BF16, H.F16, H.F32


def _layout_windows(c):
    return sorted({H.layout_shape(c.m, c.n, ta, tb) for ta, tb in H.LAYOUTS if min(H.layout_shape(c.m, c.n, ta, tb)) > 0})


@pytest.mark.parametrize("c", H.PLAIN_CASES + H.T208 + H.AUTO, ids=lambda c: "%s-%dx%dx%d-%d" % (c.family, c.m, c.n, c.k, c.ldc_pad))
def test_plain_case_preconditions(c):
    d = H.exact_operands(c.m, c.n, c.k)
    assert d["a"].abs().max() <= 3 and d["b"].abs().max() <= 3 and d["prod"].abs().max() < 2 ** 24
    assert set(d["rs"].tolist()) <= {0.5, 1.0, 2.0} and d["res"].abs().max() <= 64 and d["cold"].abs().max() <= 64
    assert bool((d["odd"] % 2 == 1).all())
    for rows, cols in _layout_windows(c):
        for dt in (BF16, F16, F32):
            H.check_preconditions(H.exact_ref(d, dt, rows=rows, cols=cols), dt, c.k)


@pytest.mark.parametrize("c", H.EPILOGUE_CASES, ids=lambda c: "%s-%dx%dx%d-%d" % (c.family, c.m, c.n, c.k, c.ldc_pad))
def test_epilogue_case_preconditions(c):
    d = H.exact_operands(c.m, c.n, c.k)
    H.check_preconditions(H.exact_ref(d, F32, residual=True), F32, c.k)
    H.check_preconditions(H.exact_ref(d, F32, beta=0.5), F32, c.k)
    for dt in H.HALF:
        H.check_preconditions(H.exact_ref(d, dt, beta=0.5), dt, c.k)
        H.check_preconditions(H.exact_ref(d, dt) * d["sel"], dt, c.k)                    # GELU_BWD | AUX_GRAD: value * saved gelu'


@pytest.mark.parametrize("s", H.SPLITK_CASES, ids=lambda s: "%dx%dx%d-%s-t%d-s%d" % (s.m, s.n, s.k, "".join(s.flags) or "none", s.ta, s.splitk))
def test_splitk_case_preconditions(s):
    d = H.exact_operands(s.m, s.n, s.k)
    for beta in (0.0, 1.0, 0.5):
        H.check_preconditions(H.exact_ref(d, F32, beta=beta), F32, s.k)


def test_gelu_sets():
    m, n, k = H.GELU_TABLE_SHAPE
    a, b, bias, pre = H.gelu_operands("table", m, n, k)
    assert int((a != 0).sum(1).max()) <= 7 and a.abs().max() == 1 and b.abs().max() == 2 and bool((bias == 0.5).all())
    assert bool(((pre * 2) % 2 == 1).all()) and 0.5 <= pre.abs().min() and pre.abs().max() <= 14.5 and pre.unique().numel() <= 29
    assert torch.equal(pre.to(BF16).double(), pre)                                        # exact in bf16: the table's input IS the sum
    bits = pre.to(BF16).view(torch.int16).int() & 0x7FFF                                  # inside the table: 2^-12 <= |x| < 16
    assert int(bits.min()) >= 115 << 7 and int(bits.max()) < (115 << 7) + 2048
    _, _, _, fb = H.gelu_operands("fallback", m, n, k)
    assert bool((fb % 1 == 0).all()) and bool((fb == 0).any()) and bool((fb.abs() >= 16).any())
    # every wave chunk of the fallback set (two tile rows of 256 columns) holds a value outside the table
    out = ((fb == 0) | (fb.abs() >= 16))
    for n0 in range(0, n, 256):
        blk = out[:m // 2 * 2, n0:n0 + 256]
        assert bool(blk.reshape(m // 2, 2, -1).any(2).any(1).all())
    _, _, _, mx = H.gelu_operands("mixed", m, n, k)
    assert bool((mx[1::2].abs() >= 16).any(1).all()) and mx[0::2].abs().max() <= 14.5     # dense rows next to table-range rows
    for kind in H.GELU_SETS:
        assert torch.equal(H.gelu_operands(kind, m, n, k)[3].to(F32).double(), H.gelu_operands(kind, m, n, k)[3])


@pytest.mark.parametrize("m,n,k,flags", H.SPLIT_MODE_CASES)
def test_pair_operands(m, n, k, flags):
    d = H.pair_operands(m, n, k)
    for name in ("a", "b"):
        x = d[name + "_hi"] + d[name + "_lo"]
        hi = x.to(F32).to(F16)
        assert torch.equal(hi.double(), d[name + "_hi"]) and torch.equal((x - hi.double()).to(F32).to(F16).double(), d[name + "_lo"])
    plain = (d["prod"] + d["ibias"]) * d["rs"][:, None]
    for ref in (plain, d["prod"] + d["res"], d["prod"] + d["ibias"]):
        H.check_preconditions(ref, F32, k)
        assert ref.abs().max() < 60000
    hi, lo = H.pair_of(plain)
    assert torch.equal(hi.double() + lo.double(), plain)                                  # the pair holds the exact value
    if m * n >= 1024:
        assert 0.6 < (d["a_lo"] != 0).double().mean() < 0.72 and (lo != 0).double().mean() > 0.85


@pytest.mark.parametrize("m,n,k", H.F32_SHAPES + [H.F32_CHUNKED])
def test_f32_case_preconditions(m, n, k):
    d = H.exact_operands(m, n, k)
    for beta in (0.0, 0.5):
        H.check_preconditions(H.exact_ref(d, F32, beta=beta), F32, k)
    H.check_preconditions(H.exact_ref(d, F32, residual=True), F32, k)


def test_wgrad_group_preconditions():
    for m in H.WGRAD_M:
        for n, k in H.WGRAD_PROBLEMS:
            d = H.exact_operands(n, k, m)
            H.check_preconditions(0.5 * d["prod"], F32, m)
        assert m % 64 == 0 and all(n % 256 == 0 and k % 256 == 0 for n, k in H.WGRAD_PROBLEMS)


# ---------------------------------------------------------------------------------------------------------------------------
# coverage of the dispatch
# ---------------------------------------------------------------------------------------------------------------------------
def _plain_plans():
    plans = set()
    for c in H.PLAIN_CASES:
        for ta, tb in H.LAYOUTS:
            m, n = H.layout_shape(c.m, c.n, ta, tb)
            if min(m, n) == 0:
                continue
            for c_f32 in (False, True):
                p = H.dispatch(m, n, c.k, ta, tb, c_f32, c.flags, ldc=n + c.ldc_pad, ldaux=n + H.PAD)
                assert p.family == c.family, (c, ta, tb, p)
                plans.add((p.family, p.epilogue, c_f32, (ta, tb)))
    return plans


def test_plain_cases_reach_every_family_layout_and_epilogue_path():
    plans = _plain_plans()
    for fam in ("small_reg", "small_glds", "pipe128", "pp256"):
        assert {lay for f, _, _, lay in plans if f == fam} == set(H.LAYOUTS), fam
    have = {(f, e, cf) for f, e, cf, _ in plans}
    need = {(f, "direct", cf) for f in ("small_reg", "small_glds", "pipe128", "pp256") for cf in (False, True)}
    need |= {("pipe128", "staged", False), ("pipe128", "staged", True), ("pp256", "onepass", False), ("pp256", "staged", True)}
    assert need <= have, need - have
    # the direct epilogue of the transposed 256x128 kernel comes from N % 8 == 4 alone
    assert any(f == "pipe128" and e == "direct" and lay != (0, 0) for f, e, _, lay in plans)


def test_case_tables_cover_the_listed_branches():
    reg = [(c.m, c.n, c.k) for c in H.SMALL_REG]
    assert any(k % 64 for _, _, k in reg) and any(m < 8 and k % 64 == 0 for m, _, k in reg) and any(n < 8 for _, n, _ in reg)
    assert all(not H.dispatch(c.m, c.n, c.k).glds for c in H.SMALL_REG) and all(H.dispatch(c.m, c.n, c.k).glds for c in H.SMALL_GLDS)
    for fam in (H.SMALL_REG, H.SMALL_GLDS, H.PIPE128, H.PP256):
        assert any(c.n % 8 == 4 for c in fam), fam[0].family
    assert any(c.ldc_pad % 8 == 4 and c.n % 8 == 0 for c in H.PP256)                       # ldc % 8 == 4 with N % 8 == 0
    wgs = lambda c, bm, bn: -(-c.m // bm) * -(-c.n // bn)
    assert {wgs(c, 128, 128) for c in H.SMALL_GLDS} >= {8, 9} and 12 in {wgs(c, 256, 128) for c in H.PIPE128}
    assert any(wgs(c, 256, 256) % 8 for c in H.PP256) and any(wgs(c, 208, 256) % 8 for c in H.T208)
    for fam in (H.PIPE128, H.PP256):
        assert {c.k // 64 for c in fam} >= {1, 2, 3, 4, 5}, fam[0].family                 # the pipeline prologue's K-tile counts
    big = [c for c in H.PIPE128 if "pipe128" in c.flags]
    assert big and all(H.dispatch(c.m, c.n, c.k).family == "pp256" and H.dispatch(c.m, c.n, c.k, flags=c.flags).family == "pipe128" for c in big)
    assert max(max(c.m for c in H.PLAIN_CASES + H.AUTO), 2049) == 2049 and max(c.n for c in H.PLAIN_CASES + H.AUTO) <= 520
    assert max(c.k for c in H.PLAIN_CASES + H.AUTO) <= 320


def test_short_tile_cases():
    for c in H.T208:
        p = H.dispatch(c.m, c.n, c.k, flags=c.flags, ldc=c.n + H.PAD, ldaux=c.n + H.PAD)
        assert p.family == "pp208" or c.m < 256            # (fewer than 256 rows: the host refuses short tiles - asserted on the GPU)
    assert sum(c.m >= 256 for c in H.T208) >= 2 and {c.m % 208 for c in H.T208} >= {1}


def test_auto_dispatch_cases_straddle_both_thresholds():
    fams = {(c.m, c.n): H.dispatch(c.m, c.n, c.k, ldc=c.n + H.PAD).family for c in H.AUTO}
    assert fams == {(2047, 512): "pipe128", (2048, 512): "pp256", (2048, 504): "pipe128"}
    # through ops.gemm the tile plan decides for (2048, 512): few tiles, so the 256x128 kernel; the plan itself is pinned here
    assert ops.gemm_tile_plan(2048, 512) == (208, True) and H.wrapper_flags(2048, 512, 64, 520) == ("pipe128",)
    assert H.wrapper_flags(2047, 512, 64, 520) == () and H.wrapper_flags(2048, 504, 64, 512) == ()


def test_splitk_cases_cover_slabs_atomics_and_empty_splits():
    seen = set()
    for s in H.SPLITK_CASES:
        p = H.dispatch(s.m, s.n, s.k // 64 * 64 if s.wrapper else s.k, s.ta, s.tb, True, s.flags, s.splitk, ldc=s.n)
        kt = -(-s.k // 64)
        eff = min(s.splitk, kt)
        per = -(-kt // eff)
        seen.add((p.family, p.split, "empty" if (eff - 1) * per >= kt else "clamped" if s.splitk > kt else "even"))
    for fam in ("pipe128", "pp256"):
        for split in ("slabs", "atomics"):
            assert {(fam, split, w) for w in ("even", "empty", "clamped")} <= seen, (fam, split, seen)
    assert ("small_reg", "atomics", "empty") in seen           # (four K-tiles in three splits of two: the third is empty)
    assert sum(s.wrapper for s in H.SPLITK_CASES) == 2 and all(s.k % 64 and s.k > 64 and s.ta and s.tb for s in H.SPLITK_CASES if s.wrapper)


def test_epilogue_cases_cover_every_family_and_staging():
    plans = set()
    for c in H.EPILOGUE_CASES:
        for name, epi, c_f32, beta in (("residual_f32", ops.EPI_RESIDUAL, True, 0.0), ("gelu", ops.EPI_GELU, False, 0.0),
                                       ("gelu_bwd", ops.EPI_GELU_BWD, False, 0.0), ("beta_f32", 0, True, 0.5), ("beta_h16", 0, False, 0.5)):
            p = H.dispatch(c.m, c.n, c.k, 0, 0, c_f32, c.flags, beta=beta, ldc=c.n + c.ldc_pad, ldaux=c.n + H.PAD, epi=epi)
            assert p.family == c.family
            plans.add((p.family, name, p.epilogue))
    for fam in ("small_reg", "small_glds", "pipe128", "pp256"):
        for name in ("residual_f32", "gelu", "gelu_bwd", "beta_f32", "beta_h16"):
            assert any(f == fam and e == name for f, e, _ in plans), (fam, name)
    assert {("pp256", "gelu", "onepass"), ("pp256", "gelu", "direct"), ("pp256", "gelu_bwd", "onepass"), ("pp256", "gelu_bwd", "direct"),
            ("pp256", "residual_f32", "staged"), ("pp256", "residual_f32", "direct"), ("pp256", "beta_h16", "direct")} <= plans
    assert set(H.EPILOGUES) >= {"residual_f32", "gelu", "gelu_auxgrad", "gelu_noaux", "gelu_bwd", "gelu_bwd_auxgrad", "beta_f32", "beta_h16"}


def test_remaining_tables():
    assert H.GELU_TABLE_SHAPE == (513, 520, 64) and H.dispatch(513, 520, 64, flags=("pp",), epi=ops.EPI_GELU, ldc=528, ldaux=528).epilogue == "onepass"
    assert [c[:3] for c in H.SPLIT_MODE_CASES] == [(1, 8, 64), (255, 264, 128), (257, 520, 192), (209, 256, 64)]
    assert H.SPLIT_MODE_CASES[3][3] == ("t208",) and H.WGRAD_M == (64, 128, 320)
    assert H.F32_SHAPES == [(1, 1, 1), (64, 64, 16), (63, 65, 17), (65, 63, 33), (129, 130, 100)] and H.F32_PADS == (1, 4)
    m, n, k = H.F32_CHUNKED                                   # the wrapper's eight-chunk batch path
    assert m <= 512 and k >= 1024 and k % 128 == 0
    assert len(H.REFUSALS) == len(set(H.REFUSALS)) >= 13
    assert H.flag_bits(("pp", "pipe128", "t208")) == ops.EPI_FORCE_PP | ops.EPI_PIPE128 | ops.EPI_TILE_ROWS(208)


def test_check_exact_names_the_tile_and_the_guards():
    ref = torch.arange(20 * 12, dtype=torch.float64).reshape(20, 12) / 4 - 7
    buf, ld, off = H.padded(ref, BF16, "cpu")
    assert ld == 20 and off == 2 * 20
    H.check_exact(buf, ref, 20, 12)
    bad = buf.clone()
    bad[H.GUARD + 17, 5] = 100.0
    with pytest.raises(AssertionError, match=r"1 of 240 elements differ; first at row 17 col 5: 16-row fragment 1, 128x128 tile \(0, 0\)"):
        H.check_exact(bad, ref, 20, 12)
    bad = buf.clone()
    bad[H.GUARD + 3, 4] = float("nan")                        # an element nobody wrote
    with pytest.raises(AssertionError, match="row 3 col 4"):
        H.check_exact(bad, ref, 20, 12)
    for r, c in ((1, 3), (H.GUARD + 20, 0), (H.GUARD + 2, 12)):
        bad = buf.clone()
        bad[r, c] = 1.0
        with pytest.raises(AssertionError, match="guard elements were written"):
            H.check_exact(bad, ref, 20, 12)
    z = torch.zeros(4, 4, dtype=torch.float64)
    zb, _, _ = H.padded(z, F32, "cpu")
    zb[H.GUARD, 0] = -0.0
    H.check_exact(zb, z, 4, 4)                                # -0 for a zero reference
    one = z + 1
    ob, _, _ = H.padded(one, F32, "cpu")
    ob[H.GUARD, 0] = 1.0000001
    with pytest.raises(AssertionError, match="1 of 16"):
        H.check_exact(ob, one, 4, 4)
