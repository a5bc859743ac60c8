"""Which argument sets the 16-bit GEMM entries refuse (return code 1 = hipErrorInvalidValue) before they touch the runtime.

Every row is a call one of the GPU suites makes successfully (named beside its base) with ONE argument changed.  The addresses are made
up (16-byte aligned, never dereferenced: every row is refused ahead of the first HIP call), so this runs without a device.  There is
no accepted argument set in here on purpose: such a call would go on to the runtime."""
import ctypes

import pytest

from device_entropy_helpers import cdll

P = 0x7F0000001000                                          # a made-up device address, 16-byte aligned
COLSUM, FORCE_PP, AUX_GRAD, PIPE128 = 0x100, 0x200, 0x400, 0x800   # include/editor_hip.h
RESIDUAL, GELU, GELU_BWD = 1, 2, 3
T208, T240, STAGGER1 = 13 << 12, 15 << 12, 1 << 17
INVALID = 1


def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _ints(*vals):
    return (ctypes.c_int * len(vals))(*vals)


def _refused(entry, names, base, change):
    args = dict(base)
    assert set(change) <= set(args) and len(change) == 1, change
    args.update(change)
    rc = getattr(cdll(), entry)(*[args[k] for k in names.split()], None)           # (the stream comes last everywhere)
    assert rc == INVALID, (entry, change, rc)


def _ids(rows):
    return ["%s-%s" % (r[0], "-".join("%s=%s" % (k, v if isinstance(v, (int, float)) else "x") for k, v in r[-1].items())) for r in rows]


# ---------------------------------------------------------------------------------------------------------------------------
# editor_gemm_bf16 / _f16
# ---------------------------------------------------------------------------------------------------------------------------
H16 = "A B C c_f32 m n k lda ldb ldc ta tb alpha beta bias rs splitk epi aux ldaux ws live"
# test_gpu_gemm_edges: the forced ping-pong case 264 x 256 x 256 on padded buffers (k-major, transposed A, transposed B), its fp32
# residual epilogue, the 208-row case 417 x 520 x 192
PP = dict(A=P, B=P, C=P, c_f32=0, m=264, n=256, k=256, lda=264, ldb=264, ldc=264, ta=0, tb=0, alpha=0.5, beta=0.0, bias=P, rs=P, splitk=1,
          epi=FORCE_PP, aux=None, ldaux=264, ws=None, live=None)
PP_TA, PP_TB = dict(PP, ta=1, lda=272), dict(PP, tb=1)
PP_RES = dict(PP, c_f32=1, epi=FORCE_PP | RESIDUAL, aux=P)
SHORT = dict(PP, m=417, n=520, k=192, lda=200, ldb=200, ldc=528, ldaux=528, epi=T208)
# test_gpu_two_stage_fold.test_gemm_colsum: 2080 x 512 x 64, contiguous, with the flags ops.gemm adds there
CS = dict(A=P, B=P, C=P, c_f32=0, m=2080, n=512, k=64, lda=64, ldb=64, ldc=512, ta=0, tb=0, alpha=1.0, beta=0.0, bias=None, rs=None,
          splitk=1, epi=COLSUM | T208, aux=None, ldaux=512, ws=P, live=None)
H16_ROWS = [
    # the names of gemm_edge_helpers.REFUSALS
    ("lda", PP, dict(lda=268)), ("ldb", PP, dict(ldb=268)), ("n_mod4", PP, dict(n=254)), ("k_mod8", PP, dict(k=252)),
    ("ta_m_mod8", PP_TA, dict(m=260)), ("tb_n_mod8", PP_TB, dict(n=252)), ("pointer", PP, dict(A=P + 2)),
    ("splitk_h16_c", PP, dict(splitk=2)), ("splitk_epilogue", PP_RES, dict(splitk=2)), ("auxgrad_plain", PP, dict(epi=FORCE_PP | AUX_GRAD)),
    ("t208_transposed", SHORT, dict(tb=1)), ("t208_narrow", SHORT, dict(n=128)), ("t208_few_rows", SHORT, dict(m=208)),
    ("tile_rows_240", PP, dict(epi=T240)),
    # the other clauses ahead of the first launch
    ("no_rows", PP, dict(m=0)), ("ldc_mod4", PP, dict(ldc=266)), ("pointer_b", PP, dict(B=P + 8)), ("pointer_c", PP, dict(C=P + 4)),
    ("residual_no_aux", PP_RES, dict(aux=None)), ("ldaux_mod4", PP_RES, dict(ldaux=266)),
    ("t208_transposed_a", SHORT, dict(ta=1)), ("t208_beta", SHORT, dict(beta=0.5)), ("t208_ldc", SHORT, dict(ldc=524)),
    ("t208_ldaux", SHORT, dict(ldaux=524)), ("t208_k", SHORT, dict(k=200)), ("t208_n_mod8", SHORT, dict(n=516)),
    # EDITOR_EPI_COLSUM, clause by clause
    ("colsum_f32_c", CS, dict(c_f32=1)), ("colsum_residual", CS, dict(epi=COLSUM | T208 | RESIDUAL)), ("colsum_splitk", CS, dict(splitk=2)),
    ("colsum_no_ws", CS, dict(ws=None)), ("colsum_trans_a", CS, dict(ta=1)), ("colsum_m", CS, dict(m=2047)), ("colsum_n", CS, dict(n=504)),
    ("colsum_n_mod8", CS, dict(n=516)), ("colsum_ldc_mod8", CS, dict(ldc=516)), ("colsum_ldaux_mod8", CS, dict(ldaux=516)),
    ("colsum_k_mod64", CS, dict(k=72)), ("colsum_beta", CS, dict(beta=1.0)),
]


@pytest.mark.parametrize("entry", ["editor_gemm_bf16", "editor_gemm_f16"])
@pytest.mark.parametrize("row", H16_ROWS, ids=_ids(H16_ROWS))
def test_gemm_h16_refusals(row, entry):
    _refused(entry, H16, row[1], row[2])


def test_the_edge_suite_refusals_are_all_here():
    from gemm_edge_helpers import REFUSALS
    assert set(REFUSALS) - {r[0] for r in H16_ROWS} == {"f32_rowscale_splitk"}       # (the fp32 entry: below)


def test_gemm_f32_refuses_a_row_scale_with_split_k():
    # test_gpu_gemm_edges: the fp32 atomic split-K case 129 x 130 x 100, padded by one column
    names = "A B C m n k lda ldb ldc ta tb b1 sa1 sb1 sc1 b2 sa2 sb2 sc2 alpha beta bias rs splitk epi aux ldaux"
    base = dict(A=P, B=P, C=P, m=129, n=130, k=100, lda=101, ldb=101, ldc=131, ta=0, tb=0, b1=1, sa1=0, sb1=0, sc1=0, b2=1, sa2=0, sb2=0,
                sc2=0, alpha=0.5, beta=0.0, bias=P, rs=None, splitk=2, epi=0, aux=None, ldaux=131)
    _refused("editor_gemm_f32", names, base, dict(rs=P))


# ---------------------------------------------------------------------------------------------------------------------------
# editor_gemm_h16_rows (test_gpu_dropskip: fc2 of a compacted MLP, 24 x 129 rows, with the tile rows ops.gemm adds there)
# ---------------------------------------------------------------------------------------------------------------------------
ROWS = "dtype A B C m n k lda ldb ldc alpha bias rs epi aux ldaux live rowmap"
RM = dict(dtype=1, A=P, B=P, C=P, m=3096, n=768, k=3072, lda=3072, ldb=3072, ldc=768, alpha=1.0, bias=P, rs=P, epi=RESIDUAL | T208, aux=P,
          ldaux=768, live=P, rowmap=P)
RM_ROWS = [("rows", RM, c) for c in (dict(rowmap=None), dict(dtype=0), dict(dtype=3), dict(epi=T208), dict(epi=GELU | T208), dict(m=248),
                                     dict(n=248), dict(n=772), dict(ldc=772), dict(ldaux=772), dict(k=3080), dict(aux=None))]


@pytest.mark.parametrize("row", RM_ROWS, ids=_ids(RM_ROWS))
def test_gemm_h16_rows_refusals(row):
    _refused("editor_gemm_h16_rows", ROWS, row[1], row[2])
    if "dtype" not in row[2]:
        _refused("editor_gemm_h16_rows", ROWS, dict(row[1], dtype=2), row[2])


# ---------------------------------------------------------------------------------------------------------------------------
# editor_gemm_f16x2 / _rows (test_gpu_gemm_edges: the split-mode case 257 x 520 x 192, pair output and fp32 residual output;
# test_gpu_dropskip_edges: the compacted split-precision fc2)
# ---------------------------------------------------------------------------------------------------------------------------
X2 = "A_hi A_lo B_hi B_lo C C_lo c_f32 m n k lda ldb ldc alpha bias rs epi aux ldaux live"
SP = dict(A_hi=P, A_lo=P, B_hi=P, B_lo=P, C=P, C_lo=P, c_f32=0, m=257, n=520, k=192, lda=200, ldb=200, ldc=528, alpha=1.0, bias=P, rs=P,
          epi=0, aux=None, ldaux=528, live=None)
SP_RES = dict(SP, C_lo=None, c_f32=1, epi=RESIDUAL, aux=P)
SP_GELU = dict(SP, epi=GELU | AUX_GRAD, aux=P)
X2_ROWS = [("pair", SP, c) for c in (
    dict(m=0), dict(n=0), dict(k=0), dict(k=200), dict(n=516), dict(lda=204), dict(ldb=204), dict(ldc=532), dict(ldaux=532),
    dict(A_hi=None), dict(A_lo=None), dict(B_hi=None), dict(B_lo=None), dict(C=None), dict(C_lo=None), dict(c_f32=1),
    dict(A_hi=P + 2), dict(A_lo=P + 4), dict(B_hi=P + 8), dict(B_lo=P + 2), dict(C=P + 8), dict(C_lo=P + 8),
    dict(epi=T240), dict(epi=STAGGER1), dict(epi=PIPE128), dict(epi=COLSUM), dict(epi=GELU_BWD), dict(epi=RESIDUAL), dict(epi=GELU))]
# (two clauses no row can single out: "RESIDUAL needs fp32 C" and "GELU needs 16-bit C".  The output type is two arguments, c_f32 and
#  C_lo, so one change away from a working call the C_lo check ahead of them refuses first - the c_f32 rows below stop there)
X2_ROWS += [("residual", SP_RES, c) for c in (dict(aux=None), dict(c_f32=0), dict(C_lo=P))]
X2_ROWS += [("gelu", SP_GELU, c) for c in (dict(epi=GELU), dict(epi=GELU | AUX_GRAD | STAGGER1))]


@pytest.mark.parametrize("row", X2_ROWS, ids=_ids(X2_ROWS))
def test_gemm_f16x2_refusals(row):
    _refused("editor_gemm_f16x2", X2, row[1], row[2])


X2R = "A_hi A_lo B_hi B_lo C m n k lda ldb ldc alpha bias rs epi aux ldaux live rowmap"
SPR = dict(A_hi=P, A_lo=P, B_hi=P, B_lo=P, C=P, m=3096, n=768, k=3072, lda=3072, ldb=3072, ldc=768, alpha=1.0 / 256, bias=P, rs=P,
           epi=RESIDUAL | T208, aux=P, ldaux=768, live=P, rowmap=P)
X2R_ROWS = [("rows", SPR, c) for c in (dict(rowmap=None), dict(epi=T208), dict(m=248), dict(n=248), dict(k=3080), dict(ldc=772), dict(aux=None),
                                       dict(epi=RESIDUAL | T208 | PIPE128))]


@pytest.mark.parametrize("row", X2R_ROWS, ids=_ids(X2R_ROWS))
def test_gemm_f16x2_rows_refusals(row):
    _refused("editor_gemm_f16x2_rows", X2R, row[1], row[2])


# ---------------------------------------------------------------------------------------------------------------------------
# editor_gemm_group (test_gpu_hma_compact_edges: the three modality blocks' qkv products, shared live-row count)
# ---------------------------------------------------------------------------------------------------------------------------
GROUP = "dtype count A B C c_f32 m n k lda ldb ldc alpha bias rs epi aux ldaux live"
FOUR = _ptrs(P, P, P, P)
GR = dict(dtype=1, count=3, A=FOUR, B=FOUR, C=FOUR, c_f32=0, m=2304, n=2304, k=768, lda=768, ldb=768, ldc=2304, alpha=1.0, bias=FOUR, rs=None,
          epi=0, aux=None, ldaux=2304, live=P)
GR_RES = dict(GR, c_f32=1, n=768, ldc=768, ldaux=768, epi=RESIDUAL, aux=FOUR)
GR_ROWS = [("qkv", GR, c) for c in (
    dict(dtype=0), dict(dtype=3), dict(count=0), dict(count=5), dict(m=255), dict(n=128), dict(n=2312), dict(k=0), dict(k=776),
    dict(lda=772), dict(ldb=772), dict(ldc=2308), dict(ldaux=2308), dict(epi=T208), dict(epi=COLSUM), dict(epi=PIPE128), dict(epi=STAGGER1),
    dict(epi=4), dict(epi=AUX_GRAD), dict(epi=RESIDUAL), dict(A=_ptrs(P, None, P, P)), dict(B=_ptrs(None, P, P, P)), dict(C=_ptrs(P, P, None, P)),
    dict(A=_ptrs(P, P + 8, P, P)), dict(C=_ptrs(P + 2, P, P, P)))]
GR_ROWS += [("proj", GR_RES, c) for c in (dict(aux=None), dict(aux=_ptrs(P, P, None, P)))]


@pytest.mark.parametrize("row", GR_ROWS, ids=_ids(GR_ROWS))
def test_gemm_group_refusals(row):
    _refused("editor_gemm_group", GROUP, row[1], row[2])
    if "dtype" not in row[2]:
        _refused("editor_gemm_group", GROUP, dict(row[1], dtype=2), row[2])


# ---------------------------------------------------------------------------------------------------------------------------
# editor_gemm_wgrad_group / _live / _ln (test_gpu_gemm_edges: three problems over 128 rows; test_gpu_two_stage_fold: a ViT-B block's
# four weight gradients over 64 x 129 rows beside its LayerNorm backward)
# ---------------------------------------------------------------------------------------------------------------------------
WG = "dtype count dy x dw N K m alpha splitk ws"
WGR = dict(dtype=1, count=3, dy=FOUR, x=FOUR, dw=FOUR, N=_ints(256, 512, 256, 0), K=_ints(256, 256, 768, 0), m=128, alpha=0.5, splitk=1, ws=P)
WG_CHANGES = (dict(dtype=0), dict(dtype=3), dict(count=0), dict(count=5), dict(m=0), dict(m=100), dict(splitk=0), dict(ws=None),
              dict(N=_ints(256, 520, 256, 0)), dict(K=_ints(256, 256, 776, 0)), dict(dy=_ptrs(P, None, P, P)), dict(x=_ptrs(None, P, P, P)),
              dict(dw=_ptrs(P, P, None, P)), dict(x=_ptrs(P, P + 8, P, P)), dict(dw=_ptrs(P + 4, P, P, P)))
WG_ROWS = [("wgrad", WGR, c) for c in WG_CHANGES]


@pytest.mark.parametrize("row", WG_ROWS, ids=_ids(WG_ROWS))
def test_gemm_wgrad_group_refusals(row):
    _refused("editor_gemm_wgrad_group", WG + " live", dict(row[1], live=None), row[2])
    _refused("editor_gemm_wgrad_group_live", WG + " live", dict(row[1], live=_ptrs(P, None, P, P)), row[2])


def test_gemm_wgrad_group_live_needs_its_live_array():
    _refused("editor_gemm_wgrad_group_live", WG + " live", dict(WGR, live=FOUR), dict(live=None))


LN = WG + " ln_dy dy_scale ln_x gamma mean rstd rows d dx_in dx parts dx16 rowscale scale cparts nmem"
LNR = dict(dtype=1, count=4, dy=FOUR, x=FOUR, dw=FOUR, N=_ints(2304, 768, 3072, 768), K=_ints(768, 768, 768, 3072), m=8256, alpha=1.0,
           splitk=7, ws=P, ln_dy=P, dy_scale=0.5, ln_x=P, gamma=P, mean=P, rstd=P, rows=8256, d=768, dx_in=P, dx=P, parts=P, dx16=P, rowscale=P,
           scale=2.0, cparts=P, nmem=64)
LN_ROWS = [("ln", LNR, c) for c in (
    dict(dtype=0), dict(dtype=3), dict(d=512), dict(nmem=4), dict(nmem=12), dict(nmem=264), dict(rows=0), dict(ln_dy=None), dict(ln_x=None),
    dict(gamma=None), dict(mean=None), dict(rstd=None), dict(dx=None), dict(parts=None), dict(dx16=None), dict(ln_dy=P + 4), dict(ln_x=P + 8),
    dict(dx=P + 8), dict(dx_in=P + 4), dict(gamma=P + 8), dict(dx16=P + 2), dict(m=8250), dict(count=5), dict(ws=None),
    dict(N=_ints(2304, 768, 3080, 768)))]


@pytest.mark.parametrize("row", LN_ROWS, ids=_ids(LN_ROWS))
def test_gemm_wgrad_group_ln_refusals(row):
    _refused("editor_gemm_wgrad_group_ln", LN, row[1], row[2])
