"""ops.gemm_flags: the kernel-selection flags (tile height among them) ops.gemm / ops.gemm_split add on their own, as a pure function.
Pins the values other tests and the measured configurations rest on (tests/test_host.py, tests/gemm_edge_helpers.wrapper_flags)."""
import itertools

import pytest

from editor_amd import ops

T208 = ops.EPI_TILE_ROWS(208)
PLAIN = dict(trans_a=0, trans_b=0, splitk=1, beta=0.0)


def flags(m, n, k=768, ldc=None, colsum=False, rowmap=False, **kw):
    """-> (option word, the tile rows it says)"""
    e = ops.gemm_flags(m, n, k, n if ldc is None else ldc, needs_pp=colsum or rowmap, **kw)
    return e, ((e >> 12) & 15) * 16 or 256


def test_the_pinned_plans():
    assert ops.gemm_tile_plan(2048, 512) == (208, True)
    assert flags(2048, 512) == (ops.EPI_PIPE128, 256) and flags(2047, 512) == (0, 256) and flags(2048, 504) == (0, 256)
    m = 3 * 128 * 129                                                    # the bench workload: 49 536 token rows
    assert flags(m, 768) == (T208, 208) and flags(m, 2304) == (0, 256) and flags(m, 3072) == (0, 256)
    assert flags(6192, 768) == (ops.EPI_PIPE128, 256)                     # the strong-scaling series' B_local = 16


@pytest.mark.parametrize("m,n,want", [(8256, 768, (ops.EPI_PIPE128, 256)), (8256, 3072, (T208, 208)), (16512, 768, (T208, 208)),
                                      (16512, 2304, (T208, 208))])
def test_live_rows_plan_only_when_their_tail_is_zero(m, n, want):
    assert flags(m, n) == want
    assert flags(m, n, live=True, live_dense=True) == want                # stochastic-depth compaction: zero rows behind the prefix
    assert flags(m, n, live=True) == (0, 256)                            # the compacted HMA head: unwritten rows, full tiles only
    assert flags(m, n, live=True, pair=True) == (0, 256)


def test_no_plan_for_what_the_short_tiles_do_not_take(monkeypatch):
    m, n = 49536, 768
    assert flags(m, n, **PLAIN) == (T208, 208)
    for kw in (dict(trans_a=1), dict(trans_b=1), dict(splitk=7), dict(beta=1.0), dict(k=100), dict(ldc=772)):
        assert flags(m, n, **dict(PLAIN, **kw)) == (0, 256), kw
    assert flags(m, 772) == (0, 256)
    # an explicit tile height is kept and read back, whatever the shape (EPI_TILE_ROWS(256) is no bit at all: "not given")
    e = T208 | ops.EPI_GELU
    assert flags(m, 2304, epilogue=e) == (e, 208) and flags(6192, 768, epilogue=e) == (e, 208) and flags(300, 256, epilogue=e) == (e, 208)
    assert flags(6192, 768, epilogue=T208, pair=True) == (T208, 208)
    monkeypatch.setattr(ops, "SHORT_TILES", False)                       # read at call time
    assert flags(m, n) == (0, 256) and flags(6192, 768) == (0, 256) and flags(m, n, pair=True) == (0, 256)


def test_pipe128_never_joins_what_needs_the_ping_pong_kernel():
    for m, n in itertools.product((2048, 6192, 8256, 16512, 49536), (512, 768, 2304, 3072)):
        th, narrow = ops.gemm_tile_plan(m, n)
        for cs, rm, fp in itertools.product((False, True), repeat=3):
            e, h = flags(m, n, epilogue=ops.EPI_FORCE_PP if fp else 0, colsum=cs, rowmap=rm)
            base = ops.EPI_FORCE_PP if fp else 0
            if narrow and not (cs or rm or fp):
                assert (e, h) == (ops.EPI_PIPE128, 256)
            else:
                assert not e & ops.EPI_PIPE128 and h == th and e == base | (T208 if th == 208 else 0), (m, n, cs, rm, fp)
        # the pair form: always the ping-pong kernel, gemm_tile_rows alone - and no layout or alignment condition (C refuses those)
        tr = ops.gemm_tile_rows(m, n)
        assert flags(m, n, pair=True) == flags(m, n, k=100, pair=True) == (T208 if tr == 208 else 0, tr)


def test_the_shape_predicate_is_shared():
    bf = ops.HALF_DTYPES[0]
    for m, n, k in itertools.product((2047, 2048), (504, 512, 516), (64, 100)):
        big = m >= 2048 and n >= 512 and n % 8 == 0 and k % 64 == 0
        assert ops.gemm_colsum_ok(m, n, k, bf, 0, 1, None) == big
        assert (flags(m, n, k=k) != (0, 256)) == big
