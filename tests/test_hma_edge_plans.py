"""Host arithmetic of the edge plans the compacted HMA head is tested at (tests/hma_edges.py): every plan hits the live-row count it is
named for, so the GPU cases of tests/test_gpu_hma_compact_edges.py cannot go vacuous.  (That module is GPU-only as a whole - its
pytestmark - so the host-side assertion lives here, on the same helpers.)"""
import pytest

import hma_edges as he


def test_every_plan_is_covered_and_the_timed_shape_gets_its_plans():
    assert {n for n, _ in he.CASES} == set(he.PLANS)
    assert {b for _, b in he.CASES} == {8, 64, 128}
    for name in ("r1", "b1", "t256p1", "all", "typical"):
        assert (name, 128) in he.CASES
    assert he.up(128 * he.T, 64) == 16512 and he.up(3 * 128 * he.T, 64) == 49536


@pytest.mark.parametrize("name,b", he.CASES)
def test_edge_plan_hits_its_target(name, b):
    counts = he.counts_for(name, b)
    live = he.check_plan(name, b, counts)
    index, live2 = he.edge_plan(name, b)
    assert live2 == live == b + int(index.sum())
    ma = he.up(b * he.T, 64)
    want = {"one_token": live == b, "all": live == b * he.T and (b == 8 or live == ma), "r0": live % 64 == 0, "r1": live % 64 == 1,
            "r63": live % 64 == 63, "b0": 3 * live % 64 == 0, "b1": 3 * live % 64 == 1, "b63": 3 * live % 64 == 63,
            "t256": live % 256 == 0, "t256p1": live % 256 == 1, "small": live < 64 and ma >= 256,
            "skewed": max(counts) == 128 and sorted(counts)[-2] <= 3, "typical": abs(sum(counts) / b - 57) < 12}[name]
    assert want, (name, b, live)
    if name in ("r1", "b1", "t256p1", "skewed", "all"):             # the whole-model plans keep at least one patch per sample
        assert min(counts) >= 1


def test_host_maps_are_consistent():
    index, live = he.edge_plan("skewed", 8)
    for nmod in (2, 3, 4):
        h = he.host_maps(index, nmod)
        assert h["live"] == live and int(h["mask_a"].sum()) == live and int(h["mask_b"].sum()) == nmod * live
        named = h["map_b"][h["map_b"] >= 0]
        assert named.numel() == nmod * live and named.unique().numel() == named.numel()       # every layout-A row once
        assert bool((h["map_a"][named] >= 0).all())
        assert h["map_cls"].tolist() == [m * h["ma"] + int(h["cu"][s]) for m in range(nmod) for s in range(8)]
