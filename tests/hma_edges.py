"""Forced token selections for the compacted (variable-length) HMA head at its edges - pure host arithmetic, shared by the host test
that pins every plan's target (tests/test_hma_edge_plans.py) and the GPU tests that run them (tests/test_gpu_hma_compact_edges.py).

A plan is a list of per-sample patch counts c_b in [0, N] (N = 128 patches, T = 129 tokens with the cls token): sample b becomes a
packed sequence of L_b = 1 + c_b rows, live_a = sum_b L_b = B + sum(counts) rows per modality (layout A, MA = roundup64(B * T) rows
allocated) and live_b = nmod * live_a rows of the joint block (layout B, MB = roundup64(nmod * B * T))."""
import torch

N, T = 128, 129
PLANS = ("one_token", "all", "r0", "r1", "r63", "b0", "b1", "b63", "t256", "t256p1", "small", "skewed", "typical")
# residue targets (modulus, remainder) of live_a.  b0 / b1 / b63: (3 * live_a) % 64 == 0 / 1 / 63 <=> live_a % 64 == 0 / 43 / 21
# (3 * 43 = 129, 3 * 21 = 63).  With four modalities 4 * live_a is a multiple of 4, so it cannot hit 1 or 63; the same plans then
# put live_b on 0 / 44 / 20 - still a residue different from live_a's, which is what the b-plans are for.
RESIDUE = {"r0": (64, 0), "r1": (64, 1), "r63": (64, 63), "b0": (64, 0), "b1": (64, 43), "b63": (64, 21), "t256": (256, 0),
           "t256p1": (256, 1)}
# (plan, B) pairs every GPU section draws from; B = 128 (the timed shape: MA = 16 512, MB = 49 536) for r1, b1, t256p1, all, typical
CASES = [("one_token", 8), ("one_token", 64), ("all", 8), ("all", 64), ("all", 128), ("r0", 64), ("r1", 8), ("r1", 64), ("r1", 128),
         ("r63", 8), ("r63", 64), ("b0", 8), ("b1", 8), ("b1", 64), ("b1", 128), ("b63", 64), ("t256", 8), ("t256", 64),
         ("t256p1", 8), ("t256p1", 64), ("t256p1", 128), ("small", 8), ("skewed", 8), ("skewed", 64), ("typical", 8),
         ("typical", 128)]


def up(x, k):
    return -(-x // k) * k


def _typical(b, seed):
    """counts drawn around 57 of 128 (what a batch of 128 selects), never below one patch"""
    g = torch.Generator().manual_seed(seed)
    return [int(v) for v in (57.0 + 9.0 * torch.randn(b, generator=g)).round().clamp(1, N)]


def _with_total(counts, total):
    """move the counts one patch at a time, round robin, until b + sum(counts) == total (every count stays in [1, N])"""
    counts = list(counts)
    want = total - len(counts)
    assert len(counts) <= want <= N * len(counts), (total, len(counts))
    i = 0
    while sum(counts) != want:
        step = 1 if sum(counts) < want else -1
        if 1 <= counts[i % len(counts)] + step <= N:
            counts[i % len(counts)] += step
        i += 1
    return counts


def counts_for(name, b, seed=0):
    """per-sample patch counts of plan `name` for a batch of b"""
    if name == "one_token":
        return [0] * b
    if name == "all":
        return [N] * b
    if name == "skewed":
        c = [1 + (i % 3) for i in range(b)]
        c[b // 2] = N                                   # the longest sequence between length-2 .. 4 neighbours
        return c
    base = _typical(b, 1000 + 17 * b + seed)
    if name == "typical":
        return base
    if name == "small":
        return _with_total([1] * b, max(2 * b, min(48, 63)))       # live_a = 48 < 64 at b = 8
    q, r = RESIDUE[name]
    cur = b + sum(base)
    total = cur - (cur - r) % q                         # nearest total below with total % q == r ...
    if total < 2 * b:
        total += q                                      # ... that still leaves every sample a patch
    return _with_total(base, total)


def check_plan(name, b, counts):
    """the property each plan is FOR - asserted wherever a plan is built, so no case can go vacuous if a helper changes"""
    assert len(counts) == b and all(0 <= c <= N for c in counts), (name, b)
    live = b + sum(counts)
    ma = up(b * T, 64)
    assert live <= b * T <= ma
    if name == "one_token":
        assert live == b and set(counts) == {0}
    elif name == "all":
        assert live == b * T
        if b in (64, 128):
            assert live == ma                           # no pad rows at all
    elif name in RESIDUE:
        q, r = RESIDUE[name]
        assert live % q == r, (name, b, live)
        if name in ("b0", "b1", "b63"):
            want3 = {"b0": 0, "b1": 1, "b63": 63}[name]
            assert (3 * live) % 64 == want3, (name, b, live)
            if name != "b0":
                assert (4 * live) % 64 != live % 64 and (2 * live) % 64 != live % 64, (name, b, live)
        if name == "t256p1":
            assert live > 256
        assert min(counts) >= 1
    elif name == "small":
        assert live < 64 and ma >= 256, (b, live, ma)
    elif name == "skewed":
        assert max(counts) == N and sorted(counts)[-2] <= 3 and min(counts) >= 1
        starts = [0]
        for c in counts:
            starts.append(starts[-1] + 1 + c)
        long_i = counts.index(N)
        assert starts[long_i] // 64 != (starts[long_i + 1] - 1) // 64       # the long sequence straddles 64-row boundaries
        assert any(starts[i] // 64 != (starts[i + 1] - 1) // 64 for i in range(b) if counts[i] <= 3) or b < 64
    elif name == "typical":
        assert min(counts) >= 1 and 45 * b <= sum(counts) <= 70 * b, (b, sum(counts))
    else:
        raise KeyError(name)
    return live


def make_index(counts, seed=0):
    """(B, N) uint8 selection with counts[b] ones at random patch positions of row b"""
    g = torch.Generator().manual_seed(4242 + seed)
    index = torch.zeros(len(counts), N, dtype=torch.uint8)
    for i, c in enumerate(counts):
        index[i, torch.randperm(N, generator=g)[:c]] = 1
    assert index.sum(1).tolist() == list(counts)
    return index


def edge_plan(name, b, seed=0):
    """-> (index (B, 128) uint8 on the host, live_a)"""
    counts = counts_for(name, b, seed)
    live = check_plan(name, b, counts)
    return make_index(counts, seed), live


def host_maps(index, nmod):
    """What editor_compact_plan / editor_compact_maps must build from `index` (csrc/compact.hip, layouts A and B), as int64 / uint8
    host tensors: cu, cu3, tok, map_a, map_b, map_cls, mask_a, mask_b and the extents ma, mb."""
    b, n = index.shape
    t = n + 1
    lens = 1 + index.long().sum(1)
    cu = torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)])
    live = int(cu[-1])
    ma, mb = up(b * t, 64), up(nmod * b * t, 64)
    tok = torch.zeros(live, dtype=torch.long)
    map_a = torch.full((nmod * ma,), -1, dtype=torch.long)
    map_b = torch.full((mb,), -1, dtype=torch.long)
    map_cls = torch.zeros(nmod * b, dtype=torch.long)
    for s in range(b):
        s0, ln = int(cu[s]), int(lens[s])
        tk = torch.cat([torch.zeros(1, dtype=torch.long), torch.nonzero(index[s]).flatten() + 1])
        tok[s0:s0 + ln] = tk
        for m in range(nmod):
            map_a[m * ma + s0:m * ma + s0 + ln] = (m * b + s) * t + tk
            map_b[nmod * s0 + m * ln:nmod * s0 + (m + 1) * ln] = m * ma + s0 + torch.arange(ln)
            map_cls[m * b + s] = m * ma + s0
    mask_a = torch.zeros(ma, dtype=torch.uint8)
    mask_a[:live] = 1
    mask_b = torch.zeros(mb, dtype=torch.uint8)
    mask_b[:nmod * live] = 1
    return dict(cu=cu, cu3=nmod * cu, tok=tok, map_a=map_a, map_b=map_b, map_cls=map_cls, mask_a=mask_a, mask_b=mask_b, ma=ma, mb=mb,
                live=live)
