"""Own ground of the token-selection edge suite (tests/test_select_edges_host.py on the CPU, tests/test_gpu_select_edges.py on the
device): a plain-Python port of the lane-0 walk of topk_mask_kernel (csrc/select.hip) that records the path it took, McIlroy's
adaptive adversary run against that port, the table of top-k cases both modules share, and the case lists, operands and float64
references of the rollout and frequency-count tests.

The port mirrors select.hip function by function (push_heap_, adjust_heap_, heap_select_, insertion_sort_, introselect_ and the
`k * 64 <= n` dispatch) on a list of (value, index) pairs.  Only the 8-wide scan of heap_select_ is not mirrored: the kernel reads
eight candidates up front, but every candidate lies beyond `middle`, a replacement writes only below `middle` and the candidate's
own slot, and the candidates are still tested one after the other against the current top - the comparisons and moves are those of
the scalar loop in the same order, so the scalar loop stands for both."""
import collections
import functools
import math

import torch

I32, F32 = torch.int32, torch.float32


# ---------------------------------------------------------------------------------------------------------------------------
# the walk
# ---------------------------------------------------------------------------------------------------------------------------
def before_int(x, y):
    return x > y


def before_float(x, y):
    """select.hip: (isnan(x) && !isnan(y)) || (x > y) - NaN first, as torch.topk orders it"""
    return (x != x and y == y) or x > y


class Path:
    """What one row's walk did."""

    def __init__(self):
        self.selector = None          # "heap_select" | "introselect": the dispatch's choice
        self.scan = None              # heap_select as the selector: candidates scanned, n - k
        self.levels = 0               # introselect: partition levels used
        self.depth_limit = None       # introselect: levels allowed, 2 * floor(log2 n)
        self.fallback = None          # (first, nth, last) when the depth limit handed the rest to heap_select_
        self.insertion_only = False   # introselect that never partitioned (n <= 3)

    def key(self):
        return (self.selector, self.scan, self.levels, self.depth_limit, self.fallback, self.insertion_only)


def push_heap_(r, base, hole, top, val, before):
    parent = (hole - 1) // 2
    while hole > top and before(r[base + parent][0], val[0]):
        r[base + hole] = r[base + parent]
        hole = parent
        parent = (hole - 1) // 2
    r[base + hole] = val


def adjust_heap_(r, base, hole, length, val, before):
    top = hole
    child = hole
    while child < (length - 1) // 2:
        child = 2 * (child + 1)
        if before(r[base + child][0], r[base + child - 1][0]):
            child -= 1
        r[base + hole] = r[base + child]
        hole = child
    if (length & 1) == 0 and child == (length - 2) // 2:
        child = 2 * (child + 1)
        r[base + hole] = r[base + child - 1]
        hole = child - 1
    push_heap_(r, base, hole, top, val, before)


def heap_select_(r, base, middle, last, before):
    """heap over r[base .. base + middle), candidates r[base + middle .. base + last) (both relative to base, as in select.hip)"""
    if middle >= 2:
        parent = (middle - 2) // 2
        while True:
            adjust_heap_(r, base, parent, middle, r[base + parent], before)
            if parent == 0:
                break
            parent -= 1
    for i in range(middle, last):
        if before(r[base + i][0], r[base][0]):
            val = r[base + i]
            r[base + i] = r[base]
            adjust_heap_(r, base, 0, middle, val, before)


def insertion_sort_(r, first, last, before):
    if first == last:
        return
    for i in range(first + 1, last):
        val = r[i]
        if before(val[0], r[first][0]):
            for j in range(i, first, -1):
                r[j] = r[j - 1]
            r[first] = val
        else:
            cur, nxt = i, i - 1
            while before(val[0], r[nxt][0]):
                r[cur] = r[nxt]
                cur = nxt
                nxt -= 1
            r[cur] = val


def introselect_(r, first, nth, last, depth, before, path):
    while last - first > 3:
        if depth == 0:
            path.fallback = (first, nth, last)
            heap_select_(r, first, nth + 1 - first, last - first, before)
            r[first], r[nth] = r[nth], r[first]
            return
        depth -= 1
        path.levels += 1
        mid = first + (last - first) // 2
        a, b, c = first + 1, mid, last - 1
        va, vb, vc = r[a][0], r[b][0], r[c][0]
        if before(va, vb):
            med = b if before(vb, vc) else (c if before(va, vc) else a)
        else:
            med = a if before(va, vc) else (c if before(vb, vc) else b)
        r[first], r[med] = r[med], r[first]
        lo, hi = first + 1, last
        pv = r[first][0]
        while True:
            while before(r[lo][0], pv):
                lo += 1
            hi -= 1
            while before(pv, r[hi][0]):
                hi -= 1
            if not lo < hi:
                break
            r[lo], r[hi] = r[hi], r[lo]
            lo += 1
        if lo <= nth:
            first = lo
        else:
            last = lo
    path.insertion_only = path.levels == 0
    insertion_sort_(r, first, last, before)


def walk(values, k, before):
    """One row of topk_mask_kernel: -> (the k selected indices in the order the walk leaves them, Path)."""
    n = len(values)
    assert 1 <= k <= n
    r = [(v, i) for i, v in enumerate(values)]
    path = Path()
    if k * 64 <= n:
        path.selector, path.scan = "heap_select", n - k
        heap_select_(r, 0, k, n, before)
    else:
        path.selector, path.depth_limit = "introselect", 2 * (n.bit_length() - 1)
        introselect_(r, 0, k - 1, n, path.depth_limit, before, path)
    return [p[1] for p in r[:k]], path


def before_of(dtype):
    return before_int if dtype == I32 else before_float


def walk_rows(x, k):
    """x (rows, n) int32 / float32 CPU tensor -> (bool mask (rows, n) of the walk's selections, [Path per row])"""
    before = before_of(x.dtype)
    mask = torch.zeros(x.shape, dtype=torch.bool)
    paths = []
    for i, row in enumerate(x.tolist()):
        idx, p = walk(row, k, before)
        assert len(set(idx)) == k
        mask[i, idx] = True
        paths.append(p)
    return mask, paths


# ---------------------------------------------------------------------------------------------------------------------------
# McIlroy's adversary ("A killer adversary for quicksort", 1999) against the walk
# ---------------------------------------------------------------------------------------------------------------------------
def adversary_row(n, k, sign):
    """Runs the walk on n items whose values are decided lazily: an item is `gas` until a comparison forces a value on it; two gas
    items compared freeze one of them (the pivot candidate) at the next solid value; gas compares beyond every solid value.
    sign = +1: gas is LARGEST (it goes before every solid item, the walk's `last` creeps down); sign = -1: gas is SMALLEST (`first`
    creeps up).  -> (list of n distinct ints in [0, n) that replay the same comparisons under before_int, Path of the lazy run)."""
    gas = n
    val = [gas] * n
    state = {"solid": 0, "candidate": 0}

    def freeze(x):
        val[x] = state["solid"]
        state["solid"] += 1

    def before(x, y):
        if val[x] == gas and val[y] == gas:
            freeze(x if x == state["candidate"] else y)
        if val[x] == gas:
            state["candidate"] = x
        elif val[y] == gas:
            state["candidate"] = y
        return val[x] > val[y] if sign > 0 else val[x] < val[y]

    _, path = walk(list(range(n)), k, before)
    for x in range(n):                     # items never compared with another gas item: any distinct values beyond the solid ones
        if val[x] == gas:
            freeze(x)
    assert sorted(val) == list(range(n))
    return (val if sign > 0 else [n - 1 - v for v in val]), path


def quantise(row, d):
    """tie-bearing variant of a row of ints: row // d"""
    return [v // d for v in row]


# ---------------------------------------------------------------------------------------------------------------------------
# the top-k case table
# ---------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name dtype rows n k group values")

N_VALUES = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 210, 1023, 1024, 1025, 4096)
ROWS = (1, 3, 5, 7)
GROUPED = ((6, 3), (36, 12))               # (rows, group)
GROUPED_N = (129, 210, 1025)
FAMILIES = ("tie_i32", "tie_f32", "equal", "uniform", "special")
SPECIALS = (float("nan"), float("inf"), -float("inf"), 0.0, -0.0)
# adversary rows: (n, k) - 128 / 210 / 512 / 2048 columns; k = 10 at 512 as well (the frequency branch's keep)
ADVERSARY = ((128, 10), (210, 105), (512, 256), (512, 10), (2048, 1024))
QUANTA = (1, 2, 4, 8)


def k_values(n):
    ks = [1, 2, 3, n // 64, n // 64 + 1, n // 2, n - 1, n]
    return sorted({k for k in ks if 1 <= k <= n})


def family_values(family, rows, n, gen):
    if family == "tie_i32":
        return torch.randint(90, 110, (rows, n), generator=gen, dtype=I32)
    if family == "tie_f32":
        return torch.randint(0, 4, (rows, n), generator=gen).float()
    if family == "equal":
        return torch.full((rows, n), 7, dtype=I32) if (rows + n) & 1 else torch.full((rows, n), 0.5)
    if family == "uniform":
        return torch.rand(rows, n, generator=gen)
    assert family == "special"
    x = torch.randint(0, 4, (rows, n), generator=gen).float()
    pick = torch.randint(0, 16, (rows, n), generator=gen)
    for i, s in enumerate(SPECIALS):
        x[pick == i] = s
    return x


@functools.lru_cache(maxsize=None)
def adversary_rows():
    """{(n, k, sign): row of distinct ints}"""
    return {(n, k, s): adversary_row(n, k, s)[0] for n, k in ADVERSARY for s in (1, -1)}


@functools.lru_cache(maxsize=None)
def topk_table():
    gen = torch.Generator().manual_seed(2024)
    cases = []
    turn = 0
    for n in N_VALUES:
        for k in k_values(n):
            for fam in FAMILIES:
                rows = ROWS[turn % len(ROWS)]
                turn += 1
                v = family_values(fam, rows, n, gen)
                cases.append(Case("%s_n%d_k%d_r%d" % (fam, n, k, rows), v.dtype, rows, n, k, 1, v))
    for n in GROUPED_N:
        for rows, group in GROUPED:
            for k in (2, n // 64 + 1, n // 2):
                for fam in ("tie_i32", "special"):
                    v = family_values(fam, rows, n, gen)
                    cases.append(Case("%s_n%d_k%d_r%d_g%d" % (fam, n, k, rows, group), v.dtype, rows, n, k, group, v))
    for (n, k, s), row in adversary_rows().items():
        q = torch.tensor([quantise(row, d) for d in QUANTA], dtype=I32)            # one row per quantum: rows = 4
        name = "adversary%s_n%d_k%d" % ("+" if s > 0 else "-", n, k)
        cases.append(Case(name + "_i32", I32, len(QUANTA), n, k, 1, q))
        cases.append(Case(name + "_f32", F32, len(QUANTA), n, k, 1, q.float()))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


def table_n():
    return sorted({c.n for c in topk_table()})


def cases_for(n):
    return [c for c in topk_table() if c.n == n]


def kth_is_tied(row, k):
    """sorted[k-1] == sorted[k] in the walk's order (NaN first): another, equally large selection exists"""
    if k >= len(row):
        return False
    s = sorted(row, key=lambda v: (0, 0.0) if v != v else (1, -v))
    a, b = s[k - 1], s[k]
    return (a != a and b != b) or a == b


# the rows of tests/test_gpu_select.py::test_topk_wide_rows_and_nan that its docstring once credited with the depth limit
def wide_test_rows():
    asc = list(range(512))
    pipe = list(range(256)) + list(range(255, -1, -1))
    return {"ascending": asc, "descending": asc[::-1], "organ_pipe": pipe, "all_zero": [0] * 512}


WIDE_TEST_K = (10, 100)


# ---------------------------------------------------------------------------------------------------------------------------
# attention rollout
# ---------------------------------------------------------------------------------------------------------------------------
ROLLOUT_T = (2, 3, 5, 63, 64, 65, 129, 211, 256, 257, 511, 512, 513, 1024)
ROLLOUT_L = (1, 2, 3)
ROLLOUT_BH = (1, 3)
ROLLOUT_GAP = (0, 64)                      # floats between one layer's slab and the next
ROLLOUT_MIN_SCORE = 2.0 ** -100


def rollout_ldps(t):
    return sorted({t, (t + 3) // 4 * 4, t + 5})


def rollout_geometry(t):
    """editor_attn_rollout_f32's launch: -> (threads, row groups G, trip count of the remainder loop of row group 0)"""
    threads = (512 // t) * t
    if threads < 64:
        threads = t if t < 512 else 512
    g = max(1, threads // t)
    i = 0
    while i + 3 * g < t:
        i += 4 * g
    return threads, g, len(range(i, t, g))


def rollout_probs(t, scale=2.0):
    """(max L, max BH, t, t) fp32 softmax rows of randn * scale logits"""
    gen = torch.Generator().manual_seed(1000 + t)
    logits = torch.randn(max(ROLLOUT_L), max(ROLLOUT_BH), t, t, generator=gen, dtype=torch.float64) * scale
    return torch.softmax(logits, dim=-1).float()


def rollout_reference(probs, layers):
    """float64: r = A_{L-1}[0, :]; r = r @ A_l for l = L-2 .. 0; columns 1 onwards.  probs (>= layers, BH, t, t) fp32 -> (BH, t-1)"""
    a = probs[:layers].double()
    r = a[layers - 1][:, 0, :]
    for l in range(layers - 2, -1, -1):
        r = torch.einsum("bi,bij->bj", r, a[l])
    return r[:, 1:].contiguous()


def rollout_bound(ref, layers, t):
    """All terms are non-negative, so each of the L - 1 vector-matrix steps adds a relative error of at most about t * 2^-24 in any
    summation order (one rounding per product, at most t - 1 per sum); the fp32 inputs are the reference's inputs, exactly."""
    return layers * (t + 2) * 2.0 ** -24 * ref


# ---------------------------------------------------------------------------------------------------------------------------
# frequency counts
# ---------------------------------------------------------------------------------------------------------------------------
FREQ_GEOM = ((1, 16, 16), (1, 16, 80), (1, 48, 16), (17, 16, 16), (3, 32, 48))
FREQ_KINDS = ("noise", "zero", "cancel", "denormal", "inf", "nan")
# (form, C, byte offset of every pointer from a 16-byte boundary, modality counts)
FREQ_FORMS = (("4x4", 3, 0, (2, 3, 4)), ("2x2", 3, 8, (3, 4)), ("generic_unaligned", 3, 8, (2,)),
              ("generic_c1", 1, 0, (2, 3, 4)), ("generic_c4", 4, 0, (2, 3, 4)))


def freq_tiles(b, h, w):
    return b * (h // 16) * (w // 16)


def freq_launch_shape(b, h, w):
    """-> (tiles, blocks of the 4x4 form, its waves holding a live tile, its clamped tile slots, blocks of the 2x2 form)"""
    tiles = freq_tiles(b, h, w)
    blocks4 = -(-tiles // 16)
    return tiles, blocks4, -(-tiles // 4), blocks4 * 16 - tiles, -(-tiles // 4)


def freq_kernel(nmod, c, aligned):
    """freq_counts_launch's choice (select.hip), int32 output"""
    if c == 3 and aligned:
        return "freq_counts4_kernel<%d,3>" % nmod
    if c == 3 and nmod in (3, 4):
        return "freq_counts_kernel<%d,3>" % nmod
    return "freq_counts_kernel<0,0>"


def freq_operands(kind, nmod, c, b, h, w):
    """nmod images (b, c, h, w) of uniform noise in [-1, 1] whose LAST tile - the neighbour of the clamped slots of the 4x4 form -
    is of `kind`: left as noise, exactly zero in every modality, modalities that cancel to an exactly zero sum, denormals, or with
    one +inf / one NaN pixel in one modality."""
    gen = torch.Generator().manual_seed(7 * b + h + 3 * w + 100 * nmod + c + 1000 * FREQ_KINDS.index(kind))
    m = torch.rand(nmod, b, c, h, w, generator=gen) * 2 - 1
    ys, xs = slice(h - 16, h), slice(w - 16, w)
    if kind == "zero":
        m[:, -1, :, ys, xs] = 0.0
    elif kind == "cancel":                 # the transform is odd (haar_fwd(-x) == -haar_fwd(x) bit for bit): (a + -a) [+ c + -c | + 0] == 0
        m[1, -1, :, ys, xs] = -m[0, -1, :, ys, xs]
        if nmod == 3:
            m[2, -1, :, ys, xs] = 0.0
        elif nmod == 4:
            m[3, -1, :, ys, xs] = -m[2, -1, :, ys, xs]
    elif kind == "denormal":
        m[:, -1, :, ys, xs] *= 1e-41
    elif kind == "inf":
        m[nmod - 1, -1, c - 1, h - 11, w - 9] = float("inf")
    elif kind == "nan":
        m[0, -1, 0, h - 3, w - 6] = float("nan")
    else:
        assert kind == "noise"
    return [m[i].contiguous() for i in range(nmod)]


def freq_reference(oracle, mods):
    ref, _ = oracle.frequency_counts(mods[0], mods[1], mods[2] if len(mods) > 2 else None, extra=tuple(mods[3:]))
    return ref


GUARD_BYTE = 0xA5
GUARD_I32 = -1515870811                    # 0xA5A5A5A5
