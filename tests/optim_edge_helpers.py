"""Case tables, operand recipes, references and tolerances of the optimizer edge suite (test_optim_edges_host.py,
test_gpu_optim_edges.py): the multi-tensor SGD / AdamW updates, the overflow check, the device loss scaler, the split-precision
refresh and the multi-tensor transpose of csrc/train.hip.  Nothing here runs GPU code at import; every builder takes a device, so
the host test exercises the same code on the CPU.

ARENAS.  Every array a kernel touches is a slice of one buffer per kind (parameters, gradients, momentum / exp_avg, exp_avg_sq,
shadows, hi / lo pairs, transposes).  A slice starts GUARD sentinel elements behind a 32-byte boundary plus a chosen shift of 0..3
elements, and GUARD sentinels follow it: a write one element before or behind a tensor, or an update that runs into the neighbour,
changes a sentinel.  The sentinels are NaN bit patterns, so a kernel that READS one poisons its result or raises the overflow flag.

SGD IS EXACT.  p is a multiple of 2^-3 in [-4, 4], g an integer in [-8, 8], lr / wd / momentum / 1/scale powers of two from
2^-1 .. 2^-4 with lr * wd >= 2^-6 (EXACT_PAIRS): over three steps every product and sum is then representable in fp32 (at most
24 significant bits: asserted operation by operation on the host), so neither rounding nor the compiler's choice to contract
a * b + c into one fma can change a bit, and the reference is the float64 closed form  m <- mu m + (g s + wd p),  p <- p - lr m.

ADAMW IS HELD TO A DERIVED BOUND, one step from the device's own previous state (rounding cannot accumulate).  E = 2^-24 is the
largest relative error of one fp32 rounding; gs = g * s with s a power of two is exact.
  m' = m + fl(1 - b1) * (gs - m)         roundings: the difference (<= E (|gs| + |m|)), the constant and the product (2 E * 0.1
                                         (|gs| + |m|)), the sum (E |m'|, |m'| <= |m| + |gs|):      tol_m = 4 E (|m| + |gs|)
  v' = fl(b2) * v + fl(1 - b2) * gs^2    all terms >= 0: two roundings on the first term (constant, product), three on the second
                                         (square, constant, product), one for the sum:             tol_v = 4 E v'
  p' = p * fl(1 - fl(lr wd)) - u,  u = fl(lr / (1 - b1^t)) * (m' / (sqrt(v') / fl(sqrt(1 - b2^t)) + eps))
                                         p * decay: 3 roundings, the final difference one more (of |p'| <= |p| + |u|): 4 E |p| + E |u|;
                                         u: the device divides by ITS v' (4 E -> 2 E after the root), root, constant, quotient, + eps,
                                         m' / denom, constant, product: a worst-case count of 10 E |u| if every rounding pulled the
                                         same way.  They do not: the bound used is the one the issue states,
                                                                         tol_p = 4 E |p| + 8 E |u| + step_size * tol_m / denom,
                                         (the last term carries m's tolerance into u) and it is anchored on the host, not on the
                                         kernel: torch.optim.AdamW (CPU, fp32, foreach=False) stays below 1.0 of it (0.69 measured)
                                         at t = 1, 2, 1001 and gradient scales 1e-4, 1, 2^10, while a parameter that was not
                                         updated lies more than 1000 x outside it.  (Measured on gfx950: the kernel's worst
                                         element sits at 0.36 of tol_p, 0.22 of tol_m and 0.68 of tol_v.)
Zero-tolerance elements (m = g = 0) must be equal."""
from collections import namedtuple

import numpy as np
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
GUARD = 8                                 # sentinel elements before and after every slice
SLOT = 8                                  # slices start at a multiple of SLOT elements (+ GUARD + shift): 32 B for fp32, 16 B for 16 bit
SENT32 = 0x7FA5A5A5                       # a NaN as fp32
SENT16 = 0x7FA5                           # a NaN as bf16 and as f16
UNWRITTEN16 = 0x7FFF                      # output slices start as this NaN: an element a kernel skipped keeps it
E = 2.0 ** -24
THREADS, VEC, UNROLL = 256, 4, 8          # workgroup size, elements per 16-byte access, loads in flight of the check kernel
FLT_MAX = 3.4028234663852886e38


def chunk_elems():
    """Elements per workgroup of the multi-tensor kernels, from the library (a host function: no GPU needed)."""
    from editor_amd import _lib
    return int(_lib.lib().cdll.editor_sgd_chunk_elems())


# ---------------------------------------------------------------------------------------------------------------------------
# the size table of one launch
# ---------------------------------------------------------------------------------------------------------------------------
Entry = namedtuple("Entry", "name shape shadow grad lr wd")
# (-log2 lr, -log2 wd) with lr * wd >= 2^-6: three SGD steps stay exact for every momentum and 1/scale of 2^-1 .. 2^-4.  Unscaled
# gradients (1/scale = 1) need one bit more: twelve pairs still hold for any operands of the recipe, (2^-2, 2^-4) only for some - it
# goes to the 1-element tensor (the fourth entry), where the host test proves it for the operands used, so that all thirteen updated
# tensors have a pair of their own
EXACT_PAIRS = [(1, 1), (2, 3), (3, 1), (2, 4), (2, 2), (4, 1), (1, 3), (3, 3), (2, 1), (4, 2), (1, 2), (3, 2), (1, 4)]
MOMENTA = (2.0 ** -1, 2.0 ** -2, 2.0 ** -4)
INV_SCALES = (None, 2.0 ** -3)
SGD_STEPS = 3


def size_table(C=None):
    """Tensors of one launch, in mixed order (a chunk-to-tensor mix-up lands on a tensor of another size), each with its own
    lr / wd.  C - 1, C, C + 1, 2C + 7 straddle the chunk size; 1, 3, 5, 1023, 1027 have a tail behind the 16-byte body; the two
    weights get 16-bit shadows ((3, 5): odd numel, a tail in the shadow); `nograd` has no gradient this step."""
    C = C or chunk_elems()
    rows = [("c_plus1", (C + 1,), 0, 1), ("three", (3,), 0, 1), ("w33x64", (33, 64), 1, 1), ("one", (1,), 0, 1),
            ("two_c7", (2 * C + 7,), 0, 1), ("k1024", (1024,), 0, 1), ("five", (5,), 0, 1), ("c_minus1", (C - 1,), 0, 1),
            ("nograd", (7, 10), 1, 0), ("w3x5", (3, 5), 1, 1), ("k1027", (1027,), 0, 1), ("c", (C,), 0, 1), ("four", (4,), 0, 1),
            ("k1023", (1023,), 0, 1)]
    pairs = iter(EXACT_PAIRS)
    out = []
    for name, shape, shadow, grad in rows:
        a, b = next(pairs) if grad else (4, 3)               # (never read for a tensor without a gradient)
        out.append(Entry(name, shape, bool(shadow), bool(grad), 2.0 ** -a, 2.0 ** -b))
    return out


def numel(e):
    return int(np.prod(e.shape))


def index_of(table, name):
    return [e.name for e in table].index(name)


def chunk_tables(numels, C):
    """chunk_tensor, chunk_off as FusedSGD.__init__ builds them: chunk c covers [off, off + C) of tensor t."""
    chunk_t, chunk_o = [], []
    for i, n in enumerate(numels):
        for off in range(0, n, C):
            chunk_t.append(i)
            chunk_o.append(off)
    return chunk_t, chunk_o


# alignment classes: shift of the p, g and m / v slices from a 16-byte boundary, in floats (shadows shift with p)
ALIGN = {"aligned": (0, 0, 0), "g+1": (0, 1, 0), "g+2": (0, 2, 0), "g+3": (0, 3, 0), "p+1": (1, 0, 0), "all_off": (1, 3, 2)}
POISON_ALIGN = ("aligned", "g+1")


# ---------------------------------------------------------------------------------------------------------------------------
# arenas
# ---------------------------------------------------------------------------------------------------------------------------
class Arena:
    """One buffer holding a slice per tensor, sentinels around each.  raw: the integer view (bit patterns)."""

    def __init__(self, sizes, shift, dtype, device, fill=None):
        self.sizes, self.dtype = [int(n) for n in sizes], dtype
        self.bits = torch.int32 if dtype == F32 else torch.int16
        self.sentinel = SENT32 if dtype == F32 else SENT16
        self.offs, cur = [], 0
        for n in self.sizes:
            cur = -(-cur // SLOT) * SLOT
            self.offs.append(cur + GUARD + shift)
            cur = cur + GUARD + shift + n + GUARD
        self.total = -(-cur // SLOT) * SLOT
        host = torch.full((self.total,), self.sentinel, dtype=self.bits)
        self.inside = torch.zeros(self.total, dtype=torch.bool)
        for o, n in zip(self.offs, self.sizes):
            self.inside[o:o + n] = True
            if fill is not None:
                host[o:o + n] = fill
        self.raw = host.to(device)
        self.buf = self.raw.view(dtype)

    def view(self, i):
        return self.buf[self.offs[i]:self.offs[i] + self.sizes[i]]

    def raw_view(self, i):
        return self.raw[self.offs[i]:self.offs[i] + self.sizes[i]]

    def set(self, i, values):
        self.view(i).copy_(values.reshape(-1).to(self.dtype))

    def ptrs(self, present=None):
        es = self.buf.element_size()
        return [0 if (present is not None and not present[i]) else self.buf.data_ptr() + o * es for i, o in enumerate(self.offs)]

    def host(self):
        """-> list of CPU copies of the slices (one transfer)."""
        h = self.raw.cpu().view(self.dtype)
        return [h[o:o + n].clone() for o, n in zip(self.offs, self.sizes)]

    def snapshot(self):
        return self.raw.clone()

    def unchanged(self, snap):
        return torch.equal(self.raw, snap)

    def broken_sentinels(self):
        """Positions (arena offsets) of sentinels that no longer hold their pattern."""
        r = self.raw.cpu()
        return torch.nonzero(~self.inside & (r != self.sentinel)).flatten().tolist()


def describe(arena, pos, table):
    for i, (o, n) in enumerate(zip(arena.offs, arena.sizes)):
        if o - GUARD <= pos < o + n + GUARD:
            return "%s[%d]" % (table[i].name, pos - o)
    return "offset %d" % pos


class State:
    """All arenas and device tables of one launch over `table` in alignment class `align`."""

    def __init__(self, table, align, device, C=None, shadow_dtype=None, adam=False, shadow_all=False, pairs=False):
        self.table, self.device, self.C = table, device, C or chunk_elems()
        sp, sg, sm = ALIGN[align]
        self.n = [numel(e) for e in table]
        self.p = Arena(self.n, sp, F32, device)
        self.g = Arena(self.n, sg, F32, device)
        self.m = Arena(self.n, sm, F32, device)
        self.arenas = {"p": self.p, "g": self.g, "m": self.m}
        if adam:
            self.v = self.arenas["v"] = Arena(self.n, sm, F32, device)
        self.has_grad = [e.grad for e in table]
        self.has_shadow = [shadow_dtype is not None and (e.shadow or shadow_all) for e in table]
        self.shadow_dtype = shadow_dtype
        if shadow_dtype is not None:
            self.h = self.arenas["h"] = Arena([n if s else 0 for n, s in zip(self.n, self.has_shadow)], sp, shadow_dtype, device,
                                               fill=UNWRITTEN16)
        if pairs:
            self.has_pair = [e.name != "nograd" for e in table]       # (its hi_ptrs entry is NULL)
            self.hi = self.arenas["hi"] = Arena(self.n, 0, F16, device, fill=UNWRITTEN16)
            self.lo = self.arenas["lo"] = Arena(self.n, 0, F16, device, fill=UNWRITTEN16)
        ct, co = chunk_tables(self.n, self.C)
        self.nchunks = len(ct)
        dev = lambda v, dt: torch.tensor(v, dtype=dt, device=device)
        self.chunk_t, self.chunk_o, self.numel = dev(ct, torch.int32), dev(co, torch.int64), dev(self.n, torch.int64)
        self.lr, self.wd = dev([e.lr for e in table], F32), dev([e.wd for e in table], F32)
        self.p_ptrs, self.m_ptrs = dev(self.p.ptrs(), torch.int64), dev(self.m.ptrs(), torch.int64)
        self.g_ptrs = dev(self.g.ptrs(self.has_grad), torch.int64)
        self.v_ptrs = dev(self.v.ptrs(), torch.int64) if adam else None
        self.h_ptrs = dev(self.h.ptrs(self.has_shadow), torch.int64) if shadow_dtype is not None else None
        self.shadow_code = 2 if shadow_dtype == F16 else 1
        if pairs:
            self.hi_ptrs, self.lo_ptrs = dev(self.hi.ptrs(self.has_pair), torch.int64), dev(self.lo.ptrs(self.has_pair), torch.int64)

    def load(self, kind, values):
        for i, val in enumerate(values):
            if val is not None:
                self.arenas[kind].set(i, val.to(self.device))

    def assert_guards(self):
        for kind, a in self.arenas.items():
            bad = a.broken_sentinels()
            assert not bad, "%s arena: sentinel overwritten around %s" % (kind, describe(a, bad[0], self.table))


# ---------------------------------------------------------------------------------------------------------------------------
# SGD: exact operands and the float64 closed form
# ---------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def sgd_operands(table, seed=0, steps=SGD_STEPS):
    """-> p (float64, multiples of 2^-3 in [-4, 4]), one list of integer gradients in [-8, 8] per step."""
    gen = _gen(1000 + seed)
    p = [torch.randint(-32, 33, (numel(e),), generator=gen).double() / 8 for e in table]
    gs = [[torch.randint(-8, 9, (numel(e),), generator=gen).double() for e in table] for _ in range(steps)]
    return p, gs


def sgd_ref_step(p, g, m, lr, wd, mu, s=None):
    """float64: m <- mu m + (g s + wd p), p <- p - lr m (one tensor) -> (p, m, d)"""
    d = g * (1.0 if s is None else s) + wd * p
    m = mu * m + d
    return p - lr * m, m, d


def sgd_f32_step(p, g, m, lr, wd, mu, s=None):
    """The same in fp32, one rounding per operation, no contraction -> (p, m, d)"""
    c = lambda x: torch.tensor(x, dtype=F32)
    d = g * c(1.0 if s is None else s) + c(wd) * p
    m = c(mu) * m + d
    return p - c(lr) * m, m, d


def sgd_reference(table, p, grads, mu, s):
    """-> [(p list, m list) after each step], float64; tensors without a gradient keep p and m = 0."""
    p = [x.clone() for x in p]
    m = [torch.zeros_like(x) for x in p]
    out = []
    for gs in grads:
        for i, e in enumerate(table):
            if e.grad:
                p[i], m[i], _ = sgd_ref_step(p[i], gs[i], m[i], e.lr, e.wd, mu, s)
        out.append(([x.clone() for x in p], [x.clone() for x in m]))
    return out


def tie_operands(table, dtype, seed=0):
    """Second operand set of the shadow test: fp32 parameters at which 16-bit rounding matters.  First quarter of every tensor:
    exact ties between two neighbours of `dtype` (half of them towards an odd neighbour), with gradient 0 - run with weight decay
    0 and zero momentum they are not moved, so the tie itself is what gets rounded.  The rest: normal values over twelve binades
    (f16: down into its subnormals) with random gradients."""
    gen = _gen(2000 + seed)
    ps, gs = [], []
    for e in table:
        n = numel(e)
        k = -(-n // 4)
        if dtype == BF16:
            hi = torch.randint(0x3000, 0x4800, (k,), generator=gen, dtype=torch.int32)          # bf16 patterns 2^-31 .. 2^17
            bits = (hi << 16) | 0x8000
        else:
            h = torch.randint(0x0400, 0x7800, (k,), generator=gen, dtype=torch.int32).to(torch.int16).view(F16)   # normal halves
            bits = h.float().view(torch.int32) | 0x1000
        sign = torch.randint(0, 2, (k,), generator=gen, dtype=torch.int32) << 31
        ties = (bits | sign).view(F32)
        scale = 2.0 ** torch.randint(-18 if dtype == F16 else -6, 6, (n,), generator=gen).double()
        p = (torch.randn(n, generator=gen).double() * scale).float()
        g = torch.randn(n, generator=gen).float()
        p[:k], g[:k] = ties, 0.0
        ps.append(p)
        gs.append(g)
    return ps, gs


def is_tie(p, dtype):
    """Elements of fp32 p exactly half-way between two neighbours of dtype (normal range of dtype)."""
    d = p.double()
    r = p.to(dtype).double()
    return (d != r) & ((r - d).abs() * 2 == _spacing(p, dtype))


def _spacing(p, dtype):
    """Distance between the two neighbours of dtype around fp32 p (normal range of dtype)."""
    mant = 7 if dtype == BF16 else 10
    return 2.0 ** (torch.floor(torch.log2(p.double().abs())) - mant)


# ---------------------------------------------------------------------------------------------------------------------------
# AdamW: float64 step and the derived bound
# ---------------------------------------------------------------------------------------------------------------------------
BETAS, EPS = (0.9, 0.999), 1e-8
GRAD_SCALES = (1e-4, 1.0, 2.0 ** 10)
ADAM_INV_SCALE = 2.0 ** -10
ADAM_T = (1, 2, 1001)


def adam_hyper(table):
    """Per-tensor lr / wd of the AdamW cases, as the fp32 values the device reads (float64 copies of them)."""
    lr = torch.tensor([1e-3 * (1 + i / 8) for i in range(len(table))], dtype=F32)
    wd = torch.tensor([1e-2 * (1 + i % 5) for i in range(len(table))], dtype=F32)
    return lr, wd


def adam_operands(table, seed=0, state=False):
    """-> p, g (and m, v when state) as fp32 lists; tensor i has gradients of scale GRAD_SCALES[i % 3]."""
    gen = _gen(3000 + seed)
    p, g, m, v = [], [], [], []
    for i, e in enumerate(table):
        n, sc = numel(e), GRAD_SCALES[i % 3]
        p.append(torch.randn(n, generator=gen) * 0.25)          # (weights well below 1: |u| ~ lr stands 1000 x above 4 E |p|)
        g.append((torch.randn(n, generator=gen).double() * sc).float())
        m.append((torch.randn(n, generator=gen).double() * sc * 0.3).float())
        v.append(((torch.randn(n, generator=gen).double() * sc) ** 2 * 0.5 + (0.1 * sc) ** 2).float())
    return (p, g, m, v) if state else (p, g)


AdamStep = namedtuple("AdamStep", "p m v tol_p tol_m tol_v u")


def adam_ref_step(p, g, m, v, lr, wd, t, s=None, betas=BETAS, eps=EPS):
    """One AdamW step in float64 from fp32 state (one tensor; lr, wd: the fp32 values as Python floats) and the tolerances."""
    b1, b2 = betas
    p, g, m, v = p.double(), g.double() * (1.0 if s is None else s), m.double(), v.double()
    m1 = m + (1 - b1) * (g - m)
    v1 = b2 * v + (1 - b2) * g * g
    denom = v1.sqrt() / (1 - b2 ** t) ** 0.5 + eps
    step_size = lr / (1 - b1 ** t)
    u = step_size * m1 / denom
    p1 = p * (1 - lr * wd) - u
    tol_m = 4 * E * (m.abs() + g.abs())
    tol_v = 4 * E * v1
    tol_p = 4 * E * p.abs() + 8 * E * u.abs() + step_size * tol_m / denom
    return AdamStep(p1, m1, v1, tol_p, tol_m, tol_v, u)


def worst_ratio(got, want, tol):
    """max |got - want| / tol per element; an element with tol == 0 must be equal (-> inf otherwise)."""
    d = (got.double() - want).abs()
    r = torch.where(tol > 0, d / tol.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))))
    return float(r.max()) if r.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# overflow detection: the kernels' index maps and the poison positions derived from them
# ---------------------------------------------------------------------------------------------------------------------------
Where = namedtuple("Where", "chunk path thread iteration load lane")


def check_map(n_tensor, e, aligned, C):
    """Which lane of grad_check_multi_kernel reads element e of a tensor of n_tensor elements.  aligned gradient: quads
    q = e / 4 of the chunk's body [0, n & ~3) go to thread q % 256, load j = (q / 256) % 8 of outer iteration q / 2048; the
    n % 4 tail elements to threads 0..2.  Unaligned: element by element, thread e % 256, iteration e / 256."""
    chunk, r = divmod(e, C)
    n = min(C, n_tensor - chunk * C)
    assert 0 <= r < n
    if not aligned:
        return Where(chunk, "scalar", r % THREADS, r // THREADS, 0, 0)
    body = n - n % VEC
    if r >= body:
        return Where(chunk, "tail", r - body, 0, 0, 0)
    q = r // VEC
    return Where(chunk, "body", q % THREADS, q // (THREADS * UNROLL), (q // THREADS) % UNROLL, r % VEC)


def update_map(n_tensor, e, aligned, C):
    """The same for the body of sgd_multi_kernel (p, g and m all aligned): quad q to thread q % 256 in pass q / 256, tail and
    scalar path as above.  adamw_multi_kernel always takes the scalar path."""
    w = check_map(n_tensor, e, aligned, C)
    if w.path != "body":
        return w
    q = (e % C) // VEC
    return Where(w.chunk, "body", q % THREADS, q // THREADS, 0, w.lane)


def check_visits(n, aligned):
    """Restatement of the check kernel's loops for one chunk of n elements -> list of (element, thread, outer, load) reads."""
    out = []
    if aligned:
        n4 = n >> 2
        for tid in range(THREADS):
            for i0 in range(tid, n4, THREADS * UNROLL):
                for j in range(UNROLL):
                    i = i0 + j * THREADS
                    if i < n4:
                        out.extend((4 * i + k, tid, (i0 - tid) // (THREADS * UNROLL), j) for k in range(VEC))
            for i in range((n & ~3) + tid, n, THREADS):
                out.append((i, tid, 0, 0))
    else:
        for tid in range(THREADS):
            out.extend((i, tid, (i - tid) // THREADS, 0) for i in range(tid, n, THREADS))
    return out


Poison = namedtuple("Poison", "label tensor element")
POISON_VALUES = {"+inf": 0x7F800000, "-inf": 0xFF800000 - (1 << 32), "qnan": 0x7FC00000, "nan_0x7f800001": 0x7F800001}


def poison_positions(table, C=None):
    """Where one non-finite gradient element is planted, from the index maps above."""
    C = C or chunk_elems()
    big, one, three, late = (index_of(table, k) for k in ("two_c7", "one", "three", "k1023"))
    assert numel(table[big]) == 2 * C + 7 and late > big
    quad_pass = THREADS * VEC                                  # elements one pass of the workgroup's 16-byte accesses covers
    return [Poison("first", big, 0),
            Poison("last_thread_first_pass_end", big, quad_pass - 1),
            Poison("unroll_outer0_end", big, VEC * (THREADS * UNROLL - 1)),
            Poison("unroll_outer1_start", big, VEC * THREADS * UNROLL),
            Poison("chunk0_last", big, C - 1),
            Poison("chunk1_first", big, C),
            Poison("last_chunk_body_end", big, 2 * C + 3),
            Poison("last_chunk_tail_first", big, 2 * C + 4),
            Poison("last_chunk_tail_last", big, 2 * C + 6),
            Poison("only_element", one, 0),
            Poison("three_last", three, 2),
            Poison("later_tensor_first", late, 0),
            Poison("later_tensor_last", late, numel(table[late]) - 1)]


def clean_gradient_sets(table):
    """Negative controls: finite extremes that must raise nothing."""
    out = {}
    for name, vals in (("flt_max", (FLT_MAX, -FLT_MAX)), ("denormal", (1e-45, -1e-45, 1.1754942e-38)), ("neg_zero", (-0.0,))):
        out[name] = [torch.tensor(vals, dtype=F32).repeat(-(-numel(e) // len(vals)))[:numel(e)] for e in table]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# loss scaler: fp32 restatement of _amp_update_scale_
# ---------------------------------------------------------------------------------------------------------------------------
def scaler_ref(scale, tracker, found, growth, backoff, interval):
    """-> (scale, inv_scale, tracker, found) after one update, in fp32 (numpy scalars)."""
    f = np.float32
    s = f(scale)
    with np.errstate(over="ignore"):
        if found:
            s, tracker = f(s * f(backoff)), 0
        else:
            tracker += 1
            if tracker == interval:
                grown = f(s * f(growth))
                if np.isfinite(grown):
                    s = grown
                tracker = 0
    return s, f(f(1.0) / s), tracker, 0


# found flag per step (0: clean), growth, backoff, interval, initial scale
SCALER_CASES = {
    "backoff_then_growth": ([1, 0, 0, 0, 7, 0, 0, 0, 0], 2.0, 0.5, 3, 2.0 ** 15),
    "found_other_than_one": ([-5, 0, 1 << 20, 0], 2.0, 0.5, 2, 2.0 ** 10),
    "interval_one": ([0, 0, 1, 0, 0], 2.0, 0.5, 1, 2.0 ** 4),
    "growth_would_overflow": ([0, 0, 0, 0, 1, 0, 0], 2.0, 0.5, 2, 2.0 ** 127),
    "odd_factors": ([0, 0, 1, 0, 0, 0, 1, 1, 0], 1.75, 0.375, 2, 1000.0),       # (1 / scale is inexact; the factors are fp32 numbers)
}


# ---------------------------------------------------------------------------------------------------------------------------
# split pairs and transposes
# ---------------------------------------------------------------------------------------------------------------------------
SPLIT_SCALE = 256.0


def split_operands(table, seed=0):
    """fp32 parameters over many binades: zeros, negatives, values whose lo half is subnormal (|p * 256| below 2^-3)."""
    gen = _gen(4000 + seed)
    out = []
    for e in table:
        n = numel(e)
        p = (torch.randn(n, generator=gen).double() * 2.0 ** torch.randint(-24, 5, (n,), generator=gen).double()).float()
        p[::7] = 0.0
        if n > 1:
            p[1::7] = -0.0
        out.append(p)
    return out


def split_ref(p, scale=SPLIT_SCALE):
    v = p * scale
    hi = v.half()
    return hi, (v - hi.float()).half()


TRANSPOSE_SHAPES = ((64, 64), (128, 64), (64, 192), (512, 512))


def transpose_operands(seed=0):
    """Raw 16-bit patterns per shape; the (512, 512) tensor alone holds all 65536 of them."""
    out = []
    for k, (r, c) in enumerate(TRANSPOSE_SHAPES):
        x = (torch.arange(r * c, dtype=torch.int64) * 40503 + 977 * k + seed) & 0xFFFF
        out.append((x - ((x & 0x8000) << 1)).to(torch.int16).view(r, c))
    return out


def tile_table(shapes, seed=0):
    """(tensor, tile row, tile col) of every 64 x 64 tile, shuffled."""
    tiles = [(t, a, b) for t, (r, c) in enumerate(shapes) for a in range(r // 64) for b in range(c // 64)]
    perm = torch.randperm(len(tiles), generator=_gen(5000 + seed)).tolist()
    return [tiles[i] for i in perm]
