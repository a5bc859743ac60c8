"""Case tables, operand recipes, float64 reference, bounds and the per-row checker of the fused-attention edge suite
(test_attn_edges_host.py, test_gpu_attn_edges.py): editor_attention_fwd / _bwd / _bwd_colsum for bf16 and f16 at head widths 32, 64
and 96 (csrc/attention_bf16.hip, attn_common.h).  Nothing here runs GPU code at import; everything is CPU float64 / float32.

SHAPES.  B = 3 sequences, heads = 3 (2 at hd = 96): the qkv row is 3 * heads * hd = 576 elements at every width, the output row
96 / 192 / 192 - all multiples of 8, so every 16-byte access of the kernels is aligned and no other head count was needed.
DENSE_T lists the issue's sequence lengths (plus 193 at hd = 32 / 96, so that the unrolled 14-tile form runs at every width).

FORMS.  dispatch() restates the host-side switches of launch_all / launch_long / pick_nt / pick_threads: key tiles (10 / 14 / 26 /
38, 0 = chunked long form), FULL (unrolled), 192 or 256 threads, bitmap words of the masked form, 256-row chunks and 64-row
workgroups of the long form, staged or direct stores of the backward.  The host test proves the tables reach both sides of each.

OPERANDS.  "peaked": N(0, 1.5^2) - sharp softmax rows.  "designated": N(0, 0.5^2) plus c * e (e = ones / sqrt(hd)) on every query
and on the key rows of the designated tokens, whose V rows are multiplied by 4: the last valid key, the first key of the last
populated 16-tile, token 0 (it is the row right behind the previous sequence: that sequence's first invalid key), keys 511 and 512
beyond 513 tokens, masked form: the dead tokens next to a live one, and the rows behind the last sequence.  c^2 = ln(0.115 n /
(1 - 0.1 nd)) / scale (n valid keys, nd designated ones + 1; packed form: the longest sequence's, for all), clamped at 0.  Every designated valid key then holds 0.005 .. 0.7 of
every live query row (asserted from the reference on every case; the upper end only where a sequence has >= 8 valid keys - with
fewer, the designated keys ARE most of the keys and share the whole weight), so a dropped or leaked key moves every row.

REFERENCE.  float64 from the rounded operands; invalid keys score -inf; a masked query or one without a valid key has P = 0,
out = 0, lse = +inf; lse in log2 units.  The backward is fed the reference's out (rounded) and lse (fp32).

BOUNDS (per element, reference quantities only; u = 2^-8 bf16, 2^-11 f16; C = 2):
  tol_out = C (u (P |V| + |o|) + F_P |V|)              tol_dV = C (u (P^T |dO| + |dV|) + F_P^T |dO|)
  E       = u |dS| + P scale u sum_d |dO o| + F_P       tol_dQ = C (E |K| + u |dQ|),  tol_dK = C (E^T |Q| + u |dK|)
F_P: f16 only, 2^-25 on every (live query, valid key) pair - the absolute error of rounding a P or dS entry into f16's subnormal
range; the same 2^-25 is added once to an f16 output element for its own rounding.  Elements whose bound is 0 (masked rows)
must be exact zeros.  The CPU restatement that rounds where the kernels round (fp32 scores, P and dS rounded to 16 bits, outputs
rounded) reaches at most 0.44 (out), 0.31 (dQ), 0.25 (dK), 0.46 (dV) of these bounds over the whole table (host test: < 0.5).

fp32 OUTPUTS.  lse: |err| <= LSE_TOL max(1, |ref|); probabilities: |err| <= PROB_TOL ref + 2^-126 (flush to zero); delta
(against rowsum(dO o) of the rounded o the kernel is given): |err| <= DELTA_TOL sum_d |dO o|.  The constants are 8 x the worst
error of an fp32 CPU restatement over the whole table (the hardware's exp2 / log / rcp are 1-ulp approximations and the
summation orders differ), worst restatement errors: lse 6.48e-7, probs 6.68e-6, delta 1.26e-7.

MEASURED ON gfx950 (the kernels' worst ratio to the bound per form and output kind over test_gpu_attn_edges.py; the file's 191 tests
take 18 s, the slowest case 0.45 s):
  form        out    dQ     dK     dV     lse    delta  probs
  short       0.413  0.277  0.222  0.447  0.038  0.113  0.049
  full        0.419  0.286  0.277  0.364  0.047  0.105  0.059
  tiles26_38  0.403  0.308  0.243  0.355  0.032  0.126  0.055
  long        0.406  0.282  0.250  0.367  0.037  0.100  -
  packed      0.437  0.294  0.246  0.398  0.034  0.104  -
  masked      0.411  0.284  0.256  0.457  0.050  0.126  0.054
(the 16-bit outputs sit where the CPU rounding model sits: the error is the rounding of P, dS and the output, nothing else).
"""
import functools
import math
from collections import namedtuple

import torch

BF16, F16 = torch.bfloat16, torch.float16
DTYPES = (BF16, F16)
RECIPES = ("peaked", "designated")
B = 3
GUARD = 64                                # guard rows (2-D outputs) or elements (fp32 vectors) before and after every output slice
TRAIL = 16                                # designated-looking qkv rows behind the last sequence
SENT16 = 0x7FA5                           # a NaN as bf16 and as f16
SENT32 = 0x7FA5A5A5                       # a NaN as fp32
C_BOUND = 2.0
LOG2E = 1.4426950408889634
F16_FLOOR = 2.0 ** -25
# 8 x the fp32 restatement's worst error over the whole table (test_attn_edges_host.test_fp32_constants_hold_their_margin)
LSE_TOL = 5.2e-6
PROB_TOL = 5.3e-5
DELTA_TOL = 1.0e-6
FLUSH32 = 2.0 ** -126

# worst ratio to the bounds of everything record() has seen, per (form, output kind): how the docstring's table was measured
KERNEL_WORST = {}


def heads_of(hd):
    return 2 if hd == 96 else 3


def unit(dtype):
    return 2.0 ** -8 if dtype == BF16 else 2.0 ** -11


# ---------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------
DENSE_T = {
    64: (1, 2, 16, 17, 32, 33, 48, 128, 129, 144, 160, 161, 192, 193, 224, 225, 256, 257, 288, 416, 417, 512, 513, 608,
         609, 640, 641, 768, 769),
    32: (1, 17, 129, 160, 161, 193, 416, 417, 608, 609, 769),
    96: (1, 17, 129, 160, 161, 193, 416, 417, 609, 769),
}
MASKED_T = {
    64: (1, 17, 33, 129, 161, 193, 257, 417, 513, 608, 609, 769),
    32: (17, 129, 161, 193, 289, 417, 608, 609),
    96: (17, 129, 161, 193, 289, 417, 609),
}
PACKED_LENS = ((1, 160, 161, 17, 129, 16), (609, 64, 1, 257, 256))
# column sums from the backward's accumulators (attention_bwd_colsum_ok: T <= 608, 96-wide heads T <= 160)
COLSUM_DENSE_T = {64: (160, 161, 608), 32: (160, 161, 608), 96: (160,)}
COLSUM_MASKED_T = {64: (193, 608), 32: (193, 608), 96: (129,)}

Case = namedtuple("Case", "form hd T lens")          # form: dense | masked | packed; lens: packed only


def dense_cases():
    return [Case("dense", hd, t, None) for hd in (64, 32, 96) for t in DENSE_T[hd]]


def masked_cases():
    return [Case("masked", hd, t, None) for hd in (64, 32, 96) for t in MASKED_T[hd]]


def packed_cases():
    return [Case("packed", hd, max(lens), lens) for hd in (64, 32, 96) for lens in PACKED_LENS]


def all_cases():
    return dense_cases() + masked_cases() + packed_cases()


def case_id(c):
    return "%s-hd%d-T%d" % (c.form, c.hd, c.T) + ("" if c.lens is None else "-n%d" % len(c.lens))


Dispatch = namedtuple("Dispatch", "nt long full threads words chunks qblocks last_chunk_tiles staged_bwd colsum")


def pick_nt(hd, t):
    return 10 if t <= 160 else 14 if t <= 224 else 26 if t <= 416 else 38 if (t <= 608 and hd <= 64) else 0


def dispatch(hd, t, masked=False, packed=False):
    """The host-side switches of csrc/attention_bf16.hip (launch_all, launch_long, pick_nt, pick_threads, KeyBits) for one call."""
    nt = pick_nt(hd, t)
    rowb = 2 * hd
    if nt == 0:
        last = t - (t - 1) // 256 * 256
        return Dispatch(0, True, False, 256, 0, (t + 255) // 256, (t + 63) // 64, ((last + 31) >> 5) << 1, False, False)
    full = (not masked) and (not packed) and (((t + 31) >> 5) << 1) >= nt and nt <= 14
    threads = 192 if ((t + 15) // 16) % 3 == 0 else 256
    stg = (threads // 64) * 16 * (rowb + 32)
    staged = 2 * nt * 16 * rowb + 2 * nt * 16 * 4 + stg <= 160 * 1024
    words = ((min(nt, ((t + 31) >> 5) << 1) - 1) >> 4) + 1 if masked else 0
    return Dispatch(nt, False, full, threads, words, 0, 0, 0, staged, hd <= 64 or nt <= 10)


def family(c):
    """The dispatch family a case is tested under (one test function each)."""
    if c.form in ("packed", "masked"):
        return c.form
    d = dispatch(c.hd, c.T)
    return "long" if d.long else "full" if d.full else "short" if d.nt <= 14 else "tiles26_38"


# ---------------------------------------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------------------------------------
PATTERNS = ("cls_only", "all_live", "random_half", "dead_tiles", "ends_only", "none")


def mask_pattern(name, t, gen):
    m = torch.zeros(t, dtype=torch.bool)
    if name == "cls_only":
        m[0] = True
    elif name == "all_live":
        m[:] = True
    elif name == "random_half":
        m = torch.rand(t, generator=gen) > 0.5
        m[0] = True
    elif name == "dead_tiles":                     # tokens 16..31 and the last populated 16-key tile dead
        m[:] = True
        m[16:32] = False
        m[(t - 1) // 16 * 16:] = False
    elif name == "ends_only":
        m[0] = True
        m[t - 1] = True
    return m


def mask_batches(t, seed=0):
    """-> list of (names, (b, t) bool mask): the six patterns, those that coincide at this t once, three samples per launch."""
    gen = torch.Generator().manual_seed(1000 + t + seed)
    rows = []
    for name in PATTERNS:
        m = mask_pattern(name, t, gen)
        if any(torch.equal(m, r) for _, r in rows):
            continue
        rows.append((name, m))
    out = []
    for i in range(0, len(rows), B):
        part = rows[i:i + B]
        out.append((tuple(n for n, _ in part), torch.stack([m for _, m in part])))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------
Operands = namedtuple("Operands", "qkv do rows total seqs heads hd scale dtype designated")
# seqs: list of (row0, length, live (length,) bool); qkv has TRAIL more rows than `rows` (the kernels are given qkv[:rows])


def designated_tokens(live):
    """-> (valid, invalid) designated token indices of one sequence with key validity `live`."""
    t = live.numel()
    idx = torch.nonzero(live).flatten().tolist()
    valid, invalid = set(), (set() if live[0] else {0})
    if idx:
        valid.add(idx[-1])
        pop = idx[-1] // 16 * 16                          # first key of the last populated 16-tile
        first = [j for j in idx if j >= pop][0]
        valid.add(first)
        if live[0]:
            valid.add(0)
        if t > 513:
            valid |= {j for j in (511, 512) if live[j]}
        dead_after = [j for j in range(1, t) if not live[j] and live[j - 1]]
        dead_before = [j for j in range(0, t - 1) if not live[j] and live[j + 1]]
        invalid |= set(dead_after[:1]) | set(dead_before[-1:])
    return sorted(valid), sorted(invalid)


def boost(nlive, ndes, scale):
    if nlive == 0:
        return 0.0
    x = math.log(0.1 * 1.15 * nlive / (1.0 - 0.1 * ndes))
    return math.sqrt(max(x, 0.0) / scale)


def make_operands(hd, dtype, recipe, lens, masks=None, seed=0):
    """qkv (rows + TRAIL, 3 D) and dO (rows, D) in `dtype`.  Dense / masked: every length equal, rows = sum; packed: rows = sum
    rounded up to 64 (pad rows look like designated rows; nothing may read or write them)."""
    heads = heads_of(hd)
    d = heads * hd
    scale = hd ** -0.5
    total = sum(lens)
    packed = len(set(lens)) > 1
    rows = (total + 63) // 64 * 64 if packed else total
    gen = torch.Generator().manual_seed(seed * 7919 + hd * 131 + total + (0 if dtype == BF16 else 1) + (0 if recipe == "peaked" else 2))
    std = 1.5 if recipe == "peaked" else 0.5
    qkv = torch.randn(rows + TRAIL, 3, heads, hd, generator=gen, dtype=torch.float64) * std
    do = torch.randn(rows, d, generator=gen, dtype=torch.float64)
    e = torch.full((hd,), 1.0 / math.sqrt(hd), dtype=torch.float64)
    seqs, des, row0, c = [], [], 0, 0.0
    longest = torch.ones(max(lens), dtype=torch.bool)
    shared = boost(max(lens), len(designated_tokens(longest)[0]) + 1, scale)
    for b, n in enumerate(lens):
        live = torch.ones(n, dtype=torch.bool) if masks is None else masks[b].clone()
        seqs.append((row0, n, live))
        valid, invalid = designated_tokens(live)
        des.append((valid, invalid))
        if recipe == "designated":
            # packed: one boost for the launch, the longest sequence's - a sequence's first invalid key is its neighbour's token 0
            c = shared if packed else boost(int(live.sum()), len(valid) + 1, scale)
            qkv[row0:row0 + n, 0] += c * e
            for j in set(valid) | set(invalid):
                kj = qkv[row0 + j, 1]
                qkv[row0 + j, 1] = kj - (kj @ e)[:, None] * e + c * e         # random part orthogonal to e: the same boost for all
                qkv[row0 + j, 2] *= 4.0
        row0 += n
    if recipe == "designated":
        qkv[total:, 1] += c * e
        qkv[total:, 2] *= 4.0
    qkv = qkv.reshape(rows + TRAIL, 3 * d).to(dtype)
    return Operands(qkv, do.to(dtype), rows, total, seqs, heads, hd, scale, dtype, des)


@functools.lru_cache(maxsize=None)
def case_operands(case, dtype, recipe, batch=0):
    """Operands of one table entry (masked: launch `batch` of mask_batches)."""
    if case.form == "packed":
        return make_operands(case.hd, dtype, recipe, list(case.lens))
    if case.form == "masked":
        names, masks = mask_batches(case.T)[batch]
        return make_operands(case.hd, dtype, recipe, [case.T] * len(names), masks, seed=1 + batch)
    return make_operands(case.hd, dtype, recipe, [case.T] * B)


def cu_of(op):
    """cu (b + 1 int32) of the packed form."""
    return torch.tensor([s[0] for s in op.seqs] + [op.total], dtype=torch.int32)


def mask_of(op):
    return torch.stack([s[2] for s in op.seqs]).to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------------
# float64 reference and bounds
# ---------------------------------------------------------------------------------------------------------------------------
class Ref:
    """Reference outputs and bounds of one call, laid out as the kernels' outputs: out / tol_out (rows, D); dqkv / tol_dqkv
    (rows, 3 D); lse, delta (heads, rows); probs: list over sequences of (heads, t, t).  Rows outside every sequence are NaN here
    and are not compared (the guards cover them).  out16 / lse32: what the backward is given."""
    pass


def _sample(q, k, v, do, valid_k, valid_q, scale, dtype):
    """One sequence, all heads: q, do (h, t, hd) float64; k, v (h, t or t + 1, hd): the mutation that leaks a key adds a row."""
    u = unit(dtype)
    fl = F16_FLOOR if dtype == F16 else 0.0
    s = (q @ k.transpose(1, 2)) * scale
    s = s.masked_fill(~valid_k[None, None, :], -math.inf)
    lse_n = torch.logsumexp(s, -1)
    dead = (~valid_q)[None, :] | torch.isinf(lse_n)
    p = torch.exp(s - lse_n.masked_fill(dead, 0.0)[..., None])
    p = p.masked_fill(dead[..., None], 0.0)
    lse = (lse_n * LOG2E).masked_fill(dead, math.inf)
    o = p @ v
    o16 = o.to(dtype).double()
    delta = (do * o).sum(-1)
    delta_in = (do * o16).sum(-1)
    dabs = (do * o16).abs().sum(-1)
    dp = do @ v.transpose(1, 2)
    ds = p * (dp - delta[..., None]) * scale
    dq, dk, dv = ds @ k, ds.transpose(1, 2) @ q, p.transpose(1, 2) @ do
    pair = ((~dead)[..., None] & valid_k[None, None, :]).double()          # (live query, valid key) pairs
    fp = fl * pair
    any_q = pair.amax(-1, keepdim=True)                                     # rows / key columns that hold anything at all
    any_k = pair.amax(1)[..., None]
    tol_o = C_BOUND * (u * (p @ v.abs() + o.abs()) + fp @ v.abs() + fl * any_q)
    err = u * ds.abs() + p * scale * (u * (do * o).abs().sum(-1))[..., None] + fp
    tol_dq = C_BOUND * (err @ k.abs() + u * dq.abs() + fl * any_q)
    tol_dk = C_BOUND * (err.transpose(1, 2) @ q.abs() + u * dk.abs() + fl * any_k)
    tol_dv = C_BOUND * (u * (p.transpose(1, 2) @ do.abs() + dv.abs()) + fp.transpose(1, 2) @ do.abs() + fl * any_k)
    n = q.shape[1]
    return dict(out=o, tol_out=tol_o, lse=lse, p=p[..., :n], p_all=p, dq=dq, dk=dk[:, :n], dv=dv[:, :n], tol_dq=tol_dq,
                tol_dk=tol_dk[:, :n], tol_dv=tol_dv[:, :n], delta_in=delta_in, dabs=dabs, ds=ds)


def _heads(x2d, heads, hd):
    """(n, heads * hd) -> (heads, n, hd)"""
    return x2d.reshape(x2d.shape[0], heads, hd).permute(1, 0, 2)


def _rows(xh):
    """(heads, n, hd) -> (n, heads * hd)"""
    return xh.permute(1, 0, 2).reshape(xh.shape[1], -1)


def reference(op, drop_last=False, leak_next=False, leak_dead=False, mask_from=None):
    """float64 reference of one call.  The keyword arguments DAMAGE it (the host test's mutations): last valid key dropped, the
    row behind each sequence taken as one more key, one designated dead key treated as live, sample i using sample mask_from[i]'s
    mask."""
    heads, hd, d = op.heads, op.hd, op.heads * op.hd
    x = op.qkv.double()
    do = op.do.double()
    r = Ref()
    nan = float("nan")
    r.out, r.tol_out = torch.full((op.rows, d), nan, dtype=torch.float64), torch.full((op.rows, d), nan, dtype=torch.float64)
    r.dqkv, r.tol_dqkv = torch.full((op.rows, 3 * d), nan, dtype=torch.float64), torch.full((op.rows, 3 * d), nan, dtype=torch.float64)
    r.lse, r.delta = torch.full((heads, op.rows), nan, dtype=torch.float64), torch.full((heads, op.rows), nan, dtype=torch.float64)
    r.dabs = torch.full((heads, op.rows), nan, dtype=torch.float64)
    r.probs, r.weights = [], []
    r.row_seq = torch.full((op.rows,), -1, dtype=torch.long)
    r.row_local = torch.zeros(op.rows, dtype=torch.long)
    for b, (row0, n, live) in enumerate(op.seqs):
        if mask_from is not None:
            live = op.seqs[mask_from[b]][2]
        extra = 1 if leak_next else 0
        q = _heads(x[row0:row0 + n, :d], heads, hd)
        k = _heads(x[row0:row0 + n + extra, d:2 * d], heads, hd)
        v = _heads(x[row0:row0 + n + extra, 2 * d:], heads, hd)
        vk = torch.cat([live, torch.ones(extra, dtype=torch.bool)])
        if drop_last and live.any():
            vk[int(torch.nonzero(live).flatten()[-1])] = False
        if leak_dead:
            dead_des = [j for j in op.designated[b][1] if not live[j]]
            if dead_des and live.any():
                vk[dead_des[-1]] = True
        s = _sample(q, k, v, _heads(do[row0:row0 + n], heads, hd), vk, live, op.scale, op.dtype)
        sl = slice(row0, row0 + n)
        r.out[sl], r.tol_out[sl] = _rows(s["out"]), _rows(s["tol_out"])
        r.dqkv[sl] = torch.cat([_rows(s["dq"]), _rows(s["dk"]), _rows(s["dv"])], 1)
        r.tol_dqkv[sl] = torch.cat([_rows(s["tol_dq"]), _rows(s["tol_dk"]), _rows(s["tol_dv"])], 1)
        r.lse[:, sl], r.delta[:, sl], r.dabs[:, sl] = s["lse"], s["delta_in"], s["dabs"]
        r.probs.append(s["p"])
        r.row_seq[sl] = b
        r.row_local[sl] = torch.arange(n)
        valid = op.designated[b][0]
        liveq = ~torch.isinf(s["lse"])
        r.weights.append((s["p"][:, :, valid], liveq, int(live.sum())))
    r.out16 = torch.nan_to_num(r.out, nan=0.0).to(op.dtype)
    r.lse32 = torch.nan_to_num(r.lse, nan=0.0, posinf=math.inf).float()
    return r


def _is_masked(op):
    return any(not bool(s[2].all()) for s in op.seqs)


@functools.lru_cache(maxsize=8)
def case_reference(case, dtype, recipe, batch=0):
    return reference(case_operands(case, dtype, recipe, batch))


def designated_condition(op, ref):
    """-> (lowest, highest) weight a designated valid key holds in a live query row; highest over sequences with >= 8 valid keys
    only (see the module docstring).  (inf, -inf) parts if there is nothing to look at."""
    lo, hi = math.inf, -math.inf
    for w, liveq, nlive in ref.weights:
        if w.shape[-1] == 0 or not bool(liveq.any()):
            continue
        rows = w[liveq]
        lo = min(lo, float(rows.min()))
        if nlive >= 8:
            hi = max(hi, float(rows.max()))
    return lo, hi


# ---------------------------------------------------------------------------------------------------------------------------
# CPU restatements
# ---------------------------------------------------------------------------------------------------------------------------
def restate(op, ref, round16=True):
    """What the kernels compute, on the CPU in fp32: fp32 scores, P = exp2(s - lse) (round16: rounded to the dtype before the
    second product, as are dS and the outputs), the backward from the reference's rounded out and fp32 lse.  -> dict of outputs in
    the kernels' layout (float64 tensors), probs as a list per sequence."""
    heads, hd, d = op.heads, op.hd, op.heads * op.hd
    x = op.qkv.float()
    do = op.do.float()
    rnd = (lambda t: t.to(op.dtype).float()) if round16 else (lambda t: t)
    nan = float("nan")
    out = torch.full((op.rows, d), nan, dtype=torch.float64)
    dqkv = torch.full((op.rows, 3 * d), nan, dtype=torch.float64)
    lse = torch.full((heads, op.rows), nan, dtype=torch.float64)
    delta = torch.full((heads, op.rows), nan, dtype=torch.float64)
    probs = []
    masked = _is_masked(op)
    sc = torch.tensor(op.scale * LOG2E, dtype=torch.float32)
    for b, (row0, n, live) in enumerate(op.seqs):
        sl = slice(row0, row0 + n)
        q, k, v = (_heads(x[sl, i * d:(i + 1) * d], heads, hd) for i in range(3))
        dob = _heads(do[sl], heads, hd)
        s = ((q @ k.transpose(1, 2)) * sc).masked_fill(~live[None, None, :], -math.inf)
        m = s.amax(-1)
        ms = m.masked_fill(torch.isinf(m), 0.0)
        l_ = torch.exp2(s - ms[..., None]).sum(-1)
        dead = (l_ <= 0) | ((~live)[None, :] if masked else torch.zeros_like(l_, dtype=torch.bool))
        ls = (m + torch.log2(l_)).masked_fill(dead, math.inf)
        p = torch.exp2(s - ls[..., None])
        o = rnd(rnd(p) @ v)
        # backward from the reference's out / lse
        o_in = _heads(ref.out16[sl].float(), heads, hd)
        ls_in = ref.lse32[:, sl]
        dl = (dob * o_in).sum(-1)
        pb = torch.exp2(s - ls_in[..., None])
        ds = rnd(pb * (dob @ v.transpose(1, 2) - dl[..., None]) * op.scale)
        pr = rnd(pb)
        dq, dk, dv = rnd(ds @ k), rnd(ds.transpose(1, 2) @ q), rnd(pr.transpose(1, 2) @ dob)
        out[sl] = _rows(o).double()
        dqkv[sl] = torch.cat([_rows(dq), _rows(dk), _rows(dv)], 1).double()
        lse[:, sl], delta[:, sl] = ls.double(), dl.double()
        probs.append(p.double())
    return dict(out=out, dqkv=dqkv, lse=lse, delta=delta, probs=probs)


# ---------------------------------------------------------------------------------------------------------------------------
# the per-row checker
# ---------------------------------------------------------------------------------------------------------------------------
Worst = namedtuple("Worst", "ratio section sample head row")


def _ratio(got, ref, tol):
    """|got - ref| / tol per element; a zero bound demands equality; anything non-finite where the reference is finite is inf."""
    got, ref, tol = got.double(), ref.double(), tol.double()
    diff = (got - ref).abs()
    same = (got == ref)
    r = torch.where(tol > 0, diff / tol.clamp_min(1e-300), torch.where(same, torch.zeros_like(diff), torch.full_like(diff, math.inf)))
    r = torch.where(same, torch.zeros_like(r), r)                            # (inf == inf: the masked queries' lse)
    return torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)


def _worst_rows(ratio_hrow, section, ref, rows_idx):
    """ratio_hrow (heads, nrows) per-row maxima -> Worst with the row's sample and local index."""
    flat = int(torch.argmax(ratio_hrow))
    h, i = divmod(flat, ratio_hrow.shape[1])
    row = int(rows_idx[i])
    return Worst(float(ratio_hrow[h, i]), section, int(ref.row_seq[row]), h, int(ref.row_local[row]))


def check(op, ref, out=None, lse=None, dqkv=None, delta=None, probs=None):
    """Compares whatever outputs are given (kernel layout, any float dtype; probs: (b, heads, t, ldp) fp32, dense forms only) with
    the reference, row by row.  -> dict section -> Worst (the worst row of that section and its ratio to the bound; pass: <= 1)."""
    heads, hd, d = op.heads, op.hd, op.heads * op.hd
    inside = torch.nonzero(ref.row_seq >= 0).flatten()
    res = {}

    def per_row(r2d):                                                       # (rows, heads * hd) -> (heads, rows) row maxima
        return r2d.reshape(r2d.shape[0], heads, hd).amax(-1).t()
    if out is not None:
        r = _ratio(out[inside], ref.out[inside], ref.tol_out[inside])
        res["out"] = _worst_rows(per_row(r), "out", ref, inside)
    if dqkv is not None:
        r = _ratio(dqkv[inside], ref.dqkv[inside], ref.tol_dqkv[inside])
        for i, name in enumerate(("dq", "dk", "dv")):
            res[name] = _worst_rows(per_row(r[:, i * d:(i + 1) * d]), name, ref, inside)
    if lse is not None:
        want = ref.lse[:, inside]
        tol = LSE_TOL * want.abs().clamp_min(1.0)
        tol = torch.where(torch.isinf(want), torch.zeros_like(tol), tol)
        res["lse"] = _worst_rows(_ratio(lse.reshape(heads, -1)[:, inside], want, tol), "lse", ref, inside)
    if delta is not None:
        res["delta"] = _worst_rows(_ratio(delta.reshape(heads, -1)[:, inside], ref.delta[:, inside], DELTA_TOL * ref.dabs[:, inside]),
                                   "delta", ref, inside)
    if probs is not None:
        worst = Worst(0.0, "probs", 0, 0, 0)
        for b, p in enumerate(ref.probs):
            n = p.shape[-1]
            r = _ratio(probs[b, :, :n, :n], p, PROB_TOL * p + FLUSH32 * (p > 0)).amax(-1)          # (heads, n)
            flat = int(torch.argmax(r))
            h, i = divmod(flat, n)
            if float(r[h, i]) >= worst.ratio:
                worst = Worst(float(r[h, i]), "probs", b, h, i)
        res["probs"] = worst
    return res


def failures(res):
    return [w for w in res.values() if not w.ratio <= 1.0]


def assert_ok(res, what=""):
    bad = failures(res)
    assert not bad, "%s: %s" % (what, "; ".join("%s sample %d head %d row %d at %.3g x its bound" %
                                                (w.section, w.sample, w.head, w.row, w.ratio) for w in bad))


def record(form, res):
    """Keeps the worst ratio per (form, section) of everything checked so far (KERNEL_WORST)."""
    for w in res.values():
        key = (form, w.section)
        if w.ratio > KERNEL_WORST.get(key, (-1.0,))[0]:
            KERNEL_WORST[key] = (w.ratio, w.sample, w.head, w.row)
