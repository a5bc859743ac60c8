"""Case tables, operand pairs, float64 reference, bounds and the per-row checker of the split-precision attention edge suite
(test_split_attn_edges_host.py, test_gpu_split_attn_edges.py): editor_attention_fwd_f16x2 and editor_attn_rollout_step_f16x2 at head
widths 32, 64 and 96 (csrc/attention_split.hip, attn_common.h).  Nothing here runs GPU code at import; everything is CPU float64 /
float32.  Case, the mask patterns, the designated tokens and their boost, the operand recipes, the guard constants, the ratio rule
and record() are attn_edge_helpers.py's own, imported.

OPERANDS.  The fp32 qkv of the two recipes ("peaked", "designated": attn_edge_helpers.make_operands with dtype float32), split on
the CPU into the half pair the kernel receives: hi = x.half(), lo = (x - hi.float()).half().  The PAIR is the input: the reference
is computed from hi.double() + lo.double(), so there is no input-rounding term (ops.split_f32 has tests of its own).  B = 3
sequences, heads = 3 (2 at hd = 96), TRAIL designated-looking rows behind the last sequence, packed rows rounded up to 64.

FORMS.  split_dispatch() restates the host switches of editor_attention_fwd_f16x2 (ROWB = 2 hd, 160 KiB of LDS): reg10 (T <= 160),
reg14 (T <= 224, not at hd = 96), whole (T <= 288; hd = 96: 161 .. 192), chunked (64-query workgroups, 128-key chunks), 192 threads
where the number of 16-query tiles is a multiple of 3.  rollout_dispatch() does the same for the rollout step: 10 / 14 / 26 / 38
key tiles, or a refusal (T < 2, T > 608, hd = 96 beyond 416 where two 608-row images and the row vectors exceed the LDS).  The
tables are the issue's, plus what the host test showed unreached: T = 192 (dense, hd = 32 / 64; the other lengths launch reg14 with
256 threads only) and a fourth packed launch no longer than 160 tokens (the packed reg10 form).  At hd = 96 the whole form does
reach 192 threads: T = 192 is 12 tiles.

REFERENCE.  float64 from the pair sums; invalid keys score -inf; a masked query or one without a valid key has P = 0, out = 0,
lse = +inf; lse in log2 units.  The rollout step is fed the reference's lse (fp32), once with +inf on the rows of a mask pattern.

BOUNDS (per element, reference quantities only):
  e_s(q,k) = scale (2^-22 + hd 2^-24) sum_d |q_d||k_d|     (the dropped lo.lo pass + fp32 accumulation),  E(q) = max over valid k
  dP(q,k)  = P (2 E(q) + C_EXP 2^-24)  +  2^-22 P + 2^-37  (the 2^12-scaled P pair; 2^-37: its low half going subnormal; the last
             two on (live query, valid key) pairs)
  tol_out  = C (dP |V| + 2^-22 (P |V| + |o|) + n_valid 2^-24 P |V| + 2^-25)      (2^-25: the output pair's low half, subnormal)
Elements whose bound is 0 (masked rows) must be exact zeros - the GPU test demands it of both halves.  lse: |err| <= LSE_TOL
max(1, |ref|); probabilities: |err| <= PROB_TOL ref + 2^-126; rollout: |err| <= ROLL_TOL sum_q |r_in[q]| P[q,k], exact zeros where
that sum is 0.

CONSTANTS.  Measured on restate(), an fp32 CPU restatement that rounds where the kernels round (three-pass fp32 scores without
lo.lo, exp2 in fp32, P scaled by 2^12 and split into a half pair, three-pass P V, the output split, the rollout from the fp32
lse), over the whole table (test_split_attn_edges_host.py asserts all of it); nothing is calibrated against the kernel.
  C_EXP: 8 x the worst relative error of the restatement's fp32 probabilities against the float64 softmax of ITS OWN fp32 scores
    (exp2, the subtraction in front of it, sum, reciprocal), in units of 2^-24.
  C: the smallest power of two for which the restatement stays below 0.5 of tol_out.
  LSE_TOL, PROB_TOL, ROLL_TOL: 8 x the restatement's worst error.
Worst restatement errors over the table and what they set:
  probabilities against the softmax of their own scores  1.40e-6 = 23.4 x 2^-24   ->  C_EXP    = 187
  out against tol_out at C = 1                           0.0329 (hd 32, T = 289)  ->  C        = 2^-3  (restatement: 0.263 of the bound)
  lse                                                    7.49e-7                  ->  LSE_TOL  = 6.0e-6
  probabilities against the reference                    6.54e-6                  ->  PROB_TOL = 5.2e-5
  rollout step                                           3.01e-6                  ->  ROLL_TOL = 2.4e-5
(C is below 1 because E(q) takes the worst case of the fp32 accumulation, hd 2^-24 sum |q||k|, which sums of random signs stay far
below; the dropped Q_lo K_hi pass still lands at 18 x the bound.)

DAMAGED REFERENCES (host test: every damage on every launch of the table where it exists; the smallest ratio to the bound that the
worst section of a launch reached):
  reference from the hi halves alone (the mode degenerating to f16)   49.5   (dense, hd 64, T = 641)
  scores without the Q_lo K_hi pass                                   17.9   (masked, hd 96, T = 17)
  low half of the output pair zeroed                                  13.7   (dense, hd 96, T = 385)
  last valid key dropped                                              6.5e4  (dense, hd 96, T = 385)
  the row behind a sequence leaked as a key                           2.1e5  (dense, hd 64, T = 641)
  a designated dead key taken as live; another sample's mask          inf    (a masked key's probability, a masked row's output:
                                                                              zero bounds)

MEASURED ON gfx950 (the kernels' worst ratio to the bound per form and output kind over test_gpu_split_attn_edges.py; the file's 102
tests take 5.3 s, the slowest case 0.32 s):
  form      out    lse    probs  rollout
  reg10     0.161  0.052  0.089  -
  reg14     0.124  0.035  0.060  -
  whole     0.131  0.048  0.064  -
  chunked   0.145  0.047  0.073  -
  packed    0.145  0.096  -      -
  masked    0.224  0.075  0.065  -
  rollout   -      -      -      0.080
(out: at or below the 0.263 the CPU restatement reaches; the fp32 outputs: below the restatement's 1/8).
"""
import functools
import math
from collections import namedtuple

import torch

import attn_edge_helpers as H
from attn_edge_helpers import (B, FLUSH32, GUARD, LOG2E, PATTERNS, RECIPES, SENT16, SENT32, TRAIL, Case, Ref, Worst,  # noqa: F401
                               _heads, _ratio, _rows, _worst_rows, assert_ok, case_id, cu_of, designated_condition, failures,
                               heads_of, mask_batches, mask_of, mask_pattern, record)

WIDTHS = (64, 32, 96)
LDS_MAX = 160 * 1024
SCH = 128                                 # key chunk of the streamed form
PSCALE = 4096.0                           # 2^12: the probabilities are scaled by it before they are split
# measured on restate() over the whole table (module docstring; test_split_attn_edges_host.py holds them to the rule)
C_EXP = 187.0
C_BOUND = 0.125
LSE_TOL = 6.0e-6
PROB_TOL = 5.2e-5
ROLL_TOL = 2.4e-5

# ---------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------
DENSE_T = {
    64: (1, 2, 16, 17, 32, 33, 48, 129, 144, 160, 161, 192, 193, 224, 225, 257, 288, 289, 321, 384, 385, 513, 641),
    32: (1, 17, 129, 160, 161, 192, 224, 225, 288, 289, 385),
    96: (1, 17, 129, 160, 161, 192, 193, 257, 385),
}
MASKED_T = {
    64: (1, 17, 33, 129, 161, 225, 257, 289, 385),
    32: (17, 161, 257, 289),
    96: (17, 129, 161, 192, 193),
}
PACKED_LENS = ((1, 160, 161, 17, 129, 16), (288, 64, 1, 257, 225), (385, 64, 1, 129, 289), (144, 1, 17, 160, 33))
ROLLOUT_T = {
    64: (2, 17, 129, 160, 161, 224, 225, 416, 417, 608),
    32: (2, 160, 161, 416, 417, 608),
    96: (2, 129, 161, 225, 416),
}
ROLLOUT_REFUSED_T = {64: (1, 609), 32: (1, 609), 96: (1, 417, 609)}
INF_PATTERNS = ("random_half", "dead_tiles", "ends_only")          # rollout: the rows that carry lse = +inf, one pattern per sample


def dense_cases():
    return [Case("dense", hd, t, None) for hd in WIDTHS for t in DENSE_T[hd]]


def masked_cases():
    return [Case("masked", hd, t, None) for hd in WIDTHS for t in MASKED_T[hd]]


def packed_cases():
    return [Case("packed", hd, max(lens), lens) for hd in WIDTHS for lens in PACKED_LENS]


def rollout_cases():
    return [Case("rollout", hd, t, None) for hd in WIDTHS for t in ROLLOUT_T[hd]]


def forward_cases():
    return dense_cases() + masked_cases() + packed_cases()


SplitDispatch = namedtuple("SplitDispatch", "form threads tiles chunks qblocks last_chunk_tiles")


def split_dispatch(hd, t, masked=False, packed=False):
    """The host-side switches of editor_attention_fwd_f16x2 for one call (t: the call's T - the longest sequence of a packed one;
    neither a mask nor cu changes the form).  tiles: key tiles populated (chunked form: over all chunks)."""
    rowb = 2 * hd
    rows = ((t + 31) >> 5) << 5
    threads = 192 if ((t + 15) // 16) % 3 == 0 else 256
    if rows <= 160 and 4 * 160 * rowb <= LDS_MAX:
        return SplitDispatch("reg10", threads, rows // 16, 0, 0, 0)
    if rows <= 224 and 4 * 224 * rowb <= LDS_MAX:
        return SplitDispatch("reg14", threads, rows // 16, 0, 0, 0)
    if rows <= 288 and 4 * rows * rowb <= LDS_MAX:
        return SplitDispatch("whole", threads, rows // 16, 0, 0, 0)
    chunks = (t + SCH - 1) // SCH
    last = t - (chunks - 1) * SCH
    last_tiles = ((last + 31) >> 5) << 1
    return SplitDispatch("chunked", 256, (chunks - 1) * (SCH // 16) + last_tiles, chunks, (t + 63) // 64, last_tiles)


RolloutDispatch = namedtuple("RolloutDispatch", "nt threads refused")


def rollout_dispatch(hd, t):
    """editor_attn_rollout_step_f16x2: key tiles of the Q images (0 and refused: no launch) and the thread count."""
    if t < 2 or t > 608:
        return RolloutDispatch(0, 0, True)
    nt = 10 if t <= 160 else 14 if t <= 224 else 26 if t <= 416 else 38
    if 2 * nt * 16 * 2 * hd + 2 * nt * 16 * 4 > LDS_MAX:
        return RolloutDispatch(0, 0, True)
    return RolloutDispatch(nt, 192 if ((t + 15) // 16) % 3 == 0 else 256, False)


def family(c):
    """The test function a case runs under: the packed, masked and rollout cases their own, the dense ones by kernel form."""
    return c.form if c.form != "dense" else split_dispatch(c.hd, c.T).form


# ---------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------
SplitOperands = namedtuple("SplitOperands", "hi lo rows total seqs heads hd scale designated")
# hi, lo: (rows + TRAIL, 3 D) half - the kernels are given [:rows]; seqs: list of (row0, length, live (length,) bool)


def make_operands(hd, recipe, lens, masks=None, seed=0):
    base = H.make_operands(hd, torch.float32, recipe, lens, masks, seed)
    x = base.qkv
    hi = x.half()
    lo = (x - hi.float()).half()
    return SplitOperands(hi, lo, base.rows, base.total, base.seqs, base.heads, hd, base.scale, base.designated)


@functools.lru_cache(maxsize=None)
def case_operands(case, recipe, batch=0):
    """Operands of one table entry (masked: launch `batch` of mask_batches)."""
    if case.form == "packed":
        return make_operands(case.hd, recipe, list(case.lens))
    if case.form == "masked":
        names, masks = mask_batches(case.T)[batch]
        return make_operands(case.hd, recipe, [case.T] * len(names), masks, seed=1 + batch)
    return make_operands(case.hd, recipe, [case.T] * B, seed=3 if case.form == "rollout" else 0)


def launches(case):
    return len(mask_batches(case.T)) if case.form == "masked" else 1


# ---------------------------------------------------------------------------------------------------------------------------
# float64 reference and bounds
# ---------------------------------------------------------------------------------------------------------------------------
def _sample(q, k, v, valid_k, valid_q, scale, hd, s_minus=None):
    """One sequence, all heads: q (h, t, hd) float64; k, v (h, t or t + 1, hd): the damage that leaks a key adds a row."""
    s = q @ k.transpose(1, 2)
    if s_minus is not None:
        s = s - s_minus
    s = (s * scale).masked_fill(~valid_k[None, None, :], -math.inf)
    lse_n = torch.logsumexp(s, -1)
    dead = (~valid_q)[None, :] | torch.isinf(lse_n)
    p = torch.exp(s - lse_n.masked_fill(dead, 0.0)[..., None])
    p = p.masked_fill(dead[..., None], 0.0)
    lse = (lse_n * LOG2E).masked_fill(dead, math.inf)
    o = p @ v
    pair = ((~dead)[..., None] & valid_k[None, None, :]).double()           # (live query, valid key) pairs
    any_q = pair.amax(-1, keepdim=True)
    e_s = scale * (2.0 ** -22 + hd * 2.0 ** -24) * (q.abs() @ k.abs().transpose(1, 2)) * valid_k[None, None, :].double()
    big_e = e_s.amax(-1, keepdim=True)
    dp = p * (2.0 * big_e + C_EXP * 2.0 ** -24) + (2.0 ** -22 * p + 2.0 ** -37) * pair
    pv = p @ v.abs()
    nvalid = float(valid_k.sum())
    tol = C_BOUND * (dp @ v.abs() + 2.0 ** -22 * (pv + o.abs()) + nvalid * 2.0 ** -24 * pv + 2.0 ** -25 * any_q)
    n = q.shape[1]
    return dict(out=o, tol_out=tol, lse=lse, p=p[..., :n])


def reference(op, drop_last=False, leak_next=False, leak_dead=False, mask_from=None, hi_only=False, drop_cross=False):
    """float64 reference of one forward call.  The keyword arguments DAMAGE it (the host test's mutations): last valid key dropped,
    the row behind each sequence taken as one more key, one designated dead key treated as live, sample i using sample
    mask_from[i]'s mask; this family's own: computed from the hi halves alone, scores without the Q_lo K_hi pass."""
    heads, hd, d = op.heads, op.hd, op.heads * op.hd
    x = op.hi.double() if hi_only else op.hi.double() + op.lo.double()
    r = Ref()
    nan = float("nan")
    r.out, r.tol_out = torch.full((op.rows, d), nan, dtype=torch.float64), torch.full((op.rows, d), nan, dtype=torch.float64)
    r.lse = torch.full((heads, op.rows), nan, dtype=torch.float64)
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
        s_minus = None
        if drop_cross:
            qlo = _heads(op.lo[row0:row0 + n, :d].double(), heads, hd)
            khi = _heads(op.hi[row0:row0 + n + extra, d:2 * d].double(), heads, hd)
            s_minus = qlo @ khi.transpose(1, 2)
        s = _sample(q, k, v, vk, live, op.scale, hd, s_minus)
        sl = slice(row0, row0 + n)
        r.out[sl], r.tol_out[sl] = _rows(s["out"]), _rows(s["tol_out"])
        r.lse[:, sl] = s["lse"]
        r.probs.append(s["p"])
        r.row_seq[sl] = b
        r.row_local[sl] = torch.arange(n)
        liveq = ~torch.isinf(s["lse"])
        r.weights.append((s["p"][:, :, op.designated[b][0]], liveq, int(live.sum())))
    r.lse32 = torch.nan_to_num(r.lse, nan=0.0, posinf=math.inf).float()
    return r


@functools.lru_cache(maxsize=8)
def case_reference(case, recipe, batch=0):
    return reference(case_operands(case, recipe, batch))


def half_rounded(x):
    """The damage (c): the low half of an output pair zeroed."""
    return x.half().double()


# ---- rollout ---------------------------------------------------------------------------------------------------------------
def inf_rows(t, nb=B):
    """(nb, t) bool: the query rows whose lse the rollout is handed as +inf (the dead tokens of one mask pattern per sample)."""
    gen = torch.Generator().manual_seed(2000 + t)
    return torch.stack([~mask_pattern(INF_PATTERNS[b % len(INF_PATTERNS)], t, gen) for b in range(nb)])


def rollout_weights(op, t):
    """A positive random r_in, (B, heads, t) float32."""
    gen = torch.Generator().manual_seed(3000 + t + op.hd)
    return torch.rand(len(op.seqs), op.heads, t, generator=gen, dtype=torch.float32) + 0.01


def rollout_lse(ref, t, dead=None):
    """The fp32 lse the step is given, (heads, rows): the reference's, +inf on the rows of `dead` (B, t)."""
    lse = ref.lse32.clone()
    if dead is not None:
        lse[:, dead.flatten()] = math.inf
    return lse


def rollout_reference(op, ref, w=None, dead=None):
    """-> (want, base), both (B, heads, t) float64: want[k] = sum_q w[q] P[q, k] over the queries not in `dead`, base the same sum
    of |w[q]| P[q, k] (the bound is ROLL_TOL base).  w None: the class-token row, w = e_0."""
    want, base = [], []
    for b, p in enumerate(ref.probs):
        t = p.shape[-1]
        wb = torch.zeros(op.heads, t, dtype=torch.float64)
        if w is None:
            wb[:, 0] = 1.0
        else:
            wb = w[b].double()
        if dead is not None:
            wb = wb.masked_fill(dead[b][None, :], 0.0)
        want.append(torch.einsum("hq,hqk->hk", wb, p))
        base.append(torch.einsum("hq,hqk->hk", wb.abs(), p))
    return torch.stack(want), torch.stack(base)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _pair32(t32):
    hi = t32.half()
    return hi.float(), (t32 - hi.float()).half().float()


def restate(op, lse_in=None, w=None):
    """What the kernels compute, on the CPU in fp32: S = Q_lo K_hi + Q_hi K_lo + Q_hi K_hi, P = exp2(S sc - M) / L, P' = 2^12 P split
    into a half pair, O = (P_hi V_lo + P_lo V_hi + P_hi V_hi) 2^-12 split into a half pair.  -> dict: out (float64 sum of the pair),
    lse, probs (list per sequence), exp_err (worst relative error of the fp32 probabilities against the float64 softmax of these
    fp32 scores), and - with lse_in (heads, rows) fp32 - rollout (B, heads, t): sum_q w[q] exp2(S sc - lse_in[q]), w None = e_0."""
    heads, hd, d = op.heads, op.hd, op.heads * op.hd
    xh, xl = op.hi.float(), op.lo.float()
    nan = float("nan")
    out = torch.full((op.rows, d), nan, dtype=torch.float64)
    lse = torch.full((heads, op.rows), nan, dtype=torch.float64)
    probs, roll = [], []
    exp_err = 0.0
    masked = any(not bool(s[2].all()) for s in op.seqs)
    sc = torch.tensor(op.scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    for b, (row0, n, live) in enumerate(op.seqs):
        sl = slice(row0, row0 + n)
        qh, kh, vh = (_heads(xh[sl, i * d:(i + 1) * d], heads, hd) for i in range(3))
        ql, kl, vl = (_heads(xl[sl, i * d:(i + 1) * d], heads, hd) for i in range(3))
        acc = ql @ kh.transpose(1, 2) + qh @ kl.transpose(1, 2) + qh @ kh.transpose(1, 2)
        s = (acc * sc).masked_fill(~live[None, None, :], -math.inf)
        m = s.amax(-1)
        ms = m.masked_fill(torch.isinf(m), 0.0)
        e = torch.exp2(s - ms[..., None])
        l_ = e.sum(-1)
        dead = (l_ <= 0) | ((~live)[None, :] if masked else torch.zeros_like(l_, dtype=torch.bool))
        inv = (1.0 / l_).masked_fill(dead, 0.0)
        lse[:, sl] = (m + torch.log2(l_)).masked_fill(dead, math.inf).double()
        p = e * inv[..., None]
        ph, pl = _pair32(e * (inv * PSCALE)[..., None])
        o = (ph @ vl + pl @ vh + ph @ vh) * (1.0 / PSCALE)
        oh, ol = _pair32(o)
        out[sl] = _rows(oh.double() + ol.double())
        probs.append(p.double())
        # the exp2 / sum / reciprocal part alone: float64 softmax of these very fp32 scores
        s64 = s.double()
        l64 = torch.logsumexp(s64 * math.log(2.0), -1) / math.log(2.0)
        p64 = torch.exp2(s64 - l64.masked_fill(dead, 0.0)[..., None]).masked_fill(dead[..., None], 0.0)
        nz = p64 > 2.0 ** -100
        if bool(nz.any()):
            exp_err = max(exp_err, float(((p.double() - p64).abs()[nz] / p64[nz]).max()))
        if lse_in is not None:
            wb = torch.zeros(heads, n, dtype=torch.float32)
            if w is None:
                wb[:, 0] = 1.0
            else:
                wb = w[b]
            pr = torch.exp2((acc * sc) - lse_in[:, sl][..., None])
            roll.append(torch.einsum("hq,hqk->hk", wb, pr).double())
    res = dict(out=out, lse=lse, probs=probs, exp_err=exp_err)
    if lse_in is not None:
        res["rollout"] = torch.stack(roll)
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the per-row checker
# ---------------------------------------------------------------------------------------------------------------------------
def check(op, ref, out=None, lse=None, probs=None):
    """Compares whatever outputs are given (kernel layout; out: the float64 sum of the pair; probs: (b, heads, t, ldp) fp32 or a
    list per sequence) with the reference, row by row.  -> dict section -> Worst (pass: ratio <= 1)."""
    heads, hd = op.heads, op.hd
    inside = torch.nonzero(ref.row_seq >= 0).flatten()
    res = {}
    if out is not None:
        r = _ratio(out[inside], ref.out[inside], ref.tol_out[inside])
        res["out"] = _worst_rows(r.reshape(r.shape[0], heads, hd).amax(-1).t(), "out", ref, inside)
    if lse is not None:
        want = ref.lse[:, inside]
        tol = LSE_TOL * want.abs().clamp_min(1.0)
        tol = torch.where(torch.isinf(want), torch.zeros_like(tol), tol)
        res["lse"] = _worst_rows(_ratio(lse.reshape(heads, -1)[:, inside], want, tol), "lse", ref, inside)
    if probs is not None:
        worst = Worst(0.0, "probs", 0, 0, 0)
        for b, p in enumerate(ref.probs):
            n = p.shape[-1]
            r = _ratio(probs[b][:, :n, :n], p, PROB_TOL * p + FLUSH32 * (p > 0)).amax(-1)          # (heads, n)
            flat = int(torch.argmax(r))
            h, i = divmod(flat, n)
            if float(r[h, i]) >= worst.ratio:
                worst = Worst(float(r[h, i]), "probs", b, h, i)
        res["probs"] = worst
    return res


def check_rollout(want, base, got):
    """want, base, got (B, heads, n) -> {"rollout": Worst} (row: the key)."""
    r = _ratio(got, want, ROLL_TOL * base)
    flat = int(torch.argmax(r))
    b, rest = divmod(flat, r.shape[1] * r.shape[2])
    h, k = divmod(rest, r.shape[2])
    return {"rollout": Worst(float(r[b, h, k]), "rollout", b, h, k)}
