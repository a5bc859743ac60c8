"""Shared by tests/golden/capture_loss_options.py, tests/test_gpu_loss_options.py and tests/test_loss_options_host.py: the seeded
inputs of the loss-option cases, the case table, the bounds, and a torch restatement of the batch-hard triplet loss with masked
max / min (which, unlike the reference's view(N, -1), runs identities of unequal size).

Features carry identity structure - feat = a_id * proto[id] + noise, a_id = linspace(0, a_max, ids) - because with pure noise at
D = 2304 every anchor sits on the same side of the hinge.  The capture searches (a_max, seed) per feature set until the conditions
of `conditions()` hold and records what it chose; tests regenerate the inputs from that record.
"""
import math

import torch

from editor_amd import synth

# (B, K, D) and what each can break
SHAPES = [(4, 2, 32),            # smallest
          (6, 2, 33),            # odd D
          (32, 8, 2304),         # the f7 shape; split-K Gram with 8 slabs
          (128, 16, 2304),       # the workload's shape
          (260, 4, 768),         # B beyond one 256-thread pass, not a multiple of 64; single-slab Gram
          (1024, 16, 100)]       # the LDS-list limit; D not a multiple of 4
MARGINS = (0.3, None)
HARD_FACTORS = (0.0, 0.2)
NORMALIZE = (False, True)
A_MAX = (1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0)
MAKE_LOSS_SHAPE = (32, 8, 2304, 171)                                   # B, K, D, classes
MAKE_LOSS_CASES = {"nm1_ls1": (True, "on", "softmax_triplet"), "nm0_ls1": (False, "on", "softmax_triplet"),
                   "nm1_ls0": (True, "off", "softmax_triplet"), "nm0_ls0": (False, "off", "softmax_triplet"),
                   "softmax": (True, "on", "softmax")}

# the project's bounds for this head (tests/test_gpu_loss.py), norm-wise rel_err against the reference's fp32 output
BOUND_TRIPLET, BOUND_DIST, BOUND_CE, BOUND_DSCORE, BOUND_DFEAT = 1e-5, 1e-5, 1e-6, 1e-5, 2e-5
BOUND_HINGE_DIST = 1e-6          # hinge loss: |dloss| <= 1e-5 |loss| + 1e-6 (mean d_ap + mean d_an), the distance accuracy through z
HINGE_GAP, RUNNER_UP_GAP = 1e-3, 1e-5


def set_key(b, d, hf, norm):
    """One feature set per (shape, hard_factor, normalize): both margin settings share it."""
    return "t%dx%d_h%d_n%d" % (b, d, int(hf > 0), int(norm))


def case_key(b, d, margin, hf, norm):
    return set_key(b, d, hf, norm) + "_m%d" % int(margin is not None)


def stored_rows(b):
    """Rows of dfeat[:, :64] kept in the golden file (all up to 64 rows, then every step-th: the file stays small); the per-row
    norms of ALL rows are kept beside them."""
    return torch.arange(0, b, max(1, math.ceil(b / 64)))


def labels(seed, b, k):
    """b // k identities x k instances in a seeded order."""
    t = torch.arange(b // k).repeat_interleave(k)
    return t[synth.integers(seed, "lo/perm", (b,), 1 << 30).argsort()]


def unequal_labels(seed, b):
    """Identities of sizes 3, 2, 4, 3, 2, 4, ... and ONE single-instance identity (the last id), in a seeded order."""
    sizes, left = [], b - 1
    while left > 0:
        s = min((3, 2, 4)[len(sizes) % 3], left)
        if left - s == 1:                                               # never leave a second singleton
            s += 1
        sizes.append(s)
        left -= s
    t = torch.cat([torch.full((s,), i, dtype=torch.int64) for i, s in enumerate(sizes + [1])])
    return t[synth.integers(seed, "lo/uperm", (b,), 1 << 30).argsort()]


def features(seed, target, d, a_max):
    """feat = a_id * proto[id] + noise, fp32 (B, d)."""
    ids = int(target.max()) + 1
    proto = synth.normal(seed, "lo/proto", (ids, d), 1.0)
    a = torch.linspace(0, a_max, ids)
    return (a[target, None] * proto[target] + synth.normal(seed, "lo/noise", (target.numel(), d), 1.0)).float()


def scores(seed, b, c):
    return synth.normal(seed, "lo/score", (b, c), 2.0)


def masked_triplet(feat, target, margin=None, hard_factor=0.0, normalize_feature=False):
    """TripletLoss(margin, hard_factor)(feat, target, normalize_feature) restated with masked max / min over the distance matrix
    -> (loss, dist_ap, dist_an, z) in feat's dtype; differentiable."""
    x = feat
    if normalize_feature:
        x = x / (x.norm(dim=1, keepdim=True) + 1e-12)
    sq = (x * x).sum(1)
    dist = (sq[:, None] + sq[None, :] - 2 * x @ x.t()).clamp(min=1e-12).sqrt()
    same = target[:, None] == target[None, :]
    d_ap = dist.masked_fill(~same, -math.inf).max(1).values * (1.0 + hard_factor)
    d_an = dist.masked_fill(same, math.inf).min(1).values * (1.0 - hard_factor)
    z = d_ap - d_an
    loss = torch.nn.functional.softplus(z).mean() if margin is None else (z + margin).clamp_min(0).mean()
    return loss, d_ap, d_an, z


def conditions(feat, target, margin, hard_factor, normalize_feature):
    """Conditions (a) - (c) of the capture, measured in float64: -> dict(active, hinge_gap, runner_up).
    active: fraction of anchors with an active hinge (margin form; nan for the soft form);
    hinge_gap: min over anchors of |z + margin| / d_ap (inf for the soft form) - must be >= HINGE_GAP;
    runner_up: min over anchors of the relative lead of the hardest positive / negative over its runner-up - must be
    >= RUNNER_UP_GAP (an anchor with fewer than two candidates on a side has no runner-up there)."""
    x = feat.double()
    if normalize_feature:
        x = x / (x.norm(dim=1, keepdim=True) + 1e-12)
    sq = (x * x).sum(1)
    dist = (sq[:, None] + sq[None, :] - 2 * x @ x.t()).clamp(min=1e-12).sqrt()
    same = target[:, None] == target[None, :]
    pos = dist.masked_fill(~same, -math.inf).sort(1, descending=True).values[:, :2]
    neg = dist.masked_fill(same, math.inf).sort(1).values[:, :2]
    lead_p = ((pos[:, 0] - pos[:, 1]) / pos[:, 0])[torch.isfinite(pos[:, 1])]
    lead_n = ((neg[:, 1] - neg[:, 0]) / neg[:, 0])[torch.isfinite(neg[:, 1])]
    runner = min([v.min().item() for v in (lead_p, lead_n) if v.numel()] or [math.inf])
    d_ap, d_an = pos[:, 0] * (1.0 + hard_factor), neg[:, 0] * (1.0 - hard_factor)
    if margin is None:
        return {"active": math.nan, "hinge_gap": math.inf, "runner_up": runner}
    h = d_ap - d_an + margin
    return {"active": (h > 0).double().mean().item(), "hinge_gap": (h.abs() / d_ap).min().item(), "runner_up": runner}
