"""Loss head that CONSUMES the hot path's train-mode outputs - row N1 of SURVEY.md 8(f).

Mirrors the reference's loss assembly so that bench.py times a complete training step and a harness written for
engine/processor.py:82-92 runs unchanged:
    CrossEntropyLabelSmooth(eps=0.1) / F.cross_entropy                 layers/softmax_loss.py:4-56
    TripletLoss(margin, hard_factor), batch-hard, Euclidean            layers/triplet_loss.py:5-136
    loss_func = ID_LOSS_WEIGHT * xent + TRIPLET_LOSS_WEIGHT * triplet  layers/make_loss.py:13-80 (every cfg branch)
Both terms run as HIP kernels (csrc/loss.hip) through the C ABI; CPU tensors are rejected, there is no fallback.
"""
import torch

from . import functional as Fn


def cross_entropy_label_smooth(logits, target, eps=0.1):
    return Fn.CrossEntropyLabelSmoothFn.apply(logits, target, float(eps))


def triplet_soft_margin(feat, labels):
    return Fn.TripletSoftMarginFn.apply(feat, labels)


class CenterLoss(torch.nn.Module):
    """layers/center_loss.py:9-51: `centers` (C, feat_dim) ~ N(0,1) and forward(x, labels) = sum of the masked (B, C) squared-distance
    matrix, every entry clamped to [1e-12, 1e12], / B - as HIP kernels (csrc/loss.hip: editor_center_loss_fwd / _bwd).  make_loss builds
    it with use_gpu=False (the parameter starts on the CPU, train_net.py:72-74 hands it to make_optimizer); with the shipped
    METRIC_LOSS_TYPE ('triplet') its forward is never called (layers/make_loss.py:36-56 has no centre term; processor.py:97-100 only
    rescales its gradient when 'center' is in the loss type) - it is here so that a harness which does call it runs.  Like every op of
    this package it needs GPU tensors: move the module with .cuda() / .to(device) first."""

    def __init__(self, num_classes=751, feat_dim=2048, use_gpu=False):
        super().__init__()
        self.num_classes, self.feat_dim, self.use_gpu = num_classes, feat_dim, use_gpu
        c = torch.randn(num_classes, feat_dim)
        self.centers = torch.nn.Parameter(c.cuda() if use_gpu else c)

    def forward(self, x, labels):
        assert x.size(0) == labels.size(0), "features.size(0) is not equal to labels.size(0)"
        if not (x.is_cuda and self.centers.is_cuda):
            raise RuntimeError("CenterLoss (MI355X build): features and centers must be on the GPU; there is no CPU fallback path")
        return Fn.CenterLossFn.apply(x, self.centers, labels.to(x.device, torch.int64))


class TripletLoss(object):
    """layers/triplet_loss.py:108-136, the class layers/__init__.py exports: batch-hard mining on Euclidean distances, then
    SoftMarginLoss (margin=None) or MarginRankingLoss(margin), with the distances scaled by 1 +- hard_factor first.
    __call__(global_feat, labels, normalize_feature=False) -> (loss, dist_ap, dist_an) as HIP kernels (csrc/loss.hip:
    editor_triplet_loss_fwd / editor_triplet_bwd, editor_normalize_rows_* when normalize_feature).  dist_ap / dist_an are detached
    fp32 (B,) device tensors - nothing in the reference differentiates through them (make_loss.py takes [0]; processor.py reads
    none); only `loss` carries a gradient.  2 <= B <= 1024 (the backward lists an anchor's partners in LDS).  Identities of unequal
    size, single-instance ones included, are mined as the kernel defines them (the reference's view(N, -1) cannot run those)."""

    def __init__(self, margin=None, hard_factor=0.0):
        self.margin = margin
        self.hard_factor = hard_factor

    def __call__(self, global_feat, labels, normalize_feature=False):
        if global_feat.dim() != 2 or not 2 <= global_feat.shape[0] <= 1024:
            raise ValueError("TripletLoss: features must be (B, D) with 2 <= B <= 1024, got {}".format(tuple(global_feat.shape)))
        if labels.shape[0] != global_feat.shape[0]:
            raise ValueError("TripletLoss: {} labels for {} feature rows".format(labels.shape[0], global_feat.shape[0]))
        labels = labels.to(global_feat.device, torch.int64)
        form, margin = (0, 0.0) if self.margin is None else (1, float(self.margin))
        return Fn.TripletLossFn.apply(global_feat, labels, form, margin, float(self.hard_factor), bool(normalize_feature))


class CrossEntropyLabelSmooth(torch.nn.Module):
    """layers/softmax_loss.py:4-34: mean_b( -sum_c ((1-eps) onehot + eps/num_classes) log_softmax ) over the HIP kernel.  The smoothing
    mass is spread over the logits' own width, which is num_classes wherever the reference's forward runs; use_gpu is kept for the
    signature (every op of this package needs GPU tensors)."""

    def __init__(self, num_classes, epsilon=0.1, use_gpu=True):
        super().__init__()
        self.num_classes, self.epsilon, self.use_gpu = num_classes, epsilon, use_gpu

    def forward(self, inputs, targets):
        return cross_entropy_label_smooth(inputs, targets, self.epsilon)


class LabelSmoothingCrossEntropy(torch.nn.Module):
    """layers/softmax_loss.py:36-56: mean( (1-s) nll + s * (-mean_c log p_c) ) - the same function of s as CrossEntropyLabelSmooth
    is of epsilon, so it goes over the same kernel."""

    def __init__(self, smoothing=0.1):
        super().__init__()
        assert smoothing < 1.0
        self.smoothing = smoothing
        self.confidence = 1. - smoothing

    def forward(self, x, target):
        return cross_entropy_label_smooth(x, target, self.smoothing)


def cross_entropy(logits, target):
    """F.cross_entropy(logits, target) (mean reduction): label smoothing with eps = 0 through the same kernel."""
    return cross_entropy_label_smooth(logits, target, 0.0)


SAMPLERS = ("softmax", "softmax_triplet")


def _key(cfg, section, key, default):
    return getattr(getattr(cfg, section, None), key, default) if cfg is not None else default


def _head_tail(fn, x, target):
    """make_loss.py:41-51,58-68: a list is the mean of its tail, then 0.5 * tail + 0.5 * head."""
    if isinstance(x, list):
        tail = [fn(v, target) for v in x[1:]]
        tail = sum(tail) / len(tail)
        return 0.5 * tail + 0.5 * fn(x[0], target)
    return fn(x, target)


def _loss_func(cfg=None):
    """The reference's loss_func for cfg (layers/make_loss.py:13-80), its defaults where a key is absent (config/defaults.py:
    NO_MARGIN True, IF_LABELSMOOTH 'on', METRIC_LOSS_TYPE 'triplet', SAMPLER 'softmax_triplet', SOLVER.MARGIN 0.3).  Where the
    reference prints and then fails at the first call, this raises ValueError at once."""
    idw = float(_key(cfg, "MODEL", "ID_LOSS_WEIGHT", 1.0))
    trw = float(_key(cfg, "MODEL", "TRIPLET_LOSS_WEIGHT", 1.0))
    sampler = _key(cfg, "DATALOADER", "SAMPLER", "softmax_triplet")
    metric = _key(cfg, "MODEL", "METRIC_LOSS_TYPE", "triplet")
    no_margin = _key(cfg, "MODEL", "NO_MARGIN", True)
    smooth = _key(cfg, "MODEL", "IF_LABELSMOOTH", "on")
    if sampler not in SAMPLERS:
        raise ValueError("DATALOADER.SAMPLER: expected one of {} but got {!r}".format(SAMPLERS, sampler))
    if sampler == "softmax":                                           # make_loss.py:31-33: cross-entropy alone, no smoothing

        def loss_func(score, feat, target, target_cam=None):
            return cross_entropy(score, target)

        return loss_func
    if metric != "triplet":        # make_loss.py:39,74-76 (a name that merely contains 'triplet' passes :16 and then returns None)
        raise ValueError("MODEL.METRIC_LOSS_TYPE: expected 'triplet' under SAMPLER 'softmax_triplet' but got {!r}".format(metric))
    if no_margin:
        tri = triplet_soft_margin
    else:
        criterion = TripletLoss(float(_key(cfg, "SOLVER", "MARGIN", 0.3)))

        def tri(feat, target):
            return criterion(feat, target)[0]

    xent = cross_entropy_label_smooth if smooth == "on" else cross_entropy

    def loss_func(score, feat, target, target_cam=None):
        f0 = feat[0] if isinstance(feat, list) else feat
        if f0.shape[0] != target.shape[0]:                            # make_loss.py:37-38
            target = target.repeat(f0.shape[0] // target.shape[0])
        # (a weight of exactly 1.0 - the shipped value of both - is not multiplied in: x * 1.0 == x bit for bit, and each product is
        #  a one-element launch in the forward and another in the backward)
        ce, tr = _head_tail(xent, score, target), _head_tail(tri, feat, target)
        return (ce if idw == 1.0 else idw * ce) + (tr if trw == 1.0 else trw * tr)

    return loss_func


def make_loss(cfg=None, num_classes=None):
    """layers/make_loss.py:13-80: returns (loss_func(score, feat, target, target_cam), center_criterion) as the reference does
    (train_net.py:72 unpacks both).  loss_func follows DATALOADER.SAMPLER ('softmax': cross-entropy alone; 'softmax_triplet': identity
    + triplet term), MODEL.IF_LABELSMOOTH, MODEL.NO_MARGIN / SOLVER.MARGIN and the two loss weights; an unknown SAMPLER, or a
    METRIC_LOSS_TYPE other than 'triplet' under softmax_triplet, raises ValueError.  cfg=None or absent keys give the configuration
    the reference trains with (softmax_triplet, soft-margin triplet, label smoothing on)."""
    return _loss_func(cfg), CenterLoss(num_classes=num_classes or 751, feat_dim=2048)


def loss_pairs(output, target, loss_fn=None):
    """engine/processor.py:82-92: odd-length output = (score_i, feat_i) pairs + trailing aux loss."""
    loss_fn = loss_fn or _loss_func()
    npair = len(output) - (len(output) % 2)
    loss = output[-1] if len(output) % 2 == 1 else None
    for i in range(0, npair, 2):
        term = loss_fn(score=output[i], feat=output[i + 1], target=target)
        loss = term if loss is None else loss + term
    return loss
