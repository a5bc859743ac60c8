"""The reference's engine/processor.py - do_train (:23-214) and do_inference (:217-270) - around a training iteration that
never needs the host.

The reference's loop reads `loss.item()` twice per iteration, computes the accuracy with torch ops into a host meter,
synchronises the device every iteration and drives `amp.autocast` + `amp.GradScaler` (whose overflow flag is read on the host).
Here one iteration is `TrainStep.step`: forward, loss head, backward, gradient buckets, fused optimizer (with a
`DeviceGradScaler` if wanted) and ONE `editor_train_meter` launch that keeps the loss / accuracy meters in device memory
(`DeviceMeters`).  Nothing in it reads the device, so the same step runs eagerly or as a captured hipGraph (`graph=True`); the
host looks at the meters every `SOLVER.LOG_PERIOD` iterations and synchronises once more at the end of the epoch.

    from editor_amd.engine import do_train, do_inference          # engine/processor.py: same positional arguments
    best = do_train(cfg, model, center_criterion, train_loader, val_loader, optimizer, optimizer_center, scheduler, loss_fn,
                    num_query, local_rank, writer=None, scaler=None, graph=False)
    cmc, mAP = do_inference(cfg, model, val_loader, num_query)

Deliberate differences from the reference: `Loss` and `num_count` reach the writer at the log points, not every iteration (the
per-iteration `add_scalar('Loss', loss.item(), epoch)` is a host read; what is written is the epoch's running average); no
autocast and no torch GradScaler (the model does its own typing); `do_train` returns `best_index`; `do_inference` computes and
logs the metrics and returns `(cmc, mAP)` (the reference's stops after the feature loop).  The module imports without a GPU and
without the built library, which is loaded by the first launch; there is no fallback to torch for the meters."""
import contextlib
import logging
import os
import random
import re
import time
import warnings

import torch
import torch.distributed as dist

from . import _lib, losses

LOG_ITERATION = "Epoch[{}] Iteration[{}/{}] Loss: {:.3f}, Acc: {:.3f}, Base Lr: {:.2e}"
LOG_EPOCH = "Epoch {} done. Time per batch: {:.3f}[s] Speed: {:.1f}[samples/s]"


class _NullWriter:
    def add_scalar(self, *a, **k):
        pass


class _DeviceScalarWriter:
    """What the model is handed as `writer`: make_model.py:199-200 logs `num_count` from inside the forward; a tensorboard writer
    would read the device there.  This one keeps the device scalar (in a captured step: the graph's own output, rewritten by
    every replay)."""

    def __init__(self):
        self.num_count = None

    def add_scalar(self, tag, value, step=None):
        if tag == "num_count":
            self.num_count = value


class DeviceMeters:
    """loss_meter / acc_meter of engine/processor.py:58-59,104-105 in device memory: `update` is one editor_train_meter launch,
    `read` one device-to-host copy of six numbers and the only call that synchronises."""

    def __init__(self, device):
        self.device = torch.device(device)
        # state (double[4]: sum loss*B, sum B, sum acc, steps) and last (int[2]: correct, B of the latest update) in ONE buffer
        self._buf = torch.zeros(5, dtype=torch.float64, device=self.device)
        self.state = self._buf[:4]
        self.last = self._buf[4:].view(torch.int32)

    def reset(self):
        self._buf.zero_()

    def update(self, score, target, loss):
        """score (B, C): the first score head's logits; target (B) int64; loss: the iteration's scalar loss (device tensor)."""
        score, loss = score.detach(), loss.detach()
        if score.dim() != 2:
            raise ValueError("DeviceMeters.update: score is (B, C)")
        if score.shape[0] != target.shape[0]:                     # processor.py:97-98
            target = torch.cat((target, target), dim=0)
        if score.shape[0] != target.shape[0] or loss.numel() != 1:
            raise ValueError("DeviceMeters.update: %d score rows, %d targets, a loss of %d elements"
                             % (score.shape[0], target.shape[0], loss.numel()))
        if score.dtype != torch.float32:
            score = score.float()
        if not score.is_contiguous():
            score = score.contiguous()
        if loss.dtype != torch.float32:
            loss = loss.float()
        if target.dtype != torch.int64 or not target.is_contiguous():
            target = target.long().contiguous()
        b, c = score.shape
        _lib.call("editor_train_meter", score, c, target, loss, b, c, self.state, self.last)

    def read(self):
        host = self._buf.cpu().numpy()
        loss_sum, samples, acc_sum, steps = (float(v) for v in host[:4])
        last = host[4:].view("int32")
        return {"loss_avg": loss_sum / samples if samples else 0.0, "acc_avg": acc_sum / steps if steps else 0.0,
                "loss_sum": loss_sum, "samples": samples, "acc_sum": acc_sum, "steps": steps,
                "last_correct": int(last[0]), "last_batch": int(last[1])}


def _map_tensors(obj, fn):
    if isinstance(obj, torch.Tensor):
        return fn(obj)
    if isinstance(obj, dict):
        return {k: _map_tensors(v, fn) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_map_tensors(v, fn) for v in obj)
    return obj


def _flatten(obj, prefix=""):
    """Nested dicts (and lists of dicts: param_groups) -> {dotted key: leaf}."""
    if isinstance(obj, dict):
        items = obj.items()
    elif isinstance(obj, (list, tuple)) and obj and all(isinstance(v, dict) for v in obj):
        items = enumerate(obj)
    else:
        return {prefix[:-1]: obj}
    flat = {}
    for k, v in items:
        flat.update(_flatten(v, "%s%s." % (prefix, k)))
    return flat


def _first_difference(mine, theirs, prefix):
    """(key, what) of the first key that `theirs` lacks, has in excess or holds as a tensor of another shape; None if none."""
    for k, v in mine.items():
        if k not in theirs:
            return prefix + str(k), "missing"
        t = theirs[k]
        if isinstance(v, torch.Tensor) != isinstance(t, torch.Tensor):
            return prefix + str(k), "a tensor on one side only"
        if isinstance(v, torch.Tensor) and tuple(v.shape) != tuple(t.shape):
            return prefix + str(k), "shape %s here, %s in the state" % (tuple(v.shape), tuple(t.shape))
    for k in theirs:
        if k not in mine:
            return prefix + str(k), "unexpected"
    return None


def _plain(v):
    return tuple(float(x) for x in v) if isinstance(v, (list, tuple)) else float(v)


def _dtype_name(dtype):
    return None if dtype is None else str(dtype).replace("torch.", "")


def _compute_dtype(model):
    """cfg.MODEL.COMPUTE_DTYPE as the model took it: 'bf16' | 'f16' | 'f16x2' | 'f32' (None: not an EDITOR model)."""
    act = getattr(model, "act_dtype", None)
    if act is None:
        return None
    if getattr(model, "split_fwd", False):
        return "f16x2"
    return {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}[act]


def _signature(img, *ids):
    return (tuple((k, tuple(v.shape), v.dtype) for k, v in img.items()),
            tuple(None if t is None else (tuple(t.shape), t.dtype) for t in ids))


class TrainStep:
    """One iteration of engine/processor.py:71-96 (+ the meters of :97-105) without a host read:

        optimizer.zero_grad(set_to_none=True)
        out = model(img, label=, cam_label=, view_label=, img_path=None, writer=<keeps num_count on the device>, epoch=)
        loss = losses.loss_pairs(out, target, loss_fn)
        loss.backward()                    [scaler.scale(loss).backward()]
        buckets.finish()                   [if buckets]
        optimizer.step()                   [scaler.step(optimizer); scaler.update()]
        meters.update(out[0], target, loss)

    `step(img, target, cam, view, epoch=None)` returns the loss as a device tensor.  scaler: an editor_amd.optim.DeviceGradScaler;
    buckets: what model.enable_grad_buckets() returned; meters: a DeviceMeters.  No autocast, no torch GradScaler.
    `num_count` is the device scalar the model logged in the latest forward (None if it logged none).

    Every step of one TrainStep, eager or replayed, runs on ONE stream the object owns; the caller's current stream is waited for
    before and waits after, so the caller needs no stream code.  (Autograd's AccumulateGrad nodes remember the stream they were
    created on; one created on the default stream invalidates a later capture.)

    graph=True: the first `warmup` (>= 1) batches run eagerly - they are real training steps.  At the next batch shaped like the
    first one the inputs are copied into static tensors and the step is captured once into a hipGraph; from then on such a batch
    is a copy-in plus a replay.  A batch of another batch size, image shape or dtype (the last batch of an epoch: the loaders do
    not drop it) runs eagerly beside the graph, and later full batches replay again.  `captured` says whether a graph exists.  If
    the capture raises, the object warns once and stays eager for good.  The loss returned by a replayed step is the graph's
    own output tensor: the next replay rewrites it.  Learning-rate changes reach a captured step through FusedSGD's device tables,
    so `scheduler.step(epoch)` between replays needs no re-capture; `epoch` itself is only the step argument of the model's
    `add_scalar`, which is not read here."""

    def __init__(self, model, loss_fn, optimizer, *, scaler=None, buckets=None, meters=None, graph=False, warmup=2):
        if graph and int(warmup) < 1:
            raise ValueError("TrainStep: a captured step needs at least one eager warm-up step (warmup >= 1)")
        self.model, self.loss_fn, self.optimizer = model, loss_fn, optimizer
        self.scaler, self.buckets, self.meters = scaler, buckets, meters
        self.graph, self.warmup = bool(graph), int(warmup)
        self.captured = False
        self._writer = _DeviceScalarWriter()
        self._stream = None
        self._graph = self._static = self._static_loss = self._sig = self._first_sig = None
        self._eager_steps = 0
        self._gave_up = False

    @property
    def num_count(self):
        return self._writer.num_count

    def _body(self, img, target, cam, view, epoch):
        self.optimizer.zero_grad(set_to_none=True)
        out = self.model(img, label=target, cam_label=cam, view_label=view, img_path=None, writer=self._writer, epoch=epoch)
        loss = losses.loss_pairs(out, target, self.loss_fn)
        if self.scaler is not None:
            self.scaler.scale(loss).backward()
        else:
            loss.backward()
        if self.buckets is not None:
            self.buckets.finish()
        if self.scaler is not None:
            self.scaler.step(self.optimizer)
            self.scaler.update()
        else:
            self.optimizer.step()
        if self.meters is not None:
            self.meters.update(out[0], target, loss)
        return loss

    def step(self, img, target, cam, view, epoch=None):
        dev = next(iter(img.values())).device
        if dev.type != "cuda":                   # (nothing to order; the model's kernels refuse host tensors themselves)
            return self._body(img, target, cam, view, epoch)
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=dev)
        cur = torch.cuda.current_stream(dev)
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):
            loss = self._run(dev, img, target, cam, view, epoch)
        cur.wait_stream(self._stream)
        return loss

    def _run(self, dev, img, target, cam, view, epoch):
        if not self.graph or self._gave_up:
            return self._body(img, target, cam, view, epoch)
        sig = _signature(img, target, cam, view)
        if self._graph is not None:
            if sig != self._sig:
                return self._body(img, target, cam, view, epoch)          # odd batch: eagerly, the graph is left alone
            self._copy_in(img, target, cam, view)
            self._graph.replay()
            return self._static_loss
        if self._first_sig is None:
            self._first_sig = sig
        if self._eager_steps < self.warmup or sig != self._first_sig:
            self._eager_steps += 1
            return self._body(img, target, cam, view, epoch)
        try:
            self._capture(dev, img, target, cam, view, epoch)
        except Exception as e:                                            # capture unsupported here: eager from now on
            warnings.warn("TrainStep: hipGraph capture failed (%s: %s); the step stays eager" % (type(e).__name__, e))
            self._gave_up = True
            self._graph = self._static = self._static_loss = None
            torch.cuda.synchronize(dev)
            return self._body(img, target, cam, view, epoch)
        self.captured = True
        self._graph.replay()                                              # (the capture recorded the step; this runs it)
        return self._static_loss

    # -- the whole state of the iteration: snapshot, roll-back, resume ---------------------------------------------------------
    def state_dict(self, device=False):
        """Everything the next step reads: the model's state dict and drop-path counter, optimizer (momentum / Adam moments and
        step count, param_groups), scaler, meters, and the count of eager warm-up steps.  device=True: the tensors are device
        clones (a snapshot to roll back to, one clone of every parameter, buffer and momentum tensor); else CPU copies (what
        save_checkpoint writes).  Synchronises (the scalar states are read); call it between steps."""
        keep = (lambda t: t.detach().clone()) if device else (lambda t: t.detach().cpu() if t.is_cuda else t.detach().clone())
        return {"model": {k: keep(v) for k, v in self.model.state_dict().items()},
                "model_rng": self.model.rng_state() if hasattr(self.model, "rng_state") else None,
                "optimizer": _map_tensors(self.optimizer.state_dict(), keep),
                "optimizer_class": type(self.optimizer).__name__,
                "scaler": None if self.scaler is None else self.scaler.state_dict(),
                "meters": None if self.meters is None else keep(self.meters._buf),
                "eager_steps": self._eager_steps,
                "compute_dtype": _compute_dtype(self.model), "shadow_dtype": _dtype_name(getattr(self.optimizer, "shadow_dtype", None))}

    def _mismatch(self, sd):
        """The first key of `sd` that does not fit this step, or None.  Reads shapes only."""
        want = ("model", "model_rng", "optimizer", "optimizer_class", "scaler", "meters", "eager_steps", "compute_dtype", "shadow_dtype")
        for k in want:
            if k not in sd:
                return k, "missing"
        for k in sd:
            if k not in want:
                return k, "unexpected"
        if sd["compute_dtype"] != _compute_dtype(self.model):
            return "compute_dtype", "%s here, %s in the state" % (_compute_dtype(self.model), sd["compute_dtype"])
        mine = _dtype_name(getattr(self.optimizer, "shadow_dtype", None))
        if sd["shadow_dtype"] != mine:
            return "shadow_dtype", "%s here, %s in the state" % (mine, sd["shadow_dtype"])
        if sd["optimizer_class"] != type(self.optimizer).__name__:
            return "optimizer_class", "%s here, %s in the state" % (type(self.optimizer).__name__, sd["optimizer_class"])
        for k, here in (("scaler", self.scaler), ("meters", self.meters)):
            if (sd[k] is None) != (here is None):
                return k, "present on one side only"
        bad = _first_difference(self.model.state_dict(), sd["model"], "model.")
        if bad is None:
            bad = _first_difference(_flatten(self.optimizer.state_dict()), _flatten(sd["optimizer"]), "optimizer.")
        if bad is None and self.meters is not None:
            bad = _first_difference({"meters": self.meters._buf}, {"meters": sd["meters"]}, "")
        if bad is None and self.captured:
            # what a launch takes BY VALUE is part of the captured graph: a state that changes it needs a new TrainStep
            for k in ("betas", "eps"):
                got = {_plain(g[k]) for g in sd["optimizer"]["param_groups"] if k in g}
                if got and got != {_plain(getattr(self.optimizer, k))}:
                    return "optimizer.param_groups." + k, "differs from the value the captured graph was recorded with"
            for k in ("growth_factor", "backoff_factor", "growth_interval") if self.scaler is not None else ():
                if float(sd["scaler"][k]) != float(getattr(self.scaler, k)):
                    return "scaler." + k, "differs from the value the captured graph was recorded with"
        return bad

    def load_state_dict(self, sd):
        """Restore what state_dict() returned IN PLACE, on the step's own stream: copy_ into the existing parameters, buffers,
        momentum tensors and the meters' buffer, set_rng_state into the existing counter, then optimizer.refresh_operands() -
        without it every 16-bit shadow, W^T copy and hi / lo pair would still hold the weights from before.  Nothing is
        re-allocated, so a captured graph stays valid (`captured` does not change) and its next replay continues from the
        restored state.  Warm-up belongs to this object and its process: `eager_steps` of the state is not taken over, a fresh
        graph=True step still runs its own warm-up before it captures.

        ValueError - naming the first offending key, before anything is written - on a missing or extra key, another shape,
        another optimizer class, another COMPUTE_DTYPE / shadow dtype, or a scaler (meters) present on one side only."""
        bad = self._mismatch(sd)
        if bad is not None:
            raise ValueError("TrainStep.load_state_dict: '%s': %s" % bad)
        dev = _model_device(self.model)
        if dev is None or dev.type != "cuda":
            return self._restore(sd)
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=dev)
        cur = torch.cuda.current_stream(dev)
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):
            self._restore(sd)
        cur.wait_stream(self._stream)

    @torch.no_grad()
    def _restore(self, sd):
        for k, v in self.model.state_dict().items():
            v.copy_(sd["model"][k])
        if hasattr(self.model, "set_rng_state"):
            self.model.set_rng_state(sd["model_rng"])
        self.optimizer.load_state_dict(sd["optimizer"])
        if self.scaler is not None:
            self.scaler.load_state_dict(sd["scaler"])
        if self.meters is not None:
            self.meters._buf.copy_(sd["meters"])
        self.optimizer.refresh_operands()

    def _copy_in(self, img, target, cam, view):
        s_img, s_ids = self._static
        for k, v in img.items():
            s_img[k].copy_(v, non_blocking=True)
        for dst, src in zip(s_ids, (target, cam, view)):
            if dst is not None:
                dst.copy_(src, non_blocking=True)

    def _capture(self, dev, img, target, cam, view, epoch):
        from .ddp import graph_capture_kwargs
        static = ({k: v.clone() for k, v in img.items()}, [None if t is None else t.clone() for t in (target, cam, view)])
        torch.cuda.synchronize(dev)
        self.optimizer.zero_grad(set_to_none=True)
        # the eager steps leave their activations cached in the allocator's ordinary pool and the capture allocates the same set
        # again from the graph's private pool: hand the cached blocks back first
        torch.cuda.empty_cache()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, **graph_capture_kwargs()):           # (RCCL in the step: thread-local capture mode)
            loss = self._body(static[0], static[1][0], static[1][1], static[1][2], epoch)
        self._graph, self._static, self._static_loss = graph, static, loss
        self._sig = _signature(static[0], *static[1])


# ---- the epoch structure -------------------------------------------------------------------------------------------------------

def _is_main(cfg):
    """processor.py:121-122,130-131: with MODEL.DIST_TRAIN only rank 0 evaluates and writes files."""
    if getattr(cfg.MODEL, "DIST_TRAIN", False) and dist.is_available() and dist.is_initialized():
        return dist.get_rank() == 0
    return True


def _save(model, path):
    torch.save(model.state_dict(), path)


# ---- full-state checkpoints ------------------------------------------------------------------------------------------------------

CHECKPOINT_FORMAT = 1
_STATE_FILE = re.compile(r"_state_(\d+)\.pth$")


def _atomic_save(obj, path):
    """torch.save under a temporary name in the same directory, then os.replace: a reader (and a run killed half-way) sees the
    old file or the new one, never a part of either."""
    tmp = "%s.tmp.%d" % (path, os.getpid())
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    except BaseException:
        with contextlib.suppress(OSError):
            os.remove(tmp)
        raise


def save_checkpoint(path, step, *, epoch, scheduler=None, loaders=(), best_index=None, extra=None):
    """Everything a restarted process needs to continue as if it had not stopped, as ONE torch.save of a plain dict with CPU tensors:

        format         1
        epoch          the epoch just finished (a resumed do_train continues at epoch + 1)
        step           step.state_dict(): model, drop-path counter, optimizer, scaler, meters (TrainStep.state_dict)
        scheduler      scheduler.state_dict() or None
        loader_epochs  [loader.epoch or None]: the loaders' batches are a function of (seed, epoch); a loader without an `epoch`
                       attribute is skipped (None)
        best_index     {'mAP', 'Rank-1', 'Rank-5', 'Rank-10'} as floats, or None
        rng            {'python': random.getstate(), 'numpy': numpy.random.get_state(), 'torch': torch.get_rng_state()} - the global
                       generators the identity samplers draw from and torch's CPU generator.  Nothing in the step or the loaders
                       draws from torch's device generator (the drop-path counter is the model's own state).
        compute_dtype  cfg.MODEL.COMPUTE_DTYPE of the model
        extra          the caller's own entry, if given

    Synchronises the device (the state is copied to the host) and writes atomically."""
    import numpy as np
    sd = step.state_dict()
    ckpt = {"format": CHECKPOINT_FORMAT, "epoch": int(epoch), "step": sd,
            "scheduler": None if scheduler is None else scheduler.state_dict(),
            "loader_epochs": [int(ld.epoch) if hasattr(ld, "epoch") else None for ld in loaders],
            "best_index": None if best_index is None else {k: float(v) for k, v in best_index.items()},
            "rng": {"python": random.getstate(), "numpy": np.random.get_state(), "torch": torch.get_rng_state()},
            "compute_dtype": sd.get("compute_dtype")}
    if extra is not None:
        ckpt["extra"] = extra
    _atomic_save(ckpt, path)


def load_checkpoint(path, step, *, scheduler=None, loaders=()):
    """Restore what save_checkpoint wrote - step.load_state_dict (which refuses a state that does not fit, before anything is
    written), the scheduler, the loaders' epoch numbers and the three host generators - and return the file's dict (its `epoch`,
    `best_index` and `extra` are the caller's to use).  ValueError for a file of another format."""
    import numpy as np
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(ckpt, dict) or ckpt.get("format") != CHECKPOINT_FORMAT:
        raise ValueError("load_checkpoint: %s is not a format-%d state file (format: %r)"
                         % (path, CHECKPOINT_FORMAT, ckpt.get("format") if isinstance(ckpt, dict) else type(ckpt).__name__))
    missing = [k for k in ("epoch", "step", "scheduler", "loader_epochs", "best_index", "rng", "compute_dtype") if k not in ckpt]
    if missing:
        raise ValueError("load_checkpoint: %s lacks '%s'" % (path, missing[0]))
    step.load_state_dict(ckpt["step"])
    if scheduler is not None and ckpt["scheduler"] is not None:
        scheduler.load_state_dict(ckpt["scheduler"])
    for ld, ep in zip(loaders, ckpt["loader_epochs"]):
        if ep is not None and hasattr(ld, "epoch"):
            ld.epoch = int(ep)
    rng = ckpt["rng"]
    random.setstate(rng["python"])
    np.random.set_state(rng["numpy"])
    torch.set_rng_state(rng["torch"])
    return ckpt


def latest_state_file(out_dir, name):
    """<out_dir>/<name>_state_<epoch>.pth with the highest epoch, or None (what resume='auto' loads)."""
    best = None
    if os.path.isdir(out_dir):
        for fn in os.listdir(out_dir):
            m = _STATE_FILE.search(fn)
            if m and fn == "%s_state_%s.pth" % (name, m.group(1)) and (best is None or int(m.group(1)) > best[0]):
                best = (int(m.group(1)), os.path.join(out_dir, fn))
    return None if best is None else best[1]


def _model_device(model):
    try:
        return next(model.parameters()).device
    except (AttributeError, StopIteration, TypeError):
        return None


def _to(t, dev):
    if dev is None or not isinstance(t, torch.Tensor) or t.device == dev:
        return t                                                          # (the loaders deliver images on the device)
    return t.to(dev, non_blocking=True)


def _make_evaluator(cfg, num_query):
    from . import metrics
    feat_norm = getattr(cfg.TEST, "FEAT_NORM", "yes")
    if cfg.DATASETS.NAMES == "MSVR310":
        return metrics.R1_mAP(num_query, max_rank=50, feat_norm=feat_norm)
    return metrics.R1_mAP_eval(num_query, max_rank=50, feat_norm=feat_norm)


def _evaluate(cfg, model, val_loader, evaluator, dev):
    """processor.py:172-189 / :254-268: the eval forward over val_loader into the evaluator -> (cmc, mAP)."""
    model.eval()
    msvr = cfg.DATASETS.NAMES == "MSVR310"
    for img, vid, camid, camids, target_view, paths in val_loader:
        with torch.no_grad():
            img = {k: _to(v, dev) for k, v in img.items()}
            feat = model(img, cam_label=_to(camids, dev), view_label=_to(target_view, dev), mode=1, img_path=paths)
        evaluator.update((feat, vid, camid, target_view, paths) if msvr else (feat, vid, camid))
    cmc, m_ap = evaluator.compute()[:2]
    return cmc, m_ap


def _log_results(logger, head, cmc, m_ap):
    logger.info(head)
    logger.info("mAP: {:.2%}".format(m_ap))
    for r in (1, 5, 10):
        logger.info("CMC curve, Rank-{:<3}:{:.2%}".format(r, _rank(cmc, r)))


def _rank(cmc, r):
    return cmc[min(r, len(cmc)) - 1]          # (a gallery of fewer than r entries: the curve ends, and stays, at its last value)


def do_train(cfg, model, center_criterion, train_loader, val_loader, optimizer, optimizer_center, scheduler, loss_fn, num_query,
             local_rank, *, writer=None, scaler=None, graph=False, logger=None, save_state=False, resume=None):
    """engine/processor.py:23-214 with its positional signature (train_net.py:78-89 calls it unchanged).  writer: anything with
    `add_scalar` (None: nothing is written; tensorboard is never imported here); scaler: a DeviceGradScaler; graph: capture the
    step into a hipGraph (TrainStep).  Per epoch: meters and evaluator reset, scheduler.step(epoch), model.train(), one
    TrainStep.step per batch, a log line (one meters.read()) every SOLVER.LOG_PERIOD iterations, one device synchronisation and
    the `Epoch .. done` line, a checkpoint every CHECKPOINT_PERIOD, an evaluation every EVAL_PERIOD.  Returns best_index.
    center_criterion, optimizer_center and local_rank are taken for the signature's sake: the reference's loop only zeroes the
    centre optimizer's (never computed) gradients, and the model is expected on its device already.

    save_state=True: every CHECKPOINT_PERIOD epoch ALSO writes <OUTPUT_DIR>/<NAME>_state_<epoch>.pth (save_checkpoint: the whole
    training state), after that epoch's evaluation so that best_index is current; the previous state file is removed once the new
    one is in place.  resume=<path> loads such a file before the first epoch and continues at its epoch + 1 exactly as the
    uninterrupted run would have (same batches, same drop-path draws, same meters / scheduler / evaluator handling);
    resume='auto' takes the highest-numbered state file of OUTPUT_DIR and starts afresh if there is none.  With MODEL.DIST_TRAIN
    only the main rank writes and every rank loads the same file (checked on one rank only: no multi-rank run exists here)."""
    log_period, checkpoint_period, eval_period = cfg.SOLVER.LOG_PERIOD, cfg.SOLVER.CHECKPOINT_PERIOD, cfg.SOLVER.EVAL_PERIOD
    logger = logger or logging.getLogger("EDITOR.train")
    logger.info("start training")
    quiet = writer is None
    writer = _NullWriter() if quiet else writer
    dev = _model_device(model)
    main = _is_main(cfg)
    buckets = getattr(model, "grad_buckets", None)
    if buckets is None and hasattr(model, "enable_grad_buckets"):
        group = dist.group.WORLD if dist.is_available() and dist.is_initialized() else None
        buckets = model.enable_grad_buckets(process_group=group)
    evaluator = _make_evaluator(cfg, num_query)
    evaluator.reset()
    meters = DeviceMeters(dev)
    step = TrainStep(model, loss_fn, optimizer, scaler=scaler, buckets=buckets, meters=meters, graph=graph)
    name = os.path.join(cfg.OUTPUT_DIR, cfg.MODEL.NAME)

    best_index = {"mAP": 0, "Rank-1": 0, "Rank-5": 0, "Rank-10": 0}
    first_epoch, state_file = 1, None
    if resume is not None:
        path = latest_state_file(cfg.OUTPUT_DIR, cfg.MODEL.NAME) if resume == "auto" else resume
        if path is not None:
            ckpt = load_checkpoint(path, step, scheduler=scheduler, loaders=(train_loader, val_loader))
            first_epoch = ckpt["epoch"] + 1
            if ckpt["best_index"] is not None:
                best_index.update(ckpt["best_index"])
            if os.path.dirname(os.path.abspath(path)) == os.path.abspath(cfg.OUTPUT_DIR) and _STATE_FILE.search(path):
                state_file = path                                          # ours: replaced by the next one this run writes
            logger.info("resumed from {} (epoch {})".format(path, ckpt["epoch"]))
    for epoch in range(first_epoch, cfg.SOLVER.MAX_EPOCHS + 1):
        start_time = time.time()
        meters.reset()
        evaluator.reset()
        scheduler.step(epoch)
        model.train()
        batches = 0
        for n_iter, (img, vid, target_cam, target_view, _paths) in enumerate(train_loader):
            img = {k: _to(v, dev) for k, v in img.items()}
            step.step(img, _to(vid, dev), _to(target_cam, dev), _to(target_view, dev), epoch)
            batches = n_iter + 1
            if batches % log_period == 0:
                seen = meters.read()
                logger.info(LOG_ITERATION.format(epoch, batches, len(train_loader), seen["loss_avg"], seen["acc_avg"],
                                                 scheduler._get_lr(epoch)[0]))
                writer.add_scalar("Loss", seen["loss_avg"], epoch)
                if step.num_count is not None and not quiet:              # (a host read of its own: only for a real writer)
                    writer.add_scalar("num_count", float(step.num_count), epoch)
        if dev is not None and dev.type == "cuda":
            torch.cuda.synchronize(dev)
        time_per_batch = (time.time() - start_time) / max(batches, 1)
        logger.info(LOG_EPOCH.format(epoch, time_per_batch, train_loader.batch_size / max(time_per_batch, 1e-12)))

        if epoch % checkpoint_period == 0 and main:
            os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
            _save(model, name + "_{}.pth".format(epoch))

        if epoch % eval_period == 0 and main:
            cmc, m_ap = _evaluate(cfg, model, val_loader, evaluator, dev)
            _log_results(logger, "Validation Results - Epoch: {}".format(epoch), cmc, m_ap)
            writer.add_scalar("MM/mAP", float(m_ap), epoch)
            writer.add_scalar("MM/Rank-1", float(cmc[0]), epoch)
            if m_ap >= best_index["mAP"]:
                best_index.update({"mAP": m_ap, "Rank-1": cmc[0], "Rank-5": _rank(cmc, 5), "Rank-10": _rank(cmc, 10)})
                os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
                _save(model, name + "best.pth")
            for key in ("mAP", "Rank-1", "Rank-5", "Rank-10"):
                logger.info("Best Multi-Modal {}: {:.2%}".format(key, best_index[key]))
            if dev is not None and dev.type == "cuda":
                torch.cuda.empty_cache()

        if save_state and epoch % checkpoint_period == 0 and main:
            os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
            new = name + "_state_{}.pth".format(epoch)
            save_checkpoint(new, step, epoch=epoch, scheduler=scheduler, loaders=(train_loader, val_loader), best_index=best_index)
            if state_file is not None and os.path.abspath(state_file) != os.path.abspath(new):
                with contextlib.suppress(OSError):
                    os.remove(state_file)
            state_file = new
    return best_index


def do_inference(cfg, model, val_loader, num_query, *, logger=None):
    """engine/processor.py:217-270, then the evaluator's compute() and the result lines -> (cmc, mAP); (None, None) on the ranks
    that do not evaluate (MODEL.DIST_TRAIN, rank != 0)."""
    logger = logger or logging.getLogger("EDITOR.test")
    logger.info("Enter inferencing")
    evaluator = _make_evaluator(cfg, num_query)
    evaluator.reset()
    if not _is_main(cfg):
        return None, None
    dev = _model_device(model)
    cmc, m_ap = _evaluate(cfg, model, val_loader, evaluator, dev)
    _log_results(logger, "Validation Results ", cmc, m_ap)
    if dev is not None and dev.type == "cuda":
        torch.cuda.empty_cache()
    return cmc, m_ap
