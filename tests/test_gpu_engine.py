"""editor_amd.engine on the device: an eager TrainStep against the hand-written loop of tests/test_gpu_model.py (bit for bit,
meters included), a captured TrainStep against an eager one over a batch sequence that makes it warm up, capture, replay, step
aside for a short batch and replay again, and do_train / do_inference end to end on a small RGBNT201 tree written with Pillow."""
import contextlib
import copy
import io
import logging
import math
import os
import re

import numpy as np
import pytest
import torch

from editor_amd import config, synth

pytestmark = pytest.mark.gpu

B = 64      # 3*B*129 token rows must be a multiple of 64: otherwise the wgrad split-K falls back to fp32 atomics (test_gpu_model.py)


_TEMPLATE = []


def _build():
    """An identically seeded model and optimizer.  The host model is made and filled once; every call copies it to the device
    (the drop-path generator is seeded at the first forward, from the seed set here)."""
    from editor_amd.modeling import make_model
    from editor_amd.optim import FusedSGD
    if not _TEMPLATE:
        cfg, c, cams = config.preset("RGBNT201", compute_dtype="bf16", drop_path=0.1)
        with contextlib.redirect_stdout(io.StringIO()):
            m = make_model(cfg, c, cams)
        synth.fill_state_dict_(m.state_dict(), 31)
        _TEMPLATE.extend([m, cams])
    torch.manual_seed(77)
    m, cams = copy.deepcopy(_TEMPLATE[0]).cuda().train(), _TEMPLATE[1]
    opt = FusedSGD(m.named_parameters(), base_lr=1e-2, weight_decay=1e-4, bias_lr_factor=2.0, weight_decay_bias=1e-4, momentum=0.9)
    return m, opt, cams


_BATCHES = {}


def _batch(seed, b, cams):
    """Synthetic batches, made once and never written to."""
    if (seed, b) not in _BATCHES:
        img, label, cam, view = synth.make_batch(seed, b, 256, 128, cams, instances=8)
        _BATCHES[(seed, b)] = ({k: v.cuda() for k, v in img.items()}, label.cuda(), cam.cuda(), view.cuda())
    return _BATCHES[(seed, b)]


def _same_model(m1, m2, what):
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    assert list(sd1) == list(sd2)
    diff = [k for k in sd1 if not torch.equal(sd1[k], sd2[k])]
    assert not diff, (what, len(diff), diff[:6])
    assert torch.equal(m1._drop_state, m2._drop_state), what


class _Quiet:
    def add_scalar(self, *a, **k):
        pass


def test_eager_train_step_equals_the_hand_written_loop():
    """Three steps over three different batches: every parameter and buffer, the drop-path generator state and the meter
    averages (against loss.item() and the torch accuracy accumulated in Python doubles) are equal bit for bit."""
    from editor_amd import losses
    from editor_amd.engine import DeviceMeters, TrainStep
    m1, opt1, cams = _build()
    seeds = (5, 6, 7)
    loss_sum = samples = acc_sum = steps = 0.0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # (side stream: see bench.py on AccumulateGrad and capture)
        for s in seeds:
            img, label, cam, view = _batch(s, B, cams)
            opt1.zero_grad(set_to_none=True)
            out = m1(img, label=label, cam_label=cam, view_label=view, img_path=None, writer=_Quiet(), epoch=1)
            loss = losses.loss_pairs(out, label)
            loss.backward()
            opt1.step()
            acc = (out[0].max(1)[1] == label).float().mean()            # processor.py:102-105
            loss_sum += loss.item() * B
            samples += B
            acc_sum += acc.item()
            steps += 1
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    m2, opt2, _ = _build()
    meters = DeviceMeters("cuda")
    ts = TrainStep(m2, None, opt2, meters=meters)
    for s in seeds:
        loss2 = ts.step(*_batch(s, B, cams), epoch=1)
    got = meters.read()
    assert torch.equal(loss2.detach(), loss.detach())
    _same_model(m1, m2, "eager TrainStep")
    assert [got["loss_sum"], got["samples"], got["acc_sum"], got["steps"]] == [loss_sum, samples, acc_sum, steps]
    assert got["loss_avg"] == loss_sum / samples and got["acc_avg"] == acc_sum / steps
    assert (got["last_correct"], got["last_batch"]) == (int((out[0].max(1)[1] == label).sum()), B)
    assert ts.captured is False and ts.num_count is not None and math.isfinite(float(ts.num_count))


def test_captured_train_step_equals_eager():
    """graph=True against graph=False, two identically seeded models, batches of 64, 64, 64, 64, 32, 64 samples: two warm-up
    steps, the capture (+ its first replay), a replay, a short batch that must run eagerly beside the graph, a replay again.

    Compared bit for bit - state dict, drop-path state, meter state - after the FOURTH batch.  The short batch has
    3 * 32 * 129 = 12 384 token rows, not a multiple of 64, so both runs take the weight gradients' fp32-atomics path for it and
    neither is reproducible from run to run; after the sixth batch the two are therefore compared for finiteness only, together
    with what does not depend on arithmetic: `captured`, the count of eagerly run bodies, the meters' sample and step counts."""
    from editor_amd.engine import DeviceMeters, TrainStep
    sizes = (64, 64, 64, 64, 32, 64)
    runs = []
    for graph in (False, True):
        m, opt, cams = _build()
        meters = DeviceMeters("cuda")
        ts = TrainStep(m, None, opt, meters=meters, graph=graph, warmup=2)
        bodies = []
        body = ts._body
        ts._body = lambda *a, _body=body, _n=bodies: (_n.append(a[1].shape[0]), _body(*a))[1]
        after4 = None
        for i, b in enumerate(sizes):
            loss = ts.step(*_batch(20 + i, b, cams), epoch=1)
            if i == 1:
                assert ts.captured is False
            if i == 3:
                torch.cuda.synchronize()
                after4 = ({k: v.clone() for k, v in m.state_dict().items()}, m._drop_state.clone(), meters.state.clone(),
                          meters.last.clone(), loss.detach().clone())
        torch.cuda.synchronize()
        runs.append(dict(m=m, ts=ts, meters=meters.read(), after4=after4, bodies=bodies, loss=loss.detach().clone()))
    eager, cap = runs
    assert eager["ts"].captured is False and cap["ts"].captured is True
    # bodies run from Python: all six eagerly; captured: two warm-ups, the capture itself, the short batch
    assert eager["bodies"] == list(sizes) and cap["bodies"] == [64, 64, 64, 32]
    sd1, drop1, state1, last1, loss1 = eager["after4"]
    sd2, drop2, state2, last2, loss2 = cap["after4"]
    diff = [k for k in sd1 if not torch.equal(sd1[k], sd2[k])]
    assert not diff, (len(diff), diff[:6])
    assert torch.equal(drop1, drop2) and torch.equal(state1, state2) and torch.equal(last1, last2) and torch.equal(loss1, loss2)
    assert state1.tolist()[1] == 256.0 and state1.tolist()[3] == 4.0
    for run in runs:
        assert all(torch.isfinite(v).all() for v in run["m"].state_dict().values() if v.is_floating_point())
        assert torch.isfinite(run["loss"]).all()
        got = run["meters"]
        assert got["samples"] == 352.0 and got["steps"] == 6.0 and got["last_batch"] == 64
        assert math.isfinite(got["loss_avg"]) and 0.0 <= got["acc_avg"] <= 1.0
    assert int(eager["m"]._drop_state.item()) == int(cap["m"]._drop_state.item())


# ---- do_train / do_inference on a small tree -------------------------------------------------------------------------------------

SIZE = (96, 64)


def _image(rng, w, h):
    from PIL import Image
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 17.0) * np.cos(yy / 11.0), 128 + 90 * np.cos(xx / 29.0 + yy / 7.0),
                     255.0 * (xx + yy) / (w + h)], axis=2)
    base += rng.normal(0, 12, base.shape)
    return Image.fromarray(np.clip(base, 0, 255).astype(np.uint8))


def _write_tree(root):
    """RGBNT201 layout: 4 ids x 2 cameras x 3 images (x 3 modalities) to train on; a test split of 6 ids x 2 cameras (query =
    gallery: 12 entries, so that the CMC curve reaches rank 10)."""
    rng = np.random.default_rng(41)
    train = ["%06d_cam%d_0_%02d.jpg" % (p, c, k) for p in (258, 5, 600, 9) for c in (1, 2) for k in range(3)]
    test = ["%06d_cam%d_0_00.jpg" % (p, c) for p in (7, 301, 12, 44, 90, 133) for c in (1, 3)]
    n = 0
    for split, names in (("train_171", train), ("test", test)):
        for m in ("RGB", "NI", "TI"):
            os.makedirs(os.path.join(root, "RGBNT201", split, m))
            for name in names:
                w, h = int(rng.integers(24, 71)), int(rng.integers(40, 111))
                _image(rng, w, h).save(os.path.join(root, "RGBNT201", split, m, name), "JPEG", quality=int(rng.integers(60, 95)),
                                       subsampling=(2, 0)[n % 2])
                n += 1


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("engine_tree"))
    _write_tree(root)
    return root


def _small(root, out_dir):
    """deit_small at 96 x 64 (the model of tests/test_gpu_loader.py's training step), bf16, with its loaders."""
    from editor_amd.data import make_dataloader
    from editor_amd.modeling import make_model
    torch.manual_seed(3)
    cfg, c, cams = config.preset("RGBNT201", compute_dtype="bf16", drop_path=0.1, size_train=SIZE,
                                 transformer_type="deit_small_patch16_224")
    cfg.DATASETS.NAMES, cfg.DATASETS.ROOT_DIR = "RGBNT201", root
    cfg.SOLVER.IMS_PER_BATCH, cfg.DATALOADER.NUM_INSTANCE, cfg.TEST.IMS_PER_BATCH = 8, 4, 4
    cfg.SOLVER.MAX_EPOCHS, cfg.SOLVER.LOG_PERIOD, cfg.SOLVER.CHECKPOINT_PERIOD, cfg.SOLVER.EVAL_PERIOD = 2, 1, 1, 2
    cfg.TEST.FEAT_NORM, cfg.OUTPUT_DIR = "yes", out_dir
    with contextlib.redirect_stdout(io.StringIO()):
        loaders = make_dataloader(cfg)
        model = make_model(cfg, c, cams)
    synth.fill_state_dict_(model.state_dict(), 17)
    for ld in loaders[:3]:
        ld.timeout = 60.0
    return cfg, model.cuda(), loaders, (c, cams)


class _Counted:
    """A train loader that counts the batches it hands out."""

    def __init__(self, loader):
        self.loader, self.batch_size, self.sizes = loader, loader.batch_size, []

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            self.sizes.append(batch[0]["RGB"].shape[0])
            yield batch


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _logger():
    lg = logging.Logger("engine-gpu-test", level=logging.INFO)
    h = _Lines()
    lg.addHandler(h)
    return lg, h.lines


def test_do_train_end_to_end(tree, tmp_path):
    from editor_amd import losses, solver
    from editor_amd.engine import do_train
    from editor_amd.modeling import make_model
    out_dir = str(tmp_path / "run")
    cfg, model, (train_loader, _, val_loader, num_query, _, _, _), (c, cams) = _small(tree, out_dir)
    loss_fn, center = losses.make_loss(cfg, c)
    opt, opt_center = solver.make_optimizer(cfg, model, None)
    scheduler = solver.create_scheduler(cfg, opt)
    counted = _Counted(train_loader)
    lg, lines = _logger()
    with contextlib.redirect_stdout(io.StringIO()):
        best = do_train(cfg, model, center, counted, val_loader, opt, opt_center, scheduler, loss_fn, num_query, 0, logger=lg)
    assert sorted(os.listdir(out_dir)) == ["EDITOR_1.pth", "EDITOR_2.pth", "EDITORbest.pth"]
    # the checkpoint loads into a fresh model with load_param and holds the trained values
    with contextlib.redirect_stdout(io.StringIO()):
        fresh = make_model(cfg, c, cams)
        fresh.load_param(os.path.join(out_dir, "EDITOR_2.pth"))
    sd, fd = model.state_dict(), fresh.state_dict()
    assert all(torch.equal(sd[k].cpu(), fd[k].cpu()) for k in sd)
    # one Iteration line per batch, numbered 1..n within each epoch, finite loss, accuracy in [0, 1]
    pat = re.compile(r"Epoch\[(\d+)\] Iteration\[(\d+)/(\d+)\] Loss: (\S+), Acc: (\S+), Base Lr: (\S+)")
    its = [pat.fullmatch(ln) for ln in lines if ln.startswith("Epoch[")]
    assert all(its) and len(its) == len(counted.sizes) >= 2
    per_epoch = {e: [int(m.group(2)) for m in its if int(m.group(1)) == e] for e in (1, 2)}
    assert all(per_epoch[e] == list(range(1, len(per_epoch[e]) + 1)) and per_epoch[e] for e in (1, 2))
    for m in its:
        assert int(m.group(3)) == len(train_loader)
        assert math.isfinite(float(m.group(4))) and 0.0 <= float(m.group(5)) <= 1.0 and float(m.group(6)) > 0.0
    assert sum(ln.startswith("Epoch 1 done.") for ln in lines) == 1 and sum(ln.startswith("Epoch 2 done.") for ln in lines) == 1
    # exactly one block of validation lines (EVAL_PERIOD = 2), and the returned best_index is the logged one
    i = lines.index("Validation Results - Epoch: 2")
    assert sum(ln.startswith("Validation Results") for ln in lines) == 1
    assert lines[i + 1] == "mAP: {:.2%}".format(best["mAP"]) and lines[i + 5] == "Best Multi-Modal mAP: {:.2%}".format(best["mAP"])
    assert [ln.split(":")[0] for ln in lines[i + 2:i + 5]] == ["CMC curve, Rank-1  ", "CMC curve, Rank-5  ", "CMC curve, Rank-10 "]
    assert lines[i + 6] == "Best Multi-Modal Rank-1: {:.2%}".format(best["Rank-1"])
    assert 0.0 < best["mAP"] <= 1.0 and sum(ln.startswith("Best Multi-Modal") for ln in lines) == 4


def test_do_inference_equals_a_hand_written_loop(tree, tmp_path):
    from editor_amd.engine import do_inference
    from editor_amd.metrics import R1_mAP_eval
    cfg, model, (_, _, val_loader, num_query, _, _, _), _ = _small(tree, str(tmp_path / "unused"))
    assert num_query == 12 and len(val_loader) == 6
    lg, lines = _logger()
    with contextlib.redirect_stdout(io.StringIO()):
        cmc, m_ap = do_inference(cfg, model, val_loader, num_query, logger=lg)
        ev = R1_mAP_eval(num_query, max_rank=50, feat_norm="yes")
        ev.reset()
        model.eval()
        for img, vid, camid, camids, target_view, paths in val_loader:
            with torch.no_grad():
                feat = model(img, cam_label=camids.cuda(), view_label=target_view.cuda(), mode=1, img_path=paths)
            ev.update((feat, vid, camid))
        want_cmc, want_map = ev.compute()[:2]
    assert m_ap == want_map and np.array_equal(cmc, want_cmc)
    assert lines[:3] == ["Enter inferencing", "Validation Results ", "mAP: {:.2%}".format(want_map)]
    assert lines[3:] == ["CMC curve, Rank-{:<3}:{:.2%}".format(r, want_cmc[r - 1]) for r in (1, 5, 10)]
