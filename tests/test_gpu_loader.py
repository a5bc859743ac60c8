"""editor_amd.data.make_dataloader / editor_amd.loader.DeviceBatchLoader on the device, on small trees written with Pillow:
val batches against the Pillow chain, train batches against the Pillow chain + oracle/augment_ref.py fed the loader's own
parameter rows and noise - bit for bit - and the concurrency rules: batches do not depend on the prefetch depth, stay intact
under a busy consumer stream, errors reach the consumer, the worker thread ends.  Every wait has a timeout (the loader's)."""
import contextlib
import gc
import io
import os
import random
import shutil
import threading

import numpy as np
import pytest
import torch

from editor_amd import config

pytestmark = pytest.mark.gpu
MEAN = STD = (0.5, 0.5, 0.5)
SIZES = {"RGBNT201": (96, 64), "RGBNT100": (64, 128)}
WAIT = 60.0


def _image(rng, w, h, gray=False):
    from PIL import Image
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 17.0) * np.cos(yy / 11.0), 128 + 90 * np.cos(xx / 29.0 + yy / 7.0),
                     255.0 * (xx + yy) / (w + h)], axis=2)
    base += rng.normal(0, 12, base.shape)
    a = np.clip(base, 0, 255).astype(np.uint8)
    return Image.fromarray(a[..., 0] if gray else a)


def _write_separate(root):
    """RGBNT201 layout: 4 ids x 2 cameras x 3 images (x 3 modalities), 24x40 .. 70x110 px, 4:2:0 / 4:4:4 mixed, one grayscale and
    one progressive file; a test split of 5 samples (query = gallery)."""
    rng = np.random.default_rng(31)
    n = 0
    for split, names in (("train_171", ["%06d_cam%d_0_%02d.jpg" % (p, c, k) for p in (258, 5, 600, 9) for c in (1, 2) for k in range(3)]),
                         ("test", ["%06d_cam%d_0_00.jpg" % (p, c) for p, c in ((7, 1), (7, 3), (301, 2), (301, 4), (12, 1))])):
        for m in ("RGB", "NI", "TI"):
            os.makedirs(os.path.join(root, "RGBNT201", split, m))
            for name in names:
                w, h = (24, 40) if n == 0 else (70, 110) if n == 1 else (int(rng.integers(24, 71)), int(rng.integers(40, 111)))
                kw = dict(quality=int(rng.integers(60, 95)))
                if n != 7:
                    kw["subsampling"] = (2, 0)[n % 2]
                if n == 11:
                    kw["progressive"] = True
                _image(rng, w, h, gray=(n == 7)).save(os.path.join(root, "RGBNT201", split, m, name), "JPEG", **kw)
                n += 1


def _write_stitched(root):
    """RGBNT100 layout: 768x128 stitched files, 3 ids x 4 images; query 3, gallery 4."""
    rng = np.random.default_rng(32)
    n = 0
    for split, names in (("bounding_box_train", ["%04d_c%d_%03d.jpg" % (p, 1 + k % 2, k) for p in (258, 5, 600) for k in range(4)]),
                         ("query", ["%04d_c3_000.jpg" % p for p in (1, 41, 600)]),
                         ("bounding_box_test", ["%04d_c%d_001.jpg" % (p, c) for p, c in ((1, 4), (41, 5), (600, 8), (77, 6))])):
        os.makedirs(os.path.join(root, "RGBNT100", "rgbir", split))
        for name in names:
            _image(rng, 768, 128).save(os.path.join(root, "RGBNT100", "rgbir", split, name), "JPEG", quality=int(rng.integers(60, 95)),
                                       subsampling=(2, 0)[n % 2])
            n += 1


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("loader_trees"))
    _write_separate(root)
    _write_stitched(root)
    return root


def _cfg(root, name, **over):
    cfg = config.make_cfg(size_train=SIZES[name])
    cfg.DATASETS.NAMES, cfg.DATASETS.ROOT_DIR = name, root
    cfg.SOLVER.IMS_PER_BATCH, cfg.DATALOADER.NUM_INSTANCE, cfg.TEST.IMS_PER_BATCH = 8, 4, 4
    for k, v in over.items():
        setattr(cfg.SOLVER, k, v)
    return cfg


def _loaders(root, name, **kw):
    from editor_amd.data import make_dataloader
    with contextlib.redirect_stdout(io.StringIO()):
        out = make_dataloader(_cfg(root, name))
    for ld in out[:3]:
        ld.timeout = WAIT
        for k, v in kw.items():
            setattr(ld, k, v)
    return out


_PIL = {}


def _pillow_u8(sample, size, resample):
    """One sample -> its modality images as Pillow makes them: uint8 (nmod, H, W, 3).  Computed once per (files, size, filter)."""
    from PIL import Image
    key = (str(sample[0]), size, resample)
    if key not in _PIL:
        if isinstance(sample[0], str):
            img = Image.open(sample[0]).convert("RGB")
            mods = [img.crop((256 * i, 0, 256 * (i + 1), 128)) for i in range(img.size[0] // 256)]
        else:
            mods = [Image.open(p).convert("RGB") for p in sample[0]]
        _PIL[key] = np.stack([np.asarray(m.resize((size[1], size[0]), resample=resample)) for m in mods])
    return _PIL[key]


def _to_tensor_normalize(u8):
    """ToTensor + Normalize of a (B, H, W, 3) uint8 array, single fp32 operations."""
    x = torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255)
    return (x - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)


def _host(batch):
    """A batch with its tensors copied to the host (after the consumer stream's wait: .cpu() is ordered on it)."""
    return ({k: v.cpu() for k, v in batch[0].items()},) + tuple(batch[1:])


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert list(x) == list(y) == ["RGB", "NI", "TI"]
            for k in x:
                assert x[k].dtype == torch.float32 and torch.equal(x[k], y[k]), k
        elif isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype == torch.int64 and torch.equal(x, y)
        else:
            assert x == y


@pytest.mark.parametrize("entropy", ["host", "device", "device_split"])
@pytest.mark.parametrize("name", ["RGBNT201", "RGBNT100"])
def test_val_batches_equal_the_pillow_chain(name, entropy, trees):
    _, normal, val, num_query, _, _, _ = _loaders(trees, name, entropy=entropy)
    samples = val.samples
    assert num_query == {"RGBNT201": 5, "RGBNT100": 3}[name] and len(samples) == {"RGBNT201": 10, "RGBNT100": 7}[name]
    at = 0
    for batch in val:
        imgs, pids, camids, camids_batch, viewids, names = batch
        b = len(pids)
        rows = samples[at:at + b]
        assert isinstance(pids, tuple) and isinstance(camids, tuple) and b == min(4, len(samples) - at)
        assert pids == tuple(r[1] for r in rows) and camids == tuple(r[2] for r in rows)
        assert camids_batch.dtype == viewids.dtype == torch.int64 and camids_batch.tolist() == list(camids)
        assert viewids.tolist() == [r[3] for r in rows]
        assert list(names) == [(r[0] if isinstance(r[0], str) else r[0][0]).split("/")[-1] for r in rows]
        want = np.stack([_pillow_u8(r, SIZES[name], 2) for r in rows])                   # (B, 3, H, W, 3) uint8, BILINEAR
        for m, key in enumerate(("RGB", "NI", "TI")):
            got = imgs[key]
            assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (b, 3) + SIZES[name]
            assert torch.equal(got.cpu(), _to_tensor_normalize(want[:, m])), (key, at)
        at += b
    assert at == len(samples) and len(val) == (len(samples) + 3) // 4
    first = next(iter(normal))                                                            # the train list through the val transform
    assert first[1] == tuple(r[1] for r in normal.samples[:4])


@pytest.mark.parametrize("name", ["RGBNT201", "RGBNT100"])
def test_train_epoch_equals_the_pillow_chain_and_the_oracle_transform(name, trees):
    from oracle import augment_ref
    train = _loaders(trees, name)[0]
    size = SIZES[name]
    random.seed(4); np.random.seed(4)
    batches = train.index_batches()
    assert [len(b) for b in batches] == {"RGBNT201": [8, 8], "RGBNT100": [8]}[name]
    train.epoch = 2
    draws = train.draw_rows(2, batches)                                                   # the loader's own rows and noise seeds
    random.seed(4); np.random.seed(4)
    got = [_host(b) for b in train]
    assert len(got) == len(batches) <= len(train)                                        # (a sampler's __len__ is an upper estimate)
    full = torch.tensor([[0, 0, 0, 1, 0, 0, size[0], size[1]]] * 24, dtype=torch.int32)  # erase everything: the noise field itself
    for idx, (rows, nseed), (imgs, pids, camids, viewids, names) in zip(batches, draws, got):
        sam = [train.samples[i] for i in idx]
        assert pids.dtype == camids.dtype == viewids.dtype == torch.int64
        assert pids.tolist() == [s[1] for s in sam] and camids.tolist() == [s[2] for s in sam] and viewids.tolist() == [-1] * 8
        assert list(names) == [(s[0] if isinstance(s[0], str) else s[0][0]).split("/")[-1] for s in sam]
        assert (pids.view(2, 4) == pids.view(2, 4)[:, :1]).all()                         # 2 identities x 4 instances
        noise = train.transform(torch.zeros((24,) + size + (3,), dtype=torch.uint8, device="cuda"), params=full, seed=nseed).cpu()
        u8 = np.stack([_pillow_u8(s, size, 3) for s in sam])                             # (8, 3, H, W, 3), BICUBIC
        u8 = np.ascontiguousarray(u8.transpose(1, 0, 2, 3, 4)).reshape((24,) + size + (3,))   # modality-major, as launched
        want = augment_ref.train_transform(torch.from_numpy(u8), rows, 10, MEAN, STD, noise)
        assert int(rows[:, 3].sum()) > 0 and int(rows[:, 0].sum()) > 0
        for m, key in enumerate(("RGB", "NI", "TI")):
            assert torch.equal(imgs[key], want[m * 8:(m + 1) * 8]), key
    assert train.epoch == 3                                                               # every iter() is one epoch


def _sequential(trees, prefetch, entropy="device_split", root=None, **kw):
    from editor_amd.datasets import list_dataset
    from editor_amd.loader import DeviceBatchLoader
    ds = list_dataset("RGBNT201", root or trees, verbose=False)
    samples = sorted(ds.train, key=lambda s: s[0][0])
    return DeviceBatchLoader(samples, 4, SIZES["RGBNT201"], True, prefetch=prefetch, entropy=entropy, seed=3, timeout=WAIT, **kw)


@pytest.fixture(scope="module")
def yardstick(trees):
    """One train epoch of the sequential loader at prefetch=0 (6 batches of 4), on the host: computed once, left unchanged."""
    return [_host(b) for b in _sequential(trees, 0)]


def test_batches_do_not_depend_on_prefetch_depth_or_entropy_mode(trees, yardstick):
    assert len(yardstick) == 6
    for prefetch, entropy in ((1, "device_split"), (3, "device_split"), (3, "host"), (0, "device")):
        ld = _sequential(trees, prefetch, entropy)
        got = [_host(b) for b in ld]
        assert len(got) == 6
        for a, b in zip(got, yardstick):
            _same(a, b)
        nxt = [_host(b) for b in ld]                                                      # the next epoch: other draws
        assert not torch.equal(nxt[0][0]["RGB"], yardstick[0][0]["RGB"])
        ld.close()
    assert not [t for t in threading.enumerate() if t.name == "editor-loader-worker"]


def test_batches_stay_intact_under_a_busy_consumer_stream(trees, yardstick):
    a = torch.randn(2048, 2048, device="cuda")
    kept, clones = [], []
    for batch in _sequential(trees, 3):
        clones.append({k: v.clone() for k, v in batch[0].items()})                       # at once, on the consumer's stream
        kept.append(batch)
        if len(kept) > 3:
            kept[-4] = None                                                               # this batch and the two before it stay alive
        c = a
        for _ in range(6):
            c = torch.matmul(c, a) * 1e-2
    torch.cuda.synchronize()
    assert len(clones) == 6
    for i, (c, y) in enumerate(zip(clones, yardstick)):
        for k in c:
            assert torch.equal(c[k].cpu(), y[0][k]), (i, k)                              # the event wait: clones are the finished batch
    for i, b in enumerate(kept):
        if b is not None:
            for k in clones[i]:
                assert torch.equal(b[0][k], clones[i][k]), (i, k)                        # nothing recycled under the consumer


def _no_worker():
    return not [t for t in threading.enumerate() if t.name == "editor-loader-worker"]


@pytest.mark.parametrize("fault,entropy", [("arithmetic", "host"), ("arithmetic", "device_split"), ("deleted", "device_split")])
def test_a_bad_file_reaches_the_consumer_on_its_batch(fault, entropy, trees, yardstick, tmp_path):
    root = str(tmp_path / "copy")
    shutil.copytree(os.path.join(trees, "RGBNT201"), os.path.join(root, "RGBNT201"))
    ld = _sequential(trees, 2, entropy, root=root)
    victim = ld.samples[9][0][1]                                                          # batch 2, sample 1, NI: file 1 * 4 + 1 of its batch
    if fault == "deleted":
        os.remove(victim)
    else:                                                                                 # arithmetic-coded sequential: refused by the host parser
        data = bytearray(open(victim, "rb").read())
        data[data.index(b"\xff\xc0") + 1] = 0xC9
        open(victim, "wb").write(bytes(data))
    it = iter(ld)
    first = [_host(next(it)), _host(next(it))]
    with pytest.raises(FileNotFoundError if fault == "deleted" else ValueError) as e:
        next(it)
    assert victim in str(e.value)
    if fault != "deleted":
        assert "file 5 of the batch" in str(e.value)
    for a, b in zip(first, yardstick):                                                    # the batches before it are intact
        _same(a, b)
    assert _no_worker()
    with pytest.raises(StopIteration):
        next(it)
    # prefetch=0: the same error from the same call, no thread
    it = iter(_sequential(trees, 0, entropy, root=root))
    next(it), next(it)
    with pytest.raises(FileNotFoundError if fault == "deleted" else ValueError, match="cam"):
        next(it)


def test_close_and_garbage_collection_end_the_worker(trees, yardstick):
    ld = _sequential(trees, 2)
    it = iter(ld)
    _same(_host(next(it)), yardstick[0])
    assert not _no_worker()
    it.close()
    assert _no_worker()
    with pytest.raises(StopIteration):
        next(it)
    it = iter(ld)
    next(it)
    del it
    gc.collect()
    assert _no_worker()
    for _ in ld:                                                                          # an exception in the consumer's loop
        try:
            raise KeyError("consumer")
        except KeyError:
            break
    gc.collect()
    assert _no_worker()


class _Writer:
    def add_scalar(self, *a, **k):
        pass


def _one_step(trees, prefetch):
    """deit_small at (96, 64), B = 8, the model settings of tests/test_gpu_pipeline.py: the first train batch -> forward ->
    make_loss -> backward -> make_optimizer step.  -> the updated parameters."""
    from editor_amd import losses, solver, synth
    from editor_amd.modeling import make_model
    from editor_amd.optim import DeviceGradScaler
    torch.manual_seed(3)
    random.seed(3)
    np.random.seed(3)
    cfg, c, cams = config.preset("RGBNT201", compute_dtype="f16", drop_path=0.1, grad_scale=1.0, size_train=SIZES["RGBNT201"],
                                 transformer_type="deit_small_patch16_224")
    with contextlib.redirect_stdout(io.StringIO()):
        model = make_model(cfg, c, cams)
    synth.fill_state_dict_(model.state_dict(), 17)
    model = model.cuda().train()
    buckets = model.enable_grad_buckets()
    opt, _ = solver.make_optimizer(cfg, model, None)
    scaler = DeviceGradScaler("cuda", init_scale=2.0 ** 12, growth_interval=1000)
    loss_fn, _ = losses.make_loss(cfg, c)
    train = _loaders(trees, "RGBNT201", prefetch=prefetch)[0]
    it = iter(train)
    img, label, cam, view, _ = next(it)
    it.close()
    assert img["RGB"].shape == (8, 3, 96, 64)
    label, cam, view = label.cuda(), cam.cuda(), view.cuda()
    opt.zero_grad()
    out = model(img, label=label, cam_label=cam, view_label=view, writer=_Writer(), epoch=1)
    loss = losses.loss_pairs(out, label, loss_fn)
    scaler.scale(loss).backward()
    buckets.finish()
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    loss = float(loss.detach())
    assert np.isfinite(loss) and not opt.found_inf()
    return {k: v.detach().clone() for k, v in model.named_parameters()}, loss


def test_one_training_step_from_the_loader_equals_the_synchronous_loader(trees):
    from editor_amd import functional
    keep = functional.F16_GRAD_SCALE                                                      # grad_scale=1.0 sets a process-wide value:
    try:                                                                                  # hand it back to the tests after this file
        p2, l2 = _one_step(trees, 2)
        p0, l0 = _one_step(trees, 0)
    finally:
        functional.set_f16_grad_scale(keep)
    assert l2 == l0
    diff = [k for k in p0 if not torch.equal(p0[k], p2[k])]
    assert not diff, diff[:6]
