"""Full-state checkpoints on the device: the operand-refresh kernel against the update kernel's own shadows, a resume into
differently seeded fresh objects (eager, captured, AdamW), a roll-back into a live captured step, the refusals, and do_train
stopped and resumed against the uninterrupted run.  Every comparison is bit for bit; B = 64 as in tests/test_gpu_engine.py, where
the weight gradients take no fp32-atomics path and the step is reproducible from run to run."""
import contextlib
import copy
import gc
import io
import os
import random

import numpy as np
import pytest
import torch

import resume_helpers as R
from editor_amd import config, synth

pytestmark = pytest.mark.gpu

B = 64      # 3*B*129 token rows must be a multiple of 64 (tests/test_gpu_engine.py)


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------

def _edge_params(shadow_dtype):
    """Hand-made parameters: numels 1, 3, chunk - 1, chunk, chunk + 1, 2 chunk + 5 (2-D, so that they have shadows), two views at
    4-byte and 8-byte aligned addresses (the kernel's scalar path), one (512, 512) weight (it gets a W^T copy), a 1-D tensor between
    two 2-D ones (a NULL entry in the shadow table), and a last 2-D tensor that never gets a gradient."""
    from editor_amd import _lib
    chunk = int(_lib.lib().cdll.editor_sgd_chunk_elems())
    g = torch.Generator().manual_seed(123)
    special = R.special_values(shadow_dtype)
    named = []
    for i, n in enumerate((1, 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 5)):
        t = 0.02 * torch.randn(1, n, generator=g)
        R.plant(t, special, 10 + i)
        named.append(("edge%d.weight" % i, t.cuda()))
    arena = torch.zeros(4096 + 8, device="cuda")
    for i, (start, n) in enumerate(((1, 1001), (1030, 2050))):                       # element offsets 1 (4 B) and 1030 (8 B) of the arena
        t = 0.02 * torch.randn(n, generator=g)
        R.plant(t, special, 20 + i)
        view = arena[start:start + n].view(1, n)
        view.copy_(t.view(1, n))
        named.append(("view%d.weight" % i, view))
    big = 0.02 * torch.randn(512, 512, generator=g)
    R.plant(big, special, 30)
    named.append(("big.weight", big.cuda()))
    named.append(("flat.gain", (0.02 * torch.randn(37, generator=g)).cuda()))
    named.append(("after.weight", (0.02 * torch.randn(3, 5, generator=g)).cuda()))
    named.append(("nograd.weight", (0.02 * torch.randn(7, 9, generator=g)).cuda()))
    return [(n, torch.nn.Parameter(t)) for n, t in named], arena


@pytest.mark.parametrize("shadow,pairs", [(torch.bfloat16, False), (torch.float16, False), (torch.float16, True)],
                         ids=["bf16", "f16", "f16-pairs"])
def test_refresh_writes_the_update_kernels_bits(shadow, pairs):
    """The yardstick is the update kernel: one step() with zero gradients, lr = 0 and wd = 0 leaves the parameters as they are (a
    planted +-inf becomes NaN there: wd * inf = 0 * inf, in the parameter itself, so both kernels convert the same NaN) and
    writes the shadows.  Scrambled shadows, W^T copies and pairs come back bit for bit from refresh_operands(), which also covers
    the weight that never had a gradient, and every copy is installed in the operand cache."""
    from editor_amd import functional
    from editor_amd.optim import FusedSGD
    named, arena = _edge_params(shadow)
    opt = FusedSGD(named, base_lr=0.0, weight_decay=0.0, bias_lr_factor=1.0, weight_decay_bias=0.0, momentum=0.9,
                   shadow_dtype=shadow, split_pairs=pairs)
    before = [p.detach().clone() for _, p in named]
    for n, p in named:
        p.grad = None if n == "nograd.weight" else torch.zeros_like(p)
    opt.step()
    torch.cuda.synchronize()
    for (n, p), old in zip(named, before):
        was_inf = torch.isinf(old)
        assert R.same_bits(p.detach().masked_fill(was_inf, 0), old.masked_fill(was_inf, 0)), n
        assert torch.isnan(p.detach()[was_inf]).all(), n
    assert [h is None for h in opt.shadows] == [p.dim() < 2 for _, p in named]
    assert [h is not None for h in opt.shadows_t] == [n == "big.weight" for n, _ in named]
    want_h = [None if h is None else h.clone() for h in opt.shadows]
    want_pairs = None if not pairs else [None if pr is None else (pr[0].clone(), pr[1].clone()) for pr in opt.pairs]
    nograd = [n for n, _ in named].index("nograd.weight")
    want_h[nograd] = named[nograd][1].detach().to(shadow)          # (plain values: torch rounds to nearest even as well)

    def scramble():
        for group in (opt.shadows, opt.shadows_t):
            for h in group:
                if h is not None:
                    h.view(torch.int16).fill_(0x5A5A)
        for pr in opt.pairs or ():
            if pr is not None:
                pr[0].view(torch.int16).fill_(0x5A5A)
                pr[1].view(torch.int16).fill_(0x5A5A)

    scramble()
    arena_before = arena.clone()
    opt.refresh_operands()
    torch.cuda.synchronize()
    assert R.same_bits(arena, arena_before)                        # (the parameters are only read)
    for (n, p), h, want in zip(named, opt.shadows, want_h):
        if h is not None:
            assert h.dtype == shadow and R.same_bits(h, want), "shadow of %s" % n
    big = [n for n, _ in named].index("big.weight")
    assert R.same_bits(opt.shadows_t[big], opt.shadows[big].t().contiguous()), "W^T copy"
    if pairs:
        for (n, p), pr, want in zip(named, opt.pairs, want_pairs):
            if pr is not None:                                     # (the step's split launch skips no 2-D tensor: it is the yardstick)
                assert R.same_bits(pr[0], want[0]) and R.same_bits(pr[1], want[1]), "pair of %s" % n
    # installed for every weight that has a copy, the one without a gradient included
    for (n, p), h in zip(named, opt.shadows):
        if h is not None:
            assert functional.act_weight(p, shadow) is h, n
    assert functional.act_weight_t(named[big][1], shadow) is opt.shadows_t[big]
    # a second refresh changes nothing
    again = [None if h is None else h.clone() for h in opt.shadows]
    opt.refresh_operands()
    torch.cuda.synchronize()
    assert all(h is None or R.same_bits(h, a) for h, a in zip(opt.shadows, again))


def test_cast_multi_refuses_bad_arguments_and_refresh_refuses_a_capture(monkeypatch):
    from editor_amd import _lib
    from editor_amd.optim import FusedSGD
    p = torch.nn.Parameter(torch.ones(4, 4, device="cuda"))
    opt = FusedSGD([("w.weight", p)], base_lr=0.0, shadow_dtype=torch.bfloat16)
    opt.shadows[0].view(torch.int16).fill_(0x5A5A)
    fn = _lib.lib().cdll.editor_cast_multi
    good = [opt.p_ptrs.data_ptr(), opt.h_ptrs.data_ptr(), opt.chunk_t.data_ptr(), opt.chunk_o.data_ptr(), opt.numel.data_ptr(),
            opt.nchunks, 1, None]
    invalid = 1                                                     # hipErrorInvalidValue
    for i in range(5):
        bad = list(good)
        bad[i] = None
        assert fn(*bad) == invalid, "NULL argument %d" % i
    for nchunks, dtype in ((-1, 1), (1, 0), (1, 3), (1, -1)):
        bad = list(good)
        bad[5], bad[6] = nchunks, dtype
        assert fn(*bad) == invalid, (nchunks, dtype)
    bad = list(good)
    bad[5] = 0
    assert fn(*bad) == 0                                            # nothing to do: no launch, no error
    torch.cuda.synchronize()
    assert (opt.shadows[0].view(torch.int16) == 0x5A5A).all()       # none of these launched
    assert fn(*good) == 0
    torch.cuda.synchronize()
    assert torch.equal(opt.shadows[0], torch.ones(4, 4, device="cuda", dtype=torch.bfloat16))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capturing"):
        opt.refresh_operands()


# ---- the training step of tests/test_gpu_engine.py -----------------------------------------------------------------------------------

_TEMPLATES = {}
_BATCHES = {}
SEEDS = (40, 41, 42, 43, 44)


@pytest.fixture(autouse=True)
def _options_and_memory():
    """A model built with cfg.MODEL.GRAD_SCALE installs a process-wide loss scale: put the earlier one back, and free the models."""
    from editor_amd import functional as fn
    old = (fn.F16_GRAD_SCALE, fn.ACT_LIGHT)
    yield
    fn.set_model_options(grad_scale_f16=old[0], act_light=old[1])
    gc.collect()
    torch.cuda.empty_cache()


def _template(dtype):
    from editor_amd.modeling import make_model
    if dtype not in _TEMPLATES:
        over = {"grad_scale": 1} if dtype == "f16-scaler" else {}
        cfg, c, cams = config.preset("RGBNT201", compute_dtype="f16" if dtype == "f16-scaler" else dtype, drop_path=0.1, **over)
        with contextlib.redirect_stdout(io.StringIO()):
            m = make_model(cfg, c, cams)
        first = next(iter(_TEMPLATES.values()), None)
        if first is None:
            synth.fill_state_dict_(m.state_dict(), 31)
        else:
            m.load_state_dict(first[0].state_dict())               # (the same values: filling is the slow part)
        _TEMPLATES[dtype] = (m, cams)
    return _TEMPLATES[dtype]


def _build(dtype="bf16", opt="sgd", seed=77, scramble=None, betas=(0.8, 0.95)):
    """Model, optimizer, scaler (f16-scaler only), meters.  scramble: a seed - the parameters and buffers are refilled with other
    values on the device and torch is seeded differently, so nothing of a restored run can come from the construction."""
    from editor_amd.engine import DeviceMeters
    from editor_amd.optim import DeviceGradScaler, FusedAdamW, FusedSGD
    tmpl, cams = _template(dtype)
    torch.manual_seed(seed)
    m = copy.deepcopy(tmpl).cuda().train()
    if scramble is not None:
        g = torch.Generator(device="cuda").manual_seed(scramble)
        with torch.no_grad():
            for k, v in m.state_dict().items():
                if v.is_floating_point() and not k.startswith("FREQ_INDEX."):
                    v.copy_(0.02 * torch.randn(v.shape, generator=g, device="cuda") + (1.0 if "running_var" in k else 0.0))
    common = dict(shadow_dtype=m.act_dtype, split_pairs=m.split_fwd)
    if opt == "sgd":
        o = FusedSGD(m.named_parameters(), base_lr=1e-2, weight_decay=1e-4, bias_lr_factor=2.0, weight_decay_bias=1e-4, momentum=0.9,
                     **common)
    else:
        o = FusedAdamW(m.named_parameters(), base_lr=1e-4, weight_decay=1e-2, betas=betas, **common)
    scaler = DeviceGradScaler("cuda", init_scale=2.0 ** 10, growth_interval=2) if dtype == "f16-scaler" else None
    return m, o, scaler, DeviceMeters("cuda"), cams


def _step(parts, **kw):
    from editor_amd.engine import TrainStep
    m, o, scaler, meters, _ = parts
    return TrainStep(m, None, o, scaler=scaler, meters=meters, **kw)


def _batch(seed, cams):
    """Synthetic batches, made once and never written to."""
    if seed not in _BATCHES:
        img, label, cam, view = synth.make_batch(seed, B, 256, 128, cams, instances=8)
        _BATCHES[seed] = ({k: v.cuda() for k, v in img.items()}, label.cuda(), cam.cuda(), view.cuda())
    return _BATCHES[seed]


def _record(parts, loss):
    """Everything the issue compares, as clones: state dict, momentum / moments (+ AdamW's step count), the drop-path counter, the
    scaler's scale and tracker, the meters and the loss."""
    m, o, scaler, meters, _ = parts
    torch.cuda.synchronize()
    rec = {"sd." + k: v.clone() for k, v in m.state_dict().items()}
    rec.update({"momentum.%d" % i: b.clone() for i, b in enumerate(o.bufs)})
    if hasattr(o, "bufs_sq"):
        rec.update({"exp_avg_sq.%d" % i: b.clone() for i, b in enumerate(o.bufs_sq)})
        rec["adam.step"] = o.step_count.clone()
    if scaler is not None:
        rec["scaler.scale"], rec["scaler.tracker"] = scaler._scale.clone(), scaler._tracker.clone()
    rec["drop_state"] = m._drop_state.clone()
    rec["meters"] = meters._buf.clone()
    rec["meters.read"] = meters.read()
    rec["loss"] = loss.detach().clone()
    return rec


def _differences(a, b):
    assert list(a) == list(b)
    return [k for k in a if not (a[k] == b[k] if isinstance(a[k], dict) else torch.equal(a[k], b[k]))]


def _run(parts, seeds, record_at, **kw):
    ts = _step(parts, **kw)
    recs = {}
    for i, s in enumerate(seeds):
        loss = ts.step(*_batch(s, parts[4]), epoch=1)
        if i + 1 in record_at:
            recs[i + 1] = _record(parts, loss)
    return ts, recs


_WHOLE = {}


def _whole_run(opt):
    """Run A: the uninterrupted eager run over SEEDS, recorded after steps 4 and 5 - executed TWICE, the control: if the two
    differ the step itself is not reproducible here and no resume can be judged."""
    if opt not in _WHOLE:
        n = 5 if opt == "sgd" else 4
        first = _run(_build(opt=opt), SEEDS[:n], (4, 5))[1]
        second = _run(_build(opt=opt), SEEDS[:n], (4, 5))[1]
        bad = {k: _differences(first[k], second[k]) for k in first}
        _WHOLE[opt] = (first, {k: v for k, v in bad.items() if v})
    first, bad = _WHOLE[opt]
    assert not bad, "step not reproducible: the same run executed twice differs in %s" % {k: v[:4] for k, v in bad.items()}
    return first


def _first_half(opt, n=2):
    """Run B's first process: n eager steps, then the CPU state dict (what save_checkpoint writes)."""
    parts = _build(opt=opt)
    ts, _ = _run(parts, SEEDS[:n], ())
    return ts.state_dict()


# ---- 2., 3., 5. a resume into fresh, differently seeded objects ---------------------------------------------------------------------

def test_resume_into_fresh_objects_eager():
    whole = _whole_run("sgd")
    sd = _first_half("sgd")
    assert all(not t.is_cuda for t in sd["model"].values()) and sd["model_rng"] is not None and sd["optimizer_class"] == "FusedSGD"
    parts = _build(seed=991, scramble=5)
    ts = _step(parts)
    assert parts[0].rng_state() is None
    ts.load_state_dict(sd)
    assert parts[0].rng_state() == sd["model_rng"]
    for i, s in enumerate(SEEDS[2:4]):
        loss = ts.step(*_batch(s, parts[4]), epoch=1)
    bad = _differences(whole[4], _record(parts, loss))
    assert not bad, "resumed run differs from the uninterrupted one in %d entries: %s" % (len(bad), bad[:6])


def test_resume_into_fresh_objects_then_capture_and_replay():
    """The resumed half under graph=True, warmup=1: one eager step, the capture (+ its first replay) and one more replay."""
    whole = _whole_run("sgd")
    sd = _first_half("sgd")
    parts = _build(seed=992, scramble=6)
    ts = _step(parts, graph=True, warmup=1)
    ts.load_state_dict(sd)
    bodies = []
    body = ts._body
    ts._body = lambda *a, _body=body, _n=bodies: (_n.append(1), _body(*a))[1]
    for s in SEEDS[2:5]:
        loss = ts.step(*_batch(s, parts[4]), epoch=1)
    assert ts.captured is True and len(bodies) == 2                 # the eager step and the capture; the last batch only replayed
    bad = _differences(whole[5], _record(parts, loss))
    assert not bad, "resumed and captured run differs from the uninterrupted one in %d entries: %s" % (len(bad), bad[:6])


def test_resume_adamw_takes_moments_step_count_and_betas():
    """FusedAdamW(betas=(0.8, 0.95)): the fresh optimizer is CONSTRUCTED with torch's default betas and must continue with the
    checkpoint's - equal to the run constructed with them; groups that disagree among themselves are refused."""
    whole = _whole_run("adamw")
    sd = _first_half("adamw")
    assert sd["optimizer_class"] == "FusedAdamW" and float(sd["optimizer"]["state"][0]["step"]) == 2.0
    assert sd["optimizer"]["param_groups"][0]["betas"] == (0.8, 0.95)
    parts = _build(opt="adamw", seed=993, scramble=7, betas=(0.9, 0.999))
    ts = _step(parts)
    ts.load_state_dict(sd)
    assert parts[1].betas == (0.8, 0.95) and float(parts[1].step_count.item()) == 2.0
    for s in SEEDS[2:4]:
        loss = ts.step(*_batch(s, parts[4]), epoch=1)
    bad = _differences(whole[4], _record(parts, loss))
    assert not bad, "resumed AdamW run differs from the uninterrupted one in %d entries: %s" % (len(bad), bad[:6])
    mixed = copy.deepcopy(sd["optimizer"])
    mixed["param_groups"][3]["betas"] = (0.9, 0.95)
    with pytest.raises(ValueError, match="betas"):
        parts[1].load_state_dict(mixed)


# ---- 4. roll-back into a live captured step -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f16x2", "f16-scaler"])
def test_rollback_into_a_live_captured_step(dtype):
    """Warm-up, capture, a replay; a device snapshot; replays on X and Y, recorded; load_state_dict(snapshot) - no new capture;
    replays on X and Y again are bit-equal to the recording.  Parameters restored without their operand copies fail at X: the
    graph's forward reads the shadows' addresses.  'f16-scaler': a DeviceGradScaler(growth_interval=2) whose scale / tracker
    move inside the window."""
    parts = _build(dtype)
    ts = _step(parts, graph=True, warmup=1)
    for s in SEEDS[:3]:                                             # eager, capture (+ replay), replay
        ts.step(*_batch(s, parts[4]), epoch=1)
    assert ts.captured is True
    graph = ts._graph
    snap = ts.state_dict(device=True)
    assert all(t.is_cuda for t in snap["model"].values()) and snap["meters"].is_cuda
    at_snap = _record(parts, torch.zeros((), device="cuda"))
    rec = [_record(parts, ts.step(*_batch(s, parts[4]), epoch=1)) for s in SEEDS[3:5]]
    moved = _differences(at_snap, rec[1])
    assert "drop_state" in moved and "meters" in moved and any(k.startswith("momentum.") for k in moved)
    if dtype == "f16-scaler":
        assert "scaler.scale" in _differences(at_snap, rec[0]) or "scaler.tracker" in _differences(at_snap, rec[0])
        assert snap["scaler"] is not None
    bodies = []
    body = ts._body
    ts._body = lambda *a, _body=body, _n=bodies: (_n.append(1), _body(*a))[1]
    ts.load_state_dict(snap)
    assert ts.captured is True and ts._graph is graph
    back = _record(parts, torch.zeros((), device="cuda"))
    bad = _differences(at_snap, back)
    assert not bad, "the snapshot did not come back: %s" % bad[:6]
    for i, s in enumerate(SEEDS[3:5]):
        got = _record(parts, ts.step(*_batch(s, parts[4]), epoch=1))
        bad = _differences(rec[i], got)
        assert not bad, "replay %d after the roll-back differs in %d entries: %s" % (i + 1, len(bad), bad[:6])
    assert bodies == [] and ts._graph is graph                      # replays only: nothing ran from Python, nothing was re-captured


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------

def test_states_that_do_not_fit_are_refused_and_nothing_is_written():
    from editor_amd.optim import DeviceGradScaler
    src = _build()
    sd = _step(src).state_dict(device=True)

    def refused(ts, state, key):
        m, o = ts.model, ts.optimizer
        before = [p.detach().clone() for p in m.parameters()] + [b.clone() for b in o.bufs]
        with pytest.raises(ValueError, match=key):
            ts.load_state_dict(state)
        torch.cuda.synchronize()
        after = [p.detach() for p in m.parameters()] + list(o.bufs)
        assert all(torch.equal(a, b) for a, b in zip(before, after)), "a refused state was partly written (%s)" % key

    # make the target differ from the state everywhere, so that a partial write would show
    target = _build(seed=5, scramble=8)
    for b in target[1].bufs:
        b.fill_(0.25)
    refused(_step(_build("f16", seed=5, scramble=8)), sd, "compute_dtype")                     # bf16 state -> f16 step
    m = target[0]
    from editor_amd.optim import FusedAdamW
    adam = FusedAdamW(m.named_parameters(), base_lr=1e-4, shadow_dtype=m.act_dtype)
    refused(_step((m, adam, None, target[3], target[4])), sd, "optimizer_class")               # SGD state -> AdamW
    names = list(sd["model"])
    last = [k for k in names if sd["model"][k].dim() == 2][-1]
    shaped = dict(sd, model=dict(sd["model"]))
    shaped["model"][last] = torch.zeros(sd["model"][last].shape[0] + 1, sd["model"][last].shape[1], device="cuda")
    refused(_step(target), shaped, "model." + last.replace(".", r"\."))                        # one parameter's shape
    n = len(target[1].bufs) - 1
    mom = dict(sd, optimizer=copy.copy(sd["optimizer"]))
    mom["optimizer"]["state"] = dict(sd["optimizer"]["state"])
    mom["optimizer"]["state"][n] = {"momentum_buffer": torch.zeros(3, device="cuda")}
    refused(_step(target), mom, r"optimizer\.state\.%d\.momentum_buffer" % n)                  # one momentum buffer's shape
    missing = dict(sd, model={k: v for k, v in sd["model"].items() if k != names[-1]})
    refused(_step(target), missing, "model." + names[-1].replace(".", r"\."))                  # a missing key
    extra = dict(sd, model=dict(sd["model"], intruder=torch.zeros(1)))
    refused(_step(target), extra, "model.intruder")                                            # an extra key
    scaler = DeviceGradScaler("cuda")
    refused(_step((target[0], target[1], scaler, target[3], target[4])), sd, "scaler")         # scaler here, none in the state
    with_scaler = dict(sd, scaler=scaler.state_dict())
    refused(_step(target), with_scaler, "scaler")                                              # and the other way round
    # the untouched state still loads
    ts = _step(target)
    ts.load_state_dict(sd)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(target[0].parameters(), src[0].parameters()))
    assert all(torch.equal(a, b) for a, b in zip(target[1].bufs, src[1].bufs))


# ---- 7. do_train ------------------------------------------------------------------------------------------------------------------------

SIZE = (96, 64)        # 6 x 4 patches + the class token: T = 25, so 3 * B * T % 64 == 0 needs B = 64
IDS, TRAIN_B = 32, 64  # 32 identities x 2 cameras x 2 images = 128 training images: two full batches of 64 an epoch


def _image(rng, w, h):
    from PIL import Image
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 17.0) * np.cos(yy / 11.0), 128 + 90 * np.cos(xx / 29.0 + yy / 7.0),
                     255.0 * (xx + yy) / (w + h)], axis=2)
    base += rng.normal(0, 12, base.shape)
    return Image.fromarray(np.clip(base, 0, 255).astype(np.uint8))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """RGBNT201 layout, written with Pillow: IDS identities x 2 cameras x 2 images (x 3 modalities) to train on; a test split of
    6 identities x 2 cameras (query = gallery: 12 entries)."""
    root = str(tmp_path_factory.mktemp("resume_tree"))
    rng = np.random.default_rng(43)
    train = ["%06d_cam%d_0_%02d.jpg" % (p, c, k) for p in range(3, 3 + 7 * IDS, 7) for c in (1, 2) for k in range(2)]
    test = ["%06d_cam%d_0_00.jpg" % (p, c) for p in (7, 301, 12, 44, 90, 133) for c in (1, 3)]
    for split, names in (("train_171", train), ("test", test)):
        for m in ("RGB", "NI", "TI"):
            os.makedirs(os.path.join(root, "RGBNT201", split, m))
            for name in names:
                w, h = int(rng.integers(24, 71)), int(rng.integers(40, 111))
                _image(rng, w, h).save(os.path.join(root, "RGBNT201", split, m, name), "JPEG", quality=int(rng.integers(60, 95)))
    return root


class _Preempted(Exception):
    pass


class _Hashed:
    """A train loader that hashes every batch it hands out, under the loader's epoch number; stop_before: the (0-based) epoch at
    whose start the process is taken away."""

    def __init__(self, loader):
        self.loader, self.batch_size, self.served, self.stop_before = loader, loader.batch_size, [], None

    epoch = property(lambda self: self.loader.epoch, lambda self, v: setattr(self.loader, "epoch", v))

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        epoch = self.loader.epoch
        if epoch == self.stop_before:
            raise _Preempted()
        for batch in self.loader:
            self.served.append((epoch, batch[0]["RGB"].shape[0], R.batch_hash(batch)))
            yield batch


def _objects(root, out_dir, seed, fill, epochs=3):
    """A process' worth of objects: loaders, model, optimizer, scheduler - seeded by `seed`, parameters filled by `fill`."""
    from editor_amd import losses, solver
    from editor_amd.data import make_dataloader
    from editor_amd.modeling import make_model
    torch.manual_seed(seed)
    random.seed(seed + 1)
    np.random.seed(seed + 2)
    cfg, c, cams = config.preset("RGBNT201", compute_dtype="bf16", drop_path=0.1, size_train=SIZE,
                                 transformer_type="deit_small_patch16_224")
    cfg.DATASETS.NAMES, cfg.DATASETS.ROOT_DIR = "RGBNT201", root
    cfg.SOLVER.IMS_PER_BATCH, cfg.DATALOADER.NUM_INSTANCE, cfg.TEST.IMS_PER_BATCH = TRAIN_B, 4, 4
    cfg.SOLVER.MAX_EPOCHS, cfg.SOLVER.LOG_PERIOD, cfg.SOLVER.CHECKPOINT_PERIOD, cfg.SOLVER.EVAL_PERIOD = epochs, 1, 1, 1
    cfg.TEST.FEAT_NORM, cfg.OUTPUT_DIR = "yes", out_dir
    with contextlib.redirect_stdout(io.StringIO()):
        loaders = make_dataloader(cfg)
        model = make_model(cfg, c, cams)
    synth.fill_state_dict_(model.state_dict(), fill)
    for ld in loaders[:3]:
        ld.timeout = 60.0
    model = model.cuda()
    loss_fn, center = losses.make_loss(cfg, c)
    opt, opt_center = solver.make_optimizer(cfg, model, None)
    scheduler = solver.create_scheduler(cfg, opt)
    return dict(cfg=cfg, model=model, train=_Hashed(loaders[0]), val=loaders[2], num_query=loaders[3], opt=opt, opt_center=opt_center,
                scheduler=scheduler, loss_fn=loss_fn, center=center, c=c, cams=cams)


def _train(o, **kw):
    from editor_amd.engine import do_train
    lg, lines = R.logger()
    with contextlib.redirect_stdout(io.StringIO()):
        best = do_train(o["cfg"], o["model"], o["center"], o["train"], o["val"], o["opt"], o["opt_center"], o["scheduler"],
                        o["loss_fn"], o["num_query"], 0, logger=lg, **kw)
    torch.cuda.synchronize()
    return best, lines


def _epoch3(lines):
    """Epoch 3's lines without the one that carries wall-clock time."""
    start = next(i for i, ln in enumerate(lines) if ln.startswith("Epoch[3]"))
    return [ln for ln in lines[start:] if not ln.startswith("Epoch 3 done.")]


def _final(o):
    return dict({k: v.clone() for k, v in o["model"].state_dict().items()}, _drop_state=o["model"]._drop_state.clone())


def test_do_train_stopped_and_resumed_equals_the_uninterrupted_run(tree, tmp_path):
    from editor_amd.modeling import make_model
    # the control: the uninterrupted configuration twice, without the new keywords
    whole = []
    for tag in ("whole", "again"):
        o = _objects(tree, str(tmp_path / tag), seed=3, fill=17)
        best, lines = _train(o)
        assert sorted(os.listdir(o["cfg"].OUTPUT_DIR)) == ["EDITOR_1.pth", "EDITOR_2.pth", "EDITOR_3.pth", "EDITORbest.pth"]
        whole.append(dict(best=best, lines=lines, served=o["train"].served, final=_final(o)))
        del o
    assert [s[:2] for s in whole[0]["served"]] == [(e, TRAIN_B) for e in (0, 1, 2) for _ in range(2)]
    assert whole[0]["served"] == whole[1]["served"], "step not reproducible: the loaders served other batches in the second run"
    control = [k for k in whole[0]["final"] if not torch.equal(whole[0]["final"][k], whole[1]["final"][k])]
    assert not control, "step not reproducible: the uninterrupted run executed twice differs in %s" % control[:6]
    assert _epoch3(whole[0]["lines"]) == _epoch3(whole[1]["lines"]), "step not reproducible: the log lines differ"

    # the same run in two processes' worth of objects: pre-empted at the start of epoch 3 (MAX_EPOCHS stays 3: the schedule depends
    # on it), then other seeds, other initial values and resume='auto'
    out = str(tmp_path / "parts")
    o = _objects(tree, out, seed=3, fill=17)
    o["train"].stop_before = 2
    with pytest.raises(_Preempted):
        _train(o, save_state=True)
    assert sorted(os.listdir(out)) == ["EDITOR_1.pth", "EDITOR_2.pth", "EDITOR_state_2.pth", "EDITORbest.pth"]
    del o
    o = _objects(tree, out, seed=1000, fill=99)
    best, lines = _train(o, save_state=True, resume="auto")
    assert o["train"].served == whole[0]["served"][4:], "epoch 3's batches differ"
    assert _epoch3(lines) == _epoch3(whole[0]["lines"])
    assert not any(ln.startswith("Epoch[1]") or ln.startswith("Epoch[2]") for ln in lines)
    assert best == whole[0]["best"]
    assert sorted(os.listdir(out)) == ["EDITOR_1.pth", "EDITOR_2.pth", "EDITOR_3.pth", "EDITOR_state_3.pth", "EDITORbest.pth"]
    with contextlib.redirect_stdout(io.StringIO()):
        fresh = make_model(o["cfg"], o["c"], o["cams"])
        fresh.load_param(os.path.join(out, "EDITOR_3.pth"))
    final = _final(o)
    assert all(torch.equal(final[k].cpu(), v) for k, v in fresh.state_dict().items())
    bad = [k for k in final if not torch.equal(final[k], whole[0]["final"][k])]
    assert not bad, "the resumed run's final state differs from the uninterrupted run's in %d entries: %s" % (len(bad), bad[:6])
