"""What tests/test_resume_host.py and tests/test_gpu_resume.py share: stand-ins for the step, the loaders and the evaluator where a
device would be needed, the special fp32 values planted for the operand-refresh kernel, and bit-level comparisons."""
import hashlib
import logging
import os

import numpy as np
import torch

STATE_KEYS = ("format", "epoch", "step", "scheduler", "loader_epochs", "best_index", "rng", "compute_dtype")


class Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def logger():
    lg = logging.Logger("resume-test", level=logging.INFO)
    h = Lines()
    lg.addHandler(h)
    return lg, h.lines


# ---- host fakes ---------------------------------------------------------------------------------------------------------------------

class FakeStep:
    """A step whose whole state is one tensor and a counter."""
    num_count = None

    def __init__(self, value=0.0):
        self.w = torch.full((3,), float(value))
        self.steps = 0
        self.loaded = []

    def step(self, img, target, cam, view, epoch=None):
        self.w += 1.0
        self.steps += 1

    def state_dict(self, device=False):
        return {"model": {"w": self.w.clone()}, "steps": self.steps, "compute_dtype": "bf16"}

    def load_state_dict(self, sd):
        self.loaded.append(sd)
        self.w.copy_(sd["model"]["w"])
        self.steps = sd["steps"]


class EpochLoader:
    """A loader with the `epoch` attribute of editor_amd.loader.DeviceBatchLoader: iter() starts one epoch and advances it."""

    def __init__(self, n=3, b=4, epoch=0):
        self.n, self.batch_size, self.epoch, self.served = n, b, epoch, []

    def __len__(self):
        return self.n

    def __iter__(self):
        epoch = self.epoch
        self.epoch += 1
        ids = torch.zeros(self.batch_size, dtype=torch.int64)
        for i in range(self.n):
            self.served.append((epoch, i))
            yield {k: torch.zeros(self.batch_size, 1) for k in ("RGB", "NI", "TI")}, ids, ids, ids, ["p"] * self.batch_size


class PlainLoader:
    """No `epoch` attribute: skipped by save_checkpoint / load_checkpoint."""
    batch_size = 4

    def __len__(self):
        return 1

    def __iter__(self):
        ids = torch.zeros(4, dtype=torch.int64)
        yield {k: torch.zeros(4, 1) for k in ("RGB", "NI", "TI")}, [1] * 4, [2] * 4, ids, ids, ["p"] * 4


class FakeScheduler:
    def __init__(self):
        self.stepped, self.tag = [], "fresh"

    def step(self, epoch):
        self.stepped.append(epoch)

    def _get_lr(self, epoch):
        return [1e-3 * epoch]

    def state_dict(self):
        return {"tag": self.tag}

    def load_state_dict(self, sd):
        self.tag = sd["tag"]


class FakeModel:
    def train(self):
        pass

    def eval(self):
        pass

    def __call__(self, img, **kw):
        return torch.zeros(img["RGB"].shape[0], 3)

    def state_dict(self):
        return {"w": torch.zeros(1)}


class World:
    """do_train with everything that needs a device replaced: `steps` collects the FakeStep of every do_train call, `maps` feeds
    the evaluator's results."""

    def __init__(self, monkeypatch, maps, out_dir):
        from editor_amd import config, engine, metrics
        self.steps, self.engine = [], engine
        world = self

        class Meters:
            def __init__(self, device):
                pass

            def reset(self):
                pass

            def read(self):
                return {"loss_avg": 1.0, "acc_avg": 0.5}

        class Eval:
            def __init__(self, num_query, max_rank=20, feat_norm=True, **kw):
                pass

            def reset(self):
                pass

            def update(self, output):
                pass

            def compute(self, *a):
                m_ap = maps.pop(0)
                return (np.linspace(m_ap, 1.0, 50).astype(np.float32), m_ap)

        def make_step(model, loss_fn, optimizer, **kw):
            world.steps.append(FakeStep())
            return world.steps[-1]

        monkeypatch.setattr(engine, "DeviceMeters", Meters)
        monkeypatch.setattr(engine, "TrainStep", make_step)
        monkeypatch.setattr(metrics, "R1_mAP_eval", Eval)
        self.cfg = config.make_cfg()
        self.cfg.DATASETS.NAMES, self.cfg.TEST.FEAT_NORM, self.cfg.OUTPUT_DIR = "RGBNT201", "yes", str(out_dir)
        s = self.cfg.SOLVER
        s.MAX_EPOCHS, s.CHECKPOINT_PERIOD, s.EVAL_PERIOD, s.LOG_PERIOD = 5, 2, 2, 100

    def train(self, train_loader, scheduler, **kw):
        lg, lines = logger()
        best = self.engine.do_train(self.cfg, FakeModel(), None, train_loader, PlainLoader(), object(), None, scheduler, None, 3, 0,
                                    logger=lg, **kw)
        return best, lines

    def listing(self):
        return sorted(os.listdir(self.cfg.OUTPUT_DIR))


# ---- values for the operand refresh -------------------------------------------------------------------------------------------------

def special_values(shadow_dtype):
    """fp32 values at which a float -> 16-bit conversion can go wrong: signed zeros, fp32 denormals, exact round-to-nearest-even
    ties of the target format (between neighbours whose lower one is even and odd, both signs), the largest finite fp32, 65504
    (the largest half) and the next fp32 above it, infinities and NaN."""
    drop = 16 if shadow_dtype == torch.bfloat16 else 13                  # fp32 mantissa bits the target format does not keep
    base = np.array([0x3F800000, 0x3F800000 + (1 << drop), 0x40490000, 0x3DCC0000 + (1 << drop)], dtype=np.uint32)
    ties = base | np.uint32(1 << (drop - 1))                             # exactly half way to the next value of the target format
    ties = np.concatenate([ties, ties | np.uint32(0x80000000), ties + np.uint32(1), ties - np.uint32(1)])
    fixed = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F7FFFFF, 0xFF7FFFFF,
                      0x477FE000, 0x477FE001, 0xC77FE000, 0x477FEFFF, 0x477FF000,          # 65504, next above, -65504, around 65520
                      0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001], dtype=np.uint32)
    return torch.from_numpy(np.concatenate([fixed, ties]).view(np.float32).copy())


def plant(t, values, seed):
    """Write `values` into the flat view of t: at its head, its tail and scattered positions (as many as fit)."""
    flat = t.view(-1)
    n, k = flat.numel(), values.numel()
    g = torch.Generator().manual_seed(seed)
    if n >= 3 * k:
        flat[:k] = values.to(flat.device)
        flat[n - k:] = values.flip(0).to(flat.device)
        pos = (torch.randperm(n - 2 * k, generator=g)[:k] + k).to(flat.device)
        flat[pos] = values.to(flat.device)
    else:
        pick = torch.randperm(k, generator=g)[:n]
        flat.copy_(values[pick].to(flat.device))


def same_bits(a, b):
    """Bit equality of two tensors of one dtype, NaN positions compared as positions."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        na, nb = torch.isnan(a), torch.isnan(b)
        if not torch.equal(na, nb):
            return False
        ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return torch.equal(a.masked_fill(na, 0).contiguous().view(ints), b.masked_fill(nb, 0).contiguous().view(ints))
    return torch.equal(a, b)


def batch_hash(batch):
    """One hash over everything a train loader's batch holds (image tensors by modality, the id tensors, the paths)."""
    h = hashlib.sha256()
    img = batch[0]
    for k in sorted(img):
        h.update(k.encode())
        h.update(img[k].detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    for t in batch[1:]:
        if isinstance(t, torch.Tensor):
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        else:
            h.update(repr(list(t)).encode())
    return h.hexdigest()
