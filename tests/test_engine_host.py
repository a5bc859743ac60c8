"""editor_amd.engine on the host: the log lines, the epoch schedule (checkpoints, evaluations, meter reads, best_index), the
evaluator choice, the rank gating and the order in which a TrainStep calls its collaborators - with a fake step, fake loaders,
fake evaluators and a logging handler that collects the lines.  Nothing here touches a GPU or the built library."""
import logging
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from editor_amd import config


def test_engine_imports_without_gpu_or_library():
    code = ("import editor_amd._lib as l; l.LIB_PATH = '/nonexistent/libeditor_hip.so'; import editor_amd.engine as e; "
            "assert l._LIB is None; assert callable(e.do_train) and callable(e.do_inference); "
            "assert e.TrainStep and e.DeviceMeters; print('ok')")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ---- fakes -----------------------------------------------------------------------------------------------------------------------

class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _logger():
    lg = logging.Logger("engine-test", level=logging.INFO)
    h = _Lines()
    lg.addHandler(h)
    return lg, h.lines


class _Loader:
    def __init__(self, batches, batch_size):
        self.batches, self.batch_size = batches, batch_size

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def _train_loader(n=7, b=4):
    ids = torch.zeros(b, dtype=torch.int64)
    return _Loader([({"RGB": torch.zeros(b, 1), "NI": torch.zeros(b, 1), "TI": torch.zeros(b, 1)}, ids, ids, ids, ["p"] * b)
                    for _ in range(n)], b)


def _val_loader(n=2, b=4):
    ids = torch.zeros(b, dtype=torch.int64)
    return _Loader([({"RGB": torch.zeros(b, 1), "NI": torch.zeros(b, 1), "TI": torch.zeros(b, 1)}, [1] * b, [2] * b, ids, ids,
                     ["p"] * b) for _ in range(n)], b)


class _Model:
    def __init__(self, events):
        self.events = events

    def train(self):
        self.events.append("train")

    def eval(self):
        self.events.append("eval")

    def __call__(self, img, **kw):
        assert kw["mode"] == 1 and set(kw) == {"cam_label", "view_label", "mode", "img_path"}
        self.events.append("eval_forward")
        return torch.zeros(img["RGB"].shape[0], 3)

    def state_dict(self):
        return {"w": torch.zeros(1)}


class _Scheduler:
    def __init__(self, events):
        self.events = events

    def step(self, epoch):
        self.events.append(("sched", epoch))

    def _get_lr(self, epoch):
        return [3.5e-4 * epoch, 1.0]


class _Writer:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step=None):
        self.rows.append((tag, value, step))


class _World:
    """What do_train sees through its patched module-level names."""

    def __init__(self, monkeypatch, maps, dataset="RGBNT201", dist_rank=None):
        from editor_amd import engine, metrics
        self.events, self.saved, self.evaluators = [], [], []
        world = self

        class FakeMeters:
            def __init__(self, device):
                self.iteration = 0

            def reset(self):
                world.events.append("meters.reset")
                self.iteration = 0

            def read(self):
                world.events.append(("meters.read", self.iteration))
                return {"loss_avg": 1.23456, "acc_avg": 0.5, "loss_sum": 0.0, "samples": 0.0, "acc_sum": 0.0, "steps": 0.0,
                        "last_correct": 0, "last_batch": 0}

        class FakeStep:
            num_count = None

            def __init__(self, model, loss_fn, optimizer, *, scaler=None, buckets=None, meters=None, graph=False, warmup=2):
                self.meters = meters
                world.step_kwargs = dict(scaler=scaler, buckets=buckets, graph=graph)

            def step(self, img, target, cam, view, epoch=None):
                self.meters.iteration += 1
                world.events.append(("step", epoch))

        class FakeEval:
            kind = "eval"

            def __init__(self, num_query, max_rank=20, feat_norm=True, **kw):
                self.args = (num_query, max_rank, feat_norm)
                self.updates, self.fields = [], []
                world.evaluators.append(self)

            def reset(self):
                world.events.append("evaluator.reset")
                self.updates = []

            def update(self, output):
                self.updates.append(len(output))
                self.fields.append(len(output))                  # (never reset: what the evaluator was fed over its life)

            def compute(self, *a):
                world.events.append("compute")
                m_ap = maps.pop(0)
                cmc = np.linspace(m_ap, 1.0, 50).astype(np.float32)
                return (cmc, m_ap, None, None, None, None, None)

        class FakeEvalMsvr(FakeEval):
            kind = "msvr"

        monkeypatch.setattr(engine, "DeviceMeters", FakeMeters)
        monkeypatch.setattr(engine, "TrainStep", FakeStep)
        monkeypatch.setattr(engine, "_save", lambda model, path: (world.saved.append(os.path.basename(path)),
                                                                  world.events.append(("save", os.path.basename(path)))))
        monkeypatch.setattr(metrics, "R1_mAP_eval", FakeEval)
        monkeypatch.setattr(metrics, "R1_mAP", FakeEvalMsvr)
        if dist_rank is not None:
            monkeypatch.setattr(engine, "dist", types.SimpleNamespace(
                is_available=lambda: True, is_initialized=lambda: True, get_rank=lambda: dist_rank,
                group=types.SimpleNamespace(WORLD="world")))
        self.engine = engine
        self.cfg = config.make_cfg()
        self.cfg.DATASETS.NAMES = dataset
        self.cfg.TEST.FEAT_NORM = "yes"
        s = self.cfg.SOLVER
        s.MAX_EPOCHS, s.CHECKPOINT_PERIOD, s.EVAL_PERIOD, s.LOG_PERIOD = 5, 2, 2, 3

    def train(self, tmp_path, **kw):
        self.cfg.OUTPUT_DIR = str(tmp_path / "out")
        lg, lines = _logger()
        best = self.engine.do_train(self.cfg, _Model(self.events), None, _train_loader(), _val_loader(), object(), None,
                                    _Scheduler(self.events), None, 3, 0, logger=lg, **kw)
        return best, lines


# ---- log lines ---------------------------------------------------------------------------------------------------------------------

def test_log_lines_are_the_references(monkeypatch, tmp_path):
    w = _World(monkeypatch, [0.25, 0.5])
    writer = _Writer()
    best, lines = w.train(tmp_path, writer=writer)
    assert lines[0] == "start training"
    assert "Epoch[1] Iteration[3/7] Loss: 1.235, Acc: 0.500, Base Lr: 3.50e-04" in lines
    assert "Epoch[2] Iteration[6/7] Loss: 1.235, Acc: 0.500, Base Lr: 7.00e-04" in lines
    done = [ln for ln in lines if ln.startswith("Epoch 3 done.")]
    assert len(done) == 1
    import re
    assert re.fullmatch(r"Epoch 3 done\. Time per batch: \d+\.\d{3}\[s\] Speed: \d+\.\d\[samples/s\]", done[0])
    i = lines.index("Validation Results - Epoch: 2")
    cmc = np.linspace(0.25, 1.0, 50).astype(np.float32)
    assert lines[i + 1:i + 9] == [
        "mAP: 25.00%",
        "CMC curve, Rank-1  :25.00%",
        "CMC curve, Rank-5  :{:.2%}".format(cmc[4]),
        "CMC curve, Rank-10 :{:.2%}".format(cmc[9]),
        "Best Multi-Modal mAP: 25.00%",
        "Best Multi-Modal Rank-1: 25.00%",
        "Best Multi-Modal Rank-5: {:.2%}".format(cmc[4]),
        "Best Multi-Modal Rank-10: {:.2%}".format(cmc[9]),
    ]
    assert "CMC curve, Rank-5  :31.12%" == lines[i + 3] and "CMC curve, Rank-10 :38.78%" == lines[i + 4]
    # the writer: Loss at the log points only (the documented difference), MM/* as the reference writes them
    assert [r for r in writer.rows if r[0] == "Loss"] == [("Loss", 1.23456, e) for e in (1, 2, 3, 4, 5) for _ in range(2)]
    assert [r for r in writer.rows if r[0].startswith("MM/")] == [("MM/mAP", 0.25, 2), ("MM/Rank-1", 0.25, 2),
                                                                  ("MM/mAP", 0.5, 4), ("MM/Rank-1", 0.5, 4)]
    assert best["mAP"] == 0.5


def test_do_inference_lines_and_result(monkeypatch):
    w = _World(monkeypatch, [0.75])
    lg, lines = _logger()
    cmc, m_ap = w.engine.do_inference(w.cfg, _Model(w.events), _val_loader(), 3, logger=lg)
    want = np.linspace(0.75, 1.0, 50).astype(np.float32)
    assert m_ap == 0.75 and np.array_equal(cmc, want)
    assert lines == ["Enter inferencing", "Validation Results ", "mAP: 75.00%", "CMC curve, Rank-1  :75.00%",
                     "CMC curve, Rank-5  :{:.2%}".format(want[4]), "CMC curve, Rank-10 :{:.2%}".format(want[9])]
    assert w.events.count("eval_forward") == 2 and w.evaluators[0].updates == [3, 3]


# ---- schedule ----------------------------------------------------------------------------------------------------------------------

def test_epoch_schedule(monkeypatch, tmp_path):
    w = _World(monkeypatch, [0.4, 0.4])
    best, lines = w.train(tmp_path)
    ev = w.events
    # every epoch: meters and evaluator reset, scheduler.step(epoch), model.train(), seven steps
    for epoch in range(1, 6):
        i = ev.index(("sched", epoch))
        assert ev[i - 2:i] == ["meters.reset", "evaluator.reset"] and ev[i + 1] == "train"
        assert ev.count(("step", epoch)) == 7
    # meters.read() at iterations 3 and 6 of every epoch and nowhere else
    assert [e[1] for e in ev if isinstance(e, tuple) and e[0] == "meters.read"] == [3, 6] * 5
    # checkpoints at epochs 2 and 4, evaluations at 2 and 4; an EQUAL mAP still overwrites best.pth (the reference's >=)
    assert w.saved == ["EDITOR_2.pth", "EDITORbest.pth", "EDITOR_4.pth", "EDITORbest.pth"]
    assert ev.count("compute") == 2
    assert [ln for ln in lines if ln.startswith("Validation Results")] == ["Validation Results - Epoch: 2",
                                                                          "Validation Results - Epoch: 4"]
    assert best == {"mAP": 0.4, "Rank-1": np.float32(0.4), "Rank-5": np.linspace(0.4, 1.0, 50).astype(np.float32)[4],
                    "Rank-10": np.linspace(0.4, 1.0, 50).astype(np.float32)[9]}
    # order inside an evaluating epoch: the checkpoint, then eval mode, the forwards, compute, best.pth
    i = ev.index(("save", "EDITOR_2.pth"))
    assert ev[i + 1:i + 6] == ["eval", "eval_forward", "eval_forward", "compute", ("save", "EDITORbest.pth")]


def test_lower_map_keeps_best(monkeypatch, tmp_path):
    w = _World(monkeypatch, [0.6, 0.3])
    best, lines = w.train(tmp_path)
    assert w.saved == ["EDITOR_2.pth", "EDITORbest.pth", "EDITOR_4.pth"]
    assert best["mAP"] == 0.6
    assert [ln for ln in lines if ln.startswith("Best Multi-Modal mAP")] == ["Best Multi-Modal mAP: 60.00%"] * 2


@pytest.mark.parametrize("dataset,kind,fields", [("RGBNT201", "eval", 3), ("RGBNT100", "eval", 3), ("MSVR310", "msvr", 5)])
def test_evaluator_follows_dataset_name(monkeypatch, tmp_path, dataset, kind, fields):
    w = _World(monkeypatch, [0.1, 0.2, 0.3], dataset=dataset)
    w.train(tmp_path)
    lg, _ = _logger()
    w.engine.do_inference(w.cfg, _Model(w.events), _val_loader(), 3, logger=lg)
    assert [e.kind for e in w.evaluators] == [kind, kind]
    for e in w.evaluators:
        assert e.args == (3, 50, "yes") and e.fields and set(e.fields) == {fields}


def test_rank_one_neither_evaluates_nor_writes(monkeypatch, tmp_path):
    w = _World(monkeypatch, [0.9, 0.9], dist_rank=1)
    w.cfg.MODEL.DIST_TRAIN = True
    best, lines = w.train(tmp_path)
    assert w.saved == [] and "compute" not in w.events and "eval_forward" not in w.events
    assert not os.path.exists(w.cfg.OUTPUT_DIR)
    assert not any(ln.startswith("Validation") or ln.startswith("Best") for ln in lines)
    assert sum(ln.startswith("Epoch[") for ln in lines) == 10              # (it still trains and logs)
    assert best == {"mAP": 0, "Rank-1": 0, "Rank-5": 0, "Rank-10": 0}
    lg, inf_lines = _logger()
    assert w.engine.do_inference(w.cfg, _Model(w.events), _val_loader(), 3, logger=lg) == (None, None)
    assert inf_lines == ["Enter inferencing"] and "eval_forward" not in w.events


def test_rank_zero_of_a_group_does_both(monkeypatch, tmp_path):
    w = _World(monkeypatch, [0.9, 0.9], dist_rank=0)
    w.cfg.MODEL.DIST_TRAIN = True
    w.train(tmp_path)
    assert w.saved == ["EDITOR_2.pth", "EDITORbest.pth", "EDITOR_4.pth", "EDITORbest.pth"]


def test_grad_buckets_enabled_once_and_handed_to_the_step(monkeypatch, tmp_path):
    w = _World(monkeypatch, [0.1, 0.2], dist_rank=0)
    calls = []

    class Bucketed(_Model):
        grad_buckets = None

        def enable_grad_buckets(self, process_group=None):
            calls.append(process_group)
            self.grad_buckets = "buckets"
            return self.grad_buckets

    w.cfg.OUTPUT_DIR = str(tmp_path / "out")
    lg, _ = _logger()
    w.engine.do_train(w.cfg, Bucketed(w.events), None, _train_loader(), _val_loader(), object(), None, _Scheduler(w.events), None,
                      3, 0, logger=lg, scaler="scaler", graph=True)
    assert calls == ["world"]
    assert w.step_kwargs == dict(scaler="scaler", buckets="buckets", graph=True)


# ---- TrainStep's order of calls ------------------------------------------------------------------------------------------------------

class _Recorder:
    def __init__(self):
        self.calls = []


def _fake_step_parts(rec):
    class Model:
        def __call__(self, img, label=None, cam_label=None, view_label=None, img_path=None, writer=None, epoch=None):
            rec.calls.append("model")
            assert img_path is None and epoch == 7
            writer.add_scalar("num_count", torch.tensor(4.0), epoch)
            score = img["RGB"] * 1.0
            score.register_hook(lambda g: rec.calls.append("backward"))
            return [score, score + 1.0]

    def loss_fn(score=None, feat=None, target=None, target_cam=None):
        rec.calls.append("loss_fn")
        return (score * feat).sum()

    class Optimizer:
        def zero_grad(self, set_to_none=False):
            rec.calls.append("zero_grad(set_to_none=%s)" % set_to_none)

        def step(self):
            rec.calls.append("optimizer.step")

    class Scaler:
        def scale(self, loss):
            rec.calls.append("scaler.scale")
            return loss * 2.0

        def step(self, optimizer):
            rec.calls.append("scaler.step")

        def update(self):
            rec.calls.append("scaler.update")

    class Buckets:
        def finish(self):
            rec.calls.append("buckets.finish")

    class Meters:
        def update(self, score, target, loss):
            rec.calls.append("meters.update")
            rec.meter_args = (score, target, loss)

    return Model(), loss_fn, Optimizer(), Scaler(), Buckets(), Meters()


def _batch():
    img = {k: torch.ones(2, 3, requires_grad=True) for k in ("RGB", "NI", "TI")}
    ids = torch.zeros(2, dtype=torch.int64)
    return img, ids, ids, ids


def test_train_step_order_plain():
    from editor_amd.engine import TrainStep
    rec = _Recorder()
    model, loss_fn, opt, _, buckets, meters = _fake_step_parts(rec)
    ts = TrainStep(model, loss_fn, opt, buckets=buckets, meters=meters)
    assert ts.graph is False and ts.captured is False and ts.num_count is None
    img, target, cam, view = _batch()
    loss = ts.step(img, target, cam, view, epoch=7)
    assert rec.calls == ["zero_grad(set_to_none=True)", "model", "loss_fn", "backward", "buckets.finish", "optimizer.step",
                         "meters.update"]
    assert float(loss.detach()) == 12.0 and float(ts.num_count) == 4.0
    assert rec.meter_args[1] is target and rec.meter_args[2] is loss and rec.meter_args[0].shape == (2, 3)
    assert ts.captured is False


def test_train_step_order_with_scaler_and_bare():
    from editor_amd.engine import TrainStep
    rec = _Recorder()
    model, loss_fn, opt, scaler, buckets, meters = _fake_step_parts(rec)
    TrainStep(model, loss_fn, opt, scaler=scaler, buckets=buckets, meters=meters).step(*_batch(), epoch=7)
    assert rec.calls == ["zero_grad(set_to_none=True)", "model", "loss_fn", "scaler.scale", "backward", "buckets.finish",
                         "scaler.step", "scaler.update", "meters.update"]
    rec.calls.clear()
    TrainStep(model, loss_fn, opt).step(*_batch(), epoch=7)
    assert rec.calls == ["zero_grad(set_to_none=True)", "model", "loss_fn", "backward", "optimizer.step"]


def test_train_step_refuses_a_capture_without_warmup():
    from editor_amd.engine import TrainStep
    with pytest.raises(ValueError):
        TrainStep(None, None, None, graph=True, warmup=0)
