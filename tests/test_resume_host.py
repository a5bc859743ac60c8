"""Full-state checkpoints on the host: the file's schema and format check, the atomic write, what resume='auto' picks, the
restoration of the global generators the identity samplers draw from and of the loaders' epoch, and do_train's schedule of state
files - with stand-ins (tests/resume_helpers.py) wherever a device would be needed.  Nothing here touches a GPU."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import resume_helpers as R
from conftest import ROOT


def test_engine_with_checkpoints_imports_without_gpu_or_library():
    code = ("import editor_amd._lib as l; l.LIB_PATH = '/nonexistent/libeditor_hip.so'; import editor_amd.engine as e; "
            "assert l._LIB is None; assert callable(e.save_checkpoint) and callable(e.load_checkpoint); "
            "assert callable(e.latest_state_file) and e.CHECKPOINT_FORMAT == 1; "
            "assert hasattr(e.TrainStep, 'state_dict') and hasattr(e.TrainStep, 'load_state_dict'); print('ok')")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_header_declares_the_cast_entry_point():
    from editor_amd import _lib
    import ctypes
    protos = _lib.parse_header()
    assert protos["editor_cast_multi"] == [ctypes.c_void_p] * 5 + [ctypes.c_long, ctypes.c_int, ctypes.c_void_p]


# ---- the file ---------------------------------------------------------------------------------------------------------------------

def test_checkpoint_schema_and_round_trip(tmp_path):
    from editor_amd.engine import load_checkpoint, save_checkpoint
    path = str(tmp_path / "EDITOR_state_4.pth")
    step, sched = R.FakeStep(2.5), R.FakeScheduler()
    step.steps, sched.tag = 9, "epoch-4"
    loaders = (R.EpochLoader(epoch=4), R.PlainLoader(), R.EpochLoader(epoch=2))
    save_checkpoint(path, step, epoch=4, scheduler=sched, loaders=loaders,
                    best_index={"mAP": np.float64(0.5), "Rank-1": np.float32(0.25), "Rank-5": 1, "Rank-10": 1.0}, extra={"note": "x"})
    assert sorted(os.listdir(tmp_path)) == ["EDITOR_state_4.pth"]                      # (no temporary file left)
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert set(raw) == set(R.STATE_KEYS) | {"extra"}
    assert raw["format"] == 1 and raw["epoch"] == 4 and raw["compute_dtype"] == "bf16" and raw["scheduler"] == {"tag": "epoch-4"}
    assert raw["loader_epochs"] == [4, None, 2]
    assert raw["best_index"] == {"mAP": 0.5, "Rank-1": 0.25, "Rank-5": 1.0, "Rank-10": 1.0}
    assert all(type(v) is float for v in raw["best_index"].values())
    assert set(raw["rng"]) == {"python", "numpy", "torch"} and raw["rng"]["torch"].dtype == torch.uint8
    assert torch.equal(raw["step"]["model"]["w"], torch.full((3,), 2.5)) and raw["step"]["steps"] == 9
    assert all(not t.is_cuda for t in raw["step"]["model"].values())

    step2, sched2 = R.FakeStep(), R.FakeScheduler()
    loaders2 = (R.EpochLoader(), R.PlainLoader(), R.EpochLoader())
    got = load_checkpoint(path, step2, scheduler=sched2, loaders=loaders2)
    assert got["epoch"] == 4 and got["extra"] == {"note": "x"} and got["best_index"]["mAP"] == 0.5
    assert torch.equal(step2.w, step.w) and step2.steps == 9 and sched2.tag == "epoch-4"
    assert (loaders2[0].epoch, loaders2[2].epoch) == (4, 2) and not hasattr(loaders2[1], "epoch")


def test_minimal_checkpoint_has_exactly_the_documented_keys(tmp_path):
    from editor_amd.engine import save_checkpoint
    path = str(tmp_path / "s.pth")
    save_checkpoint(path, R.FakeStep(), epoch=1)
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert set(raw) == set(R.STATE_KEYS)
    assert raw["scheduler"] is None and raw["loader_epochs"] == [] and raw["best_index"] is None


@pytest.mark.parametrize("fmt", [0, 2, "1", None])
def test_unknown_format_is_refused_before_anything_is_restored(tmp_path, fmt):
    from editor_amd.engine import load_checkpoint, save_checkpoint
    path = str(tmp_path / "s.pth")
    save_checkpoint(path, R.FakeStep(1.0), epoch=1)
    raw = torch.load(path, map_location="cpu", weights_only=False)
    if fmt is None:
        del raw["format"]
    else:
        raw["format"] = fmt
    torch.save(raw, path)
    step, loader = R.FakeStep(7.0), R.EpochLoader(epoch=5)
    before = random.getstate()
    with pytest.raises(ValueError, match="format"):
        load_checkpoint(path, step, loaders=(loader,))
    assert step.loaded == [] and loader.epoch == 5 and random.getstate() == before
    torch.save({"w": torch.zeros(1)}, path)                                           # a reference-format model file
    with pytest.raises(ValueError, match="format"):
        load_checkpoint(path, step)


def test_a_refusing_step_leaves_generators_and_loaders_alone(tmp_path):
    from editor_amd.engine import load_checkpoint, save_checkpoint
    path = str(tmp_path / "s.pth")
    save_checkpoint(path, R.FakeStep(), epoch=3, loaders=(R.EpochLoader(epoch=3),))

    class Refusing(R.FakeStep):
        def load_state_dict(self, sd):
            raise ValueError("'model.w': shape")

    random.seed(99)
    before, loader = random.getstate(), R.EpochLoader(epoch=0)
    with pytest.raises(ValueError, match="model.w"):
        load_checkpoint(path, Refusing(), loaders=(loader,))
    assert random.getstate() == before and loader.epoch == 0


def test_atomic_write_leaves_the_old_file_or_the_new_one(tmp_path, monkeypatch):
    from editor_amd import engine
    path = str(tmp_path / "EDITOR_state_2.pth")
    engine.save_checkpoint(path, R.FakeStep(1.0), epoch=1)
    old = open(path, "rb").read()
    real_save = torch.save

    def half_way(obj, f, *a, **k):
        with open(f, "wb") as out:                   # (the name save_checkpoint handed over: half a file appears under it)
            out.write(b"half a checkpoint")
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", half_way)
    with pytest.raises(OSError, match="disk full"):
        engine.save_checkpoint(path, R.FakeStep(2.0), epoch=2)
    assert open(path, "rb").read() == old                                              # the old file, whole
    assert sorted(os.listdir(tmp_path)) == ["EDITOR_state_2.pth"]                      # and no debris beside it
    fresh = str(tmp_path / "EDITOR_state_3.pth")
    with pytest.raises(OSError):
        engine.save_checkpoint(fresh, R.FakeStep(2.0), epoch=3)
    assert not os.path.exists(fresh)                                                   # no old file: then none, not half of one
    monkeypatch.setattr(torch, "save", real_save)
    engine.save_checkpoint(path, R.FakeStep(2.0), epoch=2)
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert raw["epoch"] == 2 and torch.equal(raw["step"]["model"]["w"], torch.full((3,), 2.0))
    assert sorted(os.listdir(tmp_path)) == ["EDITOR_state_2.pth"]


def test_auto_picks_the_highest_numbered_state_file(tmp_path):
    from editor_amd.engine import latest_state_file
    assert latest_state_file(str(tmp_path), "EDITOR") is None
    assert latest_state_file(str(tmp_path / "missing"), "EDITOR") is None
    for name in ("EDITOR_state_9.pth", "EDITOR_state_12.pth", "EDITOR_12.pth", "EDITOR_40.pth", "EDITORbest.pth",
                 "OTHER_state_99.pth", "EDITOR_state_30.pth.tmp.1", "EDITOR_state_x.pth"):
        (tmp_path / name).write_bytes(b"")
    assert latest_state_file(str(tmp_path), "EDITOR") == str(tmp_path / "EDITOR_state_12.pth")      # 12 > 9 as numbers
    assert latest_state_file(str(tmp_path), "OTHER") == str(tmp_path / "OTHER_state_99.pth")


# ---- generators and loaders ---------------------------------------------------------------------------------------------------------

def _source():
    return [("img%03d.jpg" % i, pid, i % 3, 0) for i, pid in enumerate([p for p in (3, 8, 1, 20, 15, 4) for _ in range(5 + p % 3)])]


def _samplers():
    from editor_amd.data import RandomIdentitySampler, RandomIdentitySampler_DDP
    src = _source()
    return (RandomIdentitySampler(src, 8, 4), RandomIdentitySampler(src, 8, 6),          # (6 instances: numpy's with-replacement fill)
            RandomIdentitySampler_DDP(src, 8, 4, rank=0, world_size=1), RandomIdentitySampler_DDP(src, 16, 4, rank=1, world_size=2, seed=None))


def _epoch_lists(samplers):
    return [list(s) for s in samplers], float(torch.rand(1))


def test_samplers_continue_as_in_an_uninterrupted_process(tmp_path):
    """Process A draws epochs 1, 2, (checkpoint), 3.  Process B - other seeds, generators disturbed by its own start-up - loads
    the checkpoint and draws epoch 3: the identity samplers (global `random` and `numpy.random`, both the plain and the DDP one)
    yield the same index lists, and torch's CPU generator continues as well."""
    from editor_amd.engine import load_checkpoint, save_checkpoint
    path = str(tmp_path / "s.pth")
    random.seed(5); np.random.seed(6); torch.manual_seed(7)
    samplers = _samplers()
    _epoch_lists(samplers)
    second = _epoch_lists(samplers)
    save_checkpoint(path, R.FakeStep(), epoch=2)
    want = _epoch_lists(samplers)
    assert want[0] != second[0]                                                        # (the epochs do differ)

    random.seed(1234); np.random.seed(4321); torch.manual_seed(1)
    samplers = _samplers()
    _epoch_lists(samplers)                                                             # start-up noise
    load_checkpoint(path, R.FakeStep())
    got = _epoch_lists(samplers)
    assert got[0] == want[0], "sampler index lists differ after the resume"
    assert got[1] == want[1], "torch's CPU generator was not restored"


def test_loader_epoch_is_restored_and_continues(tmp_path):
    from editor_amd.engine import load_checkpoint, save_checkpoint
    path = str(tmp_path / "s.pth")
    a = R.EpochLoader()
    for _ in range(2):
        list(a)
    save_checkpoint(path, R.FakeStep(), epoch=2, loaders=(a, R.PlainLoader()))
    list(a)
    b = R.EpochLoader()
    load_checkpoint(path, R.FakeStep(), loaders=(b, R.PlainLoader()))
    assert b.epoch == 2
    list(b)
    assert b.served == a.served[-3:] == [(2, 0), (2, 1), (2, 2)]


# ---- do_train's schedule --------------------------------------------------------------------------------------------------------------

def test_do_train_without_the_keywords_writes_todays_files(monkeypatch, tmp_path):
    w = R.World(monkeypatch, [0.3, 0.4], tmp_path / "out")
    w.train(R.EpochLoader(), R.FakeScheduler())
    assert w.listing() == ["EDITOR_2.pth", "EDITOR_4.pth", "EDITORbest.pth"]


def test_do_train_state_files_and_resume(monkeypatch, tmp_path):
    """CHECKPOINT_PERIOD 2, five epochs: state files at epochs 2 and 4, one at a time, beside the reference-format files.  A run
    stopped after epoch 3 and resumed with 'auto' continues at epoch 3 (its latest state is epoch 2's) with the scheduler, loader
    epoch, step state and best_index of that moment, and ends where the uninterrupted run ends."""
    w = R.World(monkeypatch, [0.3, 0.4], tmp_path / "whole")
    whole_loader, whole_sched = R.EpochLoader(), R.FakeScheduler()
    best_whole, _ = w.train(whole_loader, whole_sched, save_state=True)
    assert w.listing() == ["EDITOR_2.pth", "EDITOR_4.pth", "EDITOR_state_4.pth", "EDITORbest.pth"]
    assert whole_sched.stepped == [1, 2, 3, 4, 5] and w.steps[-1].steps == 15

    w2 = R.World(monkeypatch, [0.3], tmp_path / "parts")
    w2.cfg.SOLVER.MAX_EPOCHS = 3
    first_sched = R.FakeScheduler()
    first_sched.tag = "first process"
    best_first, _ = w2.train(R.EpochLoader(), first_sched, save_state=True, resume="auto")       # nothing to resume: a fresh start
    assert first_sched.stepped == [1, 2, 3] and w2.steps[-1].loaded == []
    assert w2.listing() == ["EDITOR_2.pth", "EDITOR_state_2.pth", "EDITORbest.pth"]

    w3 = R.World(monkeypatch, [0.4], tmp_path / "parts")
    loader, sched = R.EpochLoader(), R.FakeScheduler()
    best, lines = w3.train(loader, sched, save_state=True, resume="auto")
    step = w3.steps[-1]
    assert len(step.loaded) == 1 and sched.tag == "first process"
    assert sched.stepped == [3, 4, 5]                                                  # scheduler.step(epoch) as in the whole run
    assert loader.served[0] == (2, 0) and loader.epoch == 5                            # the loader's third epoch comes first
    assert step.steps == 15 and torch.equal(step.w, w.steps[0].w)
    assert best == best_whole and best["mAP"] == 0.4
    assert w3.listing() == ["EDITOR_2.pth", "EDITOR_4.pth", "EDITOR_state_4.pth", "EDITORbest.pth"]
    assert any(ln.startswith("resumed from ") and ln.endswith("(epoch 2)") for ln in lines)

    # an explicit path, and a finished run: nothing left to do, best_index is the file's
    w4 = R.World(monkeypatch, [], tmp_path / "elsewhere")
    w4.cfg.SOLVER.MAX_EPOCHS = 4
    best4, _ = w4.train(R.EpochLoader(), R.FakeScheduler(), resume=os.path.join(w3.cfg.OUTPUT_DIR, "EDITOR_state_4.pth"))
    assert best4["mAP"] == 0.4 and w4.steps[-1].steps == 12 and not os.path.exists(w4.cfg.OUTPUT_DIR)
    assert os.path.exists(os.path.join(w3.cfg.OUTPUT_DIR, "EDITOR_state_4.pth"))       # (another directory's file is not removed)


def test_non_main_rank_loads_but_does_not_write(monkeypatch, tmp_path):
    import types
    w = R.World(monkeypatch, [0.3, 0.4], tmp_path / "out")
    w.train(R.EpochLoader(), R.FakeScheduler(), save_state=True)
    before = w.listing()
    w2 = R.World(monkeypatch, [], tmp_path / "out")
    monkeypatch.setattr(w2.engine, "dist", types.SimpleNamespace(is_available=lambda: True, is_initialized=lambda: True,
                                                                 get_rank=lambda: 1, group=types.SimpleNamespace(WORLD="world")))
    w2.cfg.MODEL.DIST_TRAIN = True
    w2.cfg.SOLVER.MAX_EPOCHS = 6
    sched = R.FakeScheduler()
    w2.train(R.EpochLoader(), sched, save_state=True, resume="auto")
    assert sched.stepped == [5, 6] and len(w2.steps[-1].loaded) == 1 and w2.listing() == before
