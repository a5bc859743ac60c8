"""Loss-head options, the part that needs no GPU: which terms make_loss assembles for a cfg (the kernels' wrappers replaced by
recorders), its errors, TripletLoss's batch limits, the header's new entries and the conditions recorded in the golden file."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loss_options_helpers as H
from conftest import load_golden


def _cfg(**kw):
    model = {k: v for k, v in kw.items() if k in ("METRIC_LOSS_TYPE", "NO_MARGIN", "IF_LABELSMOOTH", "ID_LOSS_WEIGHT", "TRIPLET_LOSS_WEIGHT")}
    cfg = SimpleNamespace(MODEL=SimpleNamespace(**model), DATALOADER=SimpleNamespace(), SOLVER=SimpleNamespace())
    if "SAMPLER" in kw:
        cfg.DATALOADER.SAMPLER = kw["SAMPLER"]
    if "MARGIN" in kw:
        cfg.SOLVER.MARGIN = kw["MARGIN"]
    return cfg


@pytest.fixture
def recorded(monkeypatch):
    """Replace the four loss terms by recorders returning distinct constants -> the list of calls."""
    from editor_amd import losses
    calls = []

    def ce_smooth(logits, target, eps=0.1):
        calls.append(("ce_smooth", eps, tuple(target.tolist())))
        return torch.tensor(2.0)

    def soft(feat, labels):
        calls.append(("soft", None, tuple(labels.tolist())))
        return torch.tensor(3.0)

    class Margin:
        def __init__(self, margin=None, hard_factor=0.0):
            self.margin = margin

        def __call__(self, feat, labels, normalize_feature=False):
            calls.append(("margin", self.margin, tuple(labels.tolist())))
            return torch.tensor(5.0), None, None

    monkeypatch.setattr(losses, "cross_entropy_label_smooth", ce_smooth)
    monkeypatch.setattr(losses, "triplet_soft_margin", soft)
    monkeypatch.setattr(losses, "TripletLoss", Margin)
    return calls


S, F, T = torch.zeros(4, 5), torch.zeros(4, 8), torch.tensor([0, 0, 1, 1])


def test_defaults_for_none_and_absent_keys(recorded):
    from editor_amd import losses
    for cfg in (None, _cfg(), SimpleNamespace()):
        del recorded[:]
        fn, center = losses.make_loss(cfg, 7)
        assert isinstance(center, losses.CenterLoss) and center.centers.shape == (7, 2048)
        assert fn(S, F, T, None).item() == 5.0                          # 2 + 3, neither weight multiplied in
        assert [c[:2] for c in recorded] == [("ce_smooth", 0.1), ("soft", None)]
    del recorded[:]
    assert losses.loss_pairs((S, F, S, F, torch.tensor(0.5)), T).item() == 10.5
    assert [c[0] for c in recorded] == ["ce_smooth", "soft"] * 2


def test_cfg_selects_the_terms(recorded):
    from editor_amd import losses
    fn, _ = losses.make_loss(_cfg(NO_MARGIN=False), 7)                  # SOLVER.MARGIN absent: 0.3
    assert fn(S, F, T).item() == 7.0 and [c[:2] for c in recorded] == [("ce_smooth", 0.1), ("margin", 0.3)]
    del recorded[:]
    fn, _ = losses.make_loss(_cfg(NO_MARGIN=False, MARGIN=0.5, IF_LABELSMOOTH="off", ID_LOSS_WEIGHT=0.5, TRIPLET_LOSS_WEIGHT=2.0), 7)
    assert fn(S, F, T).item() == 11.0 and [c[:2] for c in recorded] == [("ce_smooth", 0.0), ("margin", 0.5)]
    del recorded[:]
    fn, _ = losses.make_loss(_cfg(SAMPLER="softmax", METRIC_LOSS_TYPE="anything"), 7)   # make_loss.py:31-33: plain cross-entropy alone
    assert fn(S, F, T, None).item() == 2.0 and [c[:2] for c in recorded] == [("ce_smooth", 0.0)]
    del recorded[:]
    # lists: 0.5 * mean(tail) + 0.5 * head; a short target is repeated to the features' batch
    fn, _ = losses.make_loss(_cfg(), 7)
    short = torch.tensor([0, 1])
    assert fn([S, S, S], [F, F], short).item() == 5.0
    assert [c[0] for c in recorded] == ["ce_smooth"] * 3 + ["soft"] * 2 and all(c[2] == (0, 1, 0, 1) for c in recorded)


@pytest.mark.parametrize("kw,key", [({"SAMPLER": "softmax_triplet_center"}, "SAMPLER"), ({"SAMPLER": "triplet"}, "SAMPLER"),
                                    ({"METRIC_LOSS_TYPE": "center"}, "METRIC_LOSS_TYPE"),
                                    ({"METRIC_LOSS_TYPE": "triplet_center"}, "METRIC_LOSS_TYPE")])
def test_unserved_cfg_raises(kw, key):
    from editor_amd import losses
    with pytest.raises(ValueError, match=key):
        losses.make_loss(_cfg(**kw), 7)


@pytest.mark.parametrize("b", [1, 1025])
def test_triplet_loss_batch_limits(b):
    from editor_amd import losses
    with pytest.raises(ValueError):
        losses.TripletLoss(0.3)(torch.zeros(b, 8), torch.zeros(b, dtype=torch.int64))
    with pytest.raises(ValueError):
        losses.TripletLoss()(torch.zeros(b, 8), torch.zeros(b, dtype=torch.int64), normalize_feature=True)


def test_header_declares_the_new_entries():
    from editor_amd import _lib
    protos = _lib.parse_header()
    base = protos["editor_triplet_fwd"]
    new = protos["editor_triplet_loss_fwd"]
    assert len(new) == len(base) + 4                                    # + form, margin, hard_factor, dist
    assert new[5:8] == [ctypes.c_int, ctypes.c_float, ctypes.c_float] and new[:5] == base[:5]
    assert len(protos["editor_normalize_rows_fwd"]) == 7 and len(protos["editor_normalize_rows_bwd"]) == 7
    assert len(protos["editor_triplet_bwd"]) == 9                       # unchanged: it serves every form


def test_golden_records_its_conditions_as_met():
    g = load_golden("loss_options")
    for (b, k, d) in H.SHAPES:
        for hf in H.HARD_FACTORS:
            for norm in H.NORMALIZE:
                a_max, seed, active, gap, runner, floor = g["cond/" + H.set_key(b, d, hf, norm)]
                assert 0.25 <= active <= 0.75 and gap >= H.HINGE_GAP and runner >= H.RUNNER_UP_GAP and floor <= 0.25
                # the record describes the inputs the tests regenerate
                target = H.labels(int(seed), b, k)
                c = H.conditions(H.features(int(seed), target, d, float(a_max)), target, 0.3, hf, norm)
                assert np.allclose([c["active"], c["hinge_gap"], c["runner_up"]], [active, gap, runner], rtol=1e-6)
                for margin in H.MARGINS:
                    key = H.case_key(b, d, margin, hf, norm)
                    assert g[key + "/dist_ap"].shape == (b,) and g[key + "/dfeat"].shape == (len(H.stored_rows(b)), min(d, 64))
    assert g["cond/make_loss"][2] <= 0.25
    assert set(H.MAKE_LOSS_CASES) == {k.split("/")[0][3:] for k in g if k.startswith("ml_")}
