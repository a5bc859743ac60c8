"""Two-modality models (cfg.MODEL.NUM_MODALITIES = 2, EDITOR.forward_two_modalities; the reference's make_model.py:260-360) on the
host: the oracle with MODALITIES3[:2] against the goldens captured from the reference's own method (tests/golden/capture_two_modal.py:
masks / counts bit-exact, floats <= 1e-5 as tests/test_oracle_golden.py), and the model's construction contract - state dict, signature,
gradient segments, refusals, preset."""
import inspect
import json
import os

import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err, t
from editor_amd import config, synth

DIM = 768


def _model(preset="RGBN300", **over):
    from editor_amd.modeling import make_model
    cfg, c, cams = config.preset(preset, compute_dtype="f32", **over)
    return make_model(cfg, c, cams), cfg, c, cams


def _state_dict(seed, **over):
    m, cfg, c, cams = _model(**over)
    sd = m.state_dict()
    synth.fill_state_dict_(sd, seed)
    return {k: v.clone() for k, v in sd.items()}, cfg, c, cams


# ---------------------------------------------------------------------------------------------------
# oracle == reference goldens
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,hw,kind", [("256x128", (256, 128), "u8"), ("256x128", (256, 128), "smooth"),
                                         ("128x256", (128, 256), "u8"), ("128x256", (128, 256), "smooth"),
                                         ("s12_256x128", (256, 128), "u8")])
def test_t1_frequency(oracle, tag, hw, kind):
    g = load_golden(f"t1_freq_{tag}_{kind}")
    s = int(g["stride"])
    img, _, _, _ = synth.make_batch(int(g["seed"]), 128, hw[0], hw[1], 2, smooth=bool(g["smooth"]), keys=("RGB", "NI"))
    _, inv = oracle.frequency_counts(img["RGB"], img["NI"], None)
    assert torch.equal(inv[0, :16, :16], t(g["inv_sample"]))
    counts = torch.stack([torch.nn.functional.unfold(inv[b][None, None], 16, stride=s).gt(0).sum(1).view(-1)
                          for b in range(inv.shape[0])]).to(torch.int32)
    assert torch.equal(counts, t(g["counts"]))
    mask = oracle.topk_mask(counts, 10)
    assert torch.equal(mask, t(g["mask"]))
    assert mask.sum(1).eq(10).all()
    if s == 16:
        mask16, counts16 = oracle.frequency_mask(img["RGB"], img["NI"], None, keep=10)
        assert torch.equal(counts16, counts) and torch.equal(mask16, mask)


def test_t3_eval(oracle):
    g = load_golden("t3_eval_vitb_256x128")
    seed, batch = int(g["seed"]), int(g["batch"])
    h, w = (int(v) for v in g["size"])
    sd, cfg, c, cams = _state_dict(seed, drop_path=0.0, size_train=(h, w))
    img, label, cam, view = synth.make_batch(seed + 1, batch, h, w, cams)
    with torch.no_grad():
        cls4t, aux = oracle.editor_forward(sd, img, cam, training=False, al=cfg.MODEL.AL, return_aux=True,
                                           modalities=oracle.MODALITIES3[:2])
    for i, name in enumerate(("rgb", "nir")):
        assert rel_err(aux["scores"][i], g["scores_" + name]) < 1e-5
        assert torch.equal(aux["attn_masks"][i], t(g["mask_" + name]))
    assert torch.equal(aux["mask_fre"], t(g["mask_fre"]))
    assert torch.equal(aux["index"], t(g["index"]))
    assert tuple(cls4t.shape) == (batch, 2 * DIM)
    assert rel_err(cls4t, g["cls4t"]) < 1e-5


@pytest.mark.parametrize("tag", ["vitb_al0", "vitb_al1_dp01"])
def test_t4_train_and_grads(oracle, tag):
    g = load_golden("t4_train_" + tag)
    seed, batch, inst, al = int(g["seed"]), int(g["batch"]), int(g["instances"]), int(g["al"])
    h, w = (int(v) for v in g["size"])
    dp = 0.1 if tag.endswith("dp01") else 0.0
    sd, cfg, c, cams = _state_dict(seed, drop_path=dp, al=al, size_train=(h, w))
    drop = {}
    if dp:
        rates = [x.item() for x in torch.linspace(0, dp, 12)]                 # vit_pytorch.py:511
        assert rates == [float(r) for r in g["drop_rates"]]
        drop = dict(drop_keep=torch.from_numpy(g["drop_keep"]).float(), drop_rates=rates)
        assert tuple(drop["drop_keep"].shape) == (2, 12, 2, batch)
    leaves = {}
    for k, v in sd.items():
        if v.is_floating_point() and "centers" not in k and "running" not in k and not k.startswith("FREQ"):
            v.requires_grad_(True)
            leaves[k] = v
    img, label, cam, view = synth.make_batch(seed + 1, batch, h, w, cams, instances=inst)
    out, aux = oracle.editor_forward(sd, img, cam, label=label, training=True, al=al, return_aux=True,
                                     modalities=oracle.MODALITIES3[:2], **drop)
    assert len(out) == (5 if al else 7)
    for i, o in enumerate(out):
        assert rel_err(o, g["out%d" % i]) < 1e-5, i
    assert rel_err(aux["loss_bcc"], g["loss_bcc"]) < 1e-5
    assert rel_err(aux["loss_ocfr"], g["loss_ocfr"]) < 1e-5
    loss = oracle.projection_loss(out)
    assert rel_err(loss, g["loss"]) < 1e-5
    loss.backward()
    uniq = label.unique()
    for tname in ("RGB", "NIR"):
        cen = sd["FUSE_block.memory_cls.%s_centers" % tname][uniq][:, :32]
        assert rel_err(cen, g["cen_" + tname]) < 1e-5
    assert rel_err(sd["FUSE_BN.running_mean"][:64], g["bn_mean"]) < 1e-5
    assert rel_err(sd["FUSE_BN.running_var"][:64], g["bn_var"]) < 1e-5
    checked = 0
    for key, val in g.items():
        if key.startswith("g:"):
            assert rel_err(leaves[key[2:]].grad, val) < 2e-4, key
            checked += 1
        elif key.startswith("gs:"):
            gr = leaves[key[3:]].grad
            assert rel_err(gr.reshape(gr.shape[0], -1)[:16, :16], val) < 2e-4, key
            assert abs(gr.norm().item() / float(g["gn:" + key[3:]]) - 1) < 1e-4, key
            checked += 1
    assert checked >= 20


# ---------------------------------------------------------------------------------------------------
# construction contract
# ---------------------------------------------------------------------------------------------------
_GONE = ("TIR_REDUCE.", "FUSE_block.normT.", "FUSE_block.attnT.", "FUSE_block.normT_.", "FUSE_block.mlpT.",
         "FUSE_block.memory_cls.TIR_centers")
_HEADS = ("FUSE_HEAD.", "FUSE_BN.", "AL_HEAD.", "AL_BN.")


@pytest.mark.parametrize("preset", ["RGBNT100", "RGBNT201"])           # AL = 0 / AL = 1
def test_state_dict_is_the_three_modality_contract_minus_tir(preset):
    """The reference's keys and shapes (tests/golden/state_dict_keys.json) minus everything of the third modality; the four head tensors
    at 2 * dim; nothing renamed."""
    ref = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))
    want = {}
    for k, shape in ref[preset].items():
        if k.startswith(_GONE):
            continue
        if k.startswith(_HEADS):
            shape = [2 * DIM if v == 3 * DIM else v for v in shape]
        want[k] = shape
    assert len(want) < len(ref[preset])
    m, cfg, c, cams = _model(preset, num_modalities=2)
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    assert list(got) == list(want)                     # same order as well
    assert got["FUSE_HEAD.weight"] == [c, 2 * DIM] and got["FUSE_BN.running_mean"] == [2 * DIM]
    if cfg.MODEL.AL:
        assert got["AL_HEAD.weight"] == [c, 2 * DIM] and got["AL_BN.weight"] == [2 * DIM]
    trainable = sorted(n for n, p in m.named_parameters() if p.requires_grad)
    assert trainable == [n for n in ref[preset + ":trainable"] if not n.startswith(_GONE)]
    fb = m.FUSE_block
    assert hasattr(fb, "attnR") and hasattr(fb, "attnN") and not hasattr(fb, "attnT")
    assert hasattr(fb.memory_cls, "NIR_centers") and not hasattr(fb.memory_cls, "TIR_centers")
    assert hasattr(m, "NIR_REDUCE") and not hasattr(m, "TIR_REDUCE")


def test_forward_two_modalities_signature():
    from editor_amd.modeling.make_model import EDITOR
    sig = inspect.signature(EDITOR.forward_two_modalities)
    assert list(sig.parameters) == ["self", "x", "cam_label", "label", "view_label", "cross_type", "img_path", "mode", "writer", "epoch"]
    defaults = {k: p.default for k, p in sig.parameters.items() if k not in ("self", "x")}
    assert defaults == dict(cam_label=None, label=None, view_label=None, cross_type=None, img_path=None, mode=1, writer=None, epoch=None)
    assert list(inspect.signature(EDITOR.forward).parameters) == ["self", "x", "cam_label", "label", "view_label", "img_path", "mode",
                                                                  "writer", "epoch"]


@pytest.mark.parametrize("preset,over", [("RGBN300", {}), ("RGBN300", dict(al=1)), ("RGBNT201", {}),
                                         ("RGBNT201", dict(num_modalities=4))])
def test_grad_segments_cover_each_trainable_parameter_once(preset, over):
    m, cfg, c, cams = _model(preset, **over)
    segs, tail = m.grad_segments()
    names = [s[0] for s in segs]
    assert names[:1 + m.nmod] == ["hma.joint"] + ["hma." + mod[2] for mod in reversed(m.modalities)]
    listed = [id(p) for _, ps in segs for p in ps if p is not None] + [id(p) for p in tail]
    assert len(listed) == len(set(listed))
    assert set(listed) == {id(p) for p in m.parameters()}
    assert {id(p) for p in m.parameters() if p.requires_grad} <= set(listed)


@pytest.mark.parametrize("nmod", [1, 5, 0])
def test_other_modality_counts_are_refused(nmod):
    with pytest.raises(NotImplementedError) as e:
        _model("RGBNT201", num_modalities=nmod)
    assert all(s in str(e.value) for s in ("2", "3", "4"))
    assert "2, 3 or 4" in str(e.value)


@pytest.mark.parametrize("nmod", [3, 4])
def test_forward_two_modalities_on_a_wider_model_raises(nmod):
    m, cfg, c, cams = _model("RGBNT201", num_modalities=nmod)
    img, label, cam, view = synth.make_batch(1, 2, 256, 128, cams)
    with pytest.raises(ValueError, match="sized at construction"):
        m.forward_two_modalities(img, cam_label=cam)


def test_preset_rgbn300_builds():
    m, cfg, c, cams = _model("RGBN300")
    assert (m.nmod, c, cams, cfg.MODEL.AL, list(cfg.INPUT.SIZE_TRAIN)) == (2, 150, 8, 0, [128, 256])
    assert [mod[0] for mod in m.modalities] == list(config.MODALITY_KEYS[:2])
    assert m.FUSE_HEAD.weight.shape == (150, 2 * DIM) and m.FUSE_BN.num_features == 2 * DIM
    assert not hasattr(m, "AL_HEAD")
    img, label, cam, view = synth.make_batch(1, 2, 128, 256, cams)
    with pytest.raises(RuntimeError):                   # no CPU path, as for every other model
        m.forward_two_modalities(img, cam_label=cam)
