"""Overlapping patch embedding (MODEL.STRIDE_SIZE below 16), host side: the factory builds the model on the CPU with the
reference's patch grid, checkpoints resize onto it, and every setting the reference itself cannot run is refused at construction."""
import json
import os

import pytest
import torch

from conftest import GOLDEN
from editor_amd import config, synth


@pytest.mark.parametrize("preset,h,w,ny,nx", [("RGBNT201", 256, 128, 21, 10), ("RGBNT100", 128, 256, 10, 21)])
def test_make_model_stride12_builds_with_the_reference_grid(preset, h, w, ny, nx):
    from editor_amd.modeling import make_model
    ref = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))
    cfg, c, cams = config.preset(preset, stride=(12, 12))
    assert cfg.INPUT.SIZE_TRAIN == [h, w]
    m = make_model(cfg, c, cams)
    base = m.BACKBONE.base
    assert (base.num_y, base.num_x) == (ny, nx)
    assert tuple(base.pos_embed.shape) == (1, 211, 768)
    assert base.patch_embed.proj.stride == (12, 12) and base.patch_embed.proj.kernel_size == (16, 16)
    assert m.FREQ_INDEX.stride == 12
    # make_model.py:91-92, SFTS.py:155: num_patches = (H // s) * (W // s) = 210, k = int(210 * (2 / 210))
    assert m.num_patches == 210 and m.head_k == int(210 * ((1 / 210) * 2))
    sd = m.state_dict()
    assert set(sd) == set(ref[preset])
    other = {k: list(v.shape) for k, v in sd.items() if k != "BACKBONE.base.pos_embed"}
    assert other == {k: v for k, v in ref[preset].items() if k != "BACKBONE.base.pos_embed"}
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == ref[preset + ":trainable"]


def test_an_int_stride_means_both_directions():
    from editor_amd.modeling import make_model
    cfg, c, cams = config.preset("RGBNT201")
    cfg.MODEL.STRIDE_SIZE = 12                       # to_2tuple in the reference's patch embedding (vit_pytorch.py:428)
    m = make_model(cfg, c, cams)
    assert m.BACKBONE.base.stride == (12, 12) and m.num_patches == 210 and m.FREQ_INDEX.stride == 12


def test_stride16_explicit_is_the_default_model():
    from editor_amd.modeling import make_model
    torch.manual_seed(3)
    a = make_model(*config.preset("RGBNT201"))
    torch.manual_seed(3)
    b = make_model(*config.preset("RGBNT201", stride=(16, 16)))
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert a.BACKBONE.base.patch_embed.proj.stride == (16, 16)


def test_load_param_resizes_a_14x14_checkpoint_to_the_stride12_grid(tmp_path):
    from editor_amd.modeling.make_model import Trans, resize_pos_embed
    d = 64
    tr = Trans((256, 128), d, 1, 2, 4.0, True, 4, 3.0, 0.0, stride=(12, 12))
    ck = {"pos_embed": synth.normal(7, "ck/pos", (1, 197, d), 0.02), "cls_token": synth.normal(7, "ck/cls", (1, 1, d), 0.02),
          "patch_embed.proj.weight": synth.normal(7, "ck/pe", (d, 768), 0.05)}
    path = str(tmp_path / "jx_vit_base_p16_224.pth")
    torch.save({"model": ck}, path)
    tr.load_param(path)
    want = resize_pos_embed(ck["pos_embed"], 21, 10)
    assert tuple(want.shape) == (1, 211, d)
    assert torch.equal(tr.pos_embed.detach(), want)
    assert torch.equal(tr.patch_embed.proj.weight.detach().reshape(d, -1), ck["patch_embed.proj.weight"])


@pytest.mark.parametrize("size,stride", [((384, 128), (12, 12)), ((256, 128), (8, 8)), ((256, 128), (16, 12)), ((256, 128), (20, 20)),
                                         ((256, 128), (11, 11))])
def test_unsupported_strides_are_refused_at_construction(size, stride):
    """384x128 at s = 12 ((384-16)//12 + 1 = 31 windows against 384//12 = 32), s = 8 and the non-square [16, 12] are where the
    reference's own frequency mask fails; s > 16 leaves pixels between the windows."""
    from editor_amd.modeling import make_model
    cfg = config.make_cfg(size_train=size, stride=stride)
    with pytest.raises(NotImplementedError, match="square stride s <= 16"):
        make_model(cfg, 8, 2)


@pytest.mark.parametrize("s", [12, 13, 14, 15, 16])
def test_supported_strides_at_the_shipped_geometries(s):
    from editor_amd.modeling.make_model import check_stride
    assert check_stride((256, 128), (s, s)) == s and check_stride((128, 256), (s, s)) == s


def test_no_refusal_names_stride_16_any_more():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dirpath, _, files in os.walk(os.path.join(root, "editor_amd")):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dirpath, f)).read()
                for line in text.splitlines():
                    assert not ("NotImplementedError" in line and "STRIDE_SIZE 16" in line), (f, line)
