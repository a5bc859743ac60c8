"""End-to-end parity of the model with an overlapping patch embedding (MODEL.STRIDE_SIZE = [12, 12] / [14, 14]: 16x16 windows,
T = 211 / 163 tokens) against the REFERENCE's own outputs (tests/golden/s3_eval_*, s4_train_*: captured by
tests/golden/capture_stride.py; the oracle's patch embedding is stride = kernel by construction, so it is no yardstick here).
Assertions and tolerances of the f32 mode are those of tests/test_gpu_model.py::test_eval_parity_f32 / test_train_parity_f32."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, t
from editor_amd import config, synth
from test_gpu_fullsize import TOL
from test_gpu_model import _Writer, _cuda_batch, _model

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_f16_loss_scale():
    """The static loss scale of the f16 backward is a process-wide option that a model built with cfg.MODEL.GRAD_SCALE installs and a
    model built without it keeps (functional.set_model_options: None = keep) - tests/test_gpu_pipeline.py builds models with
    GRAD_SCALE = 1 for the device grad scaler.  The f16 gradient checks here are stated for the library's default scale (2^15; at 1
    the half-precision gradients underflow), so every test of this file runs with it, whatever ran before in the process."""
    from editor_amd import functional as fn
    old = fn.F16_GRAD_SCALE
    fn.set_f16_grad_scale(32768.0)
    yield
    fn.set_f16_grad_scale(old)


@pytest.mark.parametrize("tag,preset,s,tokens", [("s12_vitb_256x128", "RGBNT201", 12, 211), ("s12_vitb_128x256", "RGBNT100", 12, 211),
                                                 ("s14_vitb_256x128", "RGBNT201", 14, 163)])
def test_eval_parity_f32_stride(tag, preset, s, tokens):
    g = load_golden("s3_eval_" + tag)
    seed, batch = int(g["seed"]), int(g["batch"])
    assert int(g["stride"]) == s
    m, cfg, c, cams = _model(preset, seed, "f32", drop_path=0.0, stride=(s, s))
    assert m.BACKBONE.base.num_patches + 1 == tokens
    m.eval()
    h, w = cfg.INPUT.SIZE_TRAIN
    img, label, cam, view = _cuda_batch(*synth.make_batch(seed + 1, batch, h, w, cams))
    with torch.no_grad():
        cls4t = m(img, cam_label=cam, view_label=view)
    aux = m.last_aux
    for i, name in enumerate(("rgb", "nir", "tir")):
        sc = aux["scores"].view(3, batch, 12, -1)[i].cpu()
        e = rel_err(sc, g["scores_" + name])
        print(tag, name, "scores rel err %.2e" % e)
        assert e < 1e-4
        assert torch.equal(aux["attn_masks"][i].cpu().bool(), t(g["mask_" + name]))
    assert torch.equal(aux["mask_fre"].cpu().bool(), t(g["mask_fre"]))
    assert torch.equal(aux["index"].cpu().bool(), t(g["index"]))
    e = rel_err(cls4t.cpu(), g["cls4t"])
    print(tag, "cls4t rel err %.2e" % e)
    assert e < 1e-3


def test_train_parity_f32_stride12(oracle):
    """The reference's own training step at stride 12 (AL = 1, DROP_PATH = 0.1, B = 16): its recorded torch.rand keep masks are
    teacher-forced, outputs / losses / gradients must follow."""
    g = load_golden("s4_train_s12_vitb_al1_dp01")
    seed, batch, inst = int(g["seed"]), int(g["batch"]), int(g["instances"])
    m, cfg, c, cams = _model("RGBNT201", seed, "f32", drop_path=0.1, stride=(12, 12))
    assert m.BACKBONE.base.drop_rates == [float(r) for r in g["drop_rates"]]
    m.teacher_drop_keep = t(g["drop_keep"])
    m.train()
    h, w = cfg.INPUT.SIZE_TRAIN
    img, label, cam, view = _cuda_batch(*synth.make_batch(seed + 1, batch, h, w, cams, instances=inst))
    wr = _Writer()
    out = m(img, label=label, cam_label=cam, view_label=view, writer=wr, epoch=1)
    assert len(out) == 5 and int(g["al"]) == 1
    for i, o in enumerate(out):
        e = rel_err(o.detach().cpu(), g["out%d" % i])
        print("out%d rel err %.2e" % (i, e))
        assert e < 1e-3, i
    assert rel_err(m.last_aux["loss_bcc"].detach().cpu(), g["loss_bcc"]) < 1e-4
    assert rel_err(m.last_aux["loss_ocfr"].detach().cpu(), g["loss_ocfr"]) < 1e-4
    assert abs(wr.scalars["num_count"] - float(g["num_count"])) < 1e-6
    loss = oracle.projection_loss([o.cpu() for o in out][:-1] + [out[-1].cpu()])
    assert rel_err(loss.detach(), g["loss"]) < 1e-3
    total = out[-1]
    for i, o in enumerate(out[:-1]):
        total = total + (o * synth.uniform(5, "proj/%d" % i, tuple(o.shape)).cuda()).mean()
    total.backward()
    named = dict(m.named_parameters())
    checked, worst = 0, 0.0
    for key, val in g.items():
        if key.startswith("g:"):
            e = rel_err(named[key[2:]].grad.cpu(), val)
            worst = max(worst, e)
            assert e < 2e-3, (key, e)
            checked += 1
        elif key.startswith("gs:"):
            gr = named[key[3:]].grad
            e = rel_err(gr.reshape(gr.shape[0], -1)[:16, :16].cpu(), val)
            worst = max(worst, e)
            assert e < 2e-3, (key, e)
            assert abs(gr.norm().item() / float(g["gn:" + key[3:]]) - 1) < 1e-3, key
            checked += 1
    print("gradient keys checked: %d, worst rel err %.2e" % (checked, worst))
    assert checked >= 20
    assert tuple(named["BACKBONE.base.pos_embed"].grad.shape) == (1, 211, 768)
    uniq = label.unique()
    for tname in ("RGB", "NIR", "TIR"):
        cen = getattr(m.FUSE_block.memory_cls, tname + "_centers")[uniq][:, :32]
        assert rel_err(cen.cpu(), g["cen_" + tname]) < 1e-4
    assert rel_err(m.FUSE_BN.running_mean[:64].cpu(), g["bn_mean"]) < 1e-4


def _golden_b128():
    a, b = load_golden("s3_eval_s12_vitb_256x128_b128_a"), load_golden("s3_eval_s12_vitb_256x128_b128_b")
    a["cls4t"] = np.concatenate([a["cls4t"], b["cls4t"]], 0)
    assert a["cls4t"].shape == (128, 2304) and a["index"].shape == (128, 210)
    return a


@pytest.mark.parametrize("dtype", ["f32", "f16x2", "f16x2s", "f16", "bf16"])
def test_eval_b128_stride12_against_the_reference(dtype):
    """B = 128 at stride 12 (3 x 128 x 211 token rows) in all five compute modes.  f32 / f16x2 / f16x2 with selection scope run
    free: the selection must equal the reference's in all 128 rows, features within the north star's 1e-3.  bf16 / f16: the
    reference's selection teacher-forced (16-bit scores cannot be bit-identical to fp32 ones), cls4t against the entries of
    tests/test_gpu_fullsize.py's TOL table (the B = 128 one) for that quantity."""
    g = _golden_b128()
    seed, batch = int(g["seed"]), int(g["batch"])
    assert batch == 128
    m, cfg, c, cams = _model("RGBNT201", seed, dtype, drop_path=0.0, stride=(12, 12))
    m.eval()
    img, label, cam, view = _cuda_batch(*synth.make_batch(seed + 1, batch, 256, 128, cams))
    free = dtype in ("f32", "f16x2", "f16x2s")
    if not free:
        m.teacher_index = t(g["index"])
    with torch.no_grad():
        cls4t = m(img, cam_label=cam, view_label=view)
    aux = m.last_aux
    assert torch.equal(aux["mask_fre"].cpu().bool(), t(g["mask_fre"]))                  # integer path: exact in any mode
    if free:
        for i, n in enumerate(("rgb", "nir", "tir")):
            bad = (aux["attn_masks"][i].cpu().bool() != t(g["mask_" + n])).any(1).nonzero().flatten().tolist()
            assert not bad, (dtype, n, "rows whose attention mask differs from the reference's:", bad)
        bad = (aux["index"].cpu().bool() != t(g["index"])).any(1).nonzero().flatten().tolist()
        assert not bad, (dtype, "rows whose index differs:", bad)
    else:
        agree = [(aux["attn_masks"][i].cpu().bool() == t(g["mask_" + n])).float().mean().item() for i, n in enumerate(("rgb", "nir", "tir"))]
        print(dtype, "per-modality attention-mask agreement (reported):", agree)
    if dtype not in ("f32",):
        assert "plan" in aux                                                          # the compacted HMA head ran
    err = rel_err(cls4t.cpu(), g["cls4t"])
    row = ((cls4t.cpu().double() - t(g["cls4t"]).double()).norm(dim=1) / t(g["cls4t"]).double().norm(dim=1)).max().item()
    print(dtype, "B=128 stride 12 cls4t rel err %.3e (worst row %.3e)" % (err, row))
    assert err < (1e-3 if free else TOL[dtype]["cls4t"])


def test_dense_hma_form_at_stride12_bf16():
    """both HMA forms run at T = 211: the dense-masked form against the compacted one (as test_hma_compact_equals_dense_bf16)"""
    seed, batch = 31, 16
    img, label, cam, view = _cuda_batch(*synth.make_batch(seed + 1, batch, 256, 128, 4, instances=8))
    res = {}
    for compact in (False, True):
        m, cfg, c, cams = _model("RGBNT201", seed, "bf16", drop_path=0.0, hma_compact=compact, stride=(12, 12))
        m.train()
        out = m(img, label=label, cam_label=cam, view_label=view, writer=_Writer(), epoch=1)
        assert ("plan" in m.last_aux) == compact
        res[compact] = ([o.detach().float().cpu() for o in out], m.last_aux["index"].cpu())
    assert torch.equal(res[False][1], res[True][1])
    for a, b in zip(res[False][0], res[True][0]):
        assert rel_err(a, b) < 1.5e-2


def test_stride16_given_explicitly_is_bit_identical_bf16():
    """STRIDE_SIZE = [16, 16] spelled out == a cfg without the override: every output and every gradient of a training step
    (bf16, B = 16, stochastic depth on), bit for bit - and through the same entry points (the stride-16 wrappers keep calling
    editor_im2col16 / editor_freq_counts_f32)."""
    from editor_amd import ops
    seed, batch = 31, 16
    img, label, cam, view = _cuda_batch(*synth.make_batch(seed + 1, batch, 256, 128, 4, instances=8))
    res = []
    names = []
    real = ops.call

    def spy(name, *a):
        names[-1].add(name)
        return real(name, *a)
    for over in ({}, {"stride": (16, 16)}):
        torch.manual_seed(9)
        m, cfg, c, cams = _model("RGBNT201", seed, "bf16", drop_path=0.1, **over)
        m.train()
        names.append(set())
        ops.call = spy
        try:
            out = m(img, label=label, cam_label=cam, view_label=view, writer=_Writer(), epoch=1)
            total = out[-1]
            for i, o in enumerate(out[:-1]):
                total = total + (o * synth.uniform(5, "proj/%d" % i, tuple(o.shape)).cuda()).mean()
            total.backward()
            torch.cuda.synchronize()
        finally:
            ops.call = real
        res.append(([o.detach().clone() for o in out], {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    assert names[0] == names[1]
    assert {"editor_im2col16", "editor_freq_counts_f32"} <= names[1]
    assert not any("im2col_patch" in n or "freq_counts_stride" in n for n in names[1])
    (o0, g0), (o1, g1) = res
    assert all(torch.equal(a, b) for a, b in zip(o0, o1))
    assert g0.keys() == g1.keys() and len(g0) > 150
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_train_step_stride12_options(dtype):
    """ACT_LIGHT, DROP_SKIP off and ungrouped blocks need no special-casing at T = 211 (3 x 16 x 211 rows, not a multiple of 64):
    each runs a training step whose outputs equal the default's (bit for bit where the option promises it)."""
    from editor_amd import functional as fn
    seed, batch = 41, 16
    img, label, cam, view = _cuda_batch(*synth.make_batch(seed + 1, batch, 256, 128, 4, instances=4))

    def step(group=True, **over):
        old = fn.GROUP_BLOCKS
        fn.GROUP_BLOCKS = group
        try:
            torch.manual_seed(5)
            m, cfg, c, cams = _model("RGBNT201", seed, dtype, drop_path=0.1, stride=(12, 12), **over)
            m.train()
            out = m(img, label=label, cam_label=cam, view_label=view, writer=_Writer(), epoch=1)
            total = out[-1] + sum((o * synth.uniform(5, "proj/%d" % i, tuple(o.shape)).cuda()).mean() for i, o in enumerate(out[:-1]))
            total.backward()
            torch.cuda.synchronize()
            grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
            assert all(torch.isfinite(v).all() for v in grads.values())
            return [o.detach().clone() for o in out], grads
        finally:
            fn.GROUP_BLOCKS = old
            fn.ACT_LIGHT = False
    base_o, base_g = step()
    o, g = step(group=False)                               # three TransformerBlockFn nodes instead of the grouped node: same bits
    assert all(torch.equal(a, b) for a, b in zip(base_o, o)) and all(torch.equal(base_g[k], g[k]) for k in base_g)
    o, g = step(act_light=True)                            # forward bit-identical, gradients to 16-bit rounding
    assert all(torch.equal(a, b) for a, b in zip(base_o, o))
    errs = sorted(((rel_err(g[k].cpu(), base_g[k].cpu()), k) for k in base_g if base_g[k].abs().max() > 0), reverse=True)
    worst = errs[0][0]
    print(dtype, "stride 12 activation-light vs default: worst gradient rel err %.2e" % worst, ["%.2e %s" % e for e in errs[:5]])
    assert worst < (2e-2 if dtype == "bf16" else 3e-3)     # the bounds of test_activation_light_blocks_match_default
    o, g = step(drop_skip=False)                           # dropped samples computed and multiplied by zero: forward bit-identical
    assert all(torch.equal(a, b) for a, b in zip(base_o, o))     # (as test_training_step_with_skipping_equals_the_step_without)
