"""Generate the overlapping-patch-embedding fixtures (tests/golden/s*_*.npz) from the REFERENCE itself (build container only).

    python tests/golden/capture_stride.py [freq] [eval] [train] [eval128]

Same protocol as capture_golden.py (whose helpers it imports, and which stays as it is): the reference runs on the CPU through
tools/ref_shims.py, driven by editor_amd/synth.py (inputs AND weights by parameter name) with MODEL.STRIDE_SIZE = [s, s], and only
small OUTPUTS are stored - tests regenerate the inputs from (seed, cfg).  The supported strides are the ones the reference itself
runs: square, s <= 16, (H-16)//s + 1 == H//s and (W-16)//s + 1 == W//s (its mask() sizes the count tensor by H//s x W//s and fills
it from an unfold that yields (H-16)//s + 1 windows per column, Frequency.py:46-56).
"""
import os
import sys

import torch
import torch.nn.functional as F

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import capture_golden as cg                    # noqa: E402  (sets sys.path for the repository root, seeds, thread count)
from editor_amd import config, synth           # noqa: E402
from tools import ref_shims                    # noqa: E402


def s1_frequency(s=12):
    """As f1_freq_*: mask_fre + positive counts per 16x16 window at stride s, B = 128 (Frequency.py:42-84)."""
    for tag, (h, w) in {"256x128": (256, 128), "128x256": (128, 256)}.items():
        cfg = config.make_cfg(size_train=(h, w), stride=(s, s))
        m = ref_shims.build_reference_model(cfg, 8, 2)
        for kind, smooth in (("u8", False), ("smooth", True)):
            img, _, _, _ = synth.make_batch(11, 128, h, w, 2, smooth=smooth)
            fi = m.FREQ_INDEX
            with torch.no_grad():
                mask = fi(x=img["RGB"], y=img["NI"], z=img["TI"], img_path=None)
                coeff = [fi.DWT(img[k]) for k in ("RGB", "NI", "TI")]
                low = (coeff[0][0] + coeff[1][0] + coeff[2][0]) / 3
                high = [(coeff[0][1][j] + coeff[1][1][j] + coeff[2][1][j]) / 3 for j in range(4)]
                inv = fi.IDWT((low, high)).mean(dim=1)
                cnt = torch.stack([F.unfold(inv[b][None, None], 16, stride=s).gt(0).sum(1).view(-1)
                                   for b in range(inv.shape[0])]).to(torch.int32)
            cg.save(f"s1_freq_s{s}_{tag}_{kind}", mask=mask, counts=cnt, seed=11, smooth=smooth, stride=s,
                    inv_sample=inv[0, :16, :16])


def s3_eval(preset, seed, batch, s, tag, full=True):
    """As f3_eval_* (full) - or, for the B = 128 case, only what the north-star check reads: cls4t, index, mask_fre and the
    per-modality attention masks."""
    m, cfg, c, cams = cg.build(preset, seed, drop_path=0.0, stride=(s, s))
    m.eval()
    h, w = cfg.INPUT.SIZE_TRAIN
    img, label, cam, view = synth.make_batch(seed + 1, batch, h, w, cams)
    rec = {}
    with torch.no_grad():
        for key, name in (("RGB", "rgb"), ("NI", "nir"), ("TI", "tir")):
            feat, attn = m.BACKBONE(img[key], cam_label=cam, view_label=view)
            _, pm = m.SFTS.part_select(attn)
            rec["mask_" + name] = pm
            if full:
                last = attn[0]
                for a in attn[1:]:
                    last = torch.matmul(a, last)
                rec["scores_" + name] = last[:, :, 0, 1:]
                rec["feat_" + name] = feat[:, :3, :16]
                rec["attn0_" + name] = attn[0][:2, :2, :4, :]
                rec["attn11_" + name] = attn[-1][:2, :2, :4, :]
            del attn
        cls4t = m(img, cam_label=cam, view_label=view)
        mask_fre = m.FREQ_INDEX(x=img["RGB"], y=img["NI"], z=img["TI"], img_path=None)
    rec["index"] = rec["mask_rgb"] | rec["mask_nir"] | rec["mask_tir"] | mask_fre
    if full:
        cg.save(tag, cls4t=cls4t, mask_fre=mask_fre, seed=seed, batch=batch, preset=preset, stride=s, **rec)
    else:
        save_halves(tag, cls4t, mask_fre=mask_fre, seed=seed, batch=batch, preset=preset, stride=s, **rec)


def save_halves(tag, cls4t, **rest):
    """(128, 2304) fp32 features do not compress under the repository's 1 MiB file limit: rows [0, B/2) travel with everything else
    in <tag>_a, rows [B/2, B) in <tag>_b."""
    half = cls4t.shape[0] // 2
    cg.save(tag + "_a", cls4t=cls4t[:half], **rest)
    cg.save(tag + "_b", cls4t=cls4t[half:])


def s4_train(s=12):
    """As f4_train_vitb_al1_dp01: one training step of the reference, AL = 1, DROP_PATH = 0.1, torch.rand draws recorded."""
    real_build = cg.build
    cg.build = lambda preset, seed, **over: real_build(preset, seed, stride=(s, s), **over)
    real_save = cg.save
    cg.save = lambda name, **arrs: real_save(name.replace("f4_train_", "s4_train_s%d_" % s), stride=s, **arrs)
    try:
        cg.f4_f5_train("RGBNT201", 39, 16, 8, "vitb_al1_dp01", drop_path=0.1)
    finally:
        cg.build, cg.save = real_build, real_save


if __name__ == "__main__":
    assert ref_shims.have_reference(), "run in the build container (needs the reference checkout)"
    which = sys.argv[1:] or ["freq", "eval", "train", "eval128"]
    if "freq" in which:
        s1_frequency(12)
    if "eval" in which:
        s3_eval("RGBNT201", 21, 4, 12, "s3_eval_s12_vitb_256x128")
        s3_eval("RGBNT100", 25, 4, 12, "s3_eval_s12_vitb_128x256")
        s3_eval("RGBNT201", 27, 4, 14, "s3_eval_s14_vitb_256x128")
    if "train" in which:
        s4_train(12)
    if "eval128" in which:
        s3_eval("RGBNT201", 29, 128, 12, "s3_eval_s12_vitb_256x128_b128", full=False)
