"""Overlapping patch embedding (MODEL.STRIDE_SIZE = [12, 12]): HIP-event timings of its two kernels at B = 128 beside their stride-16
counterparts in the same run (rotating operand sets: HBM, not the Infinity Cache), and the step time of bench.py's workload
(RGBNT201, B = 128, bf16, DROP_PATH 0.1, fused SGD; eager, no feeding) built at stride 12 and at stride 16:
    python tools/stride_time.py [--stride 12] [--steps 10] [--dtype bf16]"""
import argparse
import contextlib
import io
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from editor_amd import config, losses, ops, solver, synth  # noqa: E402
from editor_amd.modeling import make_model                  # noqa: E402


def ev(fn, nsets, reps=30):
    for i in range(nsets):
        fn(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i % nsets)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def kernels(s, b=128, h=256, w=128):
    img, _, _, _ = synth.make_batch(1111, b, h, w, 4)
    sets = [[img[k].cuda().clone() for k in ("RGB", "NI", "TI")] for _ in range(5)]
    rows = {}
    rows["editor_im2col16 (bf16, 3 modalities)"] = ev(lambda i: ops.im2col16(sets[i], torch.bfloat16), 5)
    rows["editor_im2col_patch s=%d (bf16, 3 modalities)" % s] = ev(lambda i: ops.im2col_patch(sets[i], torch.bfloat16, (s, s)), 5)
    rows["editor_freq_counts_f32"] = ev(lambda i: ops.freq_counts(*sets[i]), 5)
    rows["editor_freq_counts_stride_f32 s=%d (2 launches)" % s] = ev(lambda i: ops.freq_counts(*sets[i], stride=s), 5)
    for k, v in rows.items():
        print("%-52s %8.1f us" % (k, v))


def step_ms(stride, dtype, steps, warmup=3, b=128):
    cfg, num_class, cams = config.preset("RGBNT201", compute_dtype=dtype, drop_path=0.1, stride=(stride, stride))
    torch.manual_seed(1111)
    with contextlib.redirect_stdout(io.StringIO()):
        model = make_model(cfg, num_class, cams)
    synth.fill_state_dict_(model.state_dict(), 1111)
    model = model.cuda().train()
    buckets = model.enable_grad_buckets()
    opt, _ = solver.make_optimizer(cfg, model, None)
    h, w = cfg.INPUT.SIZE_TRAIN
    img, label, cam, view = synth.make_batch(1111, b, h, w, cams, instances=16)
    img = {k: v.cuda() for k, v in img.items()}
    label, cam, view = label.cuda(), cam.cuda(), view.cuda()

    class W:
        def add_scalar(self, *a, **k):
            pass

    def step():
        opt.zero_grad(set_to_none=True)
        out = model(img, label=label, cam_label=cam, view_label=view, img_path=None, writer=W(), epoch=1)
        loss = losses.loss_pairs(out, label)
        loss.backward()
        buckets.finish()
        opt.step()
        return loss
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    t = model.BACKBONE.base.num_patches + 1
    print("step RGBNT201 B=%d %s stride %d (T = %d): %.2f ms  %.0f img/s  loss %.4f" % (b, dtype, stride, t, ms, b / ms * 1e3, float(loss)))
    return ms


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--stride", type=int, default=12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dtype", default="bf16")
    a = ap.parse_args()
    kernels(a.stride)
    m16 = step_ms(16, a.dtype, a.steps)
    ms = step_ms(a.stride, a.dtype, a.steps)
    print("stride %d / stride 16 step time: x %.2f" % (a.stride, ms / m16))
