"""Two-modality models (cfg.MODEL.NUM_MODALITIES = 2): HIP-event timings of the frequency counts at B = 128 through the tile kernel
(freq_counts4_kernel<2, 3>, 16-byte-aligned inputs) and through the generic kernel (freq_counts_kernel<0, 0>: the same inputs behind a
base pointer one float further on) beside the three-modality tile kernel in the same run (rotating operand sets: HBM, not the
Infinity Cache), and the step time of bench.py's loop (B = 128, bf16, DROP_PATH 0.1, fused SGD; eager, no feeding) for the presets
RGBN300 (two modalities) and RGBNT100 (three, the same 128x256 geometry and AL = 0):
    python tools/two_modal_time.py [--steps 10] [--dtype bf16]"""
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


def off_by_one_float(x):
    buf = torch.empty(x.numel() + 1, device="cuda", dtype=torch.float32)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    return v


def kernels(b=128, h=128, w=256, s=12):
    img, _, _, _ = synth.make_batch(1111, b, h, w, 4)
    sets = [[img[k].cuda().clone() for k in ("RGB", "NI", "TI")] for _ in range(5)]
    off = [[off_by_one_float(x) for x in st[:2]] for st in sets]
    assert all(x.data_ptr() % 16 == 0 for st in sets for x in st) and all(x.data_ptr() % 16 == 4 for st in off for x in st)
    rows = {}
    rows["freq counts, 3 modalities, tile kernel <3, 3>"] = ev(lambda i: ops.freq_counts(*sets[i]), 5)
    rows["freq counts, 2 modalities, tile kernel <2, 3>"] = ev(lambda i: ops.freq_counts(sets[i][0], sets[i][1], None), 5)
    rows["freq counts, 2 modalities, generic kernel <0, 0> (base + 4 bytes)"] = ev(lambda i: ops.freq_counts(off[i][0], off[i][1], None), 5)
    rows["freq counts s=%d, 2 modalities, tile kernel <2, 3, u16> + window counts" % s] = \
        ev(lambda i: ops.freq_counts(sets[i][0], sets[i][1], None, stride=s), 5)
    rows["freq counts s=%d, 2 modalities, generic kernel <0, 0, u16> + window counts" % s] = \
        ev(lambda i: ops.freq_counts(off[i][0], off[i][1], None, stride=s), 5)
    assert torch.equal(ops.freq_counts(sets[0][0], sets[0][1], None), ops.freq_counts(off[0][0], off[0][1], None))
    for k, v in rows.items():
        print("%-78s %8.1f us" % (k, v))


def step_ms(preset, dtype, steps, warmup=3, b=128):
    cfg, num_class, cams = config.preset(preset, compute_dtype=dtype, drop_path=0.1)
    torch.manual_seed(1111)
    with contextlib.redirect_stdout(io.StringIO()):
        model = make_model(cfg, num_class, cams)
    synth.fill_state_dict_(model.state_dict(), 1111)
    model = model.cuda().train()
    buckets = model.enable_grad_buckets()
    opt, _ = solver.make_optimizer(cfg, model, None)
    h, w = cfg.INPUT.SIZE_TRAIN
    img, label, cam, view = synth.make_batch(1111, b, h, w, cams, instances=16, keys=config.MODALITY_KEYS[:model.nmod])
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
    print("step %-8s B=%d %s (%d modalities, %dx%d): %.2f ms  %.0f img/s  loss %.4f"
          % (preset, b, dtype, model.nmod, h, w, ms, b / ms * 1e3, float(loss)))
    return ms


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dtype", default="bf16")
    a = ap.parse_args()
    kernels()
    m3 = step_ms("RGBNT100", a.dtype, a.steps)
    m2 = step_ms("RGBN300", a.dtype, a.steps)
    print("RGBN300 / RGBNT100 step time: x %.2f" % (m2 / m3))
