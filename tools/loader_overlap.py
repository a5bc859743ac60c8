"""Does the device input pipeline hide under the training step?    Writes a synthetic RGBNT201-layout
tree with Pillow (the size spread of tools/ragged_input_time.py: about 60x130 to 160x340, 4:2:0, quality 75; 32 identities x 16
images x 3 modalities) and times, in ONE process on one GPU, in the order (a) (b) (c) (c) (b):
    (a) the loader alone (editor_amd.data.make_dataloader's train loader, prefetch=2): batches/s, and from a second pass its own
        per-stage timers per batch: file read, host work of the decode / resize / transform calls (plan + pack + launches),
        the side stream's time from the batch's first launch to its last
    (b) the bf16 config-2 training step (RGBNT201, ViT-B/16, 256x128, B = 128, eager, as bench.py builds it) with RESIDENT inputs
    (c) the same step taking every batch from the loader at prefetch=2
The yardstick is (b) of the same run: (c) / (b) is reported beside the spread of (b)'s two readings; if (c) is outside it, the
largest of (a)'s stage times names the limiting stage.
    python tools/loader_overlap.py [--steps 20] [--warmup 5] [--out profiles/loader_overlap.txt]
--loader-only stops after (a): under `rocprofv3 --kernel-trace --stats` it gives the kernels' own time per batch (the event pair of
the stage timers spans the host work between the launches as well)."""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from editor_amd import config, losses, solver, synth                # noqa: E402
from editor_amd.data import make_dataloader                         # noqa: E402
from editor_amd.modeling import make_model                          # noqa: E402

IDS, PER_ID, BATCH = 32, 16, 128


class _Writer:
    def add_scalar(self, *a, **k):
        pass


def write_tree(root):
    from PIL import Image
    rng = np.random.default_rng(201)
    nbytes = 0
    for split, ids, per in (("train_171", range(1, IDS + 1), PER_ID), ("test", range(201, 203), 2)):
        for m in ("RGB", "NI", "TI"):
            os.makedirs(os.path.join(root, "RGBNT201", split, m))
        for pid in ids:
            for k in range(per):
                for m in ("RGB", "NI", "TI"):
                    w, h = int(rng.integers(60, 161)), int(rng.integers(130, 341))
                    yy, xx = np.mgrid[0:h, 0:w]
                    base = np.stack([128 + 100 * np.sin(xx / 17.0) * np.cos(yy / 11.0), 128 + 90 * np.cos(xx / 29.0 + yy / 7.0),
                                     255.0 * (xx + yy) / (w + h)], axis=2) + rng.normal(0, 12, (h, w, 3))
                    path = os.path.join(root, "RGBNT201", split, m, "%06d_cam%d_0_%02d.jpg" % (pid, 1 + k % 4, k))
                    Image.fromarray(np.clip(base, 0, 255).astype(np.uint8)).save(path, "JPEG", quality=75, subsampling=2)
                    nbytes += os.path.getsize(path)
    return nbytes


def batches(loader):
    """Batch after batch, epoch after epoch."""
    while True:
        for b in loader:
            yield b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loader-only", action="store_true", help="(a) alone and stop: the run to put under a kernel trace")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as root:
        nbytes = write_tree(root)
        cfg, num_class, cams = config.preset("RGBNT201", compute_dtype="bf16", drop_path=0.1)
        cfg.DATASETS.ROOT_DIR = root
        with contextlib.redirect_stdout(io.StringIO()):
            train = make_dataloader(cfg)[0]
        say("tree: %d train samples x 3 files (%.1f MB of JPEG), batches of %d = %d files; loader: prefetch=%d, entropy=%s, read_threads=%d"
            % (len(train.samples), nbytes / 1e6, BATCH, 3 * BATCH, train.prefetch, train.entropy, train.read_threads))

        # (a) the loader alone
        def loader_alone(n, timed):
            train.time_device = timed
            for k in train.timers:
                train.timers[k] = 0
            src = batches(train)
            for _ in range(2):
                next(src)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            base = dict(train.timers)
            for _ in range(n):
                next(src)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            tm = {k: train.timers[k] - base[k] for k in base}
            src.close()
            train.time_device = False
            return dt / n, tm
        t_a, _ = loader_alone(a.steps, False)
        _, tm = loader_alone(a.steps, True)
        nb = max(1, tm["batches"])
        stages = {"file read": 1e3 * tm["read"] / nb, "host work of decode + resize + transform (plan, pack, launches, status read-back)": 1e3 * tm["host"] / nb,
                  "side stream, first launch to last (event pair: spans the host work between the launches)": tm["device_ms"] / nb}
        say("(a) loader alone: %.2f ms / batch = %.1f batches/s = %.0f files/s" % (1e3 * t_a, 1 / t_a, 3 * BATCH / t_a))
        for k, v in stages.items():
            say("      %-92s %7.2f ms / batch" % (k, v))

        if a.loader_only:
            train.close()
            return

        # the step of bench.py (eager)
        torch.manual_seed(1111)
        with contextlib.redirect_stdout(io.StringIO()):
            model = make_model(cfg, num_class, cams)
        synth.fill_state_dict_(model.state_dict(), 1111)
        model = model.to(dev).train()
        buckets = model.enable_grad_buckets()
        opt, _ = solver.make_optimizer(cfg, model, None)
        writer = _Writer()

        def step(img, label, cam, view):
            opt.zero_grad(set_to_none=True)
            out = model(img, label=label, cam_label=cam, view_label=view, img_path=None, writer=writer, epoch=1)
            loss = losses.loss_pairs(out, label)
            loss.backward()
            if buckets is not None:
                buckets.finish()
            opt.step()
            return loss

        src = batches(train)
        img0, pid0, cam0, view0, _ = next(src)
        res = (img0, pid0.to(dev), cam0.to(dev), view0.to(dev))

        def resident(n):
            for _ in range(n):
                step(*res)

        def fed(n):
            for _ in range(n):
                img, pid, cam, view, _ = next(src)
                step(img, pid.to(dev, non_blocking=True), cam.to(dev, non_blocking=True), view.to(dev, non_blocking=True))

        def timed(fn):
            fn(a.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(a.steps)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.steps
        t = [timed(f) for f in (resident, fed, fed, resident)]
        src.close()
        train.close()
    for name, v in zip(("(b) step, resident inputs", "(c) step fed by the loader", "(c) again", "(b) again"), t):
        say("%-32s %8.2f ms / step  %7.0f img/s" % (name, 1e3 * v, BATCH / v))
    b_lo, b_hi = min(t[0], t[3]), max(t[0], t[3])
    c = min(t[1], t[2])
    say("(c) / (b) = %.3f (best of each); (b)'s two readings differ by %.2f ms (%.1f %%), (c) - (b) = %.2f ms"
        % (c / b_lo, 1e3 * (b_hi - b_lo), 100 * (b_hi - b_lo) / b_lo, 1e3 * (c - b_lo)))
    if c <= b_hi:
        say("=> (c) is inside the spread of (b): the input pipeline hides under the step")
    else:
        say("=> (c) is outside the spread of (b); loader alone %.2f ms / batch against a %.2f ms step; largest stage of (a): %s"
            % (1e3 * t_a, 1e3 * b_lo, max(stages, key=stages.get)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(["python tools/loader_overlap.py --steps %d --warmup %d   (one process, one MI355X)" % (a.steps, a.warmup)] + lines) + "\n")


if __name__ == "__main__":
    main()
