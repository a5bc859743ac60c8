"""Separate-file sample layout (RGBNT201 / MSVR310: one detector crop of any size per modality): files/s of the ragged device
input path beside its host stage and beside the uniform path, on 3 x 128 Pillow-encoded files (4:2:0, quality 75) whose sizes are
drawn from a seeded spread (about 60x130 to 160x340), resized to 256x128 bicubic:
    (a) the host stage alone: parse + Huffman decode of every file on 16 threads (no device work)
    (b) DeviceJpegDecoder.decode_ragged + DeviceResize on the RaggedImages, end to end (host clock, ends in a synchronise)
    (c) the yardstick: DeviceJpegDecoder.__call__ + DeviceResize on 384 files of ONE size with the same total pixel count
    (d) the planner alone: editor_jpeg_plan of every file on the calling thread (what entropy="device" leaves on the host)
    (e) the same as (b) with DeviceJpegDecoder(entropy="device"): the scans are Huffman-decoded by editor_jpeg_entropy_device
and (b) against the 9 400 files/s the benchmarked tri-modal step consumes (about 3 100 img/s x 3 files); the host-to-device bytes
per batch of (b) and (e); the entropy kernel alone (stream time, inputs already on the device).  (b) is the yardstick for (e).
    (f) the same as (e) with DeviceJpegDecoder(entropy="device_split"): editor_jpeg_entropy_split_device, parallel inside a segment
Then (e) and (f) side by side in the order (e), (f), (f), (e), end to end and kernel alone, on this batch and on a second one in
which the last file is replaced by the 118 KB fixture stitched_444_q90.jpg (tests/golden/f14_decode.npz), the outputs asserted
equal; the kernel of (f) at every accepted sub_bytes.  The one-wave kernel of (e), in the same call, is the yardstick for (f):
(f) is ahead where its time is below (e)'s by more than the spread of (e)'s two readings.
    python tools/ragged_input_time.py [--reps 10]"""
import argparse
import ctypes
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from editor_amd.data import DeviceJpegDecoder, DeviceResize      # noqa: E402

STEP_FILES_PER_S = 9400.0
SIZE = (256, 128)


def encode(rng, w, h):
    from PIL import Image
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 17.0) * np.cos(yy / 11.0), 128 + 90 * np.cos(xx / 29.0 + yy / 7.0),
                     255.0 * (xx + yy) / (w + h)], axis=2) + rng.normal(0, 12, (h, w, 3))
    bio = io.BytesIO()
    Image.fromarray(np.clip(base, 0, 255).astype(np.uint8)).save(bio, "JPEG", quality=75, subsampling=2)
    return bio.getvalue()


def wall(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


class EntropyKernel:
    """A planned batch resident on the device: the entropy kernel alone, either entry (stream time per call)."""

    def __init__(self, dev, files):
        self.n = len(files)
        bp = dev.plan_batch(files)
        tab = np.concatenate([[0], np.cumsum(bp.infos[:, 8].astype(np.int64))])
        self.nbytes, spans, self.fdesc, self.ftab, self.segs, huff, self.nseg = dev.pack_batch(files, bp, tab[:-1])
        buf = np.zeros(self.nbytes, dtype=np.uint8)
        for i, at, lo, hi in spans:
            buf[at:at + hi - lo] = np.frombuffer(files[i], dtype=np.uint8)[lo:hi]
        self.d = [torch.from_numpy(x).cuda() for x in (buf, self.fdesc, self.ftab, self.segs, huff)]
        self.nhuff, self.blocks = int(huff.shape[0]), int(tab[-1])
        self.longest = max(hi - lo for _, _, lo, hi in spans)
        self.status = torch.empty(self.n, dtype=torch.int32, device="cuda")
        self.cd = dev._cd

    def run(self, coef_d, sub=0, work=None):
        from editor_amd._lib import call
        tables = (self.d[0], self.nbytes, ctypes.c_void_p(self.fdesc.ctypes.data), ctypes.c_void_p(self.ftab.ctypes.data),
                  ctypes.c_void_p(self.segs.ctypes.data), self.d[1], self.d[2], self.d[3], self.d[4], self.nhuff, self.n, self.nseg)
        if sub:
            call("editor_jpeg_entropy_split_device", *tables, sub, work, work.numel() * 8, coef_d, self.blocks, self.status)
        else:
            call("editor_jpeg_entropy_device", *tables, coef_d, self.blocks, self.status)

    def time(self, reps, sub=0):
        """-> (seconds per call, the coefficients it left); sub 0: the one-wave kernel"""
        coef_d = torch.full((self.blocks * 64,), 0x5A5A, dtype=torch.int16, device="cuda")
        work = None
        if sub:
            ws = ctypes.c_long(0)
            assert self.cd.editor_jpeg_entropy_split_workspace(self.nseg, sub, ctypes.byref(ws)) == 0
            work = torch.empty(ws.value // 8, dtype=torch.int64, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.run(coef_d, sub, work)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            self.run(coef_d, sub, work)
        e1.record()
        torch.cuda.synchronize()
        assert not self.status.any()
        stats = work[:2 * self.nseg].view(-1, 2).cpu().numpy() if sub else None
        return e0.elapsed_time(e1) / reps / 1e3, coef_d, stats


def split_rows(a, rs, dev, ragged, out):
    """(e) against (f), in one call: end to end and kernel alone on two batches, and the sub_bytes sweep."""
    split = DeviceJpegDecoder(crop_w=0, threads=16, entropy="device_split")
    golden = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "f14_decode.npz"))
    long_file = golden["stitched_444_q90.jpg"].tobytes()
    print("\n(f) entropy=device_split (sub_bytes %d) beside (e) entropy=device, order (e) (f) (f) (e); outputs asserted equal" % split.split_sub_bytes)
    for label, files in (("384 ragged files", ragged), ("383 ragged files + the %d-byte fixture" % len(long_file), ragged[:-1] + [long_file])):
        ref = rs(dev.decode_ragged(files, "cuda"))
        assert torch.equal(rs(split.decode_ragged(files, "cuda")), ref)
        if files is ragged:
            assert torch.equal(ref, out)
        n = len(files)
        t = [wall(lambda d=d: rs(d.decode_ragged(files, "cuda")), a.reps) for d in (dev, split, split, dev)]
        print("%s, end to end (decode + resize):" % label)
        for name, v in zip(("(e)", "(f)", "(f) again", "(e) again"), t):
            print("    %-12s %8.2f ms / batch  %9.0f files/s" % (name, 1e3 * v, n / v))
        k = EntropyKernel(dev, files)
        sub = split.split_sub_bytes
        r = [k.time(a.reps, s) for s in (0, sub, sub, 0)]
        for x in r[1:]:
            assert torch.equal(x[1], r[0][1])                                  # the same coefficients, bit for bit
        print("%s, entropy kernel alone (stream time; %d segments, longest %d bytes):" % (label, k.nseg, k.longest))
        for name, x in zip(("(e) one wave per segment", "(f) split", "(f) split again", "(e) again"), r):
            print("    %-28s %8.3f ms / batch" % (name, 1e3 * x[0]))
        te, tf = (r[0][0], r[3][0]), (r[1][0], r[2][0])
        spread = abs(te[0] - te[1])
        print("    (f) / (e): x %.3f of (e)'s time; (e) - (f) = %.3f ms against a spread of (e)'s readings of %.3f ms: %s"
              % (min(tf) / min(te), 1e3 * (min(te) - max(tf)), 1e3 * spread, "(f) ahead" if min(te) - max(tf) > spread else "(f) NOT ahead"))
        for s in (16, 32, 64, 128):
            ts, coef_s, stats = k.time(a.reps, s)
            assert torch.equal(coef_s, r[0][1])
            print("    sub_bytes %3d  %8.3f ms / batch   rounds per chunk: mean %.2f, max %d   chunks: max %d"
                  % (s, 1e3 * ts, stats[:, 0].sum() / max(1, stats[:, 1].sum()), int((stats[:, 0] / np.maximum(stats[:, 1], 1)).max()), int(stats[:, 1].max())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    rng = np.random.default_rng(201)
    n = 3 * 128
    ws, hs = rng.integers(60, 161, n), rng.integers(130, 341, n)
    ragged = [encode(rng, int(w), int(h)) for w, h in zip(ws, hs)]
    pixels = int((ws * hs).sum())
    uw = int(round(np.sqrt(pixels / n / 2.0)))                    # one size, aspect 1:2 like the spread's centre, same total pixel count
    uh = int(round(pixels / n / uw))
    uniform = [encode(rng, uw, uh) for _ in range(n)]
    print("files: %d ragged (%.1f Mpixel, %.1f MB of JPEG) | %d uniform %dx%d (%.1f Mpixel, %.1f MB)"
          % (n, pixels / 1e6, sum(map(len, ragged)) / 1e6, n, uw, uh, n * uw * uh / 1e6, sum(map(len, uniform)) / 1e6))

    dec = DeviceJpegDecoder(crop_w=0, threads=16)
    rs = DeviceResize(SIZE, 3)

    # (a) the host stage alone
    infos = np.stack([dec.parse(f) for f in ragged])
    first = np.concatenate([[0], np.cumsum(infos[:, 8].astype(np.int64))])
    coef = np.zeros((int(first[-1]), 64), dtype=np.int16)
    qt = np.zeros((n, 192), dtype=np.uint16)
    scratch = np.zeros((n, 16), dtype=np.int32)

    def host_stage():
        list(dec._pool.map(lambda i: dec._parse_rc(ragged[i], scratch[i]), range(n)))
        list(dec._pool.map(lambda i: dec._entropy(ragged[i], coef.ctypes.data + int(first[i]) * 128, int(infos[i, 8]),
                                                  qt.ctypes.data + i * 384, scratch[i]), range(n)))
    t_a = wall(host_stage, a.reps)

    # (b) ragged decode + resize, (c) uniform decode + resize
    def run_ragged():
        return rs(dec.decode_ragged(ragged, "cuda"))

    def run_uniform():
        return rs(dec(uniform, "cuda")[0])
    t_b = wall(run_ragged, a.reps)
    t_c = wall(run_uniform, a.reps)
    t_b2 = wall(run_ragged, a.reps)                               # again after (c): the spread between the two is the noise
    # the device share of (b): the two entries alone, inputs already on the device
    rag = dec.decode_ragged(ragged, "cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rs(rag)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.reps):
        rs(rag)
    e1.record()
    torch.cuda.synchronize()
    t_rs = e0.elapsed_time(e1) / a.reps / 1e3

    out = run_ragged()
    assert tuple(out.shape) == (n,) + SIZE + (3,)
    h2d_b = dec.last_h2d_bytes

    # (d) the planner alone, (e) entropy="device" end to end, between two more runs of (b)
    dev = DeviceJpegDecoder(crop_w=0, threads=16, entropy="device")
    t_d = wall(lambda: dev.plan_batch(ragged), a.reps)

    def run_device():
        return rs(dev.decode_ragged(ragged, "cuda"))
    assert torch.equal(run_device(), out)
    h2d_e = dev.last_h2d_bytes
    t_e = wall(run_device, a.reps)
    t_b3 = wall(run_ragged, a.reps)
    t_e2 = wall(run_device, a.reps)
    # the entropy kernel alone
    from editor_amd._lib import call
    bp = dev.plan_batch(ragged)
    tab = np.concatenate([[0], np.cumsum(bp.infos[:, 8].astype(np.int64))])
    nbytes, spans, fdesc, ftab, segs, huff, nseg = dev.pack_batch(ragged, bp, tab[:-1])
    buf = np.zeros(nbytes, dtype=np.uint8)
    for i, at, lo, hi in spans:
        buf[at:at + hi - lo] = np.frombuffer(ragged[i], dtype=np.uint8)[lo:hi]
    d = [torch.from_numpy(x).cuda() for x in (buf, fdesc, ftab, segs, huff)]
    coef_d = torch.empty(int(tab[-1]) * 64, dtype=torch.int16, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")

    def kernel():
        call("editor_jpeg_entropy_device", d[0], nbytes, ctypes.c_void_p(fdesc.ctypes.data), ctypes.c_void_p(ftab.ctypes.data),
             ctypes.c_void_p(segs.ctypes.data), d[1], d[2], d[3], d[4], int(huff.shape[0]), n, nseg, coef_d, int(tab[-1]), status)
    kernel()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.reps):
        kernel()
    e1.record()
    torch.cuda.synchronize()
    t_k = e0.elapsed_time(e1) / a.reps / 1e3
    assert not status.any() and np.array_equal(coef_d.cpu().numpy().reshape(-1, 64), coef)      # (a)'s host coefficients
    for name, t in (("(a) host parse + Huffman, 16 threads", t_a), ("(b) ragged decode + resize, end to end", t_b),
                    ("(b) again", t_b2), ("(c) uniform decode + resize, end to end", t_c)):
        print("%-44s %8.2f ms / batch  %9.0f files/s" % (name, 1e3 * t, n / t))
    print("%-44s %8.2f ms / batch  (host table building + 2 launches, stream time)" % ("    ragged resize alone", 1e3 * t_rs))
    for name, t in (("(b) once more, after (e)", t_b3), ("(d) planner alone, one thread", t_d), ("(e) entropy=device decode + resize, end to end", t_e),
                    ("(e) again", t_e2)):
        print("%-44s %8.2f ms / batch  %9.0f files/s" % (name, 1e3 * t, n / t))
    print("%-44s %8.2f ms / batch  (%d segments, one wave each, stream time)" % ("    entropy kernel alone", 1e3 * t_k, nseg))
    print("host-to-device bytes per batch: (b) %.2f MB   (e) %.2f MB" % (h2d_b / 1e6, h2d_e / 1e6))
    best_b, best_e = min(t_b, t_b2, t_b3), min(t_e, t_e2)
    print("(e) / (b): x %.2f of (b)'s time  (%.0f against %.0f files/s)" % (best_e / best_b, n / best_e, n / best_b))
    print("(b) / step demand (%.0f files/s): x %.2f   (b) / (c): x %.2f   (a) / (b): x %.2f of (b)'s time is the host stage"
          % (STEP_FILES_PER_S, n / best_b / STEP_FILES_PER_S, t_c / best_b, t_a / best_b))
    split_rows(a, rs, dev, ragged, out)


if __name__ == "__main__":
    main()
