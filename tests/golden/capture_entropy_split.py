"""Writes tests/golden/d2_entropy_split.npz: the subsequence-boundary cases the in-segment parallel Huffman decode
(DeviceJpegDecoder(entropy="device_split"), editor_jpeg_entropy_split_segments / editor_jpeg_entropy_split_device) needs beyond
what f14_decode.npz, r1_ragged_jpeg.npz and d1_device_entropy.npz already hold, Pillow-encoded from seeded images, with PILLOW'S
decoded pixels:
    exact128_420_72x56     a restart-less file whose scan is EXACTLY k x 128 bytes long (so k' x sub_bytes for every accepted
                           sub_bytes: the last subsequence is a full one and nothing is left over)
    plus1_444_40x48        one whose scan is k x 128 + 1 bytes long (the last subsequence holds one byte)
    tinyseg_gray_64x24     a nearly flat grayscale image with a restart interval of ONE MCU: 24 segments of a few bytes each, all
                           shorter than the smallest subsequence (16 bytes)
The first two are searched for: the noise of the seeded image is redrawn until the length fits (the count of draws is printed).
Run in the build container (Pillow 12.2.0, libjpeg-turbo) after `python -m editor_amd.build`:
    python tests/golden/capture_entropy_split.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from capture_device_entropy import host, synth                   # noqa: E402


def encode(im, **kw):
    bio = io.BytesIO()
    im.save(bio, "JPEG", **kw)
    return bio.getvalue()


def segments(data):
    """-> the planner's (start, end, first MCU) rows of an eligible file"""
    import ctypes
    from editor_amd import _lib
    cd = _lib.lib().cdll
    buf = np.frombuffer(data, dtype=np.uint8)
    info, plan = np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.int32)
    qt, huff, seg = np.zeros((3, 64), dtype=np.uint16), np.zeros((8, 272), dtype=np.uint8), np.zeros((256, 3), dtype=np.int64)
    rc = cd.editor_jpeg_plan(ctypes.c_void_p(buf.ctypes.data), buf.size, ctypes.c_void_p(info.ctypes.data), ctypes.c_void_p(plan.ctypes.data),
                             ctypes.c_void_p(qt.ctypes.data), ctypes.c_void_p(huff.ctypes.data), ctypes.c_void_p(seg.ctypes.data), 256)
    assert rc == 0 and plan[0] == 1
    return seg[:int(plan[1])]


def search(rng, w, h, ss, q, rest):
    for n in range(1, 100000):
        data = encode(synth(rng, w, h, ss), quality=q, subsampling=ss)
        a, b = host(data)[3]
        if (b - a) % 128 == rest:
            return data, n
    raise AssertionError("no image found")


def main():
    rng = np.random.default_rng(43)
    out = {}
    data, n0 = search(rng, 72, 56, 2, 85, 0)
    out["exact128_420_72x56.jpg"] = np.frombuffer(data, dtype=np.uint8)
    data, n1 = search(rng, 40, 48, 0, 80, 1)
    out["plus1_444_40x48.jpg"] = np.frombuffer(data, dtype=np.uint8)
    flat = np.clip(120 + rng.normal(0, 1.5, (24, 64)), 0, 255).astype(np.uint8)
    data = encode(Image.fromarray(flat), quality=60, restart_marker_blocks=1)
    out["tinyseg_gray_64x24.jpg"] = np.frombuffer(data, dtype=np.uint8)
    seg = segments(data)
    assert len(seg) == 24 and (seg[:, 1] - seg[:, 0]).max() < 16, seg
    for k in list(out):
        d = out[k].tobytes()
        rc, _, eligible, _ = host(d)
        assert rc == 0 and eligible, (k, rc, eligible)
        out[k[:-4] + ".rgb"] = np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))
    path = os.path.join(HERE, "d2_entropy_split.npz")
    np.savez_compressed(path, **out)
    print("wrote d2_entropy_split.npz: %d bytes; draws %d and %d; scan lengths %s"
          % (os.path.getsize(path), n0, n1, [int(np.diff(host(out[k].tobytes())[3])[0]) for k in sorted(out) if k.endswith(".jpg")]))


if __name__ == "__main__":
    main()
