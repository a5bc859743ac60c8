"""Writes tests/golden/d1_device_entropy.npz: the restart and long-code cases the device-side Huffman decode
(DeviceJpegDecoder(entropy="device"), editor_jpeg_plan / editor_jpeg_entropy_segments / editor_jpeg_entropy_device) needs beyond
what f14_decode.npz and r1_ragged_jpeg.npz already hold, Pillow-encoded from seeded images, with PILLOW'S decoded pixels:
    a restart interval of ONE MCU (every MCU its own segment; 12 MCUs, so the RSTn index wraps past D7),
    a restart interval that does not divide the MCU count (short last segment),
    grayscale with restarts,
    a quality-100 noise image with optimised tables (codes longer than the 9-bit lookahead, dense FF 00 stuffing),
and two corrupted variants whose HOST result (editor_jpeg_entropy_decode of the built library) is recorded beside them:
    bitflip.jpg   the short-last-segment file with ONE bit of its entropy data flipped, the first flip (searched from the start of
                  the data) that keeps the file device-eligible and makes the host decoder return EDITOR_JPEG_CORRUPT
    trunc.jpg     the noise file cut in the middle of its entropy data; trunc.rc / trunc.coef: what the host decoder returns
Run in the build container (Pillow 12.2.0, libjpeg-turbo) after `python -m editor_amd.build`:
    python tests/golden/capture_device_entropy.py"""
import ctypes
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CASES = [  # (name, W, H, subsampling | 'gray' | 'noise', quality, extra save options)
    ("r1mcu_420_56x40", 56, 40, 2, 80, dict(restart_marker_blocks=1)),          # 4 x 3 MCUs, 11 markers
    ("shortlast_444_41x23", 41, 23, 0, 85, dict(restart_marker_blocks=4)),      # 6 x 3 MCUs: 4 + 4 + 4 + 4 + 2
    ("gray_restart_45x37", 45, 37, "gray", 80, dict(restart_marker_blocks=4)),  # 6 x 5 MCUs: 7 x 4 + 2
    ("noise_444_q100_opt_48x32", 48, 32, "noise", 100, dict(optimize=True)),
]


def synth(rng, w, h, kind):
    if kind == "noise":
        return Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 17.0) * np.cos(yy / 11.0), 128 + 90 * np.cos(xx / 29.0 + yy / 7.0),
                     255.0 * (xx + yy) / (w + h)], axis=2)
    base += rng.normal(0, 25, base.shape)
    a = np.clip(base, 0, 255).astype(np.uint8)
    return Image.fromarray(a[..., 0] if kind == "gray" else a)


def host(data):
    """-> (rc, coef, eligible, first segment's [start, end)) of the built library's host decoder and planner."""
    from editor_amd import _lib
    cd = _lib.lib().cdll
    buf = np.frombuffer(data, dtype=np.uint8)
    info, plan = np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.int32)
    qt, huff, seg = np.zeros((3, 64), dtype=np.uint16), np.zeros((8, 272), dtype=np.uint8), np.zeros((256, 3), dtype=np.int64)
    rc = cd.editor_jpeg_plan(ctypes.c_void_p(buf.ctypes.data), buf.size, ctypes.c_void_p(info.ctypes.data), ctypes.c_void_p(plan.ctypes.data),
                             ctypes.c_void_p(qt.ctypes.data), ctypes.c_void_p(huff.ctypes.data), ctypes.c_void_p(seg.ctypes.data), 256)
    if rc:
        return rc, None, False, None
    coef = np.zeros((int(info[8]), 64), dtype=np.int16)
    rc = cd.editor_jpeg_entropy_decode(ctypes.c_void_p(buf.ctypes.data), buf.size, ctypes.c_void_p(coef.ctypes.data),
                                       ctypes.c_long(int(info[8])), ctypes.c_void_p(qt.ctypes.data), ctypes.c_void_p(info.ctypes.data))
    return rc, coef, bool(plan[0]), (int(seg[0, 0]), int(seg[int(plan[1]) - 1, 1]))


def main():
    rng = np.random.default_rng(41)
    out = {}
    for name, w, h, ss, q, kw in CASES:
        im = synth(rng, w, h, ss)
        bio = io.BytesIO()
        if ss == "gray":
            im.save(bio, "JPEG", quality=q, **kw)
        else:
            im.save(bio, "JPEG", quality=q, subsampling=0 if ss == "noise" else ss, **kw)
        data = bio.getvalue()
        out[name + ".jpg"] = np.frombuffer(data, dtype=np.uint8)
        out[name + ".rgb"] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        rc, _, eligible, _ = host(data)
        assert rc == 0 and eligible, (name, rc, eligible)
    # bit flip: first one (from the start of the entropy data) after which the file is still eligible and the host says CORRUPT
    data = out["shortlast_444_41x23.jpg"].tobytes()
    a, b = host(data)[3]
    found = None
    for bit in range(8 * a, 8 * b):
        bad = bytearray(data)
        bad[bit // 8] ^= 0x80 >> (bit % 8)
        rc, _, eligible, _ = host(bytes(bad))
        if rc == 9001 and eligible:
            found = bytes(bad)
            break
    assert found is not None
    out["bitflip.jpg"] = np.frombuffer(found, dtype=np.uint8)
    # truncation in the middle of the entropy data (no restart interval: still one segment, which now ends at the cut)
    data = out["noise_444_q100_opt_48x32.jpg"].tobytes()
    a, b = host(data)[3]
    cut = data[:(a + b) // 2]
    rc, coef, eligible, _ = host(cut)
    assert eligible and rc in (0, 9001)
    out["trunc.jpg"] = np.frombuffer(cut, dtype=np.uint8)
    out["trunc.rc"] = np.asarray(rc, dtype=np.int32)
    out["trunc.coef"] = coef
    path = os.path.join(HERE, "d1_device_entropy.npz")
    np.savez_compressed(path, **out)
    print("wrote d1_device_entropy.npz: %d bytes; bit flip at byte %d; cut at %d (rc %d)"
          % (os.path.getsize(path), [i for i in range(len(found)) if found[i] != out["shortlast_444_41x23.jpg"][i]][0], len(cut), rc))
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
