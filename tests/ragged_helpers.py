"""Shared by tests/test_ragged_host.py and tests/test_gpu_ragged_input.py: the mixed-size JPEG fixture
(tests/golden/r1_ragged_jpeg.npz, Pillow-encoded files + Pillow's pixels), the host decoder, and a numpy emulation of what
editor_resize_u8_ragged does with the tap tables DeviceResize.ragged_tables builds (Pillow's 8-bit resample: accumulator seeded
with 1 << 21, clip8(acc >> 22), uint8 intermediate after the horizontal pass)."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TARGETS = [(256, 128), (128, 256), (64, 32)]                   # (Hout, Wout)
INTERPOLATIONS = [3, 2]                                        # bicubic (train transform), bilinear (val transform)
_CACHE = {}


def fixture():
    """-> (names, {name: jpeg bytes}, {name: (H, W, 3) uint8 Pillow pixels}); loaded once, never modified."""
    if "fx" not in _CACHE:
        z = np.load(os.path.join(HERE, "golden", "r1_ragged_jpeg.npz"))
        names = sorted(k[:-4] for k in z.files if k.endswith(".rgb"))
        jpg = {n: z[n + ".jpg"].tobytes() for n in names}
        rgb = {n: z[n + ".rgb"] for n in names}
        for a in rgb.values():
            a.setflags(write=False)
        _CACHE["fx"] = (names, jpg, rgb)
    return _CACHE["fx"]


def host_decode(data):
    """file bytes -> (coef (blocks,64) int16, qt (3,64) uint16, info (16) int32) by the host half of the decoder."""
    from editor_amd import _lib
    cd = _lib.lib().cdll
    buf = np.frombuffer(data, dtype=np.uint8)
    info = np.zeros(16, dtype=np.int32)
    rc = cd.editor_jpeg_parse(ctypes.c_void_p(buf.ctypes.data), buf.size, ctypes.c_void_p(info.ctypes.data))
    assert rc == 0, rc
    coef = np.zeros((int(info[8]), 64), dtype=np.int16)
    qt = np.zeros((3, 64), dtype=np.uint16)
    rc = cd.editor_jpeg_entropy_decode(ctypes.c_void_p(buf.ctypes.data), buf.size, ctypes.c_void_p(coef.ctypes.data),
                                       ctypes.c_long(int(info[8])), ctypes.c_void_p(qt.ctypes.data), ctypes.c_void_p(info.ctypes.data))
    assert rc == 0, rc
    return coef, qt, info


def _pass(a, n_out, table, ksize):
    """One pass along axis 0 of a (n_in, m, 3) uint8 array with a table laid out as bounds (n_out,2) then taps (n_out,ksize)."""
    bounds = table[:2 * n_out].reshape(n_out, 2)
    k = table[2 * n_out:2 * n_out + n_out * ksize].reshape(n_out, ksize).astype(np.int64)
    out = np.empty((n_out,) + a.shape[1:], dtype=np.uint8)
    a = a.astype(np.int64)
    for o in range(n_out):
        x0, cnt = int(bounds[o, 0]), int(bounds[o, 1])
        acc = (1 << 21) + (a[x0:x0 + cnt] * k[o, :cnt, None, None]).sum(axis=0)
        out[o] = np.clip(acc >> 22, 0, 255)
    return out


def emulate_ragged_resize(img, size, desc_row, taps):
    """img (h,w,3) uint8, size (Hout,Wout), desc_row / taps from DeviceResize.ragged_tables -> (Hout,Wout,3) uint8."""
    h, w, xoff, xks, yoff, yks = [int(v) for v in desc_row[:6]]
    assert img.shape == (h, w, 3)
    oh, ow = size
    tmp = _pass(img.transpose(1, 0, 2), ow, taps[xoff:], xks).transpose(1, 0, 2)       # horizontal: (h, Wout, 3) uint8
    return _pass(tmp, oh, taps[yoff:], yks)                                            # vertical
