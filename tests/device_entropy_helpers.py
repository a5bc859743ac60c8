"""Shared by tests/test_device_entropy_host.py and tests/test_gpu_device_entropy.py: every JPEG file of the committed fixtures
(f14_decode.npz, r1_ragged_jpeg.npz, d1_device_entropy.npz), the host decoder as the definition of correct, and thin wrappers
of the planner (editor_jpeg_plan) and the host twin of the segment decoder (editor_jpeg_entropy_segments)."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PROGRESSIVE = ("f14/progressive", "r1/h_prog_420_53x47")
_CACHE = {}


def d1():
    if "d1" not in _CACHE:
        _CACHE["d1"] = np.load(os.path.join(HERE, "golden", "d1_device_entropy.npz"))
    return _CACHE["d1"]


def files():
    """-> {"<fixture>/<name>": bytes} of all 28 files (26 device-eligible, the 2 of PROGRESSIVE not); loaded once."""
    if "files" not in _CACHE:
        out = {}
        for tag, fn in (("f14", "f14_decode.npz"), ("r1", "r1_ragged_jpeg.npz"), ("d1", "d1_device_entropy.npz")):
            z = np.load(os.path.join(HERE, "golden", fn))
            for k in sorted(z.files):
                if k.endswith(".jpg") and k not in ("bitflip.jpg", "trunc.jpg"):
                    out[tag + "/" + k[:-4]] = z[k].tobytes()
        _CACHE["files"] = out
    return _CACHE["files"]


def eligible_names():
    return [n for n in files() if n not in PROGRESSIVE]


def pixels(name):
    tag, k = name.split("/")
    fn = {"f14": "f14_decode.npz", "r1": "r1_ragged_jpeg.npz", "d1": "d1_device_entropy.npz"}[tag]
    return np.load(os.path.join(HERE, "golden", fn))[k + ".rgb"]


def cdll():
    from editor_amd import _lib
    return _lib.lib().cdll


def host_decode(data):
    """-> (rc, coef (blocks,64) int16 | None) of editor_jpeg_parse + editor_jpeg_entropy_decode into a zero-filled buffer."""
    cd = cdll()
    buf = np.frombuffer(data, dtype=np.uint8)
    info = np.zeros(16, dtype=np.int32)
    rc = cd.editor_jpeg_parse(ctypes.c_void_p(buf.ctypes.data), buf.size, ctypes.c_void_p(info.ctypes.data))
    if rc:
        return rc, None
    coef = np.zeros((int(info[8]), 64), dtype=np.int16)
    qt = np.zeros((3, 64), dtype=np.uint16)
    rc = cd.editor_jpeg_entropy_decode(ctypes.c_void_p(buf.ctypes.data), buf.size, ctypes.c_void_p(coef.ctypes.data),
                                       ctypes.c_long(int(info[8])), ctypes.c_void_p(qt.ctypes.data), ctypes.c_void_p(info.ctypes.data))
    return rc, coef


def host_coef(name):
    """The host decoder's coefficients of a fixture file: computed once, shared, read-only."""
    key = ("coef", name)
    if key not in _CACHE:
        rc, coef = host_decode(files()[name])
        assert rc == 0, (name, rc)
        coef.setflags(write=False)
        _CACHE[key] = coef
    return _CACHE[key]


def plan(data, cap=4096):
    """-> (rc, info, plan, qt, huff, seg rows written) of editor_jpeg_plan."""
    buf = np.frombuffer(data, dtype=np.uint8)
    info, pl = np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.int32)
    qt, huff, seg = np.zeros((3, 64), dtype=np.uint16), np.zeros((8, 272), dtype=np.uint8), np.zeros((cap, 3), dtype=np.int64)
    rc = cdll().editor_jpeg_plan(ctypes.c_void_p(buf.ctypes.data), buf.size, ctypes.c_void_p(info.ctypes.data), ctypes.c_void_p(pl.ctypes.data),
                                 ctypes.c_void_p(qt.ctypes.data), ctypes.c_void_p(huff.ctypes.data), ctypes.c_void_p(seg.ctypes.data), cap)
    return rc, info, pl, qt, huff, seg[:min(cap, int(pl[1]))]


def decoder():
    if "dec" not in _CACHE:
        from editor_amd.data import DeviceJpegDecoder
        _CACHE["dec"] = DeviceJpegDecoder(crop_w=0, threads=2, entropy="device")
    return _CACHE["dec"]


def packed(datas):
    """A batch of (eligible) files planned and packed as the device path packs it, file i's blocks after file i - 1's.
    -> (bytes buffer, nbytes, fdesc, ftab, segs, huff, nseg, block offsets, total blocks)"""
    dec = decoder()
    bp = dec.plan_batch(datas)
    blocks = bp.infos[:, 8].astype(np.int64)
    off = np.cumsum(blocks) - blocks
    nbytes, spans, fdesc, ftab, segs, huff, nseg = dec.pack_batch(datas, bp, off)
    buf = np.full(nbytes, 0xA5, dtype=np.uint8)                  # (the 16-byte padding between files is never decoded)
    for i, at, s0, e1 in spans:
        buf[at:at + e1 - s0] = np.frombuffer(datas[i], dtype=np.uint8)[s0:e1]
    return buf, nbytes, fdesc, ftab, segs, huff, nseg, off, int(blocks.sum())


def host_segments(datas):
    """editor_jpeg_entropy_segments over a batch -> (rc, status (B) int32, coef (total blocks,64) int16, block offsets).
    The buffer starts as 0x5A5A everywhere: what comes back zero was written."""
    buf, nbytes, fdesc, ftab, segs, huff, nseg, off, total = packed(datas)
    coef = np.full((total, 64), 0x5A5A, dtype=np.int16)
    status = np.full(len(datas), -1, dtype=np.int32)
    rc = cdll().editor_jpeg_entropy_segments(ctypes.c_void_p(buf.ctypes.data), nbytes, ctypes.c_void_p(fdesc.ctypes.data),
                                             ctypes.c_void_p(ftab.ctypes.data), ctypes.c_void_p(segs.ctypes.data), ctypes.c_void_p(huff.ctypes.data),
                                             int(huff.shape[0]), len(datas), nseg, ctypes.c_void_p(coef.ctypes.data), total,
                                             ctypes.c_void_p(status.ctypes.data))
    return rc, status, coef, off
