"""Shared by tests/test_device_entropy_split_host.py and tests/test_gpu_device_entropy_split.py: the fixture files of
device_entropy_helpers plus those of d2_entropy_split.npz, the subsequence boundaries of a planned file, and a thin wrapper of the
host twin of the in-segment parallel decoder (editor_jpeg_entropy_split_segments)."""
import ctypes
import os

import numpy as np

import device_entropy_helpers as H

SUBS = (16, 32, 64, "default")
_CACHE = {}


def sub_bytes(sub):
    if sub == "default":
        from editor_amd.data import DeviceJpegDecoder
        return DeviceJpegDecoder.SPLIT_SUB_BYTES
    return sub


def d2():
    if "d2" not in _CACHE:
        _CACHE["d2"] = np.load(os.path.join(H.HERE, "golden", "d2_entropy_split.npz"))
    return _CACHE["d2"]


def files():
    """-> {"<fixture>/<name>": bytes}: the 26 device-eligible files of device_entropy_helpers and the 3 of d2"""
    if "files" not in _CACHE:
        out = {n: H.files()[n] for n in H.eligible_names()}
        for k in sorted(d2().files):
            if k.endswith(".jpg"):
                out["d2/" + k[:-4]] = d2()[k].tobytes()
        _CACHE["files"] = out
    return _CACHE["files"]


def pixels(name):
    tag, k = name.split("/")
    return d2()[k + ".rgb"] if tag == "d2" else H.pixels(name)


def host_coef(name):
    """The host decoder's coefficients of a file of files(): computed once, shared, read-only."""
    if not name.startswith("d2/"):
        return H.host_coef(name)
    key = ("coef", name)
    if key not in _CACHE:
        rc, coef = H.host_decode(files()[name])
        assert rc == 0, (name, rc)
        coef.setflags(write=False)
        _CACHE[key] = coef
    return _CACHE[key]


def segments(name):
    """The planner's (start, end, first MCU) rows of a file and its blocks per MCU."""
    key = ("seg", name)
    if key not in _CACHE:
        rc, info, pl, _, _, seg = H.plan(files()[name])
        assert rc == 0 and pl[0] == 1, name
        bpm = 1 if info[2] == 1 else int(info[3]) * int(info[4]) + 2
        _CACHE[key] = (seg.copy(), bpm)
    return _CACHE[key]


def workspace(nseg, sub):
    n = ctypes.c_long(0)
    rc = H.cdll().editor_jpeg_entropy_split_workspace(nseg, sub, ctypes.byref(n))
    return rc, n.value


def split_segments(datas, sub):
    """editor_jpeg_entropy_split_segments over a batch -> (rc, status (B) int32, coef (total blocks,64) int16, block offsets,
    stats (nseg,2): rounds run, chunks walked).  The coefficient buffer starts as 0x5A5A everywhere, status as -1."""
    buf, nbytes, fdesc, ftab, segs, huff, nseg, off, total = H.packed(datas)
    rc, n = workspace(nseg, sub)
    assert rc == 0
    ws = np.full(n // 8, -1, dtype=np.int64)
    coef = np.full((total, 64), 0x5A5A, dtype=np.int16)
    status = np.full(len(datas), -1, dtype=np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)                 # noqa: E731
    rc = H.cdll().editor_jpeg_entropy_split_segments(p(buf), nbytes, p(fdesc), p(ftab), p(segs), p(huff), int(huff.shape[0]), len(datas), nseg,
                                                     sub, p(ws), n, p(coef), total, p(status))
    return rc, status, coef, off, ws[:2 * nseg].reshape(nseg, 2)
