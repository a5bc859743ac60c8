"""DeviceJpegDecoder's one pipeline (describe the batch, fill the coefficients, reconstruct) at the shapes where its shared
staging can go wrong: host-routed files apart and adjacent in the coefficient tensor, batches no entropy kernel runs for, B = 1 -
stitched (__call__) and ragged (decode_ragged), entropy = host / device / device_split.  Fixture files only; every comparison is
exact, against Pillow's stored pixels and between the modes.  The corrupt inputs are ones tests/test_device_entropy_host.py and
tests/test_gpu_device_entropy.py already decode to a clean status."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ["host", "device", "device_split"]
TAGS = {"f14": "f14_decode.npz", "f15": "f15_decode_progressive.npz", "r1": "r1_ragged_jpeg.npz", "d1": "d1_device_entropy.npz",
        "d2": "d2_entropy_split.npz"}
_CACHE = {}


def _npz(tag):
    if tag not in _CACHE:
        _CACHE[tag] = np.load(os.path.join(HERE, "golden", TAGS[tag]))
    return _CACHE[tag]


def jpg(name):
    tag, k = name.split("/")
    return _npz(tag)[k + ".jpg"].tobytes()


def rgb(name):
    """Pillow's pixels of a fixture file: loaded once, shared, read-only."""
    if name not in _CACHE:
        tag, k = name.split("/")
        a = _npz(tag)[k + ".rgb"]
        a.setflags(write=False)
        _CACHE[name] = a
    return _CACHE[name]


def decoder(mode, crop_w):
    from editor_amd.data import DeviceJpegDecoder
    return DeviceJpegDecoder(crop_w=crop_w, threads=2, entropy=mode)


def check_stitched(dec, names, crop_w=256):
    crops = dec([jpg(n) for n in names], "cuda")
    cw = crop_w if crop_w > 0 else rgb(names[0]).shape[1]
    h, w = rgb(names[0]).shape[:2]
    assert tuple(crops.shape) == (w // cw, len(names), h, cw, 3)
    got = crops.cpu().numpy()
    for b, n in enumerate(names):
        for i in range(w // cw):
            assert np.array_equal(got[i, b], rgb(n)[:, cw * i:cw * (i + 1)]), (n, i)
    return crops


def check_ragged(dec, names):
    rag = dec.decode_ragged([jpg(n) for n in names], "cuda")
    assert len(rag) == len(names)
    for i, n in enumerate(names):
        assert np.array_equal(rag.image(i).cpu().numpy(), rgb(n)), n
    return rag


BASE, PROG, B444 = "f14/stitched_420_q75", "f15/prog_stitched_420_q75", "f14/stitched_444_q90"


def test_stitched_host_routed_files_apart_and_adjacent():
    """Two geometry groups with progressive (host-routed) files inside one, between eligible files; then the progressive files
    first.  All 768x128, crop_w = 256."""
    for names in ([BASE, PROG, B444, PROG], [PROG, PROG, BASE]):
        outs = [check_stitched(decoder(m, 256), names) for m in MODES]
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


RAGGED = ["d1/r1mcu_420_56x40", "r1/h_prog_420_53x47", "f15/prog_tiny_420_q50", "d1/shortlast_444_41x23", "f15/prog_flat_444_q95",
          "d2/tinyseg_gray_64x24"]


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_ragged_host_routed_files_apart_and_adjacent(order):
    names = RAGGED if order == "forward" else RAGGED[::-1]
    rags = [check_ragged(decoder(m, 0), names) for m in MODES]
    for r in rags[1:]:
        assert torch.equal(r.data, rags[0].data) and torch.equal(r.offsets, rags[0].offsets) and torch.equal(r.sizes, rags[0].sizes)


@pytest.mark.parametrize("mode", ["device", "device_split"])
def test_batch_with_no_device_eligible_file(mode):
    """Only progressive files: no segment, no eligible byte, an empty table pool, no entropy kernel."""
    dec = decoder(mode, 0)
    tiny, flat = "f15/prog_tiny_420_q50", "f15/prog_flat_444_q95"
    check_ragged(dec, [tiny, flat])
    check_ragged(dec, [tiny])
    check_ragged(dec, [flat])
    check_stitched(dec, [PROG], crop_w=0)
    check_ragged(dec, ["d2/plus1_444_40x48", tiny])                     # (and the same decoder goes on to an eligible file)


@pytest.mark.parametrize("mode", MODES)
def test_one_eligible_file(mode):
    dec = decoder(mode, 0)
    check_ragged(dec, ["d2/plus1_444_40x48"])
    check_stitched(dec, ["f14/odd_422_q95"], crop_w=0)


def test_stitched_host_path_names_the_file():
    """The host-mode mirrors of tests/test_gpu_device_entropy.py's error cases; the decoder's staging buffer and its event
    survive a raise."""
    dec = decoder("host", 0)
    short = "d1/shortlast_444_41x23"
    flip = _npz("d1")["bitflip.jpg"].tobytes()
    with pytest.raises(ValueError, match=r"file 1 of the batch: JPEG is corrupt or incomplete \(editor_jpeg_parse rc 9001\)"):
        dec([jpg(short), b"not a jpeg at all"], "cuda")
    check_stitched(dec, [short, short], crop_w=0)
    with pytest.raises(ValueError, match=r"file 1 of the batch: JPEG entropy decode failed \(rc 9001\)"):
        dec([jpg(short), flip], "cuda")
    check_stitched(dec, [short, short], crop_w=0)
