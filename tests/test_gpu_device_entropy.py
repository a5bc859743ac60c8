"""Device-side Huffman decode of sequential JPEG scans on the GPU: editor_jpeg_entropy_device (one wave per restart segment of
the batch) against the host decoder's coefficient planes - bit for bit - and DeviceJpegDecoder(entropy="device") /
load_modalities(entropy="device") against Pillow's stored pixels and against the entropy="host" path.  The shapes are the
fixtures' own, 7x9 to 768x128; every corrupt input used here is one tests/test_device_entropy_host.py has already run through
the same routine on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import device_entropy_helpers as H
from ragged_helpers import fixture

pytestmark = pytest.mark.gpu


def device_segments(datas):
    """editor_jpeg_entropy_device over a batch, packed as the CPU tests pack it -> (status (B), coef (total blocks,64), offsets).
    The coefficient tensor starts as 0x5A5A everywhere."""
    from editor_amd._lib import call
    buf, nbytes, fdesc, ftab, segs, huff, nseg, off, total = H.packed(datas)
    dev = [torch.from_numpy(a).cuda() for a in (buf, fdesc, ftab, segs, huff)]
    coef = torch.full((total, 64), 0x5A5A, dtype=torch.int16, device="cuda")
    status = torch.full((len(datas),), -1, dtype=torch.int32, device="cuda")
    call("editor_jpeg_entropy_device", dev[0], nbytes, ctypes.c_void_p(fdesc.ctypes.data), ctypes.c_void_p(ftab.ctypes.data),
         ctypes.c_void_p(segs.ctypes.data), dev[1], dev[2], dev[3], dev[4], int(huff.shape[0]), len(datas), nseg, coef, total, status)
    return status.cpu().numpy(), coef.cpu().numpy(), off


def _check(names):
    status, coef, off = device_segments([H.files()[n] for n in names])
    assert not status.any(), status
    for n, o in zip(names, off):
        want = H.host_coef(n)
        assert np.array_equal(coef[o:o + want.shape[0]], want), n
    assert not (coef == 0x5A5A).any()


def test_coefficients_equal_host_decoder_each_file_alone():
    for n in H.eligible_names():
        _check([n])


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_coefficients_equal_host_decoder_whole_batch(order):
    names = H.eligible_names()
    _check(names if order == "forward" else names[::-1])


def test_restart_files_alone_and_in_a_mixed_batch():
    one, short, gray = "d1/r1mcu_420_56x40", "d1/shortlast_444_41x23", "d1/gray_restart_45x37"
    for n in (one, short, gray):
        _check([n])
    _check(["f14/stitched_444_q90", one, "r1/a_odd_420_7x9", short, "f14/gray_q80", gray, "f14/restart_420_q80", one])
    from editor_amd.data import DeviceJpegDecoder
    dec = DeviceJpegDecoder(crop_w=0, threads=2, entropy="device")
    mixed = [one, "r1/h_prog_420_53x47", short, "r1/c_odd_444_17x33", gray]
    rag = dec.decode_ragged([H.files()[n] for n in mixed], "cuda")
    for i, n in enumerate(mixed):
        assert np.array_equal(rag.image(i).cpu().numpy(), H.pixels(n)), n


def test_decode_ragged_device_equals_pillow_and_the_host_path():
    from editor_amd.data import DeviceJpegDecoder
    names, jpg, rgb = fixture()                                           # the whole r1 set, the progressive file included
    dev = DeviceJpegDecoder(crop_w=0, threads=4, entropy="device")
    host = DeviceJpegDecoder(crop_w=0, threads=4)
    for order in (names, names[::-1]):                                    # (the second call reuses the staging buffer)
        files = [jpg[n] for n in order]
        rag = dev.decode_ragged(files, "cuda")
        ref = host.decode_ragged(files, "cuda")
        assert torch.equal(rag.data, ref.data) and torch.equal(rag.offsets, ref.offsets) and torch.equal(rag.sizes, ref.sizes)
        for i, n in enumerate(order):
            assert np.array_equal(rag.image(i).cpu().numpy(), rgb[n]), n
    assert dev.last_h2d_bytes < host.last_h2d_bytes                       # compressed bytes cross the bus, not int16 blocks


def test_uniform_call_device_equals_the_goldens():
    from editor_amd.data import DeviceJpegDecoder
    names = ["stitched_420_q75", "stitched_444_q90", "stitched_422_q85", "stitched_420_q75"]      # mixed sampling: three groups
    files = [H.files()["f14/" + n] for n in names]
    crops = DeviceJpegDecoder(crop_w=256, entropy="device")(files, "cuda")
    assert tuple(crops.shape) == (3, 4, 128, 256, 3)
    for b, n in enumerate(names):
        want = H.pixels("f14/" + n)
        for i in range(3):
            assert np.array_equal(crops[i, b].cpu().numpy(), want[:, 256 * i:256 * (i + 1)]), (n, i)
    assert torch.equal(crops, DeviceJpegDecoder(crop_w=256)(files, "cuda"))
    # one geometry, one file: the B = 1 form
    one = DeviceJpegDecoder(crop_w=0, entropy="device")([H.files()["f14/odd_422_q95"]], "cuda")
    assert np.array_equal(one[0, 0].cpu().numpy(), H.pixels("f14/odd_422_q95"))


def test_load_modalities_device_equals_host():
    from editor_amd.data import load_modalities
    names, jpg, _ = fixture()
    groups = [[jpg[n] for n in names[0:4]], [jpg[n] for n in names[4:8]], [jpg[n] for n in names[8:12]]]
    want = load_modalities(groups, (64, 32), 3, "cuda")
    got = load_modalities(groups, (64, 32), 3, "cuda", entropy="device")
    assert len(got) == 3
    for g, w in zip(got, want):
        assert tuple(g.shape) == (4, 64, 32, 3) and torch.equal(g, w)


def test_status_names_the_corrupt_file_and_truncation_matches_the_recording():
    from editor_amd.data import DeviceJpegDecoder
    z = H.d1()
    flip, trunc = z["bitflip.jpg"].tobytes(), z["trunc.jpg"].tobytes()
    good = H.files()["d1/r1mcu_420_56x40"]
    status, coef, off = device_segments([good, flip, trunc])
    assert status.tolist() == [0, 9001, int(z["trunc.rc"])]
    assert np.array_equal(coef[:off[1]], H.host_coef("d1/r1mcu_420_56x40"))
    assert not (coef == 0x5A5A).any()
    if int(z["trunc.rc"]) == 0:
        assert np.array_equal(coef[off[2]:], z["trunc.coef"])
    dec = DeviceJpegDecoder(crop_w=0, threads=2, entropy="device")
    with pytest.raises(ValueError, match=r"file 2 of the batch: JPEG entropy decode failed \(rc 9001\)"):
        dec.decode_ragged([good, good, flip, good], "cuda")
    with pytest.raises(ValueError, match=r"file 1 of the batch: JPEG entropy decode failed \(rc 9001\)"):
        dec([z["shortlast_444_41x23.jpg"].tobytes(), flip], "cuda")
    # a file the parser refuses is refused before anything is launched, by index, with the host path's text
    with pytest.raises(ValueError, match=r"file 1 of the batch: JPEG is corrupt or incomplete \(editor_jpeg_parse rc 9001\)"):
        dec.decode_ragged([good, b"not a jpeg at all"], "cuda")
