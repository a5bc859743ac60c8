"""In-segment parallel Huffman decode on the GPU: editor_jpeg_entropy_split_device (one 256-thread workgroup per restart segment,
one lane per sub_bytes of it, chunk after chunk) against the host decoder's coefficient planes - bit for bit - and
DeviceJpegDecoder(entropy="device_split") / load_modalities(entropy="device_split") against Pillow's stored pixels and against
entropy="device".  Fixtures only; every input used here is one tests/test_device_entropy_split_host.py has already run through the
same routines on the CPU, and the statistics the kernel leaves (rounds, chunks per segment) must equal the host twin's."""
import ctypes

import numpy as np
import pytest
import torch

import device_entropy_helpers as H
import device_entropy_split_helpers as S
from ragged_helpers import fixture

pytestmark = pytest.mark.gpu

LONGEST = "f14/stitched_444_q90"
MANY = "d1/r1mcu_420_56x40"


def split_device(datas, sub):
    """editor_jpeg_entropy_split_device over a batch, packed as the CPU tests pack it -> (status (B), coef (total blocks,64),
    offsets, stats (nseg,2)).  The coefficient tensor starts as 0x5A5A everywhere."""
    from editor_amd._lib import call
    buf, nbytes, fdesc, ftab, segs, huff, nseg, off, total = H.packed(datas)
    dev = [torch.from_numpy(a).cuda() for a in (buf, fdesc, ftab, segs, huff)]
    coef = torch.full((total, 64), 0x5A5A, dtype=torch.int16, device="cuda")
    status = torch.full((len(datas),), -1, dtype=torch.int32, device="cuda")
    rc, need = S.workspace(nseg, sub)
    assert rc == 0
    ws = torch.full((need // 8,), -1, dtype=torch.int64, device="cuda")
    call("editor_jpeg_entropy_split_device", dev[0], nbytes, ctypes.c_void_p(fdesc.ctypes.data), ctypes.c_void_p(ftab.ctypes.data),
         ctypes.c_void_p(segs.ctypes.data), dev[1], dev[2], dev[3], dev[4], int(huff.shape[0]), len(datas), nseg, sub, ws, need, coef, total,
         status)
    return status.cpu().numpy(), coef.cpu().numpy(), off, ws[:2 * nseg].cpu().numpy().reshape(nseg, 2)


def _check(names, sub):
    datas = [S.files()[n] for n in names]
    status, coef, off, stats = split_device(datas, sub)
    assert not status.any(), status
    for n, o in zip(names, off):
        want = S.host_coef(n)
        assert np.array_equal(coef[o:o + want.shape[0]], want), (n, sub)
    assert not (coef == 0x5A5A).any()
    assert np.array_equal(stats, S.split_segments(datas, sub)[4])          # the same rounds and chunks as the host twin
    return stats


@pytest.mark.parametrize("sub", [16, "default"])
@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_coefficients_equal_host_decoder_whole_batch(order, sub):
    names = list(S.files())
    assert len(names) == 29
    _check(names if order == "forward" else names[::-1], S.sub_bytes(sub))


@pytest.mark.parametrize("sub", [16, "default"])
def test_the_118_kb_file_spans_several_chunks_of_one_workgroup(sub):
    sub = S.sub_bytes(sub)
    seg, _ = S.segments(LONGEST)
    length = int(seg[0, 1] - seg[0, 0])
    assert len(seg) == 1 and length > 118000
    chunks = -(-length // (256 * sub))                                     # 256 lanes x sub_bytes per chunk
    assert chunks >= 4 and (sub != 16 or chunks == 29)
    stats = _check([MANY, LONGEST, "r1/a_odd_420_7x9", "d2/tinyseg_gray_64x24", "f14/gray_q80"], sub)
    assert stats[12, 1] == chunks and stats[12, 0] >= 2 * chunks, stats[12]      # (after the 12 segments of MANY)
    _check([LONGEST], sub)


def test_short_files_each_alone():
    for n in ("r1/a_odd_420_7x9", "r1/e_mcu_444_8x8", "d2/exact128_420_72x56", "d2/plus1_444_40x48", "d2/tinyseg_gray_64x24", "f14/odd_422_q95",
              "d1/noise_444_q100_opt_48x32"):
        for sub in (16, S.sub_bytes("default"), 128):
            _check([n], sub)


def test_decode_ragged_split_equals_pillow_and_the_device_path():
    from editor_amd.data import DeviceJpegDecoder
    names, jpg, rgb = fixture()                                           # the whole r1 set, the progressive file included
    split = DeviceJpegDecoder(crop_w=0, threads=4, entropy="device_split")
    dev = DeviceJpegDecoder(crop_w=0, threads=4, entropy="device")
    for order in (names, names[::-1]):                                    # (the second call reuses the staging buffer)
        files = [jpg[n] for n in order]
        rag = split.decode_ragged(files, "cuda")
        ref = dev.decode_ragged(files, "cuda")
        assert torch.equal(rag.data, ref.data) and torch.equal(rag.offsets, ref.offsets) and torch.equal(rag.sizes, ref.sizes)
        for i, n in enumerate(order):
            assert np.array_equal(rag.image(i).cpu().numpy(), rgb[n]), n
    assert split.last_h2d_bytes == dev.last_h2d_bytes                     # the same single upload
    # both progressive files are routed to the host as before, beside the new fixture's files and the longest one
    mixed = ["d2/tinyseg_gray_64x24", "f14/progressive", LONGEST, "r1/h_prog_420_53x47", "d2/plus1_444_40x48", "d2/exact128_420_72x56", MANY]
    datas = [H.files()[n] if n in H.files() else S.files()[n] for n in mixed]
    bp = split.plan_batch(datas)
    assert bp.plans[:, 0].tolist() == [1, 0, 1, 0, 1, 1, 1]
    ref = dev.decode_ragged(datas, "cuda")
    for sub in (16, None):
        dec = DeviceJpegDecoder(crop_w=0, threads=2, entropy="device_split", split_sub_bytes=sub)
        rag = dec.decode_ragged(datas, "cuda")
        assert torch.equal(rag.data, ref.data) and torch.equal(rag.offsets, ref.offsets) and torch.equal(rag.sizes, ref.sizes)
        for i, n in enumerate(mixed):
            if n != "f14/progressive":                                    # (no Pillow pixels are stored for that one)
                want = H.pixels(n) if n in H.files() else S.pixels(n)
                assert np.array_equal(rag.image(i).cpu().numpy(), want), (n, sub)


def test_uniform_call_split_equals_the_goldens():
    from editor_amd.data import DeviceJpegDecoder
    names = ["stitched_420_q75", "stitched_444_q90", "stitched_422_q85", "stitched_420_q75"]      # mixed sampling: three groups
    files = [H.files()["f14/" + n] for n in names]
    crops = DeviceJpegDecoder(crop_w=256, entropy="device_split")(files, "cuda")
    assert tuple(crops.shape) == (3, 4, 128, 256, 3)
    for b, n in enumerate(names):
        want = H.pixels("f14/" + n)
        for i in range(3):
            assert np.array_equal(crops[i, b].cpu().numpy(), want[:, 256 * i:256 * (i + 1)]), (n, i)
    assert torch.equal(crops, DeviceJpegDecoder(crop_w=256, entropy="device")(files, "cuda"))


def test_load_modalities_split_equals_device():
    from editor_amd.data import load_modalities
    names, jpg, _ = fixture()
    groups = [[jpg[n] for n in names[0:4]], [jpg[n] for n in names[4:8]], [jpg[n] for n in names[8:12]]]
    want = load_modalities(groups, (64, 32), 3, "cuda", entropy="device")
    got = load_modalities(groups, (64, 32), 3, "cuda", entropy="device_split")
    assert len(got) == 3
    for g, w in zip(got, want):
        assert tuple(g.shape) == (4, 64, 32, 3) and torch.equal(g, w)


def test_status_names_the_corrupt_file_and_truncation_matches_the_recording():
    from editor_amd.data import DeviceJpegDecoder
    z = H.d1()
    flip, trunc = z["bitflip.jpg"].tobytes(), z["trunc.jpg"].tobytes()
    good = H.files()[MANY]
    for sub in (16, S.sub_bytes("default")):
        status, coef, off, _ = split_device([good, flip, trunc], sub)
        assert status.tolist() == [0, 9001, int(z["trunc.rc"])]
        assert np.array_equal(coef[:off[1]], H.host_coef(MANY))
        assert not (coef == 0x5A5A).any()
        if int(z["trunc.rc"]) == 0:
            assert np.array_equal(coef[off[2]:], z["trunc.coef"])
    dec = DeviceJpegDecoder(crop_w=0, threads=2, entropy="device_split")
    with pytest.raises(ValueError, match=r"file 2 of the batch: JPEG entropy decode failed \(rc 9001\)"):
        dec.decode_ragged([good, good, flip, good], "cuda")
    with pytest.raises(ValueError, match=r"file 1 of the batch: JPEG entropy decode failed \(rc 9001\)"):
        dec([z["shortlast_444_41x23.jpg"].tobytes(), flip], "cuda")
    with pytest.raises(ValueError, match=r"file 1 of the batch: JPEG is corrupt or incomplete \(editor_jpeg_parse rc 9001\)"):
        dec.decode_ragged([good, b"not a jpeg at all"], "cuda")
