"""Row N3 on the device for the separate-file sample layout (RGBNT201 / MSVR310: one detector crop of any size per modality,
data/datasets/bases.py:22-30): DeviceJpegDecoder.decode_ragged (editor_jpeg_reconstruct_ragged: one IDCT launch + one colour
launch for a batch of mixed sizes / sampling factors) and DeviceResize on RaggedImages (editor_resize_u8_ragged: two launches)
against Pillow's own pixels (tests/golden/r1_ragged_jpeg.npz) and Pillow's own resize - bit for bit - and against the uniform
entries on batches both can take."""
import os
import random

import numpy as np
import pytest
import torch

from ragged_helpers import INTERPOLATIONS, TARGETS, fixture

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _check_ragged(rag, names, rgb):
    assert len(rag) == len(names)
    assert rag.sizes.dtype == torch.int32 and rag.offsets.dtype == torch.int64 and tuple(rag.offsets.shape) == (len(names) + 1,)
    assert rag.data.is_cuda and rag.data.dtype == torch.uint8 and rag.data.dim() == 1
    off = 0
    for i, n in enumerate(names):
        h, w = rgb[n].shape[:2]
        assert (int(rag.sizes[i, 0]), int(rag.sizes[i, 1])) == (h, w) and int(rag.offsets[i]) == off, n
        off += h * w * 3
    assert int(rag.offsets[-1]) == off == rag.data.numel()
    host = rag.data.cpu().numpy()                                         # one D2H copy; image(i) is checked to view the same bytes
    for i, n in enumerate(names):
        lo, hi = int(rag.offsets[i]), int(rag.offsets[i + 1])
        assert np.array_equal(host[lo:hi].reshape(rgb[n].shape), rgb[n]), n
    first = rag.image(0)
    assert tuple(first.shape) == rgb[names[0]].shape and first.data_ptr() == rag.data.data_ptr()
    assert np.array_equal(rag.image(len(names) - 1).cpu().numpy(), rgb[names[-1]])


def test_decode_ragged_equals_pillow_whole_batch_and_reversed():
    from editor_amd.data import DeviceJpegDecoder
    names, jpg, rgb = fixture()
    dec = DeviceJpegDecoder(crop_w=0, threads=4)
    for order in (names, names[::-1]):                                    # (the second call reuses the staging buffer)
        _check_ragged(dec.decode_ragged([jpg[n] for n in order], "cuda"), order, rgb)


def test_decode_ragged_each_file_alone():
    from editor_amd.data import DeviceJpegDecoder
    names, jpg, rgb = fixture()
    dec = DeviceJpegDecoder(crop_w=0, threads=2)
    for n in names:
        _check_ragged(dec.decode_ragged([jpg[n]], "cuda"), [n], rgb)


def test_same_size_batch_equals_the_uniform_decoder():
    from editor_amd.data import DeviceJpegDecoder
    g = np.load(os.path.join(HERE, "golden", "f14_decode.npz"))
    files = [g[n + ".jpg"].tobytes() for n in ("stitched_420_q75", "stitched_444_q90", "stitched_422_q85")]
    dec = DeviceJpegDecoder(crop_w=0)
    dense = dec(files, "cuda")                                            # (1, 3, 128, 768, 3)
    rag = dec.decode_ragged(files, "cuda")
    assert rag.sizes.tolist() == [[128, 768]] * 3
    assert torch.equal(rag.data.view(3, 128, 768, 3), dense[0])


@pytest.mark.parametrize("interpolation", INTERPOLATIONS)
@pytest.mark.parametrize("size", TARGETS)
def test_ragged_resize_equals_pillow(size, interpolation):
    """Independent of the decoder: Pillow's stored pixels in, Pillow's resize of the same arrays expected.  The batch holds the
    copy cases (an extent that already equals its target) and images upscaled in both axes."""
    from PIL import Image
    from editor_amd.data import DeviceResize, RaggedImages
    names, _, rgb = fixture()
    rag = RaggedImages.from_arrays([rgb[n] for n in names], "cuda")
    assert np.array_equal(rag.image(5).cpu().numpy(), rgb[names[5]])
    rs = DeviceResize(size, interpolation)
    out = rs(rag)
    assert tuple(out.shape) == (len(names),) + tuple(size) + (3,) and out.dtype == torch.uint8
    got = out.cpu().numpy()
    for i, n in enumerate(names):
        want = np.asarray(Image.fromarray(rgb[n]).resize((size[1], size[0]), resample=interpolation))
        assert np.array_equal(got[i], want), (n, size, interpolation)
    got2 = rs(RaggedImages.from_arrays([rgb[n] for n in names[::-1]], "cuda")).cpu().numpy()      # cached tables, other order
    assert np.array_equal(got2, got[::-1])


def test_uniform_batch_through_the_ragged_entry_equals_the_dense_entry():
    from editor_amd.data import DeviceResize, RaggedImages
    rng = np.random.default_rng(9)
    for (h, w), size, ip in (((131, 250), (256, 128), 3), ((77, 61), (128, 256), 2), ((256, 300), (256, 128), 3)):
        batch = rng.integers(0, 256, (5, h, w, 3), dtype=np.uint8)
        rs = DeviceResize(size, ip)
        dense = rs(torch.from_numpy(batch).cuda())
        ragged = rs(RaggedImages.from_arrays(list(batch), "cuda"))
        assert torch.equal(ragged, dense), (h, w, size, ip)


def test_load_modalities_into_the_train_transform_equals_the_pillow_chain():
    """Bytes of three modalities -> load_modalities -> DeviceTrainTransform with fixed draws == oracle.augment_ref.train_transform of
    the Pillow-decoded, Pillow-resized images.  Exact equality: every stage is integer or single fp32 operations, the comparison
    test_input_pipeline.py makes for the transform alone (torch.equal)."""
    from PIL import Image
    from editor_amd import synth
    from editor_amd.data import DeviceTrainTransform, load_modalities
    from oracle import augment_ref
    names, jpg, rgb = fixture()
    groups = [names[0:5], names[5:10], names[9:14]]
    size = (256, 128)
    got = load_modalities([[jpg[n] for n in grp] for grp in groups], size, 3, "cuda")
    assert len(got) == 3
    tf = DeviceTrainTransform(size, prob=0.5, padding=10, re_prob=0.5)
    random.seed(3)
    torch.manual_seed(3)
    params = tf.draw(5)
    noise = synth.normal(5, "ragged/noise", (5, 3) + size, 1.0)
    for grp, x in zip(groups, got):
        assert tuple(x.shape) == (5,) + size + (3,)
        pil = np.stack([np.asarray(Image.fromarray(rgb[n]).resize((size[1], size[0]), resample=3)) for n in grp])
        ref = augment_ref.train_transform(torch.from_numpy(pil), params, 10, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), noise)
        out = tf(x, params, noise.cuda())
        assert torch.equal(out.cpu(), ref), grp


def test_refusals_before_any_launch():
    from editor_amd.data import DeviceJpegDecoder, DeviceResize, RaggedImages, load_modalities
    names, jpg, rgb = fixture()
    dec = DeviceJpegDecoder(crop_w=0)
    bad = bytearray(jpg[names[1]])
    bad[bad.index(b"\xff\xc0") + 1] = 0xC9                                # arithmetic-coded sequential: unsupported
    with pytest.raises(ValueError, match="file 1 of the batch"):
        dec.decode_ragged([jpg[names[0]], bytes(bad), jpg[names[2]]], "cuda")
    with pytest.raises(ValueError):
        dec.decode_ragged([], "cuda")
    with pytest.raises(RuntimeError):
        dec.decode_ragged([jpg[names[0]]], "cpu")
    with pytest.raises(ValueError):
        dec([jpg[names[0]], jpg[names[1]]], "cuda")                       # the uniform call still refuses mixed sizes
    with pytest.raises(RuntimeError):
        RaggedImages.from_arrays([rgb[names[0]]], "cpu")
    with pytest.raises(ValueError):
        RaggedImages.from_arrays([], "cuda")
    cpu = RaggedImages(torch.zeros(27, dtype=torch.uint8), torch.tensor([0, 27]), torch.tensor([[3, 3]], dtype=torch.int32))
    with pytest.raises(RuntimeError):
        DeviceResize((256, 128))(cpu)
    with pytest.raises(ValueError):
        load_modalities([[], [], []], (256, 128), 3, "cuda")
    with pytest.raises(RuntimeError):
        load_modalities([[jpg[names[0]]]], (256, 128), 3, "cpu")
