"""Row N3, the separate-file sample layout (RGBNT201 / MSVR310: one detector crop of any size per modality,
data/datasets/bases.py:22-30) - the parts of the ragged decode + resize path that run without a GPU: the fixture lies inside what
the host decoder + oracle/jpeg_ref.py reproduce, the ragged planner's offsets, and the ragged tap tables against Pillow."""
import numpy as np
import pytest

from ragged_helpers import INTERPOLATIONS, TARGETS, emulate_ragged_resize, fixture, host_decode


def test_fixture_covers_the_cases_the_indexing_can_get_wrong():
    names, jpg, rgb = fixture()
    assert len(names) >= 14
    sizes = {rgb[n].shape[:2] for n in names}
    assert all(h >= 7 and w >= 7 for h, w in sizes)                       # (narrower subsampled files: DESIGN.md 6, known divergence)
    assert {(90, 128), (256, 200), (256, 128), (8, 8), (16, 16)} <= sizes
    assert any(h < 32 and w < 32 for h, w in sizes) and any(w > 2 * 128 for h, w in sizes)
    samp = set()
    for n in names:
        info = host_decode(jpg[n])[2]
        samp.add((int(info[2]), int(info[3]), int(info[4])))
    assert samp == {(3, 2, 2), (3, 2, 1), (3, 1, 1), (1, 1, 1)}           # 4:2:0, 4:2:2, 4:4:4, grayscale
    assert any(b"\xff\xc2" in jpg[n] for n in names) and any(b"\xff\xdd" in jpg[n] for n in names)   # progressive, restart interval


def test_every_fixture_file_equals_pillow_through_host_decoder_and_oracle():
    from oracle import jpeg_ref
    names, jpg, rgb = fixture()
    for n in names:
        coef, qt, info = host_decode(jpg[n])
        assert (int(info[1]), int(info[0])) == rgb[n].shape[:2], n
        assert np.array_equal(jpeg_ref.reconstruct(coef, qt, info), rgb[n]), n


def _expected_plan(infos):
    """Sizes from the geometry alone, image after image: component block grids padded to whole MCUs, 64 samples per block."""
    rows, cb, pb, ob, px = [], 0, 0, 0, 0
    for inf in infos:
        w, h, ncomp, hmax, vmax, mcux, mcuy = [int(v) for v in inf[:7]]
        blocks = plane = 0
        for c in range(ncomp):
            hs, vs = (hmax, vmax) if c == 0 else (1, 1)
            blocks += (mcux * hs) * (mcuy * vs)
            plane += (mcux * hs * 8) * (mcuy * vs * 8)
        rows.append((cb, pb, ob, cb + blocks, px + w * h))
        cb, pb, ob, px = cb + blocks, pb + plane, ob + w * h * 3, px + w * h
    return np.asarray(rows, dtype=np.int64).T, cb, px


@pytest.mark.parametrize("batch", ["all", "reversed", "one", "equal_neighbours"])
def test_ragged_planner_offsets(batch):
    from editor_amd.data import ragged_decode_plan
    names, jpg, _ = fixture()
    order = {"all": names, "reversed": names[::-1], "one": names[3:4], "equal_neighbours": [names[0], names[3], names[3], names[6]]}[batch]
    infos = np.stack([host_decode(jpg[n])[2] for n in order])
    tab, nblocks, npixels = ragged_decode_plan(infos)
    want, wb, wp = _expected_plan(infos)
    assert tab.dtype == np.int64 and tab.shape == (5, len(order))
    assert np.array_equal(tab, want) and (nblocks, npixels) == (wb, wp)
    assert (tab[1] % 8 == 0).all()                                        # plane bases: the IDCT stores 8 bytes at a time
    assert (np.diff(tab[3]) > 0).all() and (np.diff(tab[4]) > 0).all()    # what the binary search relies on
    assert int(tab[3, -1]) == int(infos[:, 8].sum())


@pytest.mark.parametrize("interpolation", INTERPOLATIONS)
@pytest.mark.parametrize("size", TARGETS)
def test_ragged_tap_tables_equal_pillow(size, interpolation):
    """The per-image tables (offsets into ONE tap array, per-image ksize, identity tables where an extent already fits) applied by
    the numpy emulation of the two device passes == PIL.Image.resize, bit for bit."""
    Image = pytest.importorskip("PIL.Image")
    from editor_amd.data import DeviceResize
    names, _, rgb = fixture()
    rs = DeviceResize(size, interpolation)
    sizes = np.asarray([rgb[n].shape[:2] for n in names])
    desc = rs.ragged_tables(sizes)
    again = rs.ragged_tables(sizes[::-1])                                 # cached: the same tables, no growth
    taps = rs.taps()
    assert np.array_equal(again, desc[::-1]) and rs.taps() is taps and taps.dtype == np.int32
    assert np.array_equal(desc[:, :2], sizes) and (desc[:, 6:] == 0).all()
    for i, n in enumerate(names):
        want = np.asarray(Image.fromarray(rgb[n]).resize((size[1], size[0]), resample=interpolation))
        assert np.array_equal(emulate_ragged_resize(rgb[n], size, desc[i], taps), want), (n, size, interpolation)
    # an extent that already equals its target: the identity table (one tap of 1 << 22)
    for i, n in enumerate(names):
        h, w = rgb[n].shape[:2]
        for extent, n_out, col in ((w, size[1], 2), (h, size[0], 4)):
            if extent == n_out:
                k = taps[desc[i, col] + 2 * n_out:desc[i, col] + 2 * n_out + n_out * desc[i, col + 1]].reshape(n_out, -1)
                assert (np.sort(k, axis=1)[:, -1] == 1 << 22).all() and (k.sum(axis=1) == 1 << 22).all()
