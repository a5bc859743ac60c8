"""In-segment parallel Huffman decode (DeviceJpegDecoder(entropy="device_split")), the parts that run without a GPU: the HOST twin
editor_jpeg_entropy_split_segments - the kernel's own routines, its lanes and rounds run one after another - against the host
decoder (editor_jpeg_entropy_decode), which is the definition of correct: coefficient planes bit for bit, no tolerance.  The
subsequence boundaries are start + k * sub_bytes of each of the planner's segments; every boundary case below is found from those
byte ranges and asserted to have occurred."""
import ctypes

import numpy as np
import pytest

import device_entropy_helpers as H
import device_entropy_split_helpers as S

LONGEST = "f14/stitched_444_q90"                                 # 118 KB, no restart markers
MANY = "d1/r1mcu_420_56x40"                                      # a restart interval of one MCU


def _equal(names, sub):
    rc, status, coef, off, stats = S.split_segments([S.files()[n] for n in names], sub)
    assert rc == 0 and not status.any(), (rc, status)
    for n, o in zip(names, off):
        want = S.host_coef(n)
        assert np.array_equal(coef[o:o + want.shape[0]], want), (n, sub)
    assert not (coef == 0x5A5A).any()
    return stats


@pytest.mark.parametrize("sub", S.SUBS)
def test_host_twin_equals_host_decoder_for_every_fixture_file(sub):
    sub = S.sub_bytes(sub)
    names = list(S.files())
    assert len(names) == 29 and sum(not n.startswith("d2/") for n in names) == 26      # all 26 eligible files, and the new fixture's 3
    _equal(names, sub)
    _equal(names[::-1], sub)
    for n in names:
        stats = _equal([n], sub)
        assert (stats[:, 0] >= stats[:, 1]).all() and (stats >= 0).all(), n           # a round per chunk at least
        if n == LONGEST:
            seg, _ = S.segments(n)
            assert stats[0, 1] == -(-int(seg[0, 1] - seg[0, 0]) // (256 * sub))        # every chunk of the segment was walked
            if sub == 16:
                # shorter than most blocks: lanes rarely synchronise inside their own subsequence, so chunks need more than the
                # two rounds (decode, confirm) of lanes that do - the round loop really runs
                assert stats[0, 1] == 29 and stats[0, 0] > 2 * stats[0, 1], stats


def _lengths(sub):
    """{(file, segment): byte length} and the (file, segment, boundary) triples whose boundary splits an FF 00 pair"""
    lens, split = {}, []
    for n, data in S.files().items():
        seg, _ = S.segments(n)
        for k, (a, b, _) in enumerate(seg.tolist()):
            lens[(n, k)] = b - a
            split += [(n, k, p) for p in range(a + sub, b, sub) if data[p - 1] == 0xFF and data[p] == 0x00]
    return lens, split


@pytest.mark.parametrize("sub", S.SUBS)
def test_boundary_cases_occur_in_the_fixtures_and_decode_exactly(sub):
    sub = S.sub_bytes(sub)
    lens, split = _lengths(sub)
    short = sorted({n for (n, _), v in lens.items() if 0 < v < sub})
    exact = sorted({n for (n, _), v in lens.items() if v >= sub and v % sub == 0})
    plus1 = sorted({n for (n, _), v in lens.items() if v > sub and v % sub == 1})
    pairs = sorted({n for n, _, _ in split})
    assert short and exact and plus1 and pairs, (sub, short, exact, plus1, pairs)
    assert "d2/tinyseg_gray_64x24" in short and "d2/exact128_420_72x56" in exact and "d2/plus1_444_40x48" in plus1
    # (k above 1: the last of several subsequences is a full one)
    assert any(v % sub == 0 and v // sub > 1 for v in lens.values())
    for group in (short, exact, plus1, pairs):
        _equal(group, sub)
    # a many-restart file (every MCU its own segment) beside the longest restart-less one, either way round
    assert len(S.segments(MANY)[0]) == 12 and len(S.segments(LONGEST)[0]) == 1
    assert lens[(LONGEST, 0)] == max(lens.values())
    _equal([MANY, LONGEST], sub)
    _equal([LONGEST, MANY, "d2/tinyseg_gray_64x24"], sub)
    # 1, 3, 4 and 6 blocks per MCU: grayscale, 4:4:4, 4:2:2, 4:2:0
    assert {S.segments(n)[1] for n in S.files()} == {1, 3, 4, 6}


def _same_as_segments(datas, sub):
    """status of the one-lane twin (editor_jpeg_entropy_segments); equal coefficients where it is 0, no fill left where not"""
    rc0, want_status, want, off0 = H.host_segments(datas)
    rc, status, coef, off, _ = S.split_segments(datas, sub)
    assert rc == 0 and rc0 == 0 and np.array_equal(status, want_status), (status, want_status)
    assert not (coef == 0x5A5A).any()                            # every block of every range was written
    ends = list(off[1:]) + [coef.shape[0]]
    for i, (o, e) in enumerate(zip(off, ends)):
        if status[i] == 0:
            assert np.array_equal(coef[o:e], want[o:e]), i
    return status


@pytest.mark.parametrize("sub", [16, "default"])
def test_truncation_sweep_matches_the_one_lane_twin(sub):
    """The cuts of tests/test_device_entropy_host.py (one every 7 bytes of odd_422_q95 up to 40 bytes into its data, then a few
    deeper in and near the end): a cut segment's remaining blocks come from the zeros past its data."""
    sub = S.sub_bytes(sub)
    data = H.files()["f14/odd_422_q95"]
    sos = data.index(b"\xFF\xDA")
    sos_end = sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])
    cuts = list(range(2, sos_end + 40, 7)) + list(range(sos_end + 40, len(data), 997)) + [len(data) - 1, len(data) - 2]
    compared = 0
    for cut in cuts:
        part = data[:cut]
        rc, _, pl, _, _, _ = H.plan(part)
        if rc:
            continue                                             # refused before anything would be launched
        assert pl[0] == 1, cut
        status = _same_as_segments([part], sub)
        want_rc, want = H.host_decode(part)
        assert int(status[0]) == want_rc, cut
        compared += 1
    assert compared >= 8


@pytest.mark.parametrize("sub", [16, "default"])
def test_recorded_corrupt_variants_give_the_recorded_results(sub):
    sub = S.sub_bytes(sub)
    z = H.d1()
    flip, trunc = z["bitflip.jpg"].tobytes(), z["trunc.jpg"].tobytes()
    good = H.files()[MANY]
    status = _same_as_segments([good, flip, trunc, S.files()[LONGEST][:60000]], sub)
    assert status.tolist()[:3] == [0, 9001, int(z["trunc.rc"])]
    rc, status, coef, off, _ = S.split_segments([good, flip, trunc], sub)
    assert np.array_equal(coef[:off[1]], H.host_coef(MANY))
    if int(z["trunc.rc"]) == 0:
        assert np.array_equal(coef[off[2]:], z["trunc.coef"])


def test_split_entries_refuse_tables_sub_bytes_and_workspaces_that_do_not_fit():
    data = [H.files()["d1/shortlast_444_41x23"]]
    buf, nbytes, fdesc, ftab, segs, huff, nseg, off, total = H.packed(data)
    cd = H.cdll()
    rc, need = S.workspace(nseg, 64)
    assert rc == 0 and need > 0 and need % 8 == 0
    for bad in (0, 8, 24, 48, 256, -16):
        assert S.workspace(nseg, bad)[0] != 0
    assert S.workspace(-1, 64)[0] != 0

    def run(nbytes=nbytes, fdesc=fdesc, ftab=ftab, segs=segs, nhuff=int(huff.shape[0]), total=total, sub=64, ws_bytes=need, expect_untouched=True):
        coef = np.full((total + 8, 64), 0x5A5A, dtype=np.int16)
        status = np.full(1, -1, dtype=np.int32)
        ws = np.full(need // 8, -1, dtype=np.int64)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)             # noqa: E731
        rc = cd.editor_jpeg_entropy_split_segments(p(buf), nbytes, p(fdesc), p(ftab), p(segs), p(huff), nhuff, 1, nseg, sub, p(ws), ws_bytes,
                                                   p(coef), total, p(status))
        if expect_untouched:
            assert rc == 1, rc                                   # hipErrorInvalidValue
            assert (coef == 0x5A5A).all() and status[0] == -1 and (ws == -1).all()
        return rc
    assert run(expect_untouched=False) == 0
    run(nbytes=nbytes - 16)                                      # last segment ends past the buffer
    run(total=total - 1)                                         # image does not fit the coefficient buffer
    run(nhuff=1)                                                 # table row out of the pool
    for col, val in ((3, int(fdesc[0, 3]) + 1), (0, 2), (1, 3), (5, 5)):
        bad = fdesc.copy()
        bad[0, col] = val
        run(fdesc=bad)
    bad = segs.copy()
    bad[2, 2] += 1
    run(segs=bad)
    for sub in (0, 8, 24, 256):                                  # not a power of two from 16 to 128
        run(sub=sub)
    run(ws_bytes=need - 8)                                       # workspace too small
    run(ws_bytes=0)


def test_split_entry_points_have_declared_argument_types_and_the_keyword_is_validated():
    cd = H.cdll()
    for name in ("editor_jpeg_entropy_split_workspace", "editor_jpeg_entropy_split_segments", "editor_jpeg_entropy_split_device"):
        fn = getattr(cd, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    assert cd.editor_jpeg_entropy_split_segments.argtypes[9] is ctypes.c_int and cd.editor_jpeg_entropy_split_segments.argtypes[11] is ctypes.c_long
    from editor_amd.data import DeviceJpegDecoder
    dec = DeviceJpegDecoder(crop_w=0, threads=1, entropy="device_split")
    assert dec.entropy == "device_split" and dec.split_sub_bytes == DeviceJpegDecoder.SPLIT_SUB_BYTES
    assert DeviceJpegDecoder.SPLIT_SUB_BYTES in (16, 32, 64, 128)
    assert DeviceJpegDecoder(crop_w=0, threads=1, entropy="device_split", split_sub_bytes=16).split_sub_bytes == 16
    assert DeviceJpegDecoder(crop_w=0, threads=1).entropy == "host"          # the default stays the host decoder
    with pytest.raises(ValueError):
        DeviceJpegDecoder(crop_w=0, threads=1, entropy="device_split", split_sub_bytes=24)
    with pytest.raises(ValueError):
        DeviceJpegDecoder(crop_w=0, threads=1, entropy="split")
