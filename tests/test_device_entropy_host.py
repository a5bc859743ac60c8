"""Device-side Huffman decode of sequential JPEG scans (DeviceJpegDecoder(entropy="device")), the parts that run without a GPU:
the planner (editor_jpeg_plan: eligibility, compact tables, restart-segment table) and the segment decoder's HOST twin
(editor_jpeg_entropy_segments - the very routine the kernel runs, compiled for the CPU) against the host decoder
(editor_jpeg_entropy_decode), which is the definition of correct: coefficient planes bit for bit."""
import ctypes

import numpy as np
import pytest

import device_entropy_helpers as H


def _markers(data, a, b):
    """positions of the RSTn markers in data[a:b] (a stuffed FF 00 is data)"""
    out, p = [], a
    while p + 1 < b:
        if data[p] == 0xFF:
            if 0xD0 <= data[p + 1] <= 0xD7:
                out.append(p)
            p += 2
        else:
            p += 1
    return out


def test_planner_eligibility_and_segment_tables():
    files = H.files()
    assert len(files) == 28 and len(H.eligible_names()) == 26
    restarts = 0
    for name, data in files.items():
        rc, info, pl, qt, huff, seg = H.plan(data)
        assert rc == 0, name
        # info as editor_jpeg_parse returns it
        ref = np.zeros(16, dtype=np.int32)
        buf = np.frombuffer(data, dtype=np.uint8)
        assert H.cdll().editor_jpeg_parse(ctypes.c_void_p(buf.ctypes.data), buf.size, ctypes.c_void_p(ref.ctypes.data)) == 0
        assert np.array_equal(info, ref), name
        assert bool(pl[0]) == (name not in H.PROGRESSIVE), name
        if name in H.PROGRESSIVE:
            assert pl[10] > 1                                    # several scans
            continue
        ri, nmcu = int(pl[2]), int(pl[3])
        assert nmcu == int(info[5]) * int(info[6]) and pl[10] == 1
        sos = data.index(b"\xFF\xDA")
        ecs = sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])
        marks = _markers(data, ecs, len(data) - 2)
        assert len(seg) == int(pl[1]) == len(marks) + 1, name    # segments = markers + 1
        assert len(marks) == ((nmcu + ri - 1) // ri - 1 if ri else 0), name
        restarts += bool(ri)
        assert seg[0, 0] == ecs and seg[-1, 1] == len(data) - 2 and data[-2:] == b"\xFF\xD9"
        for k, m in enumerate(marks):
            assert data[m + 1] == 0xD0 + (k & 7)
            assert seg[k, 1] == m and seg[k + 1, 0] == m + 2, (name, k)      # each segment starts right after its RSTn
        assert np.array_equal(seg[:, 2], np.arange(len(seg)) * ri), name     # first MCU k * Ri
        # the compact tables: the DHT segments' own bytes
        for c in range(int(info[2])):
            for sel, tc in ((int(pl[4 + c]), 0), (int(pl[7 + c]), 1)):
                t = huff[4 * tc + sel]
                cnt = int(t[:16].sum())
                assert 0 < cnt <= 256 and not t[16 + cnt:].any()
                assert bytes([(tc << 4) | sel]) + t[:16 + cnt].tobytes() in data[:sos], (name, c, tc)
    assert restarts >= 5


def test_planner_routes_a_file_with_a_restart_marker_removed_to_the_host():
    for name in ("r1/i_restart_422_75x40", "d1/shortlast_444_41x23", "f14/restart_420_q80"):
        data = H.files()[name]
        rc, info, pl, _, _, seg = H.plan(data)
        assert rc == 0 and pl[0] == 1
        m = int(seg[1, 1])                                       # the second marker
        cut = data[:m] + data[m + 2:]
        rc, _, pl2, _, _, _ = H.plan(cut)
        assert rc == 0 and pl2[0] == 0 and pl2[1] == pl[1] - 1, name
        # ... as is one whose markers do not cycle D0..D7 in order
        bad = bytearray(data)
        bad[m + 1] = 0xD0 + ((bad[m + 1] - 0xD0 + 3) & 7)
        rc, _, pl3, _, _, _ = H.plan(bytes(bad))
        assert rc == 0 and pl3[0] == 0 and pl3[1] == pl[1], name
    # a segment table too small for the file: the count is still reported, nothing is written past the capacity
    rc, _, pl, _, _, seg = H.plan(H.files()["d1/r1mcu_420_56x40"], cap=3)
    assert rc == 0 and pl[1] == 12 and len(seg) == 3


def test_noise_fixture_has_long_codes_and_stuffing():
    data = H.files()["d1/noise_444_q100_opt_48x32"]
    _, info, pl, _, huff, seg = H.plan(data)
    assert huff[4 + int(pl[7]), 9:16].any()                      # AC codes longer than the 9-bit lookahead
    assert data[int(seg[0, 0]):int(seg[0, 1])].count(b"\xFF\x00") >= 8


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_host_twin_equals_host_decoder_for_every_eligible_file(order):
    names = H.eligible_names()
    if order == "reversed":
        names = names[::-1]
    rc, status, coef, off = H.host_segments([H.files()[n] for n in names])
    assert rc == 0 and not status.any()
    for n, o in zip(names, off):
        want = H.host_coef(n)
        assert np.array_equal(coef[o:o + want.shape[0]], want), n
    # and each file alone
    if order == "forward":
        for n in names:
            rc, status, coef, _ = H.host_segments([H.files()[n]])
            assert rc == 0 and status[0] == 0 and np.array_equal(coef, H.host_coef(n)), n


def test_host_twin_truncation_sweep_matches_host_decoder():
    """The cuts of test_truncations_and_oversized_counts_never_crash (one every 7 bytes of odd_422_q95): where the planner accepts
    the file and calls it eligible, the segment decoder returns the host decoder's rc and, for rc 0, its coefficients."""
    data = H.files()["f14/odd_422_q95"]
    sos = data.index(b"\xFF\xDA")
    sos_end = sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])
    # (the sweep of the existing test ends 40 bytes into the data; a few cuts deeper in and near the end are added)
    cuts = list(range(2, sos_end + 40, 7)) + list(range(sos_end + 40, len(data), 997)) + [len(data) - 1, len(data) - 2]
    compared = 0
    for cut in cuts:
        part = data[:cut]
        want_rc, want = H.host_decode(part)
        rc, _, pl, _, _, _ = H.plan(part)
        if rc:
            assert want_rc == rc, cut                            # refused before anything would be launched
            continue
        assert pl[0] == 1, cut                                   # no restart interval: a cut leaves one segment
        rc, status, coef, _ = H.host_segments([part])
        assert rc == 0 and int(status[0]) == want_rc, (cut, int(status[0]), want_rc)
        if want_rc == 0:
            assert np.array_equal(coef, want), cut
        compared += 1
    assert compared >= 8
    # a restart file cut inside its data has fewer markers than its MCU count asks for: host-routed
    part = H.files()["f14/restart_420_q80"]
    part = part[:len(part) // 2]
    rc, _, pl, _, _, _ = H.plan(part)
    assert rc == 0 and pl[0] == 0


def test_host_twin_gives_the_recorded_results_for_the_corrupted_variants():
    z = H.d1()
    flip, trunc = z["bitflip.jpg"].tobytes(), z["trunc.jpg"].tobytes()
    good = H.files()["d1/r1mcu_420_56x40"]
    assert H.host_decode(flip)[0] == 9001
    rc, status, coef, off = H.host_segments([good, flip, trunc])
    assert rc == 0 and status.tolist() == [0, 9001, int(z["trunc.rc"])]
    assert np.array_equal(coef[:off[1]], H.host_coef("d1/r1mcu_420_56x40"))
    assert not (coef == 0x5A5A).any()                            # every block of every range is defined, the corrupt file's too
    if int(z["trunc.rc"]) == 0:
        assert np.array_equal(coef[off[2]:], z["trunc.coef"])
    want_rc, want = H.host_decode(trunc)                         # the recording is what this build's host decoder says
    assert want_rc == int(z["trunc.rc"]) and np.array_equal(want, z["trunc.coef"])


def test_segment_entries_refuse_tables_that_do_not_fit():
    """check_entropy_tables: what the kernel trusts is checked on the host copies - out-of-range bytes, blocks, tables, MCUs."""
    data = [H.files()["d1/shortlast_444_41x23"]]
    buf, nbytes, fdesc, ftab, segs, huff, nseg, off, total = H.packed(data)
    cd = H.cdll()

    def run(nbytes=nbytes, fdesc=fdesc, ftab=ftab, segs=segs, nhuff=int(huff.shape[0]), total=total):
        coef = np.zeros((total + 8, 64), dtype=np.int16)
        status = np.zeros(1, dtype=np.int32)
        return cd.editor_jpeg_entropy_segments(ctypes.c_void_p(buf.ctypes.data), nbytes, ctypes.c_void_p(fdesc.ctypes.data),
                                               ctypes.c_void_p(ftab.ctypes.data), ctypes.c_void_p(segs.ctypes.data),
                                               ctypes.c_void_p(huff.ctypes.data), nhuff, 1, nseg, ctypes.c_void_p(coef.ctypes.data), total,
                                               ctypes.c_void_p(status.ctypes.data))
    assert run() == 0
    assert run(nbytes=nbytes - 16) != 0                          # last segment ends past the buffer
    assert run(total=total - 1) != 0                             # image does not fit the coefficient buffer
    assert run(nhuff=1) != 0                                     # table row out of the pool
    for col, val in ((3, int(fdesc[0, 3]) + 1), (0, 2), (1, 3), (5, 5)):       # more MCUs than segments cover, bad ncomp / hmax / Ri
        bad = fdesc.copy()
        bad[0, col] = val
        assert run(fdesc=bad) != 0, col
    bad = segs.copy()
    bad[2, 2] += 1                                               # a segment that does not start at k * Ri
    assert run(segs=bad) != 0
    bad = ftab.copy()
    bad[1, 0] -= int(segs[0, 0]) + 1 + int(ftab[1, 0])           # first byte before the buffer
    assert run(ftab=bad) != 0


def test_new_entry_points_have_declared_argument_types():
    cd = H.cdll()
    for name in ("editor_jpeg_plan", "editor_jpeg_entropy_segments", "editor_jpeg_entropy_device"):
        fn = getattr(cd, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    assert cd.editor_jpeg_plan.argtypes[1] is ctypes.c_long and cd.editor_jpeg_plan.argtypes[7] is ctypes.c_long
    assert cd.editor_jpeg_entropy_segments.argtypes[1] is ctypes.c_long and cd.editor_jpeg_entropy_segments.argtypes[8] is ctypes.c_long
    assert cd.editor_jpeg_entropy_device.argtypes[1] is ctypes.c_long


def test_entropy_keyword_is_validated():
    from editor_amd.data import DeviceJpegDecoder
    assert DeviceJpegDecoder(crop_w=0, threads=1).entropy == "host"          # the default stays the host decoder
    with pytest.raises(ValueError):
        DeviceJpegDecoder(crop_w=0, threads=1, entropy="gpu")
