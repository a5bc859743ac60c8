"""editor_train_meter (csrc/meter.hip) against torch on the device - `score.max(1)[1] == target` - and Python double
accumulation for the state: every batch size and class count at which the one-wave-per-row, 16-rows-at-a-time mapping changes
shape, rows built to break a wrong (value, index) reduction, unaligned row strides, accumulation over launches, hipGraph
replays, the refusals, and a NaN-poisoned tail (and NaN-poisoned gaps between the rows) that must never be read."""
import numpy as np
import pytest
import torch

from editor_amd import _lib

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SHAPES = [(b, 171) for b in (1, 2, 3, 4, 5, 63, 64, 65, 128, 1024)] + \
         [(7, c) for c in (1, 2, 63, 64, 65, 127, 128, 129, 171, 751, 4097)]
PADS = (0, 3)                       # lds = C and lds = C + 3 (odd strides, rows off every vector alignment)
STATE0 = [1.5, 3.0, 0.25, 2.0]      # the state a launch starts from: the kernel ADDS


def _launch(buf, lds, target, loss, b, c, state, last):
    """The raw C entry -> its return code.  buf: the flat score buffer (or None)."""
    fn = _lib.lib().cdll.editor_train_meter
    ptr = lambda t: None if t is None else t.data_ptr()
    return fn(ptr(buf), lds, ptr(target), ptr(loss), b, c, ptr(state), ptr(last), torch.cuda.current_stream().cuda_stream)


def _special_rows(c):
    """(row values, expected argmax) of the rows built to break a wrong reduction, for a row of c columns."""
    base = np.linspace(-1.0, 1.0, c, dtype=np.float32) * 0.5           # distinct, all below 1
    rows = []

    def row(edit, want):
        r = base.copy()
        edit(r)
        rows.append((r, want))

    def put(r, cols, val):
        r[list(cols)] = val

    last_group = 64 * ((c - 1) // 64)                                   # first column of the last (partial) wave-width group
    row(lambda r: put(r, [0], 9.0), 0)                                  # the maximum in column 0
    row(lambda r: put(r, [c - 1], 9.0), c - 1)                          # ... in column C-1
    row(lambda r: put(r, [last_group], 9.0), last_group)                # ... in the last partial group
    row(lambda r: put(r, [min(1, c - 1), c - 1], 9.0), min(1, c - 1))   # an exact tie between columns 1 and C-1 -> 1
    row(lambda r: put(r, range(c), 0.375), 0)                           # all equal -> 0
    row(lambda r: put(r, range(c), -INF), 0)                            # a row of -inf -> 0
    if c >= 2:
        row(lambda r: (put(r, [(c - 1) // 2], 1e30), put(r, [c - 1], NAN)), c - 1)   # a NaN later than a larger finite value
        row(lambda r: put(r, [c // 2, c - 1], NAN), c // 2)             # two NaNs -> the first
    row(lambda r: put(r, [0], -0.0) or put(r, range(1, c), -1.0) or put(r, [c - 1], 0.0), 0)   # -0 and +0 tie -> the lower index
    return rows


def _case(b, c, pad, seed, specials=True):
    """-> flat buffer (rows at stride lds, NaN in every gap and in 64 bytes past the last row), its (B, C) strided view, lds."""
    lds = c + pad
    gen = torch.Generator().manual_seed(seed)
    rows = torch.randn(b, c, generator=gen)
    if specials:
        for i, (r, _) in enumerate(_special_rows(c)[:b]):
            rows[(i * 7) % b if b >= 16 else i] = torch.from_numpy(r)   # (spread over the waves when there are rows enough)
    buf = torch.full(((b - 1) * lds + c + 16,), NAN)
    view = torch.as_strided(buf, (b, c), (lds, 1))
    view.copy_(rows)
    buf = buf.cuda()
    return buf, torch.as_strided(buf, (b, c), (lds, 1)), lds


def _targets(view, seed):
    """About half the rows labelled with their argmax, the rest at random; one label C and one -1 where the batch has room."""
    b, c = view.shape
    gen = torch.Generator().manual_seed(seed + 1)
    arg = view.max(1)[1].cpu()
    target = torch.where(torch.rand(b, generator=gen) < 0.5, arg, torch.randint(0, c, (b,), generator=gen))
    if b >= 3:
        target[0] = arg[0]                                              # (at least one hit, at least two misses)
        target[b - 1] = c
        target[b - 2] = -1
    return target.cuda()


def _expected_update(view, target, loss):
    b = view.shape[0]
    correct = int((view.max(1)[1] == target).sum().item())
    return correct, [float(loss) * b, float(b), float(np.float32(correct) / np.float32(b)), 1.0]


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("b,c", SHAPES)
def test_counts_and_state_match_torch(b, c, pad):
    buf, view, lds = _case(b, c, pad, 1000 * b + c)
    target = _targets(view, b + c)
    loss = torch.tensor([0.1 * b + 1.0 / c], dtype=torch.float32).cuda()
    state = torch.tensor(STATE0, dtype=torch.float64).cuda()
    last = torch.full((2,), -7, dtype=torch.int32).cuda()
    assert _launch(buf, lds, target, loss, b, c, state, last) == 0
    correct, upd = _expected_update(view, target, loss.item())
    assert last.tolist() == [correct, b]
    assert state.tolist() == [s + u for s, u in zip(STATE0, upd)]
    if b >= 3:
        assert 0 < correct < b, "the case must hold hits and misses"


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("c", [c for _, c in SHAPES[10:]])
def test_rows_built_to_break_a_reduction(c, pad):
    special = _special_rows(c)
    b, lds = len(special), c + pad
    buf = torch.full(((b - 1) * lds + c + 16,), NAN)
    torch.as_strided(buf, (b, c), (lds, 1)).copy_(torch.from_numpy(np.stack([r for r, _ in special])))
    buf = buf.cuda()
    view = torch.as_strided(buf, (b, c), (lds, 1))
    want = [w for _, w in special]
    assert view.max(1)[1].tolist() == want                              # (the rows mean what their comments say, under torch)
    loss = torch.ones(1).cuda()
    state = torch.zeros(4, dtype=torch.float64).cuda()
    last = torch.zeros(2, dtype=torch.int32).cuda()
    # every row on its own, labelled with the wanted column: one hit each - then with the column's neighbours: none
    for r in range(b):
        row = buf[r * lds:]
        for label, hit in [(want[r], 1), (want[r] + 1, 0), (want[r] - 1, 0)]:
            target = torch.tensor([label]).cuda()
            assert _launch(row, lds, target, loss, 1, c, state, last) == 0
            assert last.tolist() == [hit, 1], (r, label)
    # all rows in one launch; then a label equal to C and one equal to -1, which never match
    target = torch.tensor(want).cuda()
    assert _launch(buf, lds, target, loss, b, c, state, last) == 0
    assert last.tolist() == [b, b]
    target[0], target[1] = c, -1
    assert _launch(buf, lds, target, loss, b, c, state, last) == 0
    assert last.tolist() == [b - 2, b]


def test_state_accumulates_like_python_doubles():
    c = 171
    state = torch.zeros(4, dtype=torch.float64).cuda()
    last = torch.zeros(2, dtype=torch.int32).cuda()
    want = [0.0, 0.0, 0.0, 0.0]
    for i, b in enumerate((64, 65, 3, 128, 7)):
        buf, view, lds = _case(b, c, 3 * (i % 2), 50 + i, specials=False)
        target = _targets(view, 60 + i)
        loss = torch.tensor([5.0 / (i + 3)], dtype=torch.float32).cuda()
        assert _launch(buf, lds, target, loss, b, c, state, last) == 0
        correct, upd = _expected_update(view, target, loss.item())
        want = [w + u for w, u in zip(want, upd)]
        assert last.tolist() == [correct, b]
    assert state.tolist() == want and want[3] == 5.0 and want[1] == 267.0


def test_graph_replays_each_add_one_update():
    b, c = 65, 171
    buf, view, lds = _case(b, c, 3, 77)
    target = _targets(view, 78)
    loss = torch.tensor([0.7], dtype=torch.float32).cuda()
    state = torch.zeros(4, dtype=torch.float64).cuda()
    last = torch.zeros(2, dtype=torch.int32).cuda()
    assert _launch(buf, lds, target, loss, b, c, state, last) == 0      # (library loaded, kernel resident)
    torch.cuda.synchronize()
    state.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = _launch(buf, lds, target, loss, b, c, state, last)
    assert rc == 0 and state.tolist() == [0.0] * 4                      # (a capture runs nothing)
    correct, upd = _expected_update(view, target, loss.item())
    want = [0.0] * 4
    for n in range(1, 4):
        g.replay()
        want = [w + u for w, u in zip(want, upd)]
        assert state.tolist() == want and last.tolist() == [correct, b], n
    # new inputs at the captured addresses are what the next replay counts
    target.copy_(view.max(1)[1])
    g.replay()
    assert last.tolist() == [b, b]


def test_invalid_arguments_launch_nothing():
    b, c = 5, 64
    buf, view, lds = _case(b, c, 3, 5)
    target = _targets(view, 6)
    loss = torch.ones(1).cuda()
    state = torch.tensor(STATE0, dtype=torch.float64).cuda()
    last = torch.tensor([11, 12], dtype=torch.int32).cuda()
    for kw in (dict(b=0), dict(b=-1), dict(c=0), dict(c=-3), dict(lds=c - 1), dict(lds=0)):
        a = dict(b=b, c=c, lds=lds)
        a.update(kw)
        assert _launch(buf, a["lds"], target, loss, a["b"], a["c"], state, last) == 1, kw
    assert _launch(None, lds, target, loss, b, c, state, last) == 1
    assert _launch(buf, lds, target, loss, b, c, None, last) == 1
    torch.cuda.synchronize()
    assert state.tolist() == STATE0 and last.tolist() == [11, 12]
    with pytest.raises(RuntimeError):
        _lib.call("editor_train_meter", buf, c - 1, target, loss, b, c, state, last)


@pytest.mark.parametrize("b,c,pad", [(1, 171, 0), (7, 63, 0), (7, 65, 3), (64, 171, 3)])
def test_poison_past_the_last_row_changes_nothing(b, c, pad):
    """The 64 bytes after the last row once NaN, once +inf, once finite: a kernel that read any of them would count differently
    (a NaN or +inf beats every column of a finite last row)."""
    results = []
    for poison in (NAN, INF, 0.0):
        buf, view, lds = _case(b, c, pad, 9, specials=False)
        buf[(b - 1) * lds + c:] = poison
        target = view.max(1)[1].clone()
        state = torch.zeros(4, dtype=torch.float64).cuda()
        last = torch.zeros(2, dtype=torch.int32).cuda()
        assert _launch(buf, lds, target, torch.ones(1).cuda(), b, c, state, last) == 0
        results.append((last.tolist(), state.tolist()))
    assert results[0] == results[1] == results[2] == ([b, b], [float(b), float(b), 1.0, 1.0])


def test_device_meters_read():
    from editor_amd.engine import DeviceMeters
    m = DeviceMeters("cuda")
    want = [0.0] * 4
    for i, b in enumerate((8, 5)):
        gen = torch.Generator().manual_seed(i)
        score = torch.randn(b, 171, generator=gen).cuda()
        target = torch.where(torch.arange(b) % 2 == 0, score.max(1)[1].cpu(), torch.full((b,), 170)).cuda()
        loss = torch.tensor(2.5 + i).cuda()
        m.update(score.to(torch.bfloat16) if i else score, target, loss)             # (a 16-bit score is made fp32 first)
        ref = score.to(torch.bfloat16).float() if i else score
        correct, upd = _expected_update(ref, target, loss.item())
        want = [w + u for w, u in zip(want, upd)]
    got = m.read()
    assert [got["loss_sum"], got["samples"], got["acc_sum"], got["steps"]] == want
    assert got["loss_avg"] == want[0] / want[1] and got["acc_avg"] == want[2] / want[3]
    assert (got["last_correct"], got["last_batch"]) == (correct, 5)
    m.reset()
    got = m.read()
    assert got["steps"] == 0.0 and got["samples"] == 0.0 and got["last_batch"] == 0 and got["loss_avg"] == 0.0
