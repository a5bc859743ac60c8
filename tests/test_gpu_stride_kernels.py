"""The two kernels of the overlapping patch embedding (MODEL.STRIDE_SIZE below 16) through the C ABI: the im2col of 16x16 windows
at any stride 1..16 and the frequency counts over overlapping windows - against torch's unfold, the reference's captured counts and
masks (tests/golden/s1_freq_*.npz, written by tests/golden/capture_stride.py) and, at stride 16, the existing entry points bit for
bit.  Plus the autograd node of the patch embedding at stride 12 against torch autograd on F.conv2d."""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_err, t
from editor_amd import synth

pytestmark = pytest.mark.gpu
GEOM = [(256, 128), (128, 256)]


@pytest.fixture(scope="module")
def ops():
    from editor_amd import ops
    return ops


def _img(b, h, w, seed):
    return torch.randn(b, 3, h, w, generator=torch.Generator().manual_seed(seed)) * torch.logspace(-2, 1, w)


def _unfold(img, s):
    """(B*N, C*256) fp32: row (b*N + p), column (c*256 + i*16 + j)"""
    u = F.unfold(img, 16, stride=s)
    return u.transpose(1, 2).reshape(-1, u.shape[1]).contiguous()


@pytest.mark.parametrize("hw", GEOM)
@pytest.mark.parametrize("b", [1, 3, 128])
@pytest.mark.parametrize("s", [12, 13, 14, 15, 16])
def test_im2col_patch_equals_unfold(ops, s, b, hw):
    h, w = hw
    img = _img(b, h, w, 100 * s + b)
    want = _unfold(img, s)
    ny, nx = ops.patch_grid(h, w, s)
    assert want.shape == (b * ny * nx, 768)
    gi = img.cuda()
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        got = torch.full((b * ny * nx, 768), float("nan"), dtype=dt, device="cuda")
        ops.call("editor_im2col_patch", gi, b, 3, h, w, s, s, got, ops._is_bf16(got))
        assert torch.equal(got.cpu(), want.to(dt)), dt
        if s != 16:
            assert torch.equal(ops.im2col_patch(gi, dt, (s, s)), got)
    # split-precision twin == editor_split_f32 of the fp32 matrix, bit for bit
    hi = torch.full((b * ny * nx, 768), float("nan"), dtype=torch.float16, device="cuda")
    lo = torch.full_like(hi, float("nan"))
    ops.call("editor_im2col_patch_f16x2", gi, b, 3, h, w, s, s, hi, lo)
    rh, rl = ops.split_f32(want.cuda(), 1.0)
    assert torch.equal(hi, rh) and torch.equal(lo, rl)
    if s == 16:                       # the existing kernel's output, bit for bit (and the wrappers keep calling it)
        for dt in (torch.bfloat16, torch.float16, torch.float32):
            old = ops.im2col16(gi, dt)
            new = torch.empty_like(old)
            ops.call("editor_im2col_patch", gi, b, 3, h, w, 16, 16, new, ops._is_bf16(new))
            assert torch.equal(old, new)
        oh, ol = ops.im2col16_split(gi)
        assert torch.equal(oh, hi) and torch.equal(ol, lo)
    else:
        ph, pl = ops.im2col_patch_split([gi, gi], (s, s))            # the modality list form: rows side by side
        assert torch.equal(ph[:hi.shape[0]], hi) and torch.equal(ph[hi.shape[0]:], hi) and torch.equal(pl[hi.shape[0]:], lo)


def test_im2col_patch_other_strides_and_refusals(ops):
    """rectangular and small strides (8-byte and scalar load forms, many windows), odd image widths; the refusals of the C entry"""
    for (h, w, sy, sx) in [(64, 48, 4, 16), (64, 48, 16, 6), (40, 37, 7, 3), (33, 50, 1, 2), (16, 16, 5, 5)]:
        img = _img(2, h, w, h + w)
        u = F.unfold(img, 16, stride=(sy, sx))
        want = u.transpose(1, 2).reshape(-1, 768)
        got = ops.im2col_patch(img.cuda(), torch.float32, (sy, sx))
        assert torch.equal(got.cpu(), want), (h, w, sy, sx)
    img = _img(1, 32, 32, 1).cuda()
    out = torch.empty(4, 768, device="cuda")
    for (h, w, sy, sx) in [(32, 32, 0, 16), (32, 32, 16, 17), (32, 32, -1, 4), (15, 32, 8, 8), (32, 8, 8, 8)]:
        with pytest.raises(RuntimeError, match="hipError 1"):
            ops.call("editor_im2col_patch", img, 1, 3, h, w, sy, sx, out, 0)


def _window_counts(pos, s):
    """pos (B,H,W) bool -> (B, ny*nx) int32 sums of the 16x16 windows at stride s"""
    u = F.unfold(pos[:, None].float(), 16, stride=s)
    return u.sum(1).to(torch.int32)


@pytest.mark.parametrize("tag,hw", [("256x128", (256, 128)), ("128x256", (128, 256))])
@pytest.mark.parametrize("kind", ["u8", "smooth"])
def test_frequency_stride12_equals_the_reference(ops, tag, hw, kind):
    g = load_golden(f"s1_freq_s12_{tag}_{kind}")
    s = int(g["stride"])
    img, _, _, _ = synth.make_batch(int(g["seed"]), 128, hw[0], hw[1], 2, smooth=bool(g["smooth"]))
    mask, counts = ops.frequency_mask(img["RGB"].cuda(), img["NI"].cuda(), img["TI"].cuda(), 10, stride=s)
    assert counts.shape == (128, 210)
    assert torch.equal(counts.cpu(), t(g["counts"]))
    assert torch.equal(mask.cpu().bool(), t(g["mask"]))


@pytest.mark.parametrize("hw", GEOM + [(384, 128), (64, 48)])
def test_frequency_stride16_equals_the_tile_kernel(ops, hw):
    h, w = hw
    img, _, _, _ = synth.make_batch(13, 32, h, w, 2)
    r, n_, t_ = (img[k].cuda() for k in ("RGB", "NI", "TI"))
    for mods in ((r, n_, t_), (r, n_, None)):
        old = ops.freq_counts(*mods)
        new = torch.full_like(old, -1)
        plane = torch.empty(32 * h * (w // 16), dtype=torch.int16, device="cuda")
        ops.call("editor_freq_counts_stride_f32", *mods, 32, 3, h, w, 16, plane, new)
        assert torch.equal(old, new)
    m4 = img["RGB"].flip(0).contiguous().cuda()
    old = ops.freq_counts(r, n_, t_, m4)
    new = torch.full_like(old, -1)
    ops.call("editor_freq_counts_stride_nmod_f32", r, n_, t_, m4, 4, 32, 3, h, w, 16, plane, new)
    assert torch.equal(old, new)


@pytest.mark.parametrize("s", [12, 13, 14, 15, 7, 1])
def test_frequency_stride_two_and_four_modalities_and_unaligned(ops, oracle, s):
    """tir = None and the 4-modality form, and three modalities at an address that is not 16-byte aligned (the 2x2-pixels-per-lane
    kernel): window sums of the bit plane the per-tile definition gives (the oracle's reconstruction, > 0)"""
    b, h, w = 6, 64, 48
    g = torch.Generator().manual_seed(40 + s)
    base = torch.rand(4, b, 3, h, w, generator=g) * 2 - 1
    base[:, 0, :, :32] = 0.0                                   # flat zero region: exact zeros are NOT positive
    base[:, 1, :, 16:48, 16:32] = 1.0
    m = [base[i].contiguous() for i in range(4)]
    for mods, extra in (((m[0], m[1], None), ()), ((m[0], m[1], m[2]), ()), ((m[0], m[1], m[2]), (m[3],))):
        _, inv = oracle.frequency_counts(*mods, extra=extra)
        want = _window_counts(inv.gt(0), s)
        got = ops.freq_counts(*[None if x is None else x.cuda() for x in mods], *[x.cuda() for x in extra], stride=s)
        assert torch.equal(got.cpu(), want), (len(mods) + len(extra), s)
    # unaligned: views that start 8 bytes into a larger buffer
    n = b * 3 * h * w
    un = []
    for x in m[:3]:
        buf = torch.empty(n + 2, device="cuda")
        v = buf[2:].view(b, 3, h, w)
        v.copy_(x)
        assert v.data_ptr() % 16 == 8
        un.append(v)
    _, inv = oracle.frequency_counts(m[0], m[1], m[2])
    assert torch.equal(ops.freq_counts(*un, stride=s).cpu(), _window_counts(inv.gt(0), s))


def test_frequency_stride_refusals(ops):
    x = torch.zeros(1, 3, 40, 32, device="cuda")
    plane = torch.empty(1 * 40 * 2, dtype=torch.int16, device="cuda")
    cnt = torch.empty(1, 4, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="hipError 1"):                  # H not a multiple of 16 (J = 4)
        ops.call("editor_freq_counts_stride_f32", x, x, x, 1, 3, 40, 32, 12, plane, cnt)
    y = torch.zeros(1, 3, 32, 32, device="cuda")
    for s in (0, 17):
        with pytest.raises(RuntimeError, match="hipError 1"):
            ops.call("editor_freq_counts_stride_f32", y, y, y, 1, 3, 32, 32, s, plane, cnt)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, "f16x2"])
@pytest.mark.parametrize("hw", GEOM)
def test_patch_embed_fn_stride12_backward(dtype, hw):
    """PatchEmbedFn at stride 12 alone: output, dw, db, dpos, dcls against torch autograd on F.conv2d(stride=12).  f32: 1e-5.  The
    16-bit modes: dpos / dcls are fp32 sums of the incoming gradient in every mode (1e-5 as well); the output, dw and db carry one
    16-bit rounding of the operands and are held to what tests/test_gpu_kernels.py::test_patch_embed_fn holds the stride-16 node to
    (bf16 1e-2, f16 a sixth of it; the split-precision forward is fp32-class, its backward is f16's)."""
    from editor_amd import functional as fn
    old_gs = fn.F16_GRAD_SCALE
    fn.set_f16_grad_scale(1.0)             # unit-scale synthetic gradients (as test_patch_embed_fn)
    try:
        h, w = hw
        b, cams, d, s = 4, 3, 256, 12
        ny, nx = (h - 16) // s + 1, (w - 16) // s + 1
        n = ny * nx
        assert n == 210
        g = torch.Generator().manual_seed(17)
        img = torch.randn(2 * b, 3, h, w, generator=g)
        cw = torch.randn(d, 3, 16, 16, generator=g) * 0.05
        cb, cls = torch.randn(d, generator=g) * 0.1, torch.randn(1, 1, d, generator=g)
        pos, sie = torch.randn(1, n + 1, d, generator=g), torch.randn(cams, 1, d, generator=g)
        cam = torch.randint(0, cams, (b,), generator=g)
        leaves = [x.clone().double().requires_grad_(True) for x in (cw, cb, cls, pos, sie)]
        x = F.conv2d(img.double(), leaves[0], leaves[1], stride=s).flatten(2).transpose(1, 2)
        x = torch.cat([leaves[2].expand(2 * b, -1, -1), x], 1) + leaves[3] + 3.0 * leaves[4][cam.repeat(2)]
        dx = torch.randn(x.shape, generator=g)
        x.backward(dx.double())
        dl = [v.clone().cuda().requires_grad_(True) for v in (cw, cb, cls, pos, sie)]
        act = fn.F16X2 if dtype == "f16x2" else dtype
        y = fn.PatchEmbedFn.apply([img[:b].cuda(), img[b:].cuda()], *dl, cam.cuda(), 3.0, act, (s, s))
        y.backward(dx.cuda())
        tol16 = {torch.float32: 1e-5, torch.bfloat16: 1e-2, torch.float16: 1e-2 / 6, "f16x2": 1e-2 / 6}[dtype]
        tol_y = 1e-5 if dtype == "f16x2" else tol16
        errs = {"y": rel_err(y.cpu(), x.detach())}
        for name, a, r in zip(("dw", "db", "dcls", "dpos", "dsie"), dl, leaves):
            errs[name] = rel_err(a.grad.cpu(), r.grad)
        print(dtype, hw, {k: "%.2e" % v for k, v in errs.items()})
        assert errs["y"] < tol_y
        assert errs["dw"] < tol16 and errs["db"] < tol16
        assert errs["dpos"] < 1e-5 and errs["dcls"] < 1e-5 and errs["dsie"] < 1e-5
    finally:
        fn.set_f16_grad_scale(old_gs)
