"""Helpers shared by the edge-case GPU test modules (test_gpu_dropskip_edges.py, test_gpu_hma_compact_edges.py): memory that holds
NaN wherever nobody wrote, seeded device tensors, the rows around a live count where a wrong tile would hide in an L2 figure, and
fp64 GELU."""
import torch

from conftest import rel_err


def _up(x, k):
    return -(-x // k) * k


class _Poison:
    """torch.empty / torch.empty_like fill every floating-point CUDA allocation with NaN (integer and bool buffers are left alone:
    an out-of-range index would fault the device, a NaN only shows up in a result).
    sync: wait for every fill - for code that hands a fresh buffer to a kernel on ANOTHER stream (the side-stream weight gradients):
    the fill runs on the current stream, where a real torch.empty launches nothing, and would otherwise race with that kernel."""

    def __init__(self, monkeypatch, sync=False):
        self.mp = monkeypatch
        self.sync = sync

    def __enter__(self):
        real_empty, real_like, sync = torch.empty, torch.empty_like, self.sync

        def fill(t):
            if t.is_cuda and t.dtype.is_floating_point:
                t.fill_(float("nan"))
                if sync:
                    torch.cuda.current_stream(t.device).synchronize()
            return t
        self.ctx = self.mp.context()
        mp = self.ctx.__enter__()
        mp.setattr(torch, "empty", lambda *a, **k: fill(real_empty(*a, **k)))
        mp.setattr(torch, "empty_like", lambda *a, **k: fill(real_like(*a, **k)))
        return self

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)


class _NoCtx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(shape, seed, std=1.0):
    return torch.randn(*shape, generator=_gen(seed), device="cuda") * std


def _boundary_rows(live, m):
    """rows of the tiles (208 and 256 rows) that hold row live - 1, live, roundup64(live) and the last row"""
    rows = set()
    for r in (live - 1, live, _up(live, 64), m - 1):
        if 0 <= r < m:
            for h in (208, 256):
                rows.update(range(r // h * h, min(r // h * h + h, m)))
    return sorted(rows)


def _check(got, ref, tol, m, what):
    """got / ref: the live rows (live, n); L2 and the worst per-row relative error of the boundary tiles' live rows"""
    live = got.shape[0]
    if live == 0:
        return
    e = rel_err(got, ref)
    assert e < tol, (what, "L2", e)
    rows = [r for r in _boundary_rows(live, m) if r < live]
    g, r_ = got[rows].double(), ref[rows].double()
    per = ((g - r_).norm(dim=1) / r_.norm(dim=1).clamp_min(1e-30)).max().item()
    assert per < tol, (what, "worst boundary row", per)


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))


def _gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x * 0.5 ** 0.5)) + x * torch.exp(-0.5 * x * x) * (2.0 * torch.pi) ** -0.5
