"""Time and peak memory of the two routes to a top-k rank list (editor_amd.metrics), in one run on one box:
    old     euclidean_distance + argsort_rows + slice   (Q x G fp32 matrix, Q x P 64-bit keys, Q x G int32 order)
    search  gallery blocks of `chunk` rows through editor_distmat_f32 into a running top-k (csrc/rank_topk.hip)
at the RGBNT100 test split's size (1 715 queries, 8 575 gallery images, 2 304-wide features) and at one deployment size
(256 queries against 1 000 000 gallery rows), k = 50, unfiltered.  Peak memory is the rise of torch.cuda.max_memory_allocated()
over the features.  The first line is bench.source_hash() of the tree that ran.

    python tools/search_time.py > profiles/search_time.txt
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from editor_amd import metrics  # noqa: E402

K = 50
SIZES = ((1715, 8575, 2304), (256, 1000000, 2304))


def old_route(qf, gf):
    order = metrics.argsort_rows(metrics.euclidean_distance(qf, gf))
    return order[:, :K].contiguous()


def new_route(qf, gf):
    return metrics.search(qf, gf, K)[0]


def measure(fn, qf, gf, reps):
    fn(qf[:8], gf[:4096])                                        # library loaded, allocator warm
    best, peak, out = None, 0, None
    for _ in range(reps):
        del out
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = fn(qf, gf)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
    return best, peak, out


def main():
    print("source hash: %s" % bench.source_hash())
    print("device: %s, k = %d, chunk = 16384, unfiltered, best of 3 (wall time, synchronised)" % (torch.cuda.get_device_name(0), K))
    for nq, ng, d in SIZES:
        gen = torch.Generator(device="cuda").manual_seed(nq + ng)
        qf = metrics.normalize(torch.randn(nq, d, device="cuda", generator=gen))
        gf = torch.empty(ng, d, device="cuda")
        for s in range(0, ng, 65536):                            # normalised block by block: one copy of the gallery at a time
            gf[s:s + 65536] = metrics.normalize(torch.randn(min(65536, ng - s), d, device="cuda", generator=gen))
        t_old, m_old, i_old = measure(old_route, qf, gf, 3)
        t_new, m_new, i_new = measure(new_route, qf, gf, 3)
        same = torch.equal(i_old, i_new)
        print("Q = %d, G = %d, D = %d   (features %.2f GB, a Q x G fp32 matrix %.1f MB)" %
              (nq, ng, d, (nq + ng) * d * 4 / 2 ** 30, nq * ng * 4 / 2 ** 20))
        print("  old route (distmat + full sort + slice)  %9.2f ms   peak memory +%9.1f MB" % (1e3 * t_old, m_old / 2 ** 20))
        print("  search    (blocked distmat + top-k)      %9.2f ms   peak memory +%9.1f MB" % (1e3 * t_new, m_new / 2 ** 20))
        print("  time x %.2f, memory x %.4f of the old route; rank lists identical: %s" % (t_new / t_old, m_new / m_old, same))
        del qf, gf, i_old, i_new
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
