"""Generate tests/golden/f20_rank_lists.npz from the REFERENCE's eval_func_msrv (run in the build container only).

    python tests/golden/capture_rank_lists.py

F20 (row N2): the `re.txt` rank-list dump of utils/metrics.py:59-60,92-99.  Two runs:
  a  the f8 case (capture_golden.retrieval_case(71, 48, 200, 64, 12, 4)), max_rank 50
  b  a tiny case, nq = 6, ng = 9, 3 ids, 2 scenes, max_rank 50: the reference clips to 9, and the junk removal leaves lists
     of unequal length
     (the reference writes its `re.txt` in full and then fails to stack its ragged cmc rows, so run b records no cmc / mAP)
Per run the fixture holds the reference's full fp32 distance matrix, the id arrays, the bytes of `re.txt` and, for run a, its
cmc / mAP: recorded data only, nothing of the reference's text.
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from editor_amd import synth          # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def retrieval_case(seed, nq, ng, d, ids, cams, scenes=3):
    """capture_golden.retrieval_case with the number of scenes as an argument."""
    n = nq + ng
    pids = synth.integers(seed, "ret/pid", (n,), ids).numpy()
    camids = synth.integers(seed, "ret/cam", (n,), cams).numpy()
    scene = synth.integers(seed, "ret/scene", (n,), scenes).numpy()
    proto = synth.normal(seed, "ret/proto", (ids, d), 1.0)
    feats = proto[torch.from_numpy(pids)] * 0.6 + synth.normal(seed, "ret/noise", (n, d), 1.0)
    return feats, pids, camids, scene


def run(M, tag, seed, nq, ng, d, ids, cams, scenes, out, ragged_ok=False):
    feats, pids, camids, scene = retrieval_case(seed, nq, ng, d, ids, cams, scenes)
    nrm = torch.nn.functional.normalize(feats, dim=1, p=2)
    dist = M.euclidean_distance(nrm[:nq], nrm[nq:])
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:       # eval_func_msrv writes re.txt into the cwd
        os.chdir(tmp)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                try:
                    cmc, m_ap = M.eval_func_msrv(dist, pids[:nq], pids[nq:], camids[:nq], camids[nq:], scene[:nq],
                                                 scene[nq:], max_rank=50)
                except ValueError:
                    # run b: with fewer than max_rank kept entries in some rows the reference's cmc rows have unequal
                    # lengths and its np.asarray(all_cmc) (utils/metrics.py:125) refuses them - AFTER the query loop, so
                    # re.txt is complete.  No cmc / mAP is recorded for such a run.
                    if not ragged_ok:
                        raise
                    cmc = m_ap = None
            text = open("re.txt", "rb").read()
        finally:
            os.chdir(cwd)
    assert text.count(b":\n") == nq
    out.update({tag + "_dist": dist.astype(np.float32), tag + "_q_pids": pids[:nq], tag + "_g_pids": pids[nq:],
                tag + "_q_cams": camids[:nq], tag + "_g_cams": camids[nq:], tag + "_q_scenes": scene[:nq],
                tag + "_g_scenes": scene[nq:], tag + "_seed": np.int64(seed),
                tag + "_re_txt": np.frombuffer(text, dtype=np.uint8)})
    if cmc is not None:
        out.update({tag + "_cmc": cmc, tag + "_mAP": np.float64(m_ap)})


def main():
    np.str = str                                     # utils/metrics.py:47 uses the removed alias
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, "/root/reference")
    import utils.metrics as M
    out = {}
    run(M, "a", 71, 48, 200, 64, 12, 4, 3, out)
    run(M, "b", 73, 6, 9, 16, 3, 2, 2, out, ragged_ok=True)
    path = os.path.join(OUT, "f20_rank_lists.npz")
    np.savez_compressed(path, **out)
    print("wrote f20_rank_lists", os.path.getsize(path) // 1024, "KiB")
    for tag in ("a", "b"):
        print(tag, "lines", bytes(out[tag + "_re_txt"]).count(b"\n"))


if __name__ == "__main__":
    main()
