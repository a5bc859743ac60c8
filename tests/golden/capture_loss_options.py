"""Generate tests/golden/loss_options.npz from the REFERENCE's own layers.make_loss / layers.triplet_loss (build container only).

    python tests/golden/capture_loss_options.py

Same protocol as capture_golden.py::f7_loss (whose helpers it imports): the reference runs on the CPU through tools/ref_shims.py on
inputs regenerated from editor_amd/synth.py seeds (tests/loss_options_helpers.py), and only small OUTPUTS are stored: the loss,
dist_ap, dist_an, dscore, dfeat[:, :64] (at most 64 rows of it, see helpers.stored_rows, with the norm of EVERY row beside it),
||dfeat||, and the seeds and conditions below.

Per feature set (shape x hard_factor x normalize_feature; both margin settings share it) the script searches (a_max, seed) until
  (a) between 25 % and 75 % of anchors have an active hinge at margin 0.3,
  (b) no anchor lies within 1e-3 * d_ap of the hinge,
  (c) every anchor's hardest positive and hardest negative beat their runners-up by >= 1e-5 relative (fp32 distance noise is about
      1e-7, so a mined pair cannot flip),
  (d) the reference's fp32 result differs from its own float64 run by at most a quarter of the test bound, for every compared
      quantity,
and records `cond/<set>` = [a_max, seed, active, hinge_gap, runner_up, worst (fp32 - float64) / bound].
"""
import contextlib
import importlib
import io
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
import capture_golden as cg                    # noqa: E402  (sets sys.path for the repository root, seeds, thread count)
import loss_options_helpers as H               # noqa: E402
from tools import ref_shims                    # noqa: E402

UP = 0.37                                      # upstream gradient of the TripletLoss cases: d(UP * loss)


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def loss_bound(loss, margin, d_ap, d_an, ce=0.0):
    """The test's bound on |dloss| for a triplet term `loss` (+ a cross-entropy term ce)."""
    b = H.BOUND_TRIPLET * abs(loss) + H.BOUND_CE * abs(ce)
    if margin is not None:
        b += H.BOUND_HINGE_DIST * (d_ap.mean().item() + d_an.mean().item())
    return b


def run_triplet(tl, feat, target, margin, hf, norm, dtype):
    f = feat.detach().to(dtype).clone().requires_grad_(True)
    loss, d_ap, d_an = tl.TripletLoss(margin, hf)(f, target, normalize_feature=norm)
    (UP * loss).backward()
    return loss.detach(), d_ap.detach(), d_an.detach(), f.grad


def triplet_set(tl, b, k, d, hf, norm, rec):
    for a_max in H.A_MAX:
        for seed in range(1, 41):
            target = H.labels(seed, b, k)
            feat = H.features(seed, target, d, a_max)
            c = H.conditions(feat, target, 0.3, hf, norm)
            if not (0.25 <= c["active"] <= 0.75 and c["hinge_gap"] >= H.HINGE_GAP and c["runner_up"] >= H.RUNNER_UP_GAP):
                continue
            out, worst = {}, 0.0
            for margin in H.MARGINS:
                l32, ap32, an32, g32 = run_triplet(tl, feat, target, margin, hf, norm, torch.float32)
                l64, ap64, an64, g64 = run_triplet(tl, feat, target, margin, hf, norm, torch.float64)
                rows = H.stored_rows(b)
                worst = max(worst, abs(l32.item() - l64.item()) / loss_bound(l32.item(), margin, ap32, an32),
                            rel(ap32, ap64) / H.BOUND_DIST, rel(an32, an64) / H.BOUND_DIST,
                            rel(g32[rows, :64], g64[rows, :64]) / H.BOUND_DFEAT, rel(g32.norm(dim=1), g64.norm(dim=1)) / H.BOUND_DFEAT)
                key = H.case_key(b, d, margin, hf, norm)
                out.update({key + "/loss": l32, key + "/dist_ap": ap32, key + "/dist_an": an32, key + "/dfeat": g32[rows, :64],
                            key + "/dfeat_rownorm": g32.norm(dim=1), key + "/dfeat_norm": g32.norm()})
            if worst > 0.25:
                continue
            rec.update(out)
            rec["cond/" + H.set_key(b, d, hf, norm)] = np.asarray([a_max, seed, c["active"], c["hinge_gap"], c["runner_up"], worst])
            print(H.set_key(b, d, hf, norm), "a_max", a_max, "seed", seed, "active %.2f gap %.1e runner-up %.1e floor/bound %.3f"
                  % (c["active"], c["hinge_gap"], c["runner_up"], worst))
            return
    raise AssertionError("no (a_max, seed) meets the conditions for " + H.set_key(b, d, hf, norm))


def make_loss_cases(mk, tl, rec):
    """layers.make_loss over NO_MARGIN x IF_LABELSMOOTH and SAMPLER 'softmax' on the (32, 8, 2304) set, C = 171."""
    b, k, d, c = H.MAKE_LOSS_SHAPE
    a_max, seed = rec["cond/" + H.set_key(b, d, 0.0, False)][:2]
    seed = int(seed)
    target = H.labels(seed, b, k)
    feat, score = H.features(seed, target, d, float(a_max)), H.scores(seed, b, c)
    worst = 0.0
    for name, (no_margin, smooth, sampler) in H.MAKE_LOSS_CASES.items():
        cfg = SimpleNamespace(DATALOADER=SimpleNamespace(SAMPLER=sampler),
                              MODEL=SimpleNamespace(METRIC_LOSS_TYPE="triplet", NO_MARGIN=no_margin, IF_LABELSMOOTH=smooth,
                                                    ID_LOSS_WEIGHT=1.0, TRIPLET_LOSS_WEIGHT=1.0),
                              SOLVER=SimpleNamespace(MARGIN=0.3))
        with contextlib.redirect_stdout(io.StringIO()):
            loss_fn, _ = mk.make_loss(cfg, num_classes=c)
        res = {}
        for dtype in (torch.float32, torch.float64):
            s, f = (v.detach().to(dtype).clone().requires_grad_(True) for v in (score, feat))
            loss = loss_fn(score=s, feat=f, target=target, target_cam=None)
            loss.backward()
            res[dtype] = (loss.detach(), s.grad, f.grad)
        (l32, ds32, df32), (l64, ds64, df64) = res[torch.float32], res[torch.float64]
        margin = None if no_margin else 0.3
        if sampler == "softmax":
            tri, ap, an = 0.0, torch.zeros(1), torch.zeros(1)
            assert df32 is None
            bound = H.BOUND_CE * abs(l32.item())
        else:
            with torch.no_grad():
                tri, ap, an = tl.TripletLoss(margin)(feat, target)
            tri = tri.item()
            bound = loss_bound(tri, margin, ap, an, ce=l32.item() - tri)
            worst = max(worst, rel(df32, df64) / H.BOUND_DFEAT)
            rec.update({"ml_%s/dfeat" % name: df32[:, :64], "ml_%s/dfeat_norm" % name: df32.norm(),
                        "ml_%s/dfeat_rownorm" % name: df32.norm(dim=1)})
        worst = max(worst, abs(l32.item() - l64.item()) / bound, rel(ds32, ds64) / H.BOUND_DSCORE)
        rec.update({"ml_%s/loss" % name: l32, "ml_%s/loss_tri" % name: np.float32(tri), "ml_%s/dscore" % name: ds32,
                    "ml_%s/dist_mean" % name: np.float32(ap.mean().item() + an.mean().item())})
    assert worst <= 0.25, worst
    rec["cond/make_loss"] = np.asarray([a_max, seed, worst])
    print("make_loss cases: floor/bound %.3f" % worst)


if __name__ == "__main__":
    assert ref_shims.have_reference(), "run in the build container (needs the reference checkout)"
    ref_shims.install()
    mk = importlib.import_module("layers.make_loss")
    tl = importlib.import_module("layers.triplet_loss")
    rec = {"up": np.float32(UP)}
    for (b, k, d) in H.SHAPES:
        for hf in H.HARD_FACTORS:
            for norm in H.NORMALIZE:
                triplet_set(tl, b, k, d, hf, norm, rec)
    make_loss_cases(mk, tl, rec)
    cg.save("loss_options", **rec)
