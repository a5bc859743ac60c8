"""Row N1 (loss head), the cfg's options: make_loss over NO_MARGIN / IF_LABELSMOOTH / SAMPLER and losses.TripletLoss(margin,
hard_factor)(feat, labels, normalize_feature) through the C ABI (editor_triplet_loss_fwd, editor_normalize_rows_*) against the golden
captured from the reference's own layers.make_loss / layers.triplet_loss (tests/golden/loss_options.npz, written by
tests/golden/capture_loss_options.py, which chose inputs away from every discontinuity and recorded the conditions), and - for
identities of unequal size, which the reference cannot run - against the masked max / min restatement of loss_options_helpers.

Bounds (norm-wise rel_err against the reference's fp32 output, tests/test_gpu_loss.py's): 1e-5 triplet loss and distances, 1e-6
cross-entropy, 1e-5 dscore, 2e-5 dfeat.  The hinge loss is a mean of small differences of distances, so its bound is
|dloss| <= 1e-5 |loss| + 1e-6 (mean d_ap + mean d_an): the distance accuracy propagated through z.
"""
import math
from types import SimpleNamespace

import pytest
import torch

import loss_options_helpers as H
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("loss_options")


def _set_inputs(g, b, k, d, hf, norm):
    a_max, seed = g["cond/" + H.set_key(b, d, hf, norm)][:2]
    target = H.labels(int(seed), b, k)
    return H.features(int(seed), target, d, float(a_max)), target, int(seed)


def _loss_ok(got, ref, ref_tri, margin, dist_mean, ce=0.0):
    bound = H.BOUND_TRIPLET * abs(ref_tri) + H.BOUND_CE * abs(ce)
    if margin is not None:
        bound += H.BOUND_HINGE_DIST * dist_mean
    err = abs(float(got) - float(ref))
    print("loss %.9g ref %.9g |d| %.3e bound %.3e" % (float(got), float(ref), err, bound))
    return err <= bound


def _cfg(no_margin, smooth, sampler, idw=1.0, trw=1.0):
    return SimpleNamespace(DATALOADER=SimpleNamespace(SAMPLER=sampler),
                           MODEL=SimpleNamespace(METRIC_LOSS_TYPE="triplet", NO_MARGIN=no_margin, IF_LABELSMOOTH=smooth,
                                                 ID_LOSS_WEIGHT=idw, TRIPLET_LOSS_WEIGHT=trw),
                           SOLVER=SimpleNamespace(MARGIN=0.3))


@pytest.mark.parametrize("name", list(H.MAKE_LOSS_CASES))
def test_make_loss_follows_cfg(golden, name):
    """Case 1: the reference's make_loss per cfg; 'nm0_*' (NO_MARGIN False) is the hinge the cfg asks for."""
    from editor_amd import losses
    g = golden
    no_margin, smooth, sampler = H.MAKE_LOSS_CASES[name]
    b, k, d, c = H.MAKE_LOSS_SHAPE
    feat, target, seed = _set_inputs(g, b, k, d, 0.0, False)
    score = H.scores(seed, b, c).cuda().requires_grad_(True)
    feat = feat.cuda().requires_grad_(True)
    loss_fn, center = losses.make_loss(_cfg(no_margin, smooth, sampler), num_classes=c)
    assert center.centers.shape == (c, 2048)
    loss = loss_fn(score=score, feat=feat, target=target.cuda(), target_cam=None)
    loss.backward()
    ref, tri = float(g["ml_%s/loss" % name]), float(g["ml_%s/loss_tri" % name])
    assert _loss_ok(loss.item(), ref, tri, None if no_margin else 0.3, float(g["ml_%s/dist_mean" % name]), ce=ref - tri)
    assert rel_err(score.grad.cpu(), g["ml_%s/dscore" % name]) < H.BOUND_DSCORE
    if sampler == "softmax":
        assert feat.grad is None                                       # cross-entropy alone: the features are not read
        return
    assert rel_err(feat.grad[:, :64].cpu(), g["ml_%s/dfeat" % name]) < H.BOUND_DFEAT
    assert rel_err(feat.grad.norm(dim=1).cpu(), g["ml_%s/dfeat_rownorm" % name]) < H.BOUND_DFEAT
    assert abs(feat.grad.norm().item() / float(g["ml_%s/dfeat_norm" % name]) - 1) < H.BOUND_DFEAT


@pytest.mark.parametrize("norm", H.NORMALIZE)
@pytest.mark.parametrize("hf", H.HARD_FACTORS)
@pytest.mark.parametrize("b,k,d", H.SHAPES)
def test_triplet_loss_matches_reference_golden(golden, b, k, d, hf, norm):
    """Case 2: TripletLoss(margin, hard_factor)(strided column slice, labels, normalize_feature) for margin 0.3 and None."""
    from editor_amd import losses
    g = golden
    feat, target, _ = _set_inputs(g, b, k, d, hf, norm)
    rows = H.stored_rows(b)
    up = float(g["up"])
    for margin in H.MARGINS:
        key = H.case_key(b, d, margin, hf, norm)
        wide = torch.zeros(b, d + 16)
        wide[:, 8:8 + d] = feat                                        # features arrive as a strided column slice
        wg = wide.cuda().requires_grad_(True)
        loss, d_ap, d_an = losses.TripletLoss(margin, hf)(wg[:, 8:8 + d], target.cuda(), normalize_feature=norm)
        assert not d_ap.requires_grad and not d_an.requires_grad and d_ap.dtype == torch.float32 and d_ap.shape == (b,) == d_an.shape
        (up * loss).backward()
        assert not wg.grad[:, :8].any() and not wg.grad[:, 8 + d:].any()
        df = wg.grad[:, 8:8 + d]
        ref_ap, ref_an = torch.from_numpy(g[key + "/dist_ap"]), torch.from_numpy(g[key + "/dist_an"])
        e = (rel_err(d_ap.cpu(), ref_ap), rel_err(d_an.cpu(), ref_an), rel_err(df[rows.cuda(), :64].cpu(), g[key + "/dfeat"]),
             rel_err(df.norm(dim=1).cpu(), g[key + "/dfeat_rownorm"]))
        print(key, "dist_ap %.2e dist_an %.2e dfeat %.2e rownorm %.2e" % e)
        ref = float(g[key + "/loss"])
        assert _loss_ok(loss.item(), ref, ref, margin, ref_ap.mean().item() + ref_an.mean().item()), key
        assert e[0] < H.BOUND_DIST and e[1] < H.BOUND_DIST, key
        assert e[2] < H.BOUND_DFEAT and e[3] < H.BOUND_DFEAT, key
        assert abs(df.norm().item() / float(g[key + "/dfeat_norm"]) - 1) < H.BOUND_DFEAT, key


UNEQUAL = {(6, 33): (1, 2.0), (260, 768): (61, 3.0)}       # (B, D) -> (seed, a_max) whose inputs meet conditions (b), (c) for all options


@pytest.mark.parametrize("b,d", list(UNEQUAL))
def test_unequal_identities_match_masked_restatement(b, d):
    """Case 3: identities of sizes 2 - 4 and one single-instance identity, against the masked max / min restatement in float64 on the
    CPU.  The singleton's only positive is itself: the restatement's d_ap there is the clamp floor 1e-6, the kernel's is the rounding
    of q_ii = 2 sq_i - 2 gram_ii, two fp32 sums of the same D products in different orders, each within D u sq_i of the exact value
    (u = 2^-24), so d_ap <= 2 sqrt(D u sq_i) (1 + hard_factor).  That element is held to this bound and left out of the vector
    comparison; its gradient term is (f_i - f_i) = 0 either way."""
    from editor_amd import losses
    seed, a_max = UNEQUAL[(b, d)]
    target = H.unequal_labels(seed, b)
    single = int((target == target.max()).nonzero().item())
    assert (target == target.max()).sum() == 1
    feat = H.features(seed, target, d, a_max)
    keep = torch.arange(b) != single
    for margin in H.MARGINS:
        for hf in H.HARD_FACTORS:
            for norm in H.NORMALIZE:
                c = H.conditions(feat, target, margin, hf, norm)
                assert c["hinge_gap"] >= H.HINGE_GAP and c["runner_up"] >= H.RUNNER_UP_GAP, ("inputs sit on a discontinuity", c)
                fr = feat.double().requires_grad_(True)
                ref, ref_ap, ref_an, _ = H.masked_triplet(fr, target, margin, hf, norm)
                ref.backward()
                fg = feat.cuda().requires_grad_(True)
                loss, d_ap, d_an = losses.TripletLoss(margin, hf)(fg, target.cuda(), normalize_feature=norm)
                loss.backward()
                tag = (margin, hf, norm)
                assert _loss_ok(loss.item(), ref.item(), ref.item(), margin, (ref_ap.mean() + ref_an.mean()).item()), tag
                sq = 1.0 if norm else float((feat[single].double() ** 2).sum())
                assert d_ap[single].item() <= 2 * math.sqrt(d * 2.0 ** -24 * sq) * (1 + hf) + 1e-6, tag
                assert rel_err(d_ap.cpu()[keep], ref_ap.detach()[keep]) < H.BOUND_DIST, tag
                assert rel_err(d_an.cpu(), ref_an.detach()) < H.BOUND_DIST, tag
                assert rel_err(fg.grad.cpu(), fr.grad) < H.BOUND_DFEAT, tag


def test_list_valued_outputs_and_target_repeat():
    """Case 4: make_loss.py:37-38 (target repeated to the features' batch) and :41-51,58-68 (a list is 0.5 * mean(tail) + 0.5 * head),
    with both weights off 1.0, against the same assembly of the float64 restatements."""
    from editor_amd import losses
    b, d, c, seed = 8, 33, 7, 2
    target = torch.arange(4)
    full = target.repeat(2)
    feats = [H.features(seed + i, full, d, 2.0) for i in range(3)]
    scores = [H.scores(seed + i, b, c) for i in range(3)]
    for f in feats:
        cond = H.conditions(f, full, 0.3, 0.0, False)
        assert cond["hinge_gap"] >= H.HINGE_GAP and cond["runner_up"] >= H.RUNNER_UP_GAP, ("inputs sit on a discontinuity", cond)

    def assemble(terms):
        tail = sum(terms[1:]) / len(terms[1:])
        return 0.5 * tail + 0.5 * terms[0]

    for no_margin, smooth in ((False, "off"), (True, "on")):
        fr = [f.double().requires_grad_(True) for f in feats]
        sr = [s.double().requires_grad_(True) for s in scores]
        ce = assemble([torch.nn.functional.cross_entropy(s, full, label_smoothing=0.1 if smooth == "on" else 0.0) for s in sr])
        tri = assemble([H.masked_triplet(f, full, None if no_margin else 0.3)[0] for f in fr])
        ref = 0.5 * ce + 2.0 * tri
        ref.backward()
        fg = [f.cuda().requires_grad_(True) for f in feats]
        sg = [s.cuda().requires_grad_(True) for s in scores]
        loss_fn, _ = losses.make_loss(_cfg(no_margin, smooth, "softmax_triplet", idw=0.5, trw=2.0), num_classes=c)
        loss = loss_fn(score=sg, feat=fg, target=target.cuda(), target_cam=None)
        loss.backward()
        with torch.no_grad():
            dm = sum(sum(v.mean().item() for v in H.masked_triplet(f.double(), full, 0.3)[1:3]) for f in feats) / 3
        assert _loss_ok(loss.item(), ref.item(), 2.0 * tri.item(), None if no_margin else 0.3, 2.0 * dm, ce=0.5 * ce.item())
        for a, r in zip(sg, sr):
            assert rel_err(a.grad.cpu(), r.grad) < H.BOUND_DSCORE
        for a, r in zip(fg, fr):
            assert rel_err(a.grad.cpu(), r.grad) < H.BOUND_DFEAT
    # a plain tensor with a short target: the repeat alone
    loss_fn, _ = losses.make_loss(_cfg(False, "off", "softmax_triplet"), num_classes=c)
    a = loss_fn(score=scores[0].cuda(), feat=feats[0].cuda(), target=target.cuda(), target_cam=None)
    e = loss_fn(score=scores[0].cuda(), feat=feats[0].cuda(), target=full.cuda(), target_cam=None)
    assert torch.equal(a, e)


@pytest.mark.parametrize("b,k,d", [(6, 2, 33), (32, 8, 2304)])
@pytest.mark.parametrize("bad", [math.nan, math.inf])
def test_non_finite_row_poisons_loss_and_gradient(golden, b, k, d, bad):
    """Case 5: one feature row NaN / inf (an overflowed f16 step): every anchor has that row among its positives or its negatives, so
    the loss is NaN and every gradient row non-finite, in both forms and with and without normalisation - the update is skipped."""
    from editor_amd import losses
    feat, target, _ = _set_inputs(golden, b, k, d, 0.0, False)
    feat = feat.clone()
    feat[b // 2] = bad
    for margin in H.MARGINS:
        for norm in H.NORMALIZE:
            fg = feat.cuda().requires_grad_(True)
            loss, d_ap, d_an = losses.TripletLoss(margin, 0.2)(fg, target.cuda(), normalize_feature=norm)
            loss.backward()
            assert torch.isnan(loss).item(), (margin, norm)
            assert bool((~torch.isfinite(fg.grad)).any(dim=1).all()), (margin, norm)
            assert bool((torch.isnan(d_ap) | torch.isnan(d_an)).all()), (margin, norm)


@pytest.mark.parametrize("b,k,d", [(128, 16, 2304), (260, 4, 768)])
def test_defaults_keep_their_bits_and_runs_repeat(golden, b, k, d):
    """Case 6: TripletLoss()(f, t)[0] and its gradient are triplet_soft_margin(f, t)'s bits; two runs of every new path agree bit
    for bit (fixed-order reductions, no atomics)."""
    from editor_amd import losses
    feat, target, _ = _set_inputs(golden, b, k, d, 0.0, False)
    tg = target.cuda()
    f0, f1 = feat.cuda().requires_grad_(True), feat.cuda().requires_grad_(True)
    l0 = losses.triplet_soft_margin(f0, tg)
    l1 = losses.TripletLoss()(f1, tg)[0]
    (0.37 * l0).backward()
    (0.37 * l1).backward()
    assert torch.equal(l0, l1) and torch.equal(f0.grad, f1.grad)
    for margin in H.MARGINS:
        for norm in H.NORMALIZE:
            runs = []
            for _ in range(2):
                f = feat.cuda().requires_grad_(True)
                out = losses.TripletLoss(margin, 0.2)(f, tg, normalize_feature=norm)
                out[0].backward()
                runs.append([o.detach().clone() for o in out] + [f.grad.clone()])
            assert all(torch.equal(x, y) for x, y in zip(*runs)), (margin, norm)


def test_margin_form_with_normalisation_replays_in_a_graph(golden):
    """Case 7: forward + backward of TripletLoss(0.3, 0.2)(f, t, normalize_feature=True) captured into a graph and replayed twice with
    changed inputs: each replay equals the eager result bit for bit (no host synchronisation, no data-dependent host control flow)."""
    from editor_amd import losses
    b, k, d = 128, 16, 2304
    crit = losses.TripletLoss(0.3, 0.2)
    inputs = []
    for hf, norm in ((0.0, False), (0.2, True), (0.2, False)):
        feat, target, _ = _set_inputs(golden, b, k, d, hf, norm)
        inputs.append((feat.cuda(), target.cuda()))

    def step(f, t):
        loss, d_ap, d_an = crit(f, t, normalize_feature=True)
        grad, = torch.autograd.grad(loss, f)
        return loss, d_ap, d_an, grad

    eager = [[o.detach().clone() for o in step(f.clone().requires_grad_(True), t)] for f, t in inputs]
    sf, st = inputs[0][0].clone().requires_grad_(True), inputs[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sf, st)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(sf, st)
    for (f, t), ref in zip(inputs[1:], eager[1:]):
        with torch.no_grad():
            sf.copy_(f)
            st.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o, r) for o, r in zip(out, ref))


def test_cross_entropy_classes_and_center_loss_labels():
    """CrossEntropyLabelSmooth / LabelSmoothingCrossEntropy / cross_entropy over the one kernel, against torch's float64
    F.cross_entropy; CenterLoss takes CPU and int32 labels (moved to the features' device as int64)."""
    from editor_amd import losses
    b, c = 37, 171
    score = H.scores(5, b, c)
    target = torch.arange(b) * 4 % c
    for fn, eps in ((losses.CrossEntropyLabelSmooth(c), 0.1), (losses.CrossEntropyLabelSmooth(c, epsilon=0.25, use_gpu=True), 0.25),
                    (losses.LabelSmoothingCrossEntropy(), 0.1), (losses.LabelSmoothingCrossEntropy(smoothing=0.3), 0.3),
                    (losses.cross_entropy, 0.0)):
        sr = score.double().requires_grad_(True)
        ref = torch.nn.functional.cross_entropy(sr, target, label_smoothing=eps)
        ref.backward()
        sg = score.cuda().requires_grad_(True)
        got = fn(sg, target.cuda())
        got.backward()
        assert rel_err(got.detach().cpu(), ref.detach()) < H.BOUND_CE and rel_err(sg.grad.cpu(), sr.grad) < H.BOUND_DSCORE
    x = H.features(3, torch.arange(8) % 4, 48, 1.0).cuda()
    cl = losses.CenterLoss(num_classes=4, feat_dim=48).cuda()
    lab = (torch.arange(8) % 4).cuda()
    want = cl(x, lab)
    assert torch.equal(cl(x, lab.cpu()), want) and torch.equal(cl(x, lab.to(torch.int32)), want)
