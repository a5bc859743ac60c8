"""Retrieval evaluation over the hot path's eval-mode features - row N2 of SURVEY.md 8(f).

Host-side mirror of the reference's utils/metrics.py (same names, argument meaning and return values) over the HIP
kernels of csrc/retrieval.hip; there is no CPU fallback.
    euclidean_distance(qf, gf)                                     utils/metrics.py:12-18
    eval_func(distmat, q_pids, g_pids, q_camids, g_camids, ...)    utils/metrics.py:132-191
    eval_func_msrv(..., q_sceneids, g_sceneids, ...)               utils/metrics.py:34-129  (MSVR310 protocol)
    R1_mAP_eval / R1_mAP                                           utils/metrics.py:242-283 / 193-239
Differences, all deliberate: distance matrices stay on the device (pass `.cpu().numpy()` yourself if a numpy array is
wanted - `compute()` does, as the reference returns one); exactly tied distances rank by gallery index (numpy's default
argsort leaves their order unspecified); eval_func_msrv's `re.txt` rank-list dump is written on request (rank_file=path), not
into the working directory of every call.
    re_ranking(qf, gf, k1, k2, lambda_value)                       utils/reranking.py:30-101 (R1_mAP_eval(reranking=True), :275-278)
Rank lists - the first k kept entries of each query's ranking, what `re.txt` holds (utils/metrics.py:92-99) - come from a running
top-k selection (csrc/rank_topk.hip), not from the full ranking:
    rank_lists(distmat, q_pids, g_pids, q_aux, g_aux, max_rank)    from a device distance matrix; no sort, no Q x P key buffer
    search(qf, gf, k, q_pids, g_pids, q_aux, g_aux, chunk)         from features, gallery block by block; no Q x G matrix
    format_rank_file(index, ...)                                   the text of `re.txt` from a host index array
"""
import numpy as np
import torch

from ._lib import call


def _dev(a, dtype, device):
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return t.to(device=device, dtype=dtype).contiguous()


def _rows(x):
    x = x.float()
    return x if x.stride(-1) == 1 else x.contiguous()


def normalize(feats, eps=1e-12):
    """torch.nn.functional.normalize(feats, dim=1, p=2)."""
    feats = _rows(feats)
    m, d = feats.shape
    out = torch.empty(m, d, dtype=torch.float32, device=feats.device)
    call("editor_l2norm_rows", feats.data_ptr(), feats.stride(0), m, d, float(eps), out)
    return out


def euclidean_distance(qf, gf):
    """(m, n) fp32 squared-distance matrix, on the device."""
    qf, gf = _rows(qf), _rows(gf)
    m, n, d = qf.shape[0], gf.shape[0], qf.shape[1]
    assert gf.shape[1] == d
    dist = torch.empty(m, n, dtype=torch.float32, device=qf.device)
    qq = torch.empty(m, dtype=torch.float32, device=qf.device)
    gg = torch.empty(n, dtype=torch.float32, device=qf.device)
    call("editor_distmat_f32", qf.data_ptr(), qf.stride(0), gf.data_ptr(), gf.stride(0), m, n, d, qq, gg, dist)
    return dist


def argsort_rows(distmat):
    """np.argsort(distmat, axis=1) as an int32 device tensor (ties by ascending column)."""
    q, g = distmat.shape
    p = 2
    while p < g:
        p *= 2
    keys = torch.empty(q * p, dtype=torch.int64, device=distmat.device)
    order = torch.empty(q, g, dtype=torch.int32, device=distmat.device)
    call("editor_rank_sort", distmat, q, g, p, keys, order)
    return order


def re_ranking(probFea, galFea, k1, k2, lambda_value, local_distmat=None, only_local=False):
    """k-reciprocal re-ranking (utils/reranking.py:30-101) on the device: (Q, G) fp32 final distance, a device tensor.
    Dense N x N stages over all N = Q + G images (csrc/rerank.hip).  The reference's float16 storage / arithmetic is followed
    operation by operation: every stage is bit-equal to numpy's FROM THE SAME INPUTS (tests/test_gpu_retrieval.py); end to end the
    result is tolerance-close, not bit-equal - expf differs from numpy's exp in the last place and near-tied distances can order
    differently.  Limits (checked here, documented divergences from the reference, which slices short neighbour lists silently and
    takes any k1): k1 <= 63, N >= k1 + 1, N <= 65 535 - the evaluator's call (utils/metrics.py:278: k1=50, k2=15, lambda=0.3) is inside
    all of them.  local_distmat (N, N; numpy or tensor): added to the global distance matrix before the normalisation
    (reranking.py:44-45) or, with only_local, used instead of it (:32-33) - one elementwise add on the device, the evaluator passes
    neither."""
    if only_local and local_distmat is None:
        raise ValueError("re_ranking(only_local=True) needs local_distmat")
    qf, gf = _rows(probFea), _rows(galFea)
    if not qf.is_cuda:
        raise RuntimeError("re_ranking: features must be on the GPU (there is no CPU fallback)")
    nq, n = qf.shape[0], qf.shape[0] + gf.shape[0]
    if n > 65535:
        raise ValueError("re_ranking: at most 65 535 images (query + gallery) - the device stages index rows through grid.y")
    if int(k1) > 63 or int(k1) + 1 > n:
        raise ValueError("re_ranking: k1 <= 63 and k1 + 1 <= Q + G (the device kernel holds a neighbour list of k1 + 1 in LDS)")
    dev = qf.device
    local = None
    if local_distmat is not None:
        local = torch.as_tensor(np.asarray(local_distmat) if not isinstance(local_distmat, torch.Tensor) else local_distmat)
        local = local.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(local.shape) != (n, n):
            raise ValueError("re_ranking: local_distmat must be (Q + G, Q + G)")
    if only_local:
        dist = local
    else:
        feat = torch.cat([qf, gf]).contiguous()
        dist = euclidean_distance(feat, feat)
        if local is not None:
            dist = dist + local
    od = torch.empty(n, n, dtype=torch.float32, device=dev)
    call("editor_rerank_normalise", dist, n, torch.empty(n, dtype=torch.float32, device=dev), od)
    del dist
    rank = argsort_rows(od)
    v = torch.empty(n, n, dtype=torch.float16, device=dev)
    call("editor_rerank_weights", od, rank, n, int(k1), int(np.around(k1 / 2)), v)
    if k2 != 1:
        vq = torch.empty_like(v)
        call("editor_rerank_expand", v, rank, n, int(k2), vq)
        v = vq
    del rank
    final = torch.empty(nq, n - nq, dtype=torch.float32, device=dev)
    w16 = int(np.float16(1 - lambda_value).view(np.uint16))
    call("editor_rerank_final", v, torch.empty_like(v), od, n, nq, w16, float(np.float32(lambda_value)), final)
    return final


MAX_RANK_LIST = 1024           # editor_rank_topk's K limit, the cap editor_rank_metrics has
MAX_GALLERY = 2 ** 31 - 1      # a key's low word holds the gallery index, and an all-ones key marks an empty slot


def _list_args(what, num_q, num_g, q_pids, g_pids, q_aux, g_aux, max_rank):
    """Argument checks shared by rank_lists and search -> (ids or None, max_rank clipped to the gallery as eval_func clips it)."""
    ids = (q_pids, g_pids, q_aux, g_aux)
    given = sum(a is not None for a in ids)
    if given not in (0, 4):
        raise ValueError(what + ": q_pids, g_pids, q_aux and g_aux are given all or none")
    if num_q < 1 or num_g < 1:
        raise ValueError(what + ": needs at least one query and one gallery entry")
    if given:
        for name, a, n in (("q_pids", q_pids, num_q), ("g_pids", g_pids, num_g), ("q_aux", q_aux, num_q), ("g_aux", g_aux, num_g)):
            if len(a) != n:
                raise ValueError("{}: {} has {} entries for {} rows".format(what, name, len(a), n))
    max_rank = int(max_rank)
    if max_rank < 1 or max_rank > MAX_RANK_LIST:
        raise ValueError("{}: 1 <= max_rank <= {} (the list is selected in LDS), got {}".format(what, MAX_RANK_LIST, max_rank))
    if num_g > MAX_GALLERY:
        raise ValueError("{}: at most 2^31 - 1 = {} gallery entries (32-bit index in the key), got {}".format(what, MAX_GALLERY, num_g))
    if num_g < max_rank:
        max_rank = num_g
        print("Note: number of gallery samples is quite small, got {}".format(num_g))
    return (ids if given else None), max_rank


def _slices(num_q, cols):
    """Workgroups per row of editor_rank_topk: one while there are queries enough to fill the chip twice over (512 workgroups
    on 256 CUs), otherwise the row is sliced - never below 2048 columns a slice, two tiles of the kernel."""
    return max(1, min(-(-512 // num_q), -(-cols // 2048), 1024))


def _topk_block(dist, ldd, num_q, cols, g0, ids, keys, work):
    k = keys.shape[1]
    s = _slices(num_q, cols)
    if s > 1 and (work is None or work.numel() < num_q * s * k):
        work = torch.empty(num_q * s * k, dtype=torch.int64, device=keys.device)
    call("editor_rank_topk", dist.data_ptr(), int(ldd), num_q, cols, int(g0), *(ids or (None,) * 4), k, keys,
         work if s > 1 else None, s)
    return work


def _topk_finish(keys):
    num_q, k = keys.shape
    index = torch.empty(num_q, k, dtype=torch.int32, device=keys.device)
    dist = torch.empty(num_q, k, dtype=torch.float32, device=keys.device)
    call("editor_rank_topk_finish", keys, num_q, k, index, dist)
    return index, dist


def rank_lists(distmat, q_pids=None, g_pids=None, q_aux=None, g_aux=None, max_rank=50):
    """The first `max_rank` kept entries of every row's stable ascending ranking, from a DEVICE distance matrix (Euclidean, or
    re_ranking's output) -> (index (Q, k) int32, dist (Q, k) fp32), device tensors, k = min(max_rank, G).  With the four id
    arrays a gallery entry that has the query's pid AND aux id (camera ids: eval_func's protocol, scene ids: eval_func_msrv's)
    is left out; a row with fewer than k kept entries ends in index -1 / distance +inf.  Equal to argsort_rows + filter + slice,
    ties by gallery index, the distances bit-equal to the matrix entries - but the matrix is not sorted and no Q x P key buffer
    is made (csrc/rank_topk.hip).  Limits: max_rank <= 1024, G <= 2^31 - 1."""
    if not isinstance(distmat, torch.Tensor):
        distmat = torch.as_tensor(np.asarray(distmat))
    if distmat.dim() != 2:
        raise ValueError("rank_lists: distmat must be (Q, G)")
    num_q, num_g = distmat.shape
    ids, k = _list_args("rank_lists", num_q, num_g, q_pids, g_pids, q_aux, g_aux, max_rank)
    if not distmat.is_cuda:
        raise RuntimeError("rank_lists: distmat must be on the GPU (there is no CPU fallback)")
    distmat = distmat.float()
    if distmat.stride(1) != 1:
        distmat = distmat.contiguous()
    dev = distmat.device
    if ids is not None:
        ids = tuple(_dev(a, torch.int64, dev) for a in ids)
    keys = torch.full((num_q, k), -1, dtype=torch.int64, device=dev)
    _topk_block(distmat, distmat.stride(0), num_q, num_g, 0, ids, keys, None)
    return _topk_finish(keys)


def search(qf, gf, k=50, q_pids=None, g_pids=None, q_aux=None, g_aux=None, chunk=16384):
    """rank_lists(euclidean_distance(qf, gf), ..., max_rank=k) straight from features, without the Q x G matrix: the gallery is
    walked in blocks of `chunk` rows, each block's distances go through editor_distmat_f32 into one reused (Q, chunk) buffer and
    from there into the running lists.  Features are taken as given (normalise with `normalize` as the evaluators do)."""
    if qf.dim() != 2 or gf.dim() != 2 or qf.shape[1] != gf.shape[1]:
        raise ValueError("search: qf (Q, D) and gf (G, D) must have the same width")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("search: chunk >= 1")
    num_q, num_g, d = qf.shape[0], gf.shape[0], qf.shape[1]
    ids, k = _list_args("search", num_q, num_g, q_pids, g_pids, q_aux, g_aux, k)
    if not (qf.is_cuda and gf.is_cuda):
        raise RuntimeError("search: features must be on the GPU (there is no CPU fallback)")
    if d < 1:
        raise ValueError("search: features have no columns")
    qf, gf = _rows(qf), _rows(gf)
    dev = qf.device
    if ids is not None:
        ids = tuple(_dev(a, torch.int64, dev) for a in ids)
    c = min(chunk, num_g)
    buf = torch.empty(num_q * c, dtype=torch.float32, device=dev)
    qq = torch.empty(num_q, dtype=torch.float32, device=dev)
    gg = torch.empty(c, dtype=torch.float32, device=dev)
    keys = torch.full((num_q, k), -1, dtype=torch.int64, device=dev)
    work = None
    for g0 in range(0, num_g, c):
        cols = min(c, num_g - g0)
        call("editor_distmat_f32", qf.data_ptr(), qf.stride(0), gf[g0:g0 + cols].data_ptr(), gf.stride(0), num_q, cols, d,
             qq, gg, buf)
        work = _topk_block(buf, cols, num_q, cols, g0, ids, keys, work)
    return _topk_finish(keys)


def format_rank_file(index, q_pids, q_cams, q_scenes, g_pids, g_cams, g_scenes):
    """The text of the reference's `re.txt` (utils/metrics.py:59-60,92-99) from a HOST index array (Q, k) as rank_lists
    returns it (-1 ends a row): a header line, then per query - in query order, queries without a match included - its own
    'pid_sscene_vcam:' line and a line of its kept gallery entries, each followed by two spaces."""
    def host(a):
        return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    index = host(index)
    q_pids, q_cams, q_scenes = host(q_pids), host(q_cams), host(q_scenes)
    g_pids, g_cams, g_scenes = host(g_pids), host(g_cams), host(g_scenes)
    out = ['rank list file\n']
    for qi in range(index.shape[0]):
        out.append('{}_s{}_v{}:\n'.format(q_pids[qi], q_scenes[qi], q_cams[qi]))
        for g in index[qi]:
            if g < 0:
                break
            out.append('{}_s{}_v{}  '.format(g_pids[g], g_scenes[g], g_cams[g]))
        out.append('\n')
    return ''.join(out)


def _device_matrix(distmat):
    if not isinstance(distmat, torch.Tensor):
        distmat = torch.as_tensor(np.asarray(distmat))
    if not distmat.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("eval_func: no GPU (there is no CPU fallback for the retrieval kernels)")
        distmat = distmat.cuda()
    return distmat.float().contiguous()


def _evaluate(distmat, q_pids, g_pids, q_aux, g_aux, max_rank):
    distmat = _device_matrix(distmat)
    dev = distmat.device
    num_q, num_g = distmat.shape
    if num_g < max_rank:
        max_rank = num_g
        print("Note: number of gallery samples is quite small, got {}".format(num_g))
    order = argsort_rows(distmat)
    ap = torch.empty(num_q, dtype=torch.float64, device=dev)
    first = torch.empty(num_q, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.float64, device=dev)
    counts = torch.empty(max_rank, dtype=torch.int32, device=dev)
    call("editor_rank_metrics", order, _dev(q_pids, torch.int64, dev), _dev(g_pids, torch.int64, dev),
         _dev(q_aux, torch.int64, dev), _dev(g_aux, torch.int64, dev), num_q, num_g, max_rank, ap, first, totals, counts)
    tot = totals.cpu().numpy()
    num_valid_q = float(tot[1])
    assert num_valid_q > 0, "Error: all query identities do not appear in gallery"
    all_cmc = counts.cpu().numpy().astype(np.float32) / num_valid_q
    m_ap = float(tot[0] / num_valid_q)
    return all_cmc, m_ap, order, ap, first


def eval_func(distmat, q_pids, g_pids, q_camids, g_camids, max_rank=50):
    """Market-1501 protocol: gallery entries with the query's pid AND camid are discarded."""
    cmc, m_ap, _, _, _ = _evaluate(distmat, q_pids, g_pids, q_camids, g_camids, max_rank)
    return cmc, m_ap


def eval_func_msrv(distmat, q_pids, g_pids, q_camids, g_camids, q_sceneids, g_sceneids, max_rank=50, rank_file=None):
    """MSVR310 protocol (utils/metrics.py:87): entries with the query's pid AND scene id are discarded.  rank_file: a path that
    receives the reference's `re.txt` (utils/metrics.py:59-60,92-99: every query's first max_rank kept gallery entries), byte for
    byte; None writes nothing."""
    if rank_file is not None:
        distmat = _device_matrix(distmat)
    cmc, m_ap, _, _, _ = _evaluate(distmat, q_pids, g_pids, q_sceneids, g_sceneids, max_rank)
    if rank_file is not None:
        index, _ = rank_lists(distmat, q_pids, g_pids, q_sceneids, g_sceneids, min(max_rank, distmat.shape[1]))
        with open(rank_file, 'w') as f:
            f.write(format_rank_file(index.cpu().numpy(), q_pids, q_camids, q_sceneids, g_pids, g_camids, g_sceneids))
    return cmc, m_ap


class R1_mAP_eval():
    def __init__(self, num_query, max_rank=20, feat_norm=True, reranking=False):
        self.num_query = num_query
        self.max_rank = max_rank
        self.feat_norm = feat_norm
        self.reranking = reranking

    def reset(self):
        self.feats = []
        self.pids = []
        self.camids = []

    def update(self, output):
        feat, pid, camid = output
        self.feats.append(feat.detach().float())          # stays on the device
        self.pids.extend(np.asarray(pid.cpu() if isinstance(pid, torch.Tensor) else pid))
        self.camids.extend(np.asarray(camid.cpu() if isinstance(camid, torch.Tensor) else camid))

    def _split(self):
        feats = torch.cat(self.feats, dim=0)
        if self.feat_norm in (True, 'yes'):
            print("The test feature is normalized")
            feats = normalize(feats)
        nq = self.num_query
        return feats[:nq], feats[nq:], np.asarray(self.pids[:nq]), np.asarray(self.pids[nq:]), \
            np.asarray(self.camids[:nq]), np.asarray(self.camids[nq:])

    def compute(self, vis=0):
        qf, gf, q_pids, g_pids, q_camids, g_camids = self._split()
        if self.reranking:
            print('=> Enter reranking')
            distmat = re_ranking(qf, gf, k1=50, k2=15, lambda_value=0.3)          # utils/metrics.py:278
        else:
            print('=> Computing DistMat with euclidean_distance')
            distmat = euclidean_distance(qf, gf)
        # the reference's max_rank attribute is not forwarded to eval_func (utils/metrics.py:282): default 50
        cmc, m_ap = eval_func(distmat, q_pids, g_pids, q_camids, g_camids)
        return cmc, m_ap, distmat.cpu().numpy(), self.pids, self.camids, qf, gf

    def _lists(self, qf, gf, q_pids, g_pids, q_aux, g_aux, max_rank):
        k = self.max_rank if max_rank is None else max_rank
        if self.reranking:
            return rank_lists(re_ranking(qf, gf, k1=50, k2=15, lambda_value=0.3), q_pids, g_pids, q_aux, g_aux, k)
        return search(qf, gf, k, q_pids, g_pids, q_aux, g_aux)

    def rank_lists(self, max_rank=None):
        """(index, dist) device tensors: every query's first max_rank (None: the constructor's) gallery matches under this
        evaluator's protocol (same pid AND camera id removed), for the features collected by update()."""
        qf, gf, q_pids, g_pids, q_camids, g_camids = self._split()
        return self._lists(qf, gf, q_pids, g_pids, q_camids, g_camids, max_rank)


class R1_mAP(R1_mAP_eval):
    def __init__(self, num_query, max_rank=50, feat_norm='yes', rank_file=None):
        super().__init__(num_query, max_rank, feat_norm)
        self.rank_file = rank_file

    def reset(self):
        super().reset()
        self.sceneids = []
        self.img_path = []

    def update(self, output):
        feat, pid, camid, sceneid, img_path = output
        super().update((feat, pid, camid))
        self.sceneids.extend(np.asarray(sceneid.cpu() if isinstance(sceneid, torch.Tensor) else sceneid))
        self.img_path.extend(img_path)

    def compute(self, cfg=None):
        qf, gf, q_pids, g_pids, q_camids, g_camids = self._split()
        nq = self.num_query
        q_s, g_s = np.asarray(self.sceneids[:nq]), np.asarray(self.sceneids[nq:])
        distmat = euclidean_distance(qf, gf)
        cmc, m_ap = eval_func_msrv(distmat, q_pids, g_pids, q_camids, g_camids, q_s, g_s, rank_file=self.rank_file)
        return cmc, m_ap, distmat.cpu().numpy(), self.pids, self.camids, qf, gf

    def rank_lists(self, max_rank=None):
        """As R1_mAP_eval.rank_lists under the MSVR310 protocol (same pid AND scene id removed)."""
        qf, gf, q_pids, g_pids, _, _ = self._split()
        nq = self.num_query
        return self._lists(qf, gf, q_pids, g_pids, np.asarray(self.sceneids[:nq]), np.asarray(self.sceneids[nq:]), max_rank)
