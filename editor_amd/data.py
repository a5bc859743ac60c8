"""Input pipeline pieces around the hot path - row N3 of SURVEY.md 8(f).

Host side (Python, as in the reference) + one HIP kernel (csrc/augment.hip):
    RandomIdentitySampler      data/datasets/sampler.py:7-66      same class name / arguments / RNG consumption: the same
                               `random` + `numpy.random` seeds give the same index list (golden-pinned)
    RandomIdentitySampler_DDP  data/datasets/sampler_ddp.py:111-196  per-rank mini-batches of one agreed global list
    ErasingParams              the rectangle selection of RandomErasing._erase (make_dataloader.py:108-130): same draws
                               from Python's `random`, returned as numbers instead of applied (golden-pinned)
    DeviceTrainTransform       T.RandomHorizontalFlip -> T.Pad -> T.RandomCrop -> T.ToTensor -> T.Normalize ->
                               RandomErasing(mode='pixel') of make_dataloader.py:245-253 for a whole batch in one launch
    make_dataloader            data/datasets/make_dataloader.py:244-308: the reference's 7-tuple, its three loaders being
                               DeviceBatchLoader (editor_amd/loader.py) over list_dataset (editor_amd/datasets.py)
    DeviceJpegDecoder / DeviceResize   `Image.open(path).convert('RGB')` + T.Resize: the stitched layout (one 768x128 file, three
                               256-wide crops: RGBNT100 / RGBNT300) through __call__, the separate-file layout (one detector
                               crop of any size per modality: RGBNT201 / MSVR310) through decode_ragged + RaggedImages +
                               load_modalities - a fixed number of launches per batch either way
The transform takes decoded, resized uint8 (B,H,W,3) images.  The flip / crop draws use torch's CPU generator the way torchvision 0.14 does
(`torch.rand(1) < p`; `torch.randint(0, h - th + 1)`, then `w`), but torchvision is not installed in the build image, so
that ORDER is restated from its documentation, not pinned ("parity unpinned" for those two draws only; what the draws do to the
pixels is pinned to Pillow: tests/golden/f19_flip_pad_crop.npz).
"""
import copy
import ctypes
import math
import random
from collections import defaultdict

import numpy as np
import torch

from ._lib import call


class RandomIdentitySampler(torch.utils.data.sampler.Sampler):
    """Randomly sample N identities, then K instances of each: batch = N*K (data/datasets/sampler.py:7-66).
    data_source: list of (img_path, pid, camid, trackid)."""

    def __init__(self, data_source, batch_size, num_instances):
        self.data_source = data_source
        self.batch_size = batch_size
        self.num_instances = num_instances
        self.num_pids_per_batch = self.batch_size // self.num_instances
        self.index_dic = defaultdict(list)
        for index, (_, pid, _, _) in enumerate(self.data_source):
            self.index_dic[pid].append(index)
        self.pids = list(self.index_dic.keys())
        self.length = 0
        for pid in self.pids:
            num = max(len(self.index_dic[pid]), self.num_instances)
            self.length += num - num % self.num_instances

    def __iter__(self):
        per_pid = defaultdict(list)
        for pid in self.pids:
            idxs = copy.deepcopy(self.index_dic[pid])
            if len(idxs) < self.num_instances:
                idxs = np.random.choice(idxs, size=self.num_instances, replace=True)
            random.shuffle(idxs)
            chunk = []
            for idx in idxs:
                chunk.append(idx)
                if len(chunk) == self.num_instances:
                    per_pid[pid].append(chunk)
                    chunk = []
        avai = copy.deepcopy(self.pids)
        final = []
        while len(avai) >= self.num_pids_per_batch:
            for pid in random.sample(avai, self.num_pids_per_batch):
                final.extend(per_pid[pid].pop(0))
                if len(per_pid[pid]) == 0:
                    avai.remove(pid)
        return iter(final)

    def __len__(self):
        return self.length


class RandomIdentitySampler_DDP(torch.utils.data.sampler.Sampler):
    """data/datasets/sampler_ddp.py:111-196: every rank builds the SAME global list of identity batches from a seed
    agreed across ranks, then keeps its own mini-batches - block j of `batch_size // world` indices goes to rank
    j % world.  Same numpy.random consumption as the reference (identity draw, optional with-replacement fill,
    shuffle on an identity's first appearance), so the same shared seed gives the same per-rank index lists
    (golden-pinned for world 1 / 2 / 4).  rank / world_size default to torch.distributed's."""

    def __init__(self, data_source, batch_size, num_instances, rank=None, world_size=None, seed=None):
        import torch.distributed as dist
        self.data_source = data_source
        self.batch_size = batch_size
        self.world_size = dist.get_world_size() if world_size is None else int(world_size)
        self.rank = dist.get_rank() if rank is None else int(rank)
        self.num_instances = num_instances
        self.mini_batch_size = self.batch_size // self.world_size
        self.num_pids_per_batch = self.mini_batch_size // self.num_instances
        self.index_dic = defaultdict(list)
        for index, (_, pid, _, _) in enumerate(self.data_source):
            self.index_dic[pid].append(index)
        self.pids = list(self.index_dic.keys())
        self.seed = seed
        total = 0
        for pid in self.pids:
            num = max(len(self.index_dic[pid]), self.num_instances)
            total += num - num % self.num_instances
        self.length = total // self.world_size

    def _shared_seed(self):
        """sampler_ddp.py:100-109: every rank draws, rank 0's draw wins."""
        import torch.distributed as dist
        mine = int(np.random.randint(2 ** 31))
        if self.seed is not None:
            return int(self.seed)
        if self.world_size == 1 or not (dist.is_available() and dist.is_initialized()):
            return mine
        box = [mine]
        dist.broadcast_object_list(box, src=0)
        return int(box[0])

    def global_list(self):
        """The batch-ordered index list every rank agrees on (sampler_ddp.py:166-190)."""
        k = self.num_instances
        live = copy.deepcopy(self.pids)
        queue = {}
        out = []
        while len(live) >= self.num_pids_per_batch:
            for pid in np.random.choice(live, self.num_pids_per_batch, replace=False).tolist():
                q = queue.get(pid)
                if q is None:
                    q = copy.deepcopy(self.index_dic[pid])
                    if len(q) < k:
                        q = np.random.choice(q, size=k, replace=True).tolist()
                    np.random.shuffle(q)
                    queue[pid] = q
                out.extend(q[:k])
                del q[:k]
                if len(q) < k:
                    live.remove(pid)
        return out

    def __iter__(self):
        np.random.seed(self._shared_seed())
        allidx = np.asarray(self.global_list(), dtype=np.int64)
        total, mini = len(allidx), self.mini_batch_size
        blocks = (int(math.ceil(total / self.world_size)) // mini)
        pos = ((np.arange(blocks) * self.world_size + self.rank)[:, None] * mini + np.arange(mini)[None, :]).reshape(-1)
        mine = allidx[pos[pos < total]].tolist()
        self.length = len(mine)
        return iter(mine)

    def __len__(self):
        return self.length


class ErasingParams:
    """RandomErasing(probability, mode='pixel', max_count=1)._erase's rectangle choice for ONE image
    (make_dataloader.py:108-130), consuming Python's `random` exactly as the reference does.
    -> (erase, top, left, h, w)."""

    def __init__(self, probability=0.5, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None):
        self.probability = probability
        self.min_area, self.max_area = min_area, max_area
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))

    def __call__(self, img_h, img_w, rng=None):
        """rng: a random.Random to draw from instead of the global `random` (editor_amd/loader.py: the worker thread's own)."""
        rng = random if rng is None else rng
        if rng.random() > self.probability:
            return (0, 0, 0, 0, 0)
        area = img_h * img_w
        for _ in range(10):
            target_area = rng.uniform(self.min_area, self.max_area) * area
            aspect_ratio = math.exp(rng.uniform(*self.log_aspect_ratio))
            h = int(round(math.sqrt(target_area * aspect_ratio)))
            w = int(round(math.sqrt(target_area / aspect_ratio)))
            if w < img_w and h < img_h:
                top = rng.randint(0, img_h - h)
                left = rng.randint(0, img_w - w)
                return (1, top, left, h, w)
        return (0, 0, 0, 0, 0)


def resize_coeffs(in_size, out_size, interpolation=3):
    """Tap table of one axis of T.Resize on uint8 images - Pillow's precompute_coeffs + normalize_coeffs_8bpc
    (src/libImaging/Resample.c; torchvision 0.14.1 resizes PIL images with PIL.Image.resize): per output coordinate the
    window [xmin, xmin + count) and its 22-bit fixed-point weights.  interpolation: 3 = bicubic (a = -0.5, support 2; the
    train transform, make_dataloader.py:246), 2 = bilinear (support 1; the val transform, :256).  All in float64 in the
    order Pillow's C doubles take, vectorised over the output coordinates -> (bounds (out,2) int32, k (out,ksize) int32)."""
    fsupport = {2: 1.0, 3: 2.0}[interpolation]
    scale = float(in_size) / out_size
    fscale = max(scale, 1.0)
    support = fsupport * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                 # C (int): truncation (values >= -0.5)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    j = np.arange(ksize, dtype=np.float64)[None, :]
    x = np.abs((j + xmin[:, None] - center[:, None] + 0.5) * (1.0 / fscale))
    if interpolation == 3:
        a = -0.5
        w = np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))
    else:
        w = np.where(x < 1.0, 1.0 - x, 0.0)
    w = np.where(j < xmax[:, None], w, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for c in range(ksize):                                                          # Pillow sums the taps left to right
        ww = ww + w[:, c]
    wn = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    fixed = wn * float(1 << 22)
    kk = np.where(wn < 0, (-0.5 + fixed).astype(np.int64), (0.5 + fixed).astype(np.int64)).astype(np.int32)
    kk = np.where(j < xmax[:, None], kk, 0).astype(np.int32)
    return np.stack([xmin, xmax], axis=1).astype(np.int32), kk


class RaggedImages:
    """A batch of decoded uint8 RGB images of DIFFERENT sizes (the separate-file data sets: one detector crop per modality,
    data/datasets/bases.py:22-30), packed one after another in one device buffer - what DeviceJpegDecoder.decode_ragged
    returns and DeviceResize accepts.
        data     flat uint8 device tensor; image i is (h_i, w_i, 3) row-major at byte offsets[i]
        offsets  int64 (B + 1), host; offsets[B] = data.numel()
        sizes    int32 (B, 2) as (h, w), host"""

    def __init__(self, data, offsets, sizes):
        self.data, self.offsets, self.sizes = data, offsets, sizes

    def __len__(self):
        return int(self.sizes.shape[0])

    def image(self, i):
        """-> (h, w, 3) view of image i."""
        h, w = int(self.sizes[i, 0]), int(self.sizes[i, 1])
        o = int(self.offsets[i])
        return self.data[o:o + h * w * 3].view(h, w, 3)

    @classmethod
    def from_arrays(cls, arrays, device):
        """list of (H, W, 3) uint8 numpy arrays (a decode of the caller's own) -> RaggedImages on `device`: one H2D copy."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("RaggedImages live on the GPU (no CPU fallback)")
        arrays = [np.asarray(a) for a in arrays]
        if not arrays:
            raise ValueError("RaggedImages: empty batch")
        for a in arrays:
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
                raise ValueError("RaggedImages: every image is a non-empty (H, W, 3) uint8 array")
        sizes = np.asarray([a.shape[:2] for a in arrays], dtype=np.int32)
        offsets = np.concatenate([[0], np.cumsum(sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3)])
        flat = np.concatenate([a.reshape(-1) for a in arrays])
        return cls(torch.from_numpy(flat).to(device), torch.from_numpy(offsets), torch.from_numpy(sizes))


def ragged_decode_plan(infos):
    """Where each file of a ragged batch lives in the buffers of editor_jpeg_reconstruct_ragged.  infos: (B,16) int32 rows
    of editor_jpeg_parse.  -> tab (5,B) int64 = first coefficient block, plane byte offset, output byte offset, inclusive
    prefix sum of blocks, inclusive prefix sum of output pixels; the totals.  A block is 64 coefficients in and 64 one-byte
    samples out, so image i's planes start at byte 64 * (its first block): a multiple of 8 (the IDCT stores 8 bytes at a
    time), and every coefficient base sits on a block boundary."""
    inf = np.asarray(infos, dtype=np.int64).reshape(-1, 16)
    blocks, pixels = inf[:, 8], inf[:, 0] * inf[:, 1]
    bsum, psum = np.cumsum(blocks), np.cumsum(pixels)
    tab = np.stack([bsum - blocks, 64 * (bsum - blocks), 3 * (psum - pixels), bsum, psum]).astype(np.int64)
    return tab, int(bsum[-1]), int(psum[-1])


class DeviceResize:
    """T.Resize(size, interpolation) for a batch of decoded uint8 images on the device: a dense (B,H,W,3) tensor
    (editor_resize_u8) or a RaggedImages batch, every image from its own size (editor_resize_u8_ragged, two launches per
    batch) -> (B,Hout,Wout,3).  Bit-exact with what the reference's PIL pipeline produces for the same pixels."""

    def __init__(self, size, interpolation=3):
        self.size = (int(size[0]), int(size[1]))
        self.interpolation = interpolation
        self._tabs = {}
        self._rag_index, self._rag_host, self._rag_len, self._rag_dev = {}, [], 0, {}

    def ragged_tables(self, sizes):
        """Tap tables of a ragged batch.  sizes: (B,2) int (h, w).  -> desc (B,8) int32 rows = h, w, index of the x table in
        the tap array, its ksize, index of the y table, its ksize, 0, 0.  One table per distinct (input extent, output
        extent), built once by resize_coeffs and kept: bounds (n_out,2) then taps (n_out,ksize), appended to self.taps()
        (ksize grows with the downscale factor, hence per image).  An extent equal to its target gets the identity table
        (one tap of 1 << 22: the byte itself), where Pillow skips the pass."""
        sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        desc = np.zeros((sizes.shape[0], 8), dtype=np.int32)
        desc[:, :2] = sizes
        for axis, n_out, col in ((1, self.size[1], 2), (0, self.size[0], 4)):
            uniq, inv = np.unique(sizes[:, axis], return_inverse=True)
            ent = []
            for n_in in uniq.tolist():
                e = self._rag_index.get((n_in, n_out))
                if e is None:
                    bounds, k = resize_coeffs(n_in, n_out, self.interpolation)
                    assert bounds.min() >= 0 and (bounds[:, 1] <= k.shape[1]).all() and (bounds.sum(axis=1) <= n_in).all()
                    e = self._rag_index[(n_in, n_out)] = (self._rag_len, int(k.shape[1]))
                    self._rag_host += [bounds.reshape(-1), k.reshape(-1)]
                    self._rag_len += bounds.size + k.size
                ent.append(e)
            desc[:, col:col + 2] = np.asarray(ent, dtype=np.int32)[inv.reshape(-1)]
        return desc

    def taps(self):
        """The tap array the desc rows index (int32, host)."""
        if len(self._rag_host) > 1:
            self._rag_host = [np.concatenate(self._rag_host)]
        return self._rag_host[0]

    def _ragged(self, rag):
        if not rag.data.is_cuda:
            raise RuntimeError("DeviceResize: images are not on the GPU (no CPU fallback)")
        b = len(rag)
        if b < 1:
            raise ValueError("DeviceResize: empty batch")
        assert rag.data.dtype == torch.uint8 and rag.data.is_contiguous()
        oh, ow = self.size
        dev = rag.data.device
        sizes = np.asarray(rag.sizes, dtype=np.int64)
        starts = np.asarray(rag.offsets, dtype=np.int64)[:b]
        if sizes.shape != (b, 2) or (sizes < 1).any() or (starts < 0).any() or (starts + 3 * sizes[:, 0] * sizes[:, 1] > rag.data.numel()).any():
            raise ValueError("DeviceResize: RaggedImages sizes / offsets do not fit its data")
        desc = self.ragged_tables(sizes)
        hsum = np.cumsum(sizes[:, 0])
        off = np.stack([starts, 3 * ow * (hsum - sizes[:, 0]), ow * hsum]).astype(np.int64)
        taps_d = self._rag_dev.get(dev)
        if taps_d is None or taps_d.numel() != self._rag_len:          # grow-only: re-sent when a new extent added a table
            taps_d = self._rag_dev[dev] = torch.from_numpy(self.taps()).to(dev)
        host = np.concatenate([desc.reshape(-1).view(np.uint8), off.reshape(-1).view(np.uint8)])     # one H2D copy for both tables
        tabs_d = torch.from_numpy(host).to(dev)
        desc_d, off_d = tabs_d[:32 * b].view(torch.int32), tabs_d[32 * b:].view(torch.int64)
        tmp = torch.empty(3 * ow * int(hsum[-1]), dtype=torch.uint8, device=dev)
        out = torch.empty(b, oh, ow, 3, dtype=torch.uint8, device=dev)
        call("editor_resize_u8_ragged", rag.data, b, oh, ow, ctypes.c_void_p(desc.ctypes.data), ctypes.c_void_p(off.ctypes.data),
             desc_d, off_d, taps_d, int(taps_d.numel()), tmp, out)
        return out

    def _tables(self, n_in, n_out, device):
        key = (n_in, n_out, device)
        t = self._tabs.get(key)
        if t is None:
            b, k = resize_coeffs(n_in, n_out, self.interpolation)
            t = self._tabs[key] = (torch.from_numpy(b).to(device).contiguous(), torch.from_numpy(k).to(device).contiguous(),
                                   int(k.shape[1]))
        return t

    def __call__(self, images_u8):
        if isinstance(images_u8, RaggedImages):
            return self._ragged(images_u8)
        if not images_u8.is_cuda:
            raise RuntimeError("DeviceResize: images are not on the GPU (no CPU fallback)")
        b, h, w, c = images_u8.shape
        assert c == 3 and images_u8.dtype == torch.uint8
        oh, ow = self.size
        dev = images_u8.device
        out = torch.empty(b, oh, ow, 3, dtype=torch.uint8, device=dev)
        xb, xk, xks = self._tables(w, ow, dev) if ow != w else (None, None, 1)
        yb, yk, yks = self._tables(h, oh, dev) if oh != h else (None, None, 1)
        tmp = torch.empty(b, h, ow, 3, dtype=torch.uint8, device=dev) if (ow != w and oh != h) else None
        call("editor_resize_u8", images_u8.contiguous(), b, h, w, oh, ow, xb, xk, xks, yb, yk, yks, tmp, out)
        return out


class DeviceTrainTransform:
    """The train transform of make_dataloader.py:245-253 after the resize, for a batch, on the device."""

    def __init__(self, size, prob=0.5, padding=10, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), re_prob=0.5):
        self.h, self.w = size
        self.prob, self.padding = prob, padding
        self.mean = (ctypes.c_float * 3)(*mean)
        self.std = (ctypes.c_float * 3)(*std)
        self.erasing = ErasingParams(re_prob)

    def draw(self, batch, generator=None, rng=None):
        """Per-image parameter rows in the order the reference's per-image chain consumes its generators: torch's global CPU
        generator and Python's global `random`, or the caller's own torch.Generator / random.Random (the globals untouched)."""
        rows = []
        for _ in range(batch):
            flip = int(torch.rand(1, generator=generator).item() < self.prob)
            top = int(torch.randint(0, 2 * self.padding + 1, size=(1,), generator=generator).item())
            left = int(torch.randint(0, 2 * self.padding + 1, size=(1,), generator=generator).item())
            rows.append((flip, top, left) + self.erasing(self.h, self.w, rng=rng))
        return torch.tensor(rows, dtype=torch.int32).reshape(batch, 8)

    def __call__(self, images_u8, params=None, noise=None, seed=0):
        """images_u8: uint8 (B,H,W,3) on the device.  params: int32 (B,8) from draw() (drawn here if None).
        noise: optional fp32 (B,3,H,W) N(0,1) fill for the erased rectangles (else generated on the device)."""
        if not images_u8.is_cuda:
            raise RuntimeError("DeviceTrainTransform: images are not on the GPU (no CPU fallback)")
        b, h, w, c = images_u8.shape
        assert (h, w, c) == (self.h, self.w, 3) and images_u8.dtype == torch.uint8
        if params is None:
            params = self.draw(b)
        params = params.to(device=images_u8.device, dtype=torch.int32).contiguous()
        out = torch.empty(b, 3, h, w, dtype=torch.float32, device=images_u8.device)
        call("editor_augment_u8", images_u8.contiguous(), params, b, h, w, int(self.padding), self.mean, self.std, noise,
             int(seed) & 0xFFFFFFFFFFFFFFFF, out)
        return out


class JpegBatchPlan:
    """What DeviceJpegDecoder.plan_batch learns about a batch without decoding it (editor_jpeg_plan, include/editor_hip.h):
    infos (B,16) int32, plans (B,16) int32 (plans[:,0]: device-eligible), qts (B,192) uint16, huffs (B,8,272) uint8, and
    segs (nseg,3) int64 - the restart segments of the ELIGIBLE files, file after file."""

    def __init__(self, b):
        self.infos, self.plans = np.zeros((b, 16), dtype=np.int32), np.zeros((b, 16), dtype=np.int32)
        self.qts, self.huffs = np.zeros((b, 192), dtype=np.uint16), np.zeros((b, 8, 272), dtype=np.uint8)
        self.segs, self.nseg = np.zeros((max(64, 4 * b), 3), dtype=np.int64), 0


class DeviceJpegDecoder:
    """`Image.open(path).convert('RGB')` + the 256-wide crops of data/datasets/bases.py:9-41 for a BATCH of baseline JPEG
    files: the host Huffman-decodes each file into quantised DCT coefficients (a thread pool; the C entry point releases
    the GIL), ONE device call per geometry does dequantisation + IDCT + chroma upsampling + YCbCr -> RGB + the crop split
    (editor_jpeg_reconstruct).  Pixels are bit-identical to Pillow's (tests/golden/f14_decode.npz).

        dec = DeviceJpegDecoder(crop_w=256)
        crops = dec([open(p, "rb").read() for p in paths], device)     # uint8 (ncrop, B, H, 256, 3): RGB, NI, TI
        x = DeviceResize(cfg.INPUT.SIZE_TRAIN)(crops[0])               # ... the rest of the transform on the device

    Files of DIFFERENT sizes (the separate-file data sets RGBNT201 / MSVR310: one detector crop per modality) go through
    decode_ragged: any mix of sizes, sampling factors, grayscale, baseline / progressive in one IDCT launch + one colour launch
    (editor_jpeg_reconstruct_ragged), packed into a RaggedImages that DeviceResize brings to one size.  __call__ keeps
    refusing such a batch.

    Baseline, extended-sequential and progressive Huffman files (round 4) are covered; arithmetic-coded / lossless / 12-bit /
    4-component files raise (EDITOR_JPEG_UNSUPPORTED) and an incomplete progressive file is corrupt: no silent host fallback.

    entropy="device" moves the Huffman decode of ordinary baseline files to the GPU, for __call__ and decode_ragged alike: the
    host plans each file (editor_jpeg_plan: one pass over its bytes), the compressed scan bytes are uploaded instead of int16
    blocks, and editor_jpeg_entropy_device - one wave per restart segment of the batch - writes the same coefficient planes, bit
    for bit; reconstruction is unchanged.  Device-eligible: SOF0 / SOF1, exactly one SOS naming every component in frame order,
    restart markers (if an interval is defined) all present and in order.  Every other file the parser accepts (progressive,
    several scans, irregular restarts) is decoded on the host as before and its coefficients copied in - a documented routing
    rule.  Same errors, same text; the one difference: corrupt ENTROPY data is found after the launch (the status
    vector is read back before the call returns), not before it.

    entropy="device_split" is the same path with editor_jpeg_entropy_split_device as its decoder: parallel INSIDE a segment too
    (256 lanes per segment, each decoding split_sub_bytes of it, re-run from the left neighbour's exit state until the states
    agree), so a batch's time no longer follows its longest restart-less file.  The setting for batches that hold long files
    (tens of KB and more); eligibility, routing, errors and the coefficients are those of "device"."""

    SPLIT_SUB_BYTES = 64                                     # (the sweep: profiles/device_entropy_split_time.txt)

    def __init__(self, crop_w=256, threads=8, entropy="host", split_sub_bytes=None):
        from concurrent.futures import ThreadPoolExecutor
        from . import _lib
        if entropy not in ("host", "device", "device_split"):
            raise ValueError("DeviceJpegDecoder: entropy is 'host', 'device' or 'device_split'")
        self.entropy = entropy
        self.split_sub_bytes = int(self.SPLIT_SUB_BYTES if split_sub_bytes is None else split_sub_bytes)
        if self.split_sub_bytes not in (16, 32, 64, 128):
            raise ValueError("DeviceJpegDecoder: split_sub_bytes is 16, 32, 64 or 128")
        self.last_h2d_bytes = 0                              # bytes the last call copied to the device (tools/ragged_input_time.py)
        self.crop_w = int(crop_w)
        self._cd = _lib.lib().cdll
        self._pool = ThreadPoolExecutor(max_workers=max(1, int(threads)))
        self._arena, self._h2d_done = None, None            # the pinned staging buffer (_stage) and its last copy's event

    @staticmethod
    def _refusal(rc):
        return "JPEG %s (editor_jpeg_parse rc %d)" % ("uses a coding mode the device decoder does not cover "
                                                      "(arithmetic / lossless / 12-bit / 4 components)" if rc == 9002 else "is corrupt or incomplete", rc)

    def _parse_rc(self, data, info):
        buf = np.frombuffer(data, dtype=np.uint8)
        return self._cd.editor_jpeg_parse(ctypes.c_void_p(buf.ctypes.data), len(data), ctypes.c_void_p(info.ctypes.data))

    def parse(self, data):
        """-> info (16 int32): W, H, ncomp, hmax, vmax, mcus_x, mcus_y, ycc_transform, blocks_per_image, ..."""
        info = np.zeros(16, dtype=np.int32)
        rc = self._parse_rc(data, info)
        if rc:
            raise ValueError(self._refusal(rc))
        return info

    def _entropy(self, data, coef_ptr, blocks, qt_ptr, info):
        buf = np.frombuffer(data, dtype=np.uint8)
        rc = self._cd.editor_jpeg_entropy_decode(ctypes.c_void_p(buf.ctypes.data), len(data), ctypes.c_void_p(coef_ptr),
                                                 ctypes.c_long(blocks), ctypes.c_void_p(qt_ptr), ctypes.c_void_p(info.ctypes.data))
        if rc:
            raise ValueError("JPEG entropy decode failed (rc %d)" % rc)

    # ---- entropy="device": the scans are Huffman-decoded by editor_jpeg_entropy_device -------------------------------------
    def plan_batch(self, files):
        """editor_jpeg_plan over a batch, on the calling thread (one pass over each file's bytes).  -> JpegBatchPlan; raises
        ValueError naming the file's index for a file editor_jpeg_parse refuses, before anything is launched."""
        b = len(files)
        bp = JpegBatchPlan(b)
        used = 0
        fn = self._cd.editor_jpeg_plan
        p_info, p_plan, p_qt, p_huff = (a.ctypes.data for a in (bp.infos, bp.plans, bp.qts, bp.huffs))
        for i, f in enumerate(files):
            buf = np.frombuffer(f, dtype=np.uint8)
            while True:
                cap = bp.segs.shape[0] - used
                rc = fn(ctypes.c_void_p(buf.ctypes.data), len(f), ctypes.c_void_p(p_info + 64 * i), ctypes.c_void_p(p_plan + 64 * i),
                        ctypes.c_void_p(p_qt + 384 * i), ctypes.c_void_p(p_huff + 2176 * i), ctypes.c_void_p(bp.segs.ctypes.data + 24 * used), cap)
                if rc:
                    raise ValueError("file %d of the batch: %s" % (i, self._refusal(rc)))
                ns = int(bp.plans[i, 1])
                if not bp.plans[i, 0] or ns <= cap:
                    break
                bp.segs = np.concatenate([bp.segs, np.zeros((max(bp.segs.shape[0], ns), 3), dtype=np.int64)])
            if bp.plans[i, 0]:                                # (a host-routed file's rows are overwritten by the next file's)
                used += ns
        bp.nseg = used
        return bp

    def pack_batch(self, files, bp, block_off):
        """The tables editor_jpeg_entropy_segments / _device take for a planned batch (include/editor_hip.h), host arrays:
        -> (nbytes, spans, fdesc, ftab, segs, huff, nseg).  spans: (file index, position in the byte buffer, first scan byte,
        end of the scan bytes) per eligible file - only those bytes travel, each file's at a multiple of 16."""
        b = len(files)
        elig = bp.plans[:, 0] != 0
        nsegs = np.where(elig, bp.plans[:, 1], 0).astype(np.int64)
        segpref = np.cumsum(nsegs)
        nseg = int(segpref[-1])
        assert nseg == bp.nseg
        segs = bp.segs[:max(nseg, 1)]
        e_idx = np.nonzero(elig)[0]
        s0 = segs[(segpref - nsegs)[e_idx], 0]
        e1 = segs[segpref[e_idx] - 1, 1]
        padded = (e1 - s0 + 15) & ~15
        pos = np.cumsum(padded) - padded
        nbytes = max(int(padded.sum()), 16)
        byte_off = np.zeros(b, dtype=np.int64)
        byte_off[e_idx] = pos - s0
        ftab = np.stack([np.asarray(block_off, dtype=np.int64), byte_off, segpref]).astype(np.int64)
        fdesc = np.zeros((b, 16), dtype=np.int32)
        fdesc[:, 0:5] = bp.infos[:, 2:7]
        fdesc[:, 5] = bp.plans[:, 2]
        pool, rows, memo = [], {}, {}
        for i in e_idx.tolist():                              # the batch's pool of distinct Huffman tables
            key = (bp.huffs[i].tobytes(), bp.plans[i, 4:10].tobytes())
            slots = memo.get(key)
            if slots is None:
                slots = []
                for c in range(3):
                    for sel in (int(bp.plans[i, 4 + c]), 4 + int(bp.plans[i, 7 + c])):
                        t = bp.huffs[i, sel].tobytes()
                        if t not in rows:
                            rows[t] = len(pool)
                            pool.append(bp.huffs[i, sel])
                        slots.append(rows[t])
                slots = memo[key] = slots[0::2] + slots[1::2]
            fdesc[i, 6:12] = slots
        huff = np.stack(pool) if pool else np.zeros((1, 272), dtype=np.uint8)
        spans = list(zip(e_idx.tolist(), pos.tolist(), s0.tolist(), e1.tolist()))
        return nbytes, spans, fdesc, ftab, segs, huff, nseg

    # ---- the pipeline: describe the batch, fill its coefficients, reconstruct ----------------------------------------------
    @staticmethod
    def _cuda(device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("DeviceJpegDecoder reconstructs on the GPU (no CPU fallback)")
        return device

    def _describe(self, files):
        """Every file parsed before anything is launched -> (infos (B,16) int32, JpegBatchPlan or None): entropy="host" runs
        editor_jpeg_parse on the pool (the planner is single-threaded), the device modes plan.  A file the parser refuses raises
        ValueError naming its index in the batch."""
        if self.entropy != "host":
            bp = self.plan_batch(files)
            return bp.infos, bp
        infos = np.zeros((len(files), 16), dtype=np.int32)
        for i, rc in enumerate(self._pool.map(lambda i: self._parse_rc(files[i], infos[i]), range(len(files)))):
            if rc:
                raise ValueError("file %d of the batch: %s" % (i, self._refusal(rc)))
        return infos, None

    def _stage(self, nbytes):
        """The pinned staging buffer: grow-only and reused across calls (pinning per call costs more than the copy it speeds
        up), so the previous call's host-to-device copies must have left it before it is written again."""
        if self._h2d_done is not None:
            self._h2d_done.synchronize()
        if self._arena is None or self._arena.numel() < nbytes:
            self._arena = torch.empty(max(nbytes, 2 * (self._arena.numel() if self._arena is not None else 0)), dtype=torch.uint8).pin_memory()
        return self._arena

    def _coefficients(self, files, infos, bp, order, device, extra=()):
        """The coefficient tensor of a described batch: flat int16 on the device, the files' blocks one after another in `order`.
        bp None (entropy="host"): every file is host-routed - decoded by editor_jpeg_entropy_decode on the pool, straight into
        the staging buffer.  Otherwise the plan's eligible files travel as scan bytes and one launch of editor_jpeg_entropy_device
        (entropy="device_split": editor_jpeg_entropy_split_device) decodes them; the rest are host-routed as above.  Staged as
        scan bytes | 16-byte-aligned tables (the entropy kernel's four, the quantisation tables in `order`, the caller's `extra`) |
        host-routed coefficients in `order`: ONE copy for bytes and tables, one per run of host-routed files adjacent in the
        tensor.  -> (coef_d, block_off, status tensor or None, quantisation tables (B*192 int16, uint16 bit patterns), device
        views of extra)."""
        b = len(files)
        order = np.asarray(order, dtype=np.int64)
        blocks = infos[:, 8].astype(np.int64)
        block_off = np.zeros(b, dtype=np.int64)
        block_off[order] = np.cumsum(blocks[order]) - blocks[order]
        nblocks = int(blocks.sum())
        if bp is None:
            nbytes, spans, tables, hosted = 0, [], [], np.ones(b, dtype=bool)
        else:
            nbytes, spans, fdesc, ftab, segs, huff, nseg = self.pack_batch(files, bp, block_off)
            tables, hosted = [fdesc, ftab, segs, huff], bp.plans[:, 0] == 0
        parts = tables + [np.zeros((b, 192), dtype=np.uint16) if bp is None else bp.qts[order]] + [np.ascontiguousarray(a) for a in extra]
        offs, o = [], nbytes
        for a in parts:
            offs.append(o)
            o += (a.nbytes + 15) & ~15
        blob = o
        ho = order[hosted[order]]                             # the host-routed files as they lie in the tensor
        hb = blocks[ho]
        c_off, q_off = np.zeros(b, dtype=np.int64), np.zeros(b, dtype=np.int64)
        c_off[ho] = blob + 128 * (np.cumsum(hb) - hb)
        q_off[order] = offs[len(tables)] + 384 * np.arange(b)
        o += 128 * int(hb.sum())
        arena = self._stage(o)
        host = arena.numpy()
        for i, at, s0, e1 in spans:
            host[at:at + e1 - s0] = np.frombuffer(files[i], dtype=np.uint8)[s0:e1]
        for a, at in zip(parts, offs):
            host[at:at + a.nbytes] = a.reshape(-1).view(np.uint8)
        base = arena.data_ptr()
        scratch = np.zeros((b, 16), dtype=np.int32)

        def entropy(i):                                       # (its quantisation tables land on the plan's copy of the same values)
            try:
                self._entropy(files[i], base + int(c_off[i]), int(blocks[i]), base + int(q_off[i]), scratch[i])
            except ValueError as e:
                raise ValueError("file %d of the batch: %s" % (i, e)) from None
        list(self._pool.map(entropy, np.nonzero(hosted)[0].tolist()))
        runs = np.nonzero(np.concatenate([[True], block_off[ho[1:]] != block_off[ho[:-1]] + hb[:-1]]))[0].tolist() if len(ho) else []
        with torch.cuda.device(device):
            coef_d = torch.empty(nblocks * 64, dtype=torch.int16, device=device)
            blob_d = torch.empty(blob, dtype=torch.uint8, device=device)
            blob_d.copy_(arena[:blob], non_blocking=True)
            for r0, r1 in zip(runs, runs[1:] + [len(ho)]):
                src, dst, n16 = int(c_off[ho[r0]]), int(block_off[ho[r0]]) * 64, int(hb[r0:r1].sum()) * 64
                coef_d[dst:dst + n16].copy_(arena[src:src + 2 * n16].view(torch.int16), non_blocking=True)
            self._h2d_done = torch.cuda.Event()
            self._h2d_done.record()
            self.last_h2d_bytes = o
            dev = [blob_d[at:at + a.nbytes] for a, at in zip(parts, offs)]
            status = None
            if bp is not None:
                status = torch.empty(b, dtype=torch.int32, device=device)
                args = (blob_d[:nbytes], nbytes, ctypes.c_void_p(fdesc.ctypes.data), ctypes.c_void_p(ftab.ctypes.data),
                        ctypes.c_void_p(segs.ctypes.data), dev[0].view(torch.int32), dev[1].view(torch.int64), dev[2].view(torch.int64), dev[3],
                        int(huff.shape[0]), b, nseg)
                if self.entropy == "device_split":
                    ws = ctypes.c_long(0)
                    if self._cd.editor_jpeg_entropy_split_workspace(nseg, self.split_sub_bytes, ctypes.byref(ws)):
                        raise RuntimeError("editor_jpeg_entropy_split_workspace refused %d segments" % nseg)
                    work = torch.empty(ws.value // 8, dtype=torch.int64, device=device)
                    call("editor_jpeg_entropy_split_device", *args, self.split_sub_bytes, work, ws.value, coef_d, nblocks, status)
                else:
                    call("editor_jpeg_entropy_device", *args, coef_d, nblocks, status)
        return coef_d, block_off, status, dev[len(tables)].view(torch.int16), dev[len(tables) + 1:]

    @staticmethod
    def _raise_status(status):
        """Reads the kernel's per-file status back (a synchronisation): corrupt entropy data is reported AFTER the launch."""
        bad = torch.nonzero(status).flatten().tolist() if status is not None else []
        if bad:
            raise ValueError("file %d of the batch: JPEG entropy decode failed (rc %d)" % (bad[0], int(status[bad[0]])))

    def __call__(self, files, device):
        device = self._cuda(device)
        files = list(files)
        infos, bp = self._describe(files)
        w, h = int(infos[0][0]), int(infos[0][1])
        cw = self.crop_w if self.crop_w > 0 else w
        ncrop = w // cw
        if ncrop < 1 or (infos[:, 0] != w).any() or (infos[:, 1] != h).any():
            raise ValueError("DeviceJpegDecoder: the files of a batch must share one image size >= the crop width")
        b = len(files)
        groups = {}
        for i, inf in enumerate(infos):                      # one reconstruct call per coefficient geometry (sampling factors)
            groups.setdefault(tuple(int(v) for v in inf[:9]), []).append(i)
        order = [i for idx in groups.values() for i in idx]  # file j of a group sits at the group's start + j * blocks_per_image
        coef_d, block_off, status, qt_d, _ = self._coefficients(files, infos, bp, order, device)
        out = torch.empty(ncrop, b, h, cw, 3, dtype=torch.uint8, device=device)
        at = 0
        for key, idx in groups.items():
            n, nb = len(idx), key[8]
            ginfo = np.ascontiguousarray(infos[idx[0]])
            pb = ctypes.c_long(0)
            self._cd.editor_jpeg_planes_bytes(ctypes.c_void_p(ginfo.ctypes.data), ctypes.byref(pb))
            planes = torch.empty(n * pb.value, dtype=torch.uint8, device=device)
            dst = out if n == b else torch.empty(ncrop, n, h, cw, 3, dtype=torch.uint8, device=device)
            first = int(block_off[idx[0]])
            call("editor_jpeg_reconstruct", coef_d[first * 64:(first + n * nb) * 64], qt_d[at * 192:(at + n) * 192],
                 ctypes.c_void_p(ginfo.ctypes.data), n, planes, cw, dst)
            if n != b:
                out[:, torch.tensor(idx, device=device)] = dst
            at += n
        self._raise_status(status)
        return out

    def decode_ragged(self, files, device):
        """A batch of JPEG files of ANY mix of sizes / sampling factors / grayscale / baseline / progressive -> RaggedImages
        (grayscale replicated to three channels, as `convert('RGB')` does).  Every file is parsed before anything is launched: a
        corrupt or unsupported one raises ValueError naming its index in the batch.  Then _coefficients fills the coefficient
        tensor (entropy="host": the pool Huffman-decodes into the staging buffer, two host-to-device copies; the device modes:
        class docstring) and ONE call of the ragged entry reconstructs: two launches per batch, whatever the sizes, three with
        the entropy kernel."""
        device = self._cuda(device)
        files = list(files)
        b = len(files)
        if b < 1:
            raise ValueError("DeviceJpegDecoder.decode_ragged: empty batch")
        infos, bp = self._describe(files)
        tab, nblocks, npixels = ragged_decode_plan(infos)
        coef_d, _, status, qt_d, (info_d, tab_d) = self._coefficients(files, infos, bp, range(b), device, extra=[infos, tab])
        with torch.cuda.device(device):
            planes = torch.empty(nblocks * 64, dtype=torch.uint8, device=device)
            data = torch.empty(npixels * 3, dtype=torch.uint8, device=device)
            call("editor_jpeg_reconstruct_ragged", coef_d, qt_d, ctypes.c_void_p(infos.ctypes.data), ctypes.c_void_p(tab.ctypes.data),
                 info_d.view(torch.int32), tab_d.view(torch.int64), b, planes, data)
        self._raise_status(status)
        offsets = np.concatenate([tab[2], [npixels * 3]]).astype(np.int64)
        sizes = np.ascontiguousarray(infos[:, [1, 0]])
        return RaggedImages(data, torch.from_numpy(offsets), torch.from_numpy(sizes))


_DEFAULT = {}


def load_modalities(files_by_modality, size, interpolation=3, device="cuda", entropy="host"):
    """The separate-file sample layout (RGBNT201 / MSVR310: img_path is a list of one path per modality, each file resized on
    its own, data/datasets/bases.py:22-30).  files_by_modality: nmod lists of B byte strings -> nmod uint8 (B,Hout,Wout,3)
    tensors in the order given: ONE ragged decode + ONE ragged resize over all nmod * B files.  entropy: where the Huffman
    decode runs, as DeviceJpegDecoder's keyword ("host", the default, "device" or "device_split")."""
    if torch.device(device).type != "cuda":
        raise RuntimeError("load_modalities decodes on the GPU (no CPU fallback)")
    groups = [list(g) for g in files_by_modality]
    if not groups or not groups[0]:
        raise ValueError("load_modalities: empty batch")
    b = len(groups[0])
    if any(len(g) != b for g in groups):
        raise ValueError("load_modalities: every modality lists the same number of files")
    dkey = ("decoder", entropy)
    dec = _DEFAULT.get(dkey)
    if dec is None:
        dec = _DEFAULT[dkey] = DeviceJpegDecoder(crop_w=0, threads=16, entropy=entropy)
    key = (int(size[0]), int(size[1]), int(interpolation))
    rs = _DEFAULT.get(key)
    if rs is None:
        rs = _DEFAULT[key] = DeviceResize(size, interpolation)
    out = rs(dec.decode_ragged([f for g in groups for f in g], device))
    return [out[m * b:(m + 1) * b] for m in range(len(groups))]


def make_dataloader(cfg, rank=None, world_size=None):
    """data/datasets/make_dataloader.py:244-308 -> (train_loader, train_loader_normal, val_loader, num_query, num_classes,
    cam_num, view_num); the loaders are DeviceBatchLoader: the reference's batch tuples with the images already on the device.
    rank / world_size (MODEL.DIST_TRAIN only) default to torch.distributed's."""
    from .datasets import list_dataset
    from .loader import DeviceBatchLoader
    ds = list_dataset(cfg.DATASETS.NAMES, cfg.DATASETS.ROOT_DIR)
    inp = cfg.INPUT
    common = dict(seed=int(cfg.SOLVER.SEED), mean=tuple(inp.PIXEL_MEAN), std=tuple(inp.PIXEL_STD))
    aug = dict(prob=inp.PROB, padding=inp.PADDING, re_prob=inp.RE_PROB, **common)
    ims, kind = int(cfg.SOLVER.IMS_PER_BATCH), cfg.DATALOADER.SAMPLER
    if "triplet" in kind:
        if cfg.MODEL.DIST_TRAIN:
            sampler = RandomIdentitySampler_DDP(ds.train, ims, cfg.DATALOADER.NUM_INSTANCE, rank=rank, world_size=world_size)
            batches = torch.utils.data.sampler.BatchSampler(sampler, ims // sampler.world_size, True)
            train_loader = DeviceBatchLoader(ds.train, ims // sampler.world_size, inp.SIZE_TRAIN, True, batch_sampler=batches, **aug)
        else:
            sampler = RandomIdentitySampler(ds.train, ims, cfg.DATALOADER.NUM_INSTANCE)
            train_loader = DeviceBatchLoader(ds.train, ims, inp.SIZE_TRAIN, True, sampler=sampler, **aug)
    elif kind == "softmax":
        train_loader = DeviceBatchLoader(ds.train, ims, inp.SIZE_TRAIN, True, sampler=torch.utils.data.RandomSampler(ds.train), **aug)   # (shuffle=True)
    else:
        raise ValueError("unsupported sampler! expected softmax or triplet but got {}".format(kind))
    test_ims = int(cfg.TEST.IMS_PER_BATCH)
    val_loader = DeviceBatchLoader(ds.query + ds.gallery, test_ims, inp.SIZE_TEST, False, **common)
    train_loader_normal = DeviceBatchLoader(ds.train, test_ims, inp.SIZE_TEST, False, **common)
    return train_loader, train_loader_normal, val_loader, len(ds.query), ds.num_train_pids, ds.num_train_cams, ds.num_train_vids

