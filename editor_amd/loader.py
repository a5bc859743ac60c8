"""DeviceBatchLoader: sampler indices -> file bytes -> decode + resize + transform on the device -> the reference's batch tuples
(train_collate_fn / val_collate_fn of data/datasets/make_dataloader.py:190-241), produced AHEAD of the training step by one
worker thread on one side stream.

What runs where
    caller's thread, at iter()   the sampler's __iter__ (global `random` / `numpy.random`, as always) -> the epoch's index batches
    worker thread, side stream   per batch: read the files (a small pool), draw the parameter rows (generators the iterator
                                 owns), DeviceJpegDecoder -> DeviceResize -> DeviceTrainTransform (every launch of the batch
                                 on the side stream), record an event, queue the batch
    caller's thread, __next__    take the batch, make the CURRENT stream wait for its event (no host synchronisation) and
                                 record_stream every tensor on it, so the caching allocator does not give the memory back to the
                                 side stream while the step still reads it

prefetch=0 is the same code without the thread and the side stream (everything on the current stream): the yardstick.

The draws.  The reference transforms each modality image of a sample on its own (three flip / crop / erase draws per sample) in
worker processes whose seeds nobody can reproduce, so the rule is fixed HERE: parameter rows are drawn sample-major,
modality-minor - per image flip, top, left, then the erase rectangle - from a torch.Generator and a random.Random seeded from
(seed, epoch); the erase noise seed of batch i comes from (seed, epoch, i); the rows are then permuted to the modality-major
layout of the one transform launch.  The batches of an epoch are a function of (samples, sampler output, seed, epoch) only.
"""
import queue
import random
import re
import threading
import time
import weakref
from concurrent.futures import ThreadPoolExecutor

import torch

MODALITIES = ("RGB", "NI", "TI")
WORKER_NAME = "editor-loader-worker"
_MASK = (1 << 63) - 1


def derive_seed(*parts):
    """(seed, epoch[, batch]) -> one 63-bit seed (splitmix64 steps): nearby inputs give unrelated generators."""
    z = 0x1F83D9ABFB41BD6B
    for p in parts:
        z = (z ^ (int(p) & 0xFFFFFFFFFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF
        z = (z + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        z ^= z >> 31
    return z & _MASK


class EpochDraws:
    """The parameter rows and noise seeds of one (seed, epoch), batch after batch."""

    def __init__(self, transform, seed, epoch):
        self.transform, self.seed, self.epoch = transform, seed, epoch
        self.generator = torch.Generator()
        self.generator.manual_seed(derive_seed(seed, epoch))
        self.rng = random.Random(derive_seed(seed, epoch))
        self.batch = 0

    def next(self, nsample, nmod):
        """-> (int32 (nmod * nsample, 8) rows in launch order: row m * nsample + s is sample s, modality m; the noise seed)."""
        rows = self.transform.draw(nsample * nmod, generator=self.generator, rng=self.rng)
        rows = rows.view(nsample, nmod, 8).transpose(0, 1).reshape(nsample * nmod, 8).contiguous()
        seed = derive_seed(self.seed, self.epoch, self.batch)
        self.batch += 1
        return rows, seed


def _nmod(img_path):
    return None if isinstance(img_path, str) else len(img_path)


class _Failure:
    def __init__(self, exc):
        self.exc = exc


_END = object()


class DeviceBatchLoader:
    """samples: list of (img_path, pid, camid, trackid) as editor_amd.datasets.list_dataset returns them.  size: (H, W) the
    images are resized to.  train: the train transform (bicubic, flip / pad / crop / erase) and train_collate_fn's 5-tuple, or
    the val transform (Pillow BILINEAR, ToTensor + Normalize) and val_collate_fn's 6-tuple.  Iterable, with __len__; every
    iter() starts one epoch (self.epoch, which it advances).  There is no fallback to Pillow: a file the decoder refuses raises."""

    def __init__(self, samples, batch_size, size, train, *, sampler=None, batch_sampler=None, device="cuda", prefetch=2,
                 entropy="device_split", seed=0, prob=0.5, padding=10, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), re_prob=0.5,
                 read_threads=8, timeout=60.0):
        from .data import DeviceTrainTransform
        if entropy not in ("host", "device", "device_split"):
            raise ValueError("DeviceBatchLoader: entropy is 'host', 'device' or 'device_split'")
        if int(prefetch) < 0 or int(batch_size) < 1 or not 1 <= int(read_threads) <= 15:
            raise ValueError("DeviceBatchLoader: prefetch >= 0, batch_size >= 1, 1 <= read_threads <= 15")
        self.samples, self.batch_size, self.size, self.train = samples, int(batch_size), (int(size[0]), int(size[1])), bool(train)
        self.sampler, self.batch_sampler = sampler, batch_sampler
        self.device = torch.device(device)
        self.prefetch, self.entropy, self.seed, self.timeout = int(prefetch), entropy, int(seed), float(timeout)
        self.read_threads = int(read_threads)
        self.epoch = 0
        if self.train:
            self.transform = DeviceTrainTransform(self.size, prob=prob, padding=padding, mean=mean, std=std, re_prob=re_prob)
        else:                                                 # the same kernel: no flip, padding 0, no erasing
            self.transform = DeviceTrainTransform(self.size, prob=0.0, padding=0, mean=mean, std=std, re_prob=0.0)
        self.timers = {"read": 0.0, "host": 0.0, "device_ms": 0.0, "batches": 0}
        self.time_device = False                              # tools/loader_overlap.py: event-time every batch on its stream
        self._pixels = None                                   # decoder / resize / pools: made by the first batch
        self._side = None
        self._busy = threading.Lock()                         # one batch at a time per loader: two live iterators share the decoder's arena

    # ---- planning (host only) -----------------------------------------------------------------------------------------
    def index_batches(self):
        """One epoch's index batches, as torch's DataLoader forms them: a batch_sampler decides its own; else the sampler's
        indices (or 0..n-1) in chunks of batch_size, the last one possibly short (drop_last=False).  Runs the sampler's
        __iter__ on the calling thread."""
        if self.batch_sampler is not None:
            return [[int(i) for i in b] for b in self.batch_sampler]
        idx = [int(i) for i in (self.sampler if self.sampler is not None else range(len(self.samples)))]
        return [idx[i:i + self.batch_size] for i in range(0, len(idx), self.batch_size)]

    def __len__(self):
        if self.batch_sampler is not None:
            return len(self.batch_sampler)
        n = len(self.sampler) if self.sampler is not None else len(self.samples)
        return (n + self.batch_size - 1) // self.batch_size

    def draw_rows(self, epoch, batches, nmod=3):
        """The (rows, noise seed) of every batch of `epoch`, as the iterator draws them (train loaders).  batches: the index
        batches, or their sizes.  nmod: images per sample."""
        draws = EpochDraws(self.transform, self.seed, epoch)
        return [draws.next(b if isinstance(b, int) else len(b), nmod) for b in batches]

    # ---- one batch (worker thread, or the caller's for prefetch=0) ------------------------------------------------------
    def _objects(self):
        if self._pixels is None:
            from .data import DeviceJpegDecoder, DeviceResize
            threads = max(1, 16 - self.read_threads)         # read pool + Huffman pool: 16 threads together
            self._pixels = dict(                              # (crop_w only matters to the stitched layout's __call__)
                decoder=DeviceJpegDecoder(crop_w=256, threads=threads, entropy=self.entropy),
                resize=DeviceResize(self.size, 3 if self.train else 2),
                readers=ThreadPoolExecutor(max_workers=self.read_threads, thread_name_prefix="editor-loader-read"))
        return self._pixels

    @staticmethod
    def _read(paths):
        out = []
        for path in paths:
            with open(path, "rb") as f:
                out.append(f.read())
        return out

    def _refused(self, err, dec, files, paths):
        """ValueError of the decoder -> ValueError naming the file's path and its index in the batch."""
        m = re.search(r"file (\d+) of the batch: (.*)", str(err))
        if not m:
            return err
        at, why = int(m.group(1)), m.group(2)
        return ValueError("%s (file %d of the batch): %s" % (paths[at], at, why))

    def _make(self, idx, draws):
        with self._busy:
            return self._make_locked(idx, draws)

    def _make_locked(self, idx, draws):
        px = self._objects()
        b = len(idx)
        rows = [self.samples[i] for i in idx]
        nmod = _nmod(rows[0][0])
        paths = [r[0] for r in rows] if nmod is None else [r[0][m] for m in range(nmod) for r in rows]   # modality-major
        t0 = time.perf_counter()
        n = -(-len(paths) // self.read_threads)              # one run of paths per reader: a task per file costs more than the read
        files = [f for part in px["readers"].map(self._read, [paths[i:i + n] for i in range(0, len(paths), n)]) for f in part]
        t1 = time.perf_counter()
        ev0 = None
        if self.time_device:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        dec = px["decoder"]
        try:
            if nmod is None:
                crops = dec(files, self.device)               # (ncrop, B, H, 256, 3)
                nmod = int(crops.shape[0])
                u8 = px["resize"](crops.view((nmod * b,) + tuple(crops.shape[2:])))
            else:
                u8 = px["resize"](dec.decode_ragged(files, self.device))
        except ValueError as e:
            raise self._refused(e, dec, files, paths) from None
        if nmod not in (2, 3):
            raise ValueError("DeviceBatchLoader: a sample holds 2 or 3 modality images, not %d (%s)" % (nmod, paths[0]))
        if self.train:
            params, nseed = draws.next(b, nmod)
        else:
            params, nseed = torch.zeros(nmod * b, 8, dtype=torch.int32), 0
        out = self.transform(u8, params=params, seed=nseed)   # (nmod * B, 3, H, W)
        mods = [out[m * b:(m + 1) * b] for m in range(nmod)]
        if nmod == 2:
            mods.append(mods[1].clone())                      # make_dataloader.py:203-210: NI stands in for TI
        imgs = dict(zip(MODALITIES, mods))
        if ev0 is not None:
            ev1.record()
        t2 = time.perf_counter()
        pids, camids, tracks = [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows]
        first = [r[0] if isinstance(r[0], str) else r[0][0] for r in rows]
        names = tuple(p.split("/")[-1] for p in first)
        view = torch.tensor(tracks, dtype=torch.int64)
        if self.train:
            batch = (imgs, torch.tensor(pids, dtype=torch.int64), torch.tensor(camids, dtype=torch.int64), view, names)
        else:
            batch = (imgs, tuple(pids), tuple(camids), torch.tensor(camids, dtype=torch.int64), view, names)
        tm = self.timers
        tm["read"] += t1 - t0
        tm["host"] += t2 - t1
        tm["batches"] += 1
        if ev0 is not None:
            ev1.synchronize()
            tm["device_ms"] += ev0.elapsed_time(ev1)
        return batch

    def __iter__(self):
        if self.device.type != "cuda":
            raise RuntimeError("DeviceBatchLoader decodes on the GPU (no CPU fallback)")
        epoch = self.epoch
        self.epoch += 1
        batches = self.index_batches()
        draws = EpochDraws(self.transform, self.seed, epoch) if self.train else None
        if self.prefetch > 0 and self._side is None:
            with torch.cuda.device(self.device):
                self._side = torch.cuda.Stream()
        return _Epoch(self, batches, draws)

    def close(self):
        """Ends the loader's thread pools (live iterators have their own close())."""
        if self._pixels is not None:
            self._pixels["readers"].shutdown(wait=True)
            self._pixels["decoder"]._pool.shutdown(wait=True)
            self._pixels = None


def _work(loader, batches, draws, out, slots, stop, side, device):
    """The worker: holds NO reference to its iterator, so dropping the iterator lets it be collected (which stops this thread).
    It takes a slot BEFORE it makes a batch and the consumer gives one back per batch taken: never more than `prefetch`
    finished batches beyond the consumer's."""
    def slot():
        while not stop.is_set():
            if slots.acquire(timeout=0.05):
                return True
        return False
    try:
        with torch.cuda.device(device), torch.cuda.stream(side):
            for idx in batches:
                if not slot():
                    return
                batch = loader._make(idx, draws)
                done = torch.cuda.Event()
                done.record()                                 # after the batch's last launch, on the side stream
                out.put((batch, done))
                del batch, done
        out.put(_END)
    except BaseException as e:                                # re-raised by the consumer's next __next__
        out.put(_Failure(e))


def _stop(stop, thread, timeout):
    stop.set()
    if thread is not None and thread is not threading.current_thread():
        thread.join(timeout)


class _Epoch:
    """One epoch's iterator.  close() - also at exhaustion, on an error and at garbage collection - ends the worker and joins it."""

    def __init__(self, loader, batches, draws):
        self.loader, self.timeout = loader, loader.timeout
        self._batches, self._draws, self._at, self._done = batches, draws, 0, False
        self._thread, self._stop = None, threading.Event()
        if loader.prefetch > 0:
            self._queue, self._slots = queue.Queue(), threading.Semaphore(loader.prefetch)
            self._thread = threading.Thread(target=_work, name=WORKER_NAME, daemon=True,
                                            args=(loader, batches, draws, self._queue, self._slots, self._stop, loader._side,
                                                  loader.device))
            self._final = weakref.finalize(self, _stop, self._stop, self._thread, self.timeout)
            self._thread.start()

    def __iter__(self):
        return self

    def __len__(self):
        return len(self._batches)

    def close(self):
        self._done = True
        if self._thread is not None:
            _stop(self._stop, self._thread, self.timeout)
            if self._thread.is_alive():
                raise RuntimeError("DeviceBatchLoader: the worker thread did not end within %.0f s" % self.timeout)
            self._final.detach()
            self._thread = None

    def __next__(self):
        if self._done:
            raise StopIteration
        if self._thread is None:                              # prefetch=0: this thread, the current stream
            if self._at == len(self._batches):
                self._done = True
                raise StopIteration
            try:
                with torch.cuda.device(self.loader.device):
                    batch = self.loader._make(self._batches[self._at], self._draws)
            except BaseException:
                self._done = True
                raise
            self._at += 1
            return batch
        try:
            item = self._queue.get(timeout=self.timeout)
        except queue.Empty:
            self._stop.set()
            self._done = True
            raise RuntimeError("DeviceBatchLoader: no batch from the worker thread within %.0f s" % self.timeout) from None
        if item is _END:
            self.close()
            raise StopIteration
        if isinstance(item, _Failure):
            self.close()
            raise item.exc
        batch, done = item
        self._slots.release()
        cur = torch.cuda.current_stream(self.loader.device)
        cur.wait_event(done)                                  # the step's stream waits; the host does not
        for t in list(batch[0].values()):
            t.record_stream(cur)
        return batch
