"""The host side of editor_amd.loader / editor_amd.data.make_dataloader: which indices make which batch (against the samplers
themselves) and the draw rule (a function of (seed, epoch) only, from generators the loader owns).  No GPU: the loaders are
built and planned, never iterated."""
import json
import os
import random

import numpy as np
import pytest
import torch

from editor_amd import config

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture()
def tree(tmp_path):
    """The RGBNT201 tree of the listing golden (empty files: nothing is decoded here)."""
    with open(os.path.join(HERE, "golden", "l1_dataset_listing.json")) as f:
        files = json.load(f)["RGBNT201"]["files"]
    for f in files:
        os.makedirs(os.path.dirname(os.path.join(str(tmp_path), f)), exist_ok=True)
        open(os.path.join(str(tmp_path), f), "wb").close()
    return str(tmp_path)


def _cfg(root, sampler="softmax_triplet", dist=False, ims=8, k=2, test_ims=4):
    cfg = config.make_cfg(size_train=(96, 64))
    cfg.DATASETS.NAMES, cfg.DATASETS.ROOT_DIR = "RGBNT201", root
    cfg.DATALOADER.SAMPLER, cfg.DATALOADER.NUM_INSTANCE = sampler, k
    cfg.SOLVER.IMS_PER_BATCH, cfg.TEST.IMS_PER_BATCH, cfg.MODEL.DIST_TRAIN = ims, test_ims, dist
    return cfg


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def test_config_carries_the_loader_keys_at_the_reference_defaults():
    cfg = config.make_cfg()
    assert (cfg.INPUT.PROB, cfg.INPUT.RE_PROB, cfg.INPUT.PADDING) == (0.5, 0.5, 10)
    assert cfg.INPUT.PIXEL_MEAN == [0.5, 0.5, 0.5] and cfg.INPUT.PIXEL_STD == [0.5, 0.5, 0.5]
    assert (cfg.DATASETS.NAMES, cfg.DATASETS.ROOT_DIR, cfg.TEST.IMS_PER_BATCH) == ("RGBNT201", "./data", 64)
    assert (cfg.DATALOADER.SAMPLER, cfg.DATALOADER.NUM_INSTANCE, cfg.SOLVER.IMS_PER_BATCH, cfg.SOLVER.SEED) == ("softmax_triplet", 16, 128, 1111)


def test_seven_tuple_and_train_batches_equal_the_identity_sampler(tree, capsys):
    from editor_amd.data import RandomIdentitySampler, make_dataloader
    from editor_amd.datasets import list_dataset
    train, normal, val, num_query, num_classes, cam_num, view_num = make_dataloader(_cfg(tree))
    ds = list_dataset("RGBNT201", tree, verbose=False)
    assert (num_query, num_classes, cam_num, view_num) == (len(ds.query), 6, 2, 1)
    assert train.samples == ds.train and train.train and not val.train and not normal.train
    assert train.size == (96, 64) and train.entropy == "device_split" and train.seed == 1111 and train.prefetch == 2
    _seed(5)
    want = list(iter(RandomIdentitySampler(ds.train, 8, 2)))
    _seed(5)
    got = train.index_batches()
    assert len(want) >= 16 and got == [want[i:i + 8] for i in range(0, len(want), 8)]
    assert len(train) == (len(train.sampler) + 7) // 8


def test_ddp_train_batches_equal_the_per_rank_mini_batches(tree):
    from editor_amd.data import RandomIdentitySampler_DDP, make_dataloader
    from editor_amd.datasets import list_dataset
    ds = list_dataset("RGBNT201", tree, verbose=False)
    seen = []
    for rank in (0, 1):
        train = make_dataloader(_cfg(tree, dist=True), rank=rank, world_size=2)[0]
        _seed(9)
        want = list(iter(RandomIdentitySampler_DDP(ds.train, 8, 2, rank=rank, world_size=2)))
        _seed(9)
        got = train.index_batches()
        assert got and all(len(b) == 4 for b in got)                          # IMS_PER_BATCH // world, the partial one dropped
        assert got == [want[i:i + 4] for i in range(0, len(want) - len(want) % 4, 4)]
        seen.append(got)
    assert seen[0] != seen[1]


def test_softmax_sampler_and_unknown_sampler(tree):
    from editor_amd.data import make_dataloader
    train = make_dataloader(_cfg(tree, sampler="softmax"))[0]
    _seed(2)
    want = list(torch.utils.data.RandomSampler(range(len(train.samples))))     # what DataLoader(shuffle=True) draws
    _seed(2)
    got = train.index_batches()
    assert got == [want[i:i + 8] for i in range(0, len(want), 8)] and len(got[-1]) == len(want) % 8 == 2
    assert len(train) == 3
    with pytest.raises(ValueError, match="unsupported sampler"):
        make_dataloader(_cfg(tree, sampler="random"))


def test_val_batches_cover_query_then_gallery_in_order(tree):
    from editor_amd.data import make_dataloader
    from editor_amd.datasets import list_dataset
    _, normal, val, num_query, _, _, _ = make_dataloader(_cfg(tree, test_ims=4))
    ds = list_dataset("RGBNT201", tree, verbose=False)
    assert val.samples == ds.query + ds.gallery and num_query == 9
    got = val.index_batches()
    assert [i for b in got for i in b] == list(range(18))
    assert [len(b) for b in got] == [4, 4, 4, 4, 2] and len(val) == 5         # the short last batch is kept
    assert normal.samples == ds.train and [i for b in normal.index_batches() for i in b] == list(range(len(ds.train)))
    assert normal.size == val.size == (96, 64)


def _loader(prefetch, seed=7, **kw):
    from editor_amd.loader import DeviceBatchLoader
    samples = [(["a.jpg", "b.jpg", "c.jpg"], i // 4, i % 2, -1) for i in range(20)]
    return DeviceBatchLoader(samples, 8, (96, 64), True, prefetch=prefetch, seed=seed, **kw)


def test_draws_depend_on_seed_and_epoch_only():
    sizes = [8, 8, 4]
    runs = [_loader(p).draw_rows(3, sizes) for p in (0, 1, 3, 3)]
    for other in runs[1:]:
        for (r0, s0), (r1, s1) in zip(runs[0], other):
            assert torch.equal(r0, r1) and s0 == s1
    rows = torch.cat([r for r, _ in runs[0]])
    assert rows.shape == (60, 8) and rows.dtype == torch.int32
    assert 10 < int(rows[:, 0].sum()) < 50 and 10 < int(rows[:, 3].sum()) < 50 and int(rows[:, 1:3].max()) <= 20
    assert len({s for _, s in runs[0]}) == 3                                  # one noise seed per batch
    nxt = _loader(0).draw_rows(4, sizes)
    assert not torch.equal(torch.cat([r for r, _ in nxt]), rows) and {s for _, s in nxt}.isdisjoint({s for _, s in runs[0]})
    oth = _loader(0, seed=8).draw_rows(3, sizes)
    assert not torch.equal(torch.cat([r for r, _ in oth]), rows)


def test_rows_are_drawn_sample_major_and_launched_modality_major():
    from editor_amd.data import DeviceTrainTransform
    from editor_amd.loader import derive_seed
    ld = _loader(0)
    (rows, nseed), = ld.draw_rows(1, [5])
    gen = torch.Generator()
    gen.manual_seed(derive_seed(7, 1))
    flat = DeviceTrainTransform((96, 64)).draw(15, generator=gen, rng=random.Random(derive_seed(7, 1)))
    for s in range(5):
        for m in range(3):
            assert torch.equal(rows[m * 5 + s], flat[s * 3 + m])
    assert nseed == derive_seed(7, 1, 0)
    two = ld.draw_rows(1, [5], nmod=2)[0][0]                                  # two-modality samples: two rows each
    assert two.shape == (10, 8) and torch.equal(two[5 + 2], flat[2 * 2 + 1])


def test_drawing_leaves_the_global_generators_untouched():
    _seed(11)
    before = (random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state().clone())
    _loader(2).draw_rows(0, [8, 8, 4])
    assert random.getstate() == before[0] and np.array_equal(np.random.get_state()[1], before[1])
    assert torch.equal(torch.get_rng_state(), before[2])
    # ... while the keyword-less calls still consume the globals, as before
    from editor_amd.data import DeviceTrainTransform
    DeviceTrainTransform((96, 64)).draw(4)
    assert random.getstate() != before[0] and not torch.equal(torch.get_rng_state(), before[2])


def test_loader_refuses_a_cpu_device_and_bad_arguments():
    from editor_amd.loader import DeviceBatchLoader
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        iter(DeviceBatchLoader([("a.jpg", 0, 0, -1)], 1, (96, 64), False, device="cpu"))
    with pytest.raises(ValueError):
        DeviceBatchLoader([], 1, (96, 64), False, entropy="pillow")
    with pytest.raises(ValueError):
        DeviceBatchLoader([], 1, (96, 64), False, prefetch=-1)
