"""editor_amd.datasets.list_dataset against what the reference's own data set classes listed on the same tree
(tests/golden/l1_dataset_listing.json, made by tests/golden/capture_listing.py): entries as multisets, the order of the
test-time glob / listdir, the counts, and the refusals."""
import glob
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("RGBNT201", "Market1501-MM", "RGBNT100", "RGBNT300", "MSVR310")
SPLITS = {"RGBNT201": ("train_171", "test", "test"), "Market1501-MM": ("train", "query", "gallery"),
          "RGBNT100": ("rgbir/bounding_box_train", "rgbir/query", "rgbir/bounding_box_test"),
          "RGBNT300": ("rgbir/bounding_box_train", "rgbir/query", "rgbir/bounding_box_test"),
          "MSVR310": ("bounding_box_train", "query3", "bounding_box_test")}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "l1_dataset_listing.json")) as f:
        return json.load(f)


def _tree(root, files):
    for f in files:
        os.makedirs(os.path.dirname(os.path.join(root, f)), exist_ok=True)
        open(os.path.join(root, f), "wb").close()


def _rel(path, root):
    return os.path.relpath(path, root) if isinstance(path, str) else [os.path.relpath(p, root) for p in path]


def _key(entry):
    return (entry[0] if isinstance(entry[0], str) else tuple(entry[0]),) + tuple(entry[1:])


def _listed_first_paths(name, split_dir):
    """The first path of every sample in the order the file system lists them NOW (junk files included)."""
    if name in ("RGBNT201", "Market1501-MM"):
        return glob.glob(os.path.join(split_dir, "RGB", "*.jpg"))
    if name in ("RGBNT100", "RGBNT300"):
        return glob.glob(os.path.join(split_dir, "*.jpg"))
    return [os.path.join(split_dir, v, "vis", img) for v in os.listdir(split_dir) for img in os.listdir(os.path.join(split_dir, v, "vis"))]


@pytest.mark.parametrize("name", NAMES)
def test_listing_matches_the_reference_classes(name, golden, tmp_path, capsys):
    from editor_amd.datasets import list_dataset
    g = golden[name]
    root = str(tmp_path)
    _tree(root, g["files"])
    ds = list_dataset(name, root)
    assert "train" in capsys.readouterr().out                                # the statistics table is printed
    labels = set()
    for split, sub in zip(("train", "query", "gallery"), SPLITS[name]):
        got = getattr(ds, split)
        rel = [[_rel(e[0], root), e[1], e[2], e[3]] for e in got]
        assert sorted(map(_key, rel)) == sorted(map(_key, g[split])), split                       # the same entries ...
        first = [e[0] if isinstance(e[0], str) else e[0][0] for e in got]
        listed = [p for p in _listed_first_paths(name, os.path.join(root, name, sub)) if not os.path.basename(p).startswith("-1_")]
        assert first == listed, split                                                               # ... in the listing's order
        counts = [getattr(ds, "num_%s_%s" % (split, k)) for k in ("pids", "imgs", "cams", "vids")]
        assert counts == g["num_" + split], split
        for e in got:                                                                               # the containers of the reference
            assert type(e) is tuple and type(e[0]) is {"RGBNT100": str, "RGBNT300": str, "MSVR310": tuple}.get(name, list)
        if split == "train":
            labels = {e[1] for e in got}
    assert labels == set(range(6))                                           # relabelled; query / gallery keep the source pids
    assert all("258" in str(e[0]) for e in ds.train if e[1] == 0)            # set order, not sorted order: 258 is label 0
    assert not any("-1_" in str(e[0]) for e in ds.train + ds.query + ds.gallery)


def test_verbose_off_prints_nothing(golden, tmp_path, capsys):
    from editor_amd.datasets import list_dataset
    _tree(str(tmp_path), golden["RGBNT100"]["files"])
    list_dataset("RGBNT100", str(tmp_path), verbose=False)
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("name", NAMES)
def test_missing_directory(name, golden, tmp_path):
    from editor_amd.datasets import list_dataset
    root = str(tmp_path)
    with pytest.raises(RuntimeError, match="is not available"):
        list_dataset(name, root)
    gallery = SPLITS[name][2]
    _tree(root, [f for f in golden[name]["files"] if "/" + gallery.split("/")[-1] + "/" not in f])
    if name == "RGBNT201":                                                   # (query = gallery = test: drop the train split instead)
        import shutil
        shutil.rmtree(os.path.join(root, name, "train_171"))
        gallery = "train_171"
    with pytest.raises(RuntimeError) as e:
        list_dataset(name, root)
    assert str(e.value) == "'%s' is not available" % os.path.join(os.path.abspath(root), name, gallery)


@pytest.mark.parametrize("name,bad", [
    ("Market1501-MM", "Market1501-MM/train/RGB/1502_c1s1_000001_01.jpg"),    # pid above 1501
    ("Market1501-MM", "Market1501-MM/gallery/RGB/0005_c7s1_000001_01.jpg"),  # camera 7 of 1..6
    ("Market1501-MM", "Market1501-MM/query/RGB/0005_c0s1_000001_01.jpg"),    # camera 0
    ("RGBNT100", "RGBNT100/rgbir/bounding_box_train/0601_c1_000.jpg"),
    ("RGBNT100", "RGBNT100/rgbir/query/0000_c1_000.jpg"),
    ("RGBNT100", "RGBNT100/rgbir/bounding_box_test/-1_c1_000.jpg"),           # junk is not skipped in the stitched sets
    ("RGBNT300", "RGBNT300/rgbir/bounding_box_test/0005_c9_000.jpg"),
    ("MSVR310", "MSVR310/bounding_box_test/0003/vis/0003_s002_v8_000.jpg"),   # camera 8 of 0..7
])
def test_out_of_range_ids(name, bad, golden, tmp_path):
    from editor_amd.datasets import list_dataset
    root = str(tmp_path)
    _tree(root, golden[name]["files"] + [bad])
    with pytest.raises(AssertionError):
        list_dataset(name, root, verbose=False)


def test_unknown_name(tmp_path):
    from editor_amd.datasets import list_dataset
    with pytest.raises(KeyError):
        list_dataset("market1501", str(tmp_path))
