"""Data set listings (data/datasets/{RGBNT201,market_to_RGBNT201,RGBNT100,RGBNT300,msvr310}.py of the reference): which files
make a sample and which pid / camera / track id each carries - one table row per data set, one walker for all of them.

    ds = list_dataset("RGBNT201", root)          # .train / .query / .gallery: lists of (img_path, pid, camid, trackid)
                                                 # .num_{train,query,gallery}_{pids,imgs,cams,vids}

img_path is a str for the stitched layout (one 768x128 file holding the modalities side by side) and a list (MSVR310: a tuple)
of one path per modality for the separate-file layouts.  Entries come in the order glob.glob / os.listdir return them (NOT
sorted) and train pids are relabelled by enumerating a `set` of the source pids, both as in the reference: on the same tree a
sampler's indices address the same files and the same labels there and here (tests/golden/l1_dataset_listing.json).
"""
import glob
import os
import os.path as osp
import re
from types import SimpleNamespace

_STITCHED = re.compile(r"([-\d]+)_c([-\d]+)")

# layout kinds
#   "modal"     <split>/{RGB,NI,TI}/<name>.jpg      sample = [RGB, NI, TI] paths of one file name; ids from the NAME
#   "stitched"  <split>/*.jpg                       sample = the file; ids from the first pattern match on the PATH
#   "tracks"    <split>/<vid>/{vis,ni,th}/<img>     sample = (vis, ni, th); labels from the <vid> directories, ids from <img>
# pid / cam: name -> source id; junk: a source pid that is dropped; pid_range / cam_range: inclusive bounds on the SOURCE ids
# (AssertionError outside); cam_shift: added to the source camera; track: name -> 4th field; abs_root: the root is made absolute
_TABLE = {
    "RGBNT201": dict(dir="RGBNT201", splits=("train_171", "test", "test"), kind="modal", abs_root=True,
                     pid=lambda n: int(n.split("_")[0][0:6]), cam=lambda n: int(n.split("_")[1][3]), junk=None,
                     pid_range=None, cam_range=None, cam_shift=-1),
    "Market1501-MM": dict(dir="Market1501-MM", splits=("train", "query", "gallery"), kind="modal", abs_root=True,
                          pid=lambda n: int(n.split("_")[0]), cam=lambda n: int(n.split("_")[1][1]), junk=-1,
                          pid_range=(0, 1501), cam_range=(1, 6), cam_shift=-1),
    "RGBNT100": dict(dir="RGBNT100/rgbir", splits=("bounding_box_train", "query", "bounding_box_test"), kind="stitched",
                     abs_root=False, pid_range=(1, 600), cam_range=(1, 8), cam_shift=-1),
    "RGBNT300": dict(dir="RGBNT300/rgbir", splits=("bounding_box_train", "query", "bounding_box_test"), kind="stitched",
                     abs_root=False, pid_range=(1, 600), cam_range=(1, 8), cam_shift=-1),
    "MSVR310": dict(dir="MSVR310", splits=("bounding_box_train", "query3", "bounding_box_test"), kind="tracks", abs_root=True,
                    pid=lambda n: int(n[0:4]), cam=lambda n: int(n[11]), track=lambda n: int(n[6:9]),
                    pid_range=None, cam_range=(0, 7), cam_shift=0),
}
NAMES = tuple(_TABLE)


def _in(v, bounds):
    return bounds is None or bounds[0] <= v <= bounds[1]


def _walk(row, dir_path, relabel):
    """One split of one data set -> [(img_path, pid, camid, trackid)]."""
    kind = row["kind"]
    if kind == "tracks":
        vids = os.listdir(dir_path)
        label = {v: i for i, v in enumerate(set(int(v) for v in vids))}
        raw = [(v, img) for v in vids for img in os.listdir(osp.join(dir_path, v, "vis"))]
        found = [(tuple(osp.join(dir_path, v, m, img) for m in ("vis", "ni", "th")), row["pid"](img), row["cam"](img),
                  row["track"](img)) for v, img in raw]
    elif kind == "stitched":
        paths = glob.glob(osp.join(dir_path, "*.jpg"))
        ids = [tuple(map(int, _STITCHED.search(p).groups())) for p in paths]
        label = {p: i for i, p in enumerate(set(pid for pid, _ in ids if pid != -1))}
        found = [(p, pid, cam, -1) for p, (pid, cam) in zip(paths, ids)]
    else:
        paths = glob.glob(osp.join(dir_path, "RGB", "*.jpg"))
        names = [p.split("/")[-1] for p in paths]
        junk = row["junk"]
        label = {p: i for i, p in enumerate(set(pid for pid in map(row["pid"], names) if pid != junk))}
        found = [([p, osp.join(dir_path, "NI", n), osp.join(dir_path, "TI", n)], row["pid"](n), row["cam"](n), -1)
                 for p, n in zip(paths, names) if row["pid"](n) != junk]
    data = []
    for img_path, pid, cam, track in found:
        assert _in(pid, row["pid_range"]), "%s: pid %d outside %s" % (img_path, pid, row["pid_range"])
        assert _in(cam, row["cam_range"]), "%s: camera %d outside %s" % (img_path, cam, row["cam_range"])
        data.append((img_path, label[pid] if relabel else pid, cam + row["cam_shift"], track))
    return data


def _info(data):
    """-> (# pids, # images, # cameras, # 4th-field values)."""
    return (len(set(d[1] for d in data)), len(data), len(set(d[2] for d in data)), len(set(d[3] for d in data)))


def list_dataset(name, root, verbose=True):
    row = _TABLE.get(name)
    if row is None:
        raise KeyError("list_dataset: unknown data set %r (one of %s)" % (name, ", ".join(NAMES)))
    if row["abs_root"]:
        root = osp.abspath(osp.expanduser(root))
    base = osp.join(root, row["dir"])
    dirs = [osp.join(base, s) for s in row["splits"]]
    for d in [base] + dirs:
        if not osp.exists(d):
            raise RuntimeError("'{}' is not available".format(d))
    ds = SimpleNamespace(name=name, dataset_dir=base, train_dir=dirs[0], query_dir=dirs[1], gallery_dir=dirs[2])
    for split, d in zip(("train", "query", "gallery"), dirs):
        data = _walk(row, d, relabel=(split == "train"))
        setattr(ds, split, data)
        for key, v in zip(("pids", "imgs", "cams", "vids"), _info(data)):
            setattr(ds, "num_%s_%s" % (split, key), v)
    if verbose:
        print("=> %s loaded" % name)
        print("Dataset statistics:")
        print("  ----------------------------------------")
        print("  subset   | # ids | # images | # cameras")
        print("  ----------------------------------------")
        for split in ("train", "query", "gallery"):
            print("  {:8s} | {:5d} | {:8d} | {:9d}".format(split, *[getattr(ds, "num_%s_%s" % (split, k)) for k in ("pids", "imgs", "cams")]))
        print("  ----------------------------------------")
    return ds
