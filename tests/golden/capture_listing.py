"""Writes tests/golden/l1_dataset_listing.json: for each of the five multi-modal data sets a small tree of EMPTY .jpg files and
what the reference's own class (data/datasets/{RGBNT201,market_to_RGBNT201,RGBNT100,RGBNT300,msvr310}.py, imported) lists on it:
the entries of train / query / gallery (paths relative to the root) and the twelve counts.  The pin of
editor_amd.datasets.list_dataset (tests/test_datasets_host.py rebuilds the tree from the file names recorded here).

The source pids (258, 5, 600, 9, 17, 44) are chosen so that enumerating a `set` of them does NOT give sorted order (the labels
follow the set: 258 -> 0) and so that no two of them share a slot of the set's table (distinct modulo 32 and modulo 8): the
labels then do not depend on the order in which the file system lists the files, and the recording holds on any machine.
Run in the build container:  python tests/golden/capture_listing.py"""
import importlib.util
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/data/datasets"
PIDS = (258, 5, 600, 9, 17, 44)


def trees():
    """name -> list of files (relative to the root)."""
    t = {}
    # RGBNT201: <pid:06d>_cam<c>_<seq>_<frame>.jpg under {train_171,test}/{RGB,NI,TI}
    names = ["%06d_cam%d_0_%02d.jpg" % (p, c, k) for p in PIDS for c in (1, 3) for k in range(1 + p % 2)]
    test = ["%06d_cam%d_0_%02d.jpg" % (p, c, 0) for p in (7, 301, 12) for c in (1, 2, 4)]
    t["RGBNT201"] = ["RGBNT201/%s/%s/%s" % (s, m, n) for s, ns in (("train_171", names), ("test", test)) for m in ("RGB", "NI", "TI")
                     for n in ns]
    # Market1501-MM: <pid:04d>_c<c>s1_<frame>_01.jpg, one junk (-1) file per split
    split = {"train": ["%04d_c%ds1_%06d_01.jpg" % (p, c, 100 + k) for p in PIDS for c in (1, 6) for k in range(1 + p % 2)],
             "query": ["%04d_c%ds1_000200_01.jpg" % (p, c) for p in (0, 1501, 33) for c in (2, 5)],
             "gallery": ["%04d_c%ds1_000300_01.jpg" % (p, c) for p in (0, 1501, 33, 71) for c in (1, 3, 4)]}
    for s in split:
        split[s].append("-1_c1s1_000401_03.jpg")
    t["Market1501-MM"] = ["Market1501-MM/%s/%s/%s" % (s, m, n) for s, ns in split.items() for m in ("RGB", "NI", "TI") for n in ns]
    # RGBNT100 / RGBNT300: <pid:04d>_c<c>_<frame>.jpg, stitched
    for name in ("RGBNT100", "RGBNT300"):
        split = {"bounding_box_train": ["%04d_c%d_%03d.jpg" % (p, c, k) for p in PIDS for c in (1, 8) for k in range(1 + p % 2)],
                 "query": ["%04d_c%d_000.jpg" % (p, c) for p in (1, 600, 41) for c in (2, 7)],
                 "bounding_box_test": ["%04d_c%d_%03d.jpg" % (p, c, k) for p in (1, 600, 41, 77) for c in (3, 5) for k in range(2)]}
        t[name] = ["%s/rgbir/%s/%s" % (name, s, n) for s, ns in split.items() for n in ns]
    # MSVR310: <vid:04d>/{vis,ni,th}/<vid:04d>_s<scene:03d>_v<cam>_<frame>.jpg
    split = {"bounding_box_train": [(p, sc, c, k) for p in PIDS for sc, c in ((1, 0), (4, 7)) for k in range(1 + p % 2)],
             "query3": [(p, sc, c, 0) for p in (3, 310, 21) for sc, c in ((2, 1), (9, 6))],
             "bounding_box_test": [(p, sc, c, k) for p in (3, 310, 21, 88) for sc, c in ((2, 2), (5, 3), (9, 6)) for k in range(2)]}
    t["MSVR310"] = ["MSVR310/%s/%04d/%s/%04d_s%03d_v%d_%03d.jpg" % (s, p, m, p, sc, c, k) for s, rows in split.items()
                    for (p, sc, c, k) in rows for m in ("vis", "ni", "th")]
    return t


def reference_class(module, cls):
    """The reference's class without its package __init__ (which pulls in cv2 / torchvision)."""
    pkg = types.ModuleType("ref_datasets")
    pkg.__path__ = [REF]
    sys.modules["ref_datasets"] = pkg
    for name in ("bases", module):
        spec = importlib.util.spec_from_file_location("ref_datasets." + name, os.path.join(REF, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["ref_datasets." + name] = mod
        spec.loader.exec_module(mod)
    return getattr(mod, cls)


def rel(path, root):
    if isinstance(path, str):
        return os.path.relpath(path, root)
    return [os.path.relpath(p, root) for p in path]


def main():
    classes = {"RGBNT201": ("RGBNT201", "RGBNT201"), "Market1501-MM": ("market_to_RGBNT201", "market_to_RGBNT201"),
               "RGBNT100": ("RGBNT100", "RGBNT100"), "RGBNT300": ("RGBNT300", "RGBNT300"), "MSVR310": ("msvr310", "MSVR310")}
    out = {}
    for name, files in trees().items():
        with tempfile.TemporaryDirectory() as root:
            root = os.path.realpath(root)
            for f in files:
                os.makedirs(os.path.dirname(os.path.join(root, f)), exist_ok=True)
                open(os.path.join(root, f), "wb").close()
            ds = reference_class(*classes[name])(root=root, verbose=False)
            rec = {"files": files}
            for split in ("train", "query", "gallery"):
                rec[split] = [[rel(p, root), int(pid), int(cam), int(track)] for p, pid, cam, track in getattr(ds, split)]
                rec["num_" + split] = [int(getattr(ds, "num_%s_%s" % (split, k))) for k in ("pids", "imgs", "cams", "vids")]
            out[name] = rec
    path = os.path.join(HERE, "l1_dataset_listing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote l1_dataset_listing.json: %d bytes" % os.path.getsize(path),
          {k: [len(v[s]) for s in ("train", "query", "gallery")] for k, v in out.items()})


if __name__ == "__main__":
    main()
