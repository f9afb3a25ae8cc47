"""Golden background replacement from the reference's OWN methods (authoring container only: needs /root/reference; never run by a test).

``Base_DatasetFromList.replace_bg``, ``trunc_mask``, ``get_bg_image`` and ``get_bg_image_v2`` (core/base_data_loader.py:413-579) and
``resize_short_edge`` (core/utils/data_utils.py:208-235) are imported from the reference's files through ``_refimport`` and run UNMODIFIED,
bound to a stand-in ``self`` (cfg, img_format "BGR", ``_bg_img_paths`` = the indices of the case's backgrounds).  Served by stand-ins, set as
globals of the two reference modules:

    cv2.resize        tests/replace_bg_ref.py's restatement, in both calling forms (dsize, and fx / fy); every request is recorded: where
                      the crop lies in its background, its size, and dsize or fx / fy
    read_image_mmcv   the case's seeded background of that index
    random            a ``random.Random`` seeded with the case's py_seed — the sequence ``random.seed`` gives the module — that records
                      what its ``random()`` returns: trunc_mask's branch draw and the u behind its ``random.uniform``
    np                a proxy of numpy that adds the removed alias ``np.bool`` and whose ``random`` is a RandomState seeded with np_seed

The one step taken from read_data_train (core/gdrn_modeling/datasets/data_loader.py:360-369) is written out here, not executed: an image
whose img_type is not "syn" draws ``np.random.rand()`` against INPUT.CHANGE_BG_PROB first and is left alone when it loses.
After each case both generators are asked for one more number, so a test can see that they were consumed exactly as far.
-> replace_bg_golden.npz: per case the seeds, the recorded requests and draws, the composite and mask_trunc.  Inputs are re-drawn from the
case's name (tests/replace_bg_ref.py ``case_inputs``), not stored."""
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import _refimport  # noqa: E402

from tests import replace_bg_ref as R  # noqa: E402


def recording_random(seed):
    """random.Random(seed) whose random() records what it returns.  The wrapper sits on the instance: a subclass that overrides random()
    makes randint draw through it (``Random.__init_subclass__``), which is not the module's sequence."""
    py = random.Random(seed)
    py.floats = []
    py.random = lambda: py.floats.append(random.Random.random(py)) or py.floats[-1]
    return py


class NpProxy:
    bool = bool

    def __init__(self, seed):
        self.random = np.random.RandomState(seed)

    def __getattr__(self, name):
        return getattr(np, name)


def main():
    _refimport.install()
    import core.base_data_loader as B
    import core.utils.data_utils as D

    cls = B.Base_DatasetFromList
    rec = dict(meta=json.dumps(dict(cases=list(R.CASES), input_seed=R.INPUT_SEED,
                                    source="core/base_data_loader.py:413-579 and core/utils/data_utils.py:208-235 run from the reference's files")))
    branches = set()
    for name, c in R.CASES.items():
        image, mask, bgs = R.case_inputs(name)
        requests = []

        def resize(src, dsize=None, dst=None, fx=None, fy=None, interpolation=None, bgs=bgs, requests=requests):
            assert interpolation is None or not isinstance(interpolation, int) or interpolation == 1      # INTER_LINEAR
            base = next(b for b in bgs if np.shares_memory(b, src))
            off = src.__array_interface__["data"][0] - base.__array_interface__["data"][0]
            y0, x0 = off // (base.shape[1] * 3), (off % (base.shape[1] * 3)) // 3
            out = R.cv2_resize(src, dsize=dsize, fx=fx, fy=fy)
            requests.append([x0, y0, src.shape[1], src.shape[0]] + ([int(dsize[0]), int(dsize[1]), 0.0, 0.0] if dsize is not None else [0, 0, fx, fy])
                            + [out.shape[1], out.shape[0]])
            return out

        cv2 = types.SimpleNamespace(resize=resize, INTER_LINEAR=1, INTER_NEAREST=0)
        py, npx = recording_random(c["py_seed"]), NpProxy(c["np_seed"])
        B.cv2 = D.cv2 = cv2
        B.random, B.np = py, npx
        B.read_image_mmcv = lambda filename, format=None, bgs=bgs: bgs[filename]
        cfg = {"INPUT": dict(BG_KEEP_ASPECT_RATIO=c["keep_aspect"], TRUNCATE_FG=c["truncate"], CHANGE_BG_PROB=c["prob"])}
        B.try_get_key = lambda cfg, *keys, default=None: cfg["INPUT"].get(keys[0].split(".")[1], default)
        self = types.SimpleNamespace(cfg=cfg, img_format="BGR", _bg_img_paths=list(range(len(bgs))))
        for m in ("trunc_mask", "get_bg_image", "get_bg_image_v2"):
            setattr(self, m, types.MethodType(getattr(cls, m), self))
        ind = []
        orig_randint = py.randint
        py.randint = lambda a, b: ind.append(orig_randint(a, b)) or ind[-1]
        do = True
        if c["img_type"] != "syn":                                   # read_data_train :362-368, written out
            do = bool(npx.random.rand() < c["prob"])
        if do:
            out, keep = cls.replace_bg(self, image.copy(), mask, return_mask=True, truncate_fg=c["truncate"])
            assert out.dtype == np.uint8 and keep.dtype == bool and len(requests) == 1 and len(ind) == 1
        else:
            out, keep = image.copy(), np.zeros(mask.shape, bool)
        floats = list(py.floats)
        cut = 0
        if do and c["truncate"]:
            cut = next((k + 1 for k, bound in enumerate((0.2, 0.4, 0.6, 0.8)) if floats[0] < bound), 0)
            assert len(floats) == (2 if cut else 1)
            branches.add(cut)
        p = name + "_"
        rec[p + "do"], rec[p + "ind"], rec[p + "cut"] = np.int64(do), np.int64(ind[0] if do else -1), np.int64(cut)
        rec[p + "rnd"] = np.float64(floats[0] if floats else -1.0)
        rec[p + "u"] = np.float64(floats[1] if cut else 0.0)
        rec[p + "request"] = np.array(requests[0] if do else [0] * 10, np.float64)     # x0, y0, cw, ch, dsize w, h (0 0: the fx form), fx, fy, returned w, h
        rec[p + "composite"], rec[p + "mask_trunc"] = out, keep.astype(np.uint8)
        rec[p + "next_py"], rec[p + "next_np"] = np.float64(random.Random.random(py)), np.float64(npx.random.rand())
        rec[p + "seeds"] = np.array([c["py_seed"], c["np_seed"]], np.int64)
        print(name, "do", int(do), "ind", ind, "cut", R.CUTS[cut], "request", requests, "kept", int(keep.sum()), "of", int((mask != 0).sum()))
    assert branches == {0, 1, 2, 3, 4}, branches
    path = os.path.join(HERE, "replace_bg_golden.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("wrote replace_bg_golden.npz", size, "bytes")


if __name__ == "__main__":
    main()
