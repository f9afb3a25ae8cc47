"""Loader of tests/golden/bop_sym_golden.npz (recorded from the reference's own ``re_sym / te_sym / arp_2d_sym`` and evaluation scripts by
tests/golden/make_golden_bop_sym.py), shared by test_bop_sym_cpu.py and test_gpu_sym_error.py.  The inputs are those of
bop_error_golden.npz (function level), bop_eval_golden.npz ("hb") and vsd_golden.npz ("lmo"): see tests/bop_golden.py, tests/vsd_golden.py."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SYM_TYPES = ("reS", "teS", "projS")


@functools.lru_cache(maxsize=None)
def load():
    z = np.load(os.path.join(GOLDEN, "bop_sym_golden.npz"))
    return dict(errors=z["errors"], sin_re=z["sin_re"], max_dist2d=z["max_dist2d"], thresholds=[float(t) for t in z["thresholds"]],
                error_types=json.loads(str(z["error_types"])), recorded=json.loads(str(z["recorded"])))


def dataset(name):
    """-> (records, BopGT) of the dataset the scripts ran on: "hb" without depth, "lmo" with depth and faces."""
    if name == "hb":
        from tests import bop_golden as BG

        g = BG.load_eval()
        return g["records"], BG.bop_gt(g)
    from tests import vsd_golden as VG

    g = VG.load()
    return g["script"]["records"], VG.bop_gt(g)


def recorded_errors(name, n_top, error_type):
    """{scene_id: [{"im_id", "obj_id", "est_id", "score", "errors": {gt_id: [...]}}]} as eval_calc_scores.py loads them (integer keys)."""
    raw = load()["recorded"][name][str(n_top)]["types"][error_type]["errors"]
    return {int(s): [dict(e, errors={int(k): [float(x) for x in v] for k, v in e["errors"].items()}) for e in errs] for s, errs in raw.items()}
