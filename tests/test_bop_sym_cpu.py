"""No device: the host side of the symmetry-aware types reS / teS / projS in ``gdrn_modeling.bop_eval`` against what the reference's own
evaluation scripts gave on the two committed datasets (tests/golden/bop_sym_golden.npz; see make_golden_bop_sym.py).  Matching and
scoring are fed with the RECORDED errors, so every match and every score field must be equal, not close."""
import json

import numpy as np
import pytest

from gdrnpp_bop2022_amd.gdrn_modeling import bop_eval as BE
from tests import bop_sym_golden as SG


@pytest.mark.parametrize("name", ["hb", "lmo"])
@pytest.mark.parametrize("n_top", [-1, 1])
def test_scores_from_the_recorded_errors_equal_the_reference_scripts(name, n_top):
    records, gt = SG.dataset(name)
    rec = SG.load()["recorded"][name][str(n_top)]
    ths = BE.SYM_CORRECT_THS                                    # KeyError / AttributeError without the feature
    BE._check_types(list(SG.SYM_TYPES), gt)                     # NotImplementedError without the feature
    for t in SG.SYM_TYPES:
        errors = SG.recorded_errors(name, n_top, t)
        want = rec["types"][t]["thresholds"]
        assert len(want) == len(ths[t]) == 3
        for th, w in zip(ths[t], want):
            assert w["sign"] == "th:" + "-".join("{:.3f}".format(x) for x in th) + "_min-visib:-1.000"
            matches, scores = BE.score_errors(errors, gt, gt.targets, gt.models_info, t, th, n_top, gt.im_width)
            got = [[m["scene_id"], m["im_id"], m["obj_id"], m["gt_id"], m["est_id"], bool(m["valid"])] for m in matches]
            assert got == w["matches"], (t, th)
            assert json.loads(json.dumps(scores)) == w["scores"], (t, th)      # recall, per-object and per-scene recalls, the counts
    final = BE.scores_from_errors({t: SG.recorded_errors(name, n_top, t) for t in SG.SYM_TYPES}, records, gt, gt.targets, gt.models_info,
                                  list(SG.SYM_TYPES), n_top, gt.im_width)
    for t in SG.SYM_TYPES:
        want = rec["types"][t]["thresholds"]
        assert final["recalls"][t] == [w["scores"]["recall"] for w in want], t
        assert json.loads(json.dumps(final["obj_recalls"][t])) == [w["scores"]["obj_recalls"] for w in want], t
        assert final[f"bop19_average_recall_{t}"] == rec["final"][f"bop19_average_recall_{t}"], t
    assert final["bop19_average_time_per_image"] == rec["final"]["bop19_average_time_per_image"]
    assert "bop19_average_recall" not in final and "bop19_average_recall" not in rec["final"]


def test_the_three_types_are_accepted_and_the_rest_is_still_refused():
    _, gt = SG.dataset("hb")
    BE._check_types(["reS", "teS", "projS", "ad", "mspd"], gt)
    for t in ("reteS", "cus", "ABSad", "ABSadd", "ABSadi", "AUCad", "AUCadd", "AUCadi"):
        with pytest.raises(NotImplementedError, match=repr(t)) as info:
            BE._check_types(["reS", t], gt)
        assert "unknown to the BOP toolkit" not in str(info.value)
        assert t in BE.KNOWN_NOT_IMPLEMENTED
    assert not set(SG.SYM_TYPES) & set(BE.KNOWN_NOT_IMPLEMENTED)
    with pytest.raises(NotImplementedError, match="unknown to the BOP toolkit"):
        BE._check_types(["reX"], gt)


def test_threshold_tables():
    """The new table holds the reference's thresholds (eval_pose_results_more.py:136-155, recorded by the generator); CORRECT_THS is what
    it was: the keys test_bop_eval_cpu.py pins, the values of the reference."""
    assert sorted(BE.SYM_CORRECT_THS) == sorted(SG.SYM_TYPES)
    for t in SG.SYM_TYPES:
        assert BE.SYM_CORRECT_THS[t] == [[th] for th in SG.load()["thresholds"]] == [[2], [5], [10]]
        assert t not in BE.NORMALIZED_BY_DIAMETER and t not in BE.NORMALIZED_BY_IM_WIDTH
    assert sorted(BE.CORRECT_THS) == ["ad", "add", "adi", "mspd", "mssd", "proj", "re", "rete", "te"]
    assert BE.CORRECT_THS["rete"] == [[2, 2], [5, 5], [10, 10]] and BE.CORRECT_THS["re"] == BE.CORRECT_THS["te"] == BE.CORRECT_THS["proj"] == [[2], [5], [10]]
    assert BE.CORRECT_THS["ad"] == BE.CORRECT_THS["add"] == BE.CORRECT_THS["adi"] == [[0.02], [0.05], [0.1]]
    assert np.array_equal(np.array(BE.CORRECT_THS["mssd"]).ravel(), np.arange(0.05, 0.51, 0.05))
    assert np.array_equal(np.array(BE.CORRECT_THS["mspd"]).ravel(), np.arange(5, 51, 5))
