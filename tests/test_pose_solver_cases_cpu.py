"""The builders of tests/pose_solver_cases.py without a GPU: every precondition that makes a case of
tests/test_gpu_pose_solver_edges.py prove something is asserted here against the oracles — the oracle's own answer does not depend on
the order of the sums or on the last bits of the image points, each case ends with the termination code it is there for, the long
runs really reject steps, the rotation cases really evaluate the first-order branch, each pi matrix takes the branch of
rodrigues_log it is named for, neither far-fallback decision is marginal, and the RANSAC runs stop where the case says they do."""
import numpy as np
import pytest

import pose_solver_cases as C
from oracle import epnp as E
from oracle import postproc as P


# ------------------------------------------------------------------------------------------------ uncertainty_pnp_batched
def test_lm_case_list_is_the_listed_one():
    assert C.LM_COUNTS == (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 700)
    assert [len(C.lm_case(n).p2) for n in C.LM_COUNT_NAMES] == list(C.LM_COUNTS)
    assert len(C.lm_case("aniso").p2) == 9 and len(C.lm_case("nonfinite").p2) == 200
    pn64 = C.lm_names_with(64)
    iters = sorted(C.lm_oracle(C.lm_case(n))[1][0] for n in pn64)
    assert len(pn64) >= 8 and iters[0] == 0 and iters[-1] == 50 and len(set(iters)) >= 6, (pn64, iters)
    assert not C.lm_case("pn64").p2.flags.writeable


@pytest.mark.parametrize("name", C.LM_NAMES)
def test_lm_case_is_order_robust_and_ends_as_intended(name):
    case = C.lm_case(name)
    out, info = C.lm_oracle(case)
    infos, moved = C.lm_robustness(case)
    assert infos == {info}, (name, infos)
    assert moved <= C.ROBUST_TOL, (name, moved)
    assert C.lm_expectation_holds(name, info), (name, info)
    assert np.isfinite(out).all()
    if name in C.LM_START_KEPT:
        assert np.array_equal(out.view(np.uint64), case.init.view(np.uint64))
    elif info[1] in (0, 1):
        assert np.abs(project_error(case, out)).max() < 5 * max(0.5, 1e-9), name     # converged onto the data, not somewhere else


def project_error(case, rt):
    """Reprojection residuals in pixels of the finite correspondences."""
    ok = np.isfinite(case.p2).all(1)
    return (C.project(case.p3[ok], rt) - case.p2[ok]).ravel()


def test_a_non_robust_case_is_told_apart():
    """The check has teeth: long runs the oracle itself is unsure about exist among the neighbours of the frozen seeds."""
    kw = {k: v for k, v in C.LM_SPECS["code3_pn64"].items() if k != "seed"}
    fragile = [s for s in range(60) if C.lm_oracle(C.lm_problem(s, **kw))[1][0] >= 30 and not C.lm_is_robust(C.lm_problem(s, **kw))]
    assert fragile, "no fragile long run among 60 neighbours"


@pytest.mark.parametrize("name", C.LM_REJECTING)
def test_long_runs_reject_steps_and_reuse_the_diagonal(name):
    tr = C.lm_trace(C.lm_case(name))
    assert tr["info"] == C.lm_oracle(C.lm_case(name))[1]
    assert tr["rejected"] >= 5 and tr["reused_diag"] == tr["rejected"] and tr["accepted"] >= 9, tr
    assert tr["accepted"] + tr["rejected"] + tr["invalid"] + int(tr["info"][1] in (0, 1)) == tr["info"][0]


def test_code5_is_five_invalid_steps_after_an_overflow():
    case = C.lm_case("code5")
    tr = C.lm_trace(case)
    assert tr["info"] == (5, 5) and tr["invalid"] == 5 and tr["accepted"] == tr["rejected"] == 0 and tr["failed_evals"] == 1


def test_rotation_cases_sit_in_the_branches_they_are_named_for():
    tr = C.lm_trace(C.lm_case("start_rot0"))
    assert tr["info"] == C.lm_oracle(C.lm_case("start_rot0"))[1] and tr["first_order"] == 1 and tr["general"] >= 3
    for name, lo, hi in (("truth_rot1e-9", 5e-10, 2e-9), ("truth_rot1e-8", 10 * C.LM_ATOL, 1.49e-8)):
        tr = C.lm_trace(C.lm_case(name))
        out, info = C.lm_oracle(C.lm_case(name))
        assert tr["info"] == info and info[0] >= 3 and tr["first_order"] == info[0] + 1 and tr["general"] == 0, tr     # every evaluation
        assert lo < np.linalg.norm(out[:3]) < hi, name                       # the optimum lies inside the first-order branch
        assert np.abs(out - C.lm_case(name).truth).max() < 1e-10
    out, info = C.lm_oracle(C.lm_case("truth_rot_pi"))
    assert abs(np.linalg.norm(out[:3]) - np.pi) < 0.02 and abs(out[0]) > 3.1


def test_weight_cases():
    a, b = C.lm_case("aniso"), C.lm_case("aniso_1e6")
    assert a.w[:, 1].min() < -0.3 and a.w[:, 1].max() > 0.3 and a.w[:, 1].all()          # off-diagonal terms of either sign
    assert np.array_equal(b.w, a.w * 1e6) and np.array_equal(a.p2, b.p2)
    assert not C.lm_case("zero_weights").w.any()
    assert (C.lm_case("code5").w == [1e160, 0.0, 1e160]).all()


def test_nonfinite_case_has_one_nan_and_one_inf_in_different_passes():
    p2 = C.lm_case("nonfinite").p2
    assert np.isnan(p2).sum() == 1 and np.isposinf(p2).sum() == 1 and np.isfinite(p2).sum() == 398
    rows = sorted(set(np.flatnonzero(~np.isfinite(p2).all(1))))
    assert rows == sorted(C.NONFINITE_ROWS) and rows[0] // 64 != rows[1] // 64 and rows[0] % 64 != rows[1] % 64
    tr = C.lm_trace(C.lm_case("nonfinite"))
    assert tr["info"] == (0, 2) and tr["failed_evals"] == 1


# ------------------------------------------------------------------------------------------ pnp_iter_from_correspondences
def _iter_precondition(case):
    lm = C.iter_as_lm(case)
    infos, moved = C.lm_robustness(lm)
    _, info = C.lm_oracle(lm)
    assert infos == {info} and moved <= C.ROBUST_TOL, (infos, moved)
    return info


@pytest.mark.parametrize("n", C.ITER_COUNTS)
def test_iter_count_cases(n):
    case = C.iter_count_case(n)
    assert len(case.img) == n and case.img.dtype == np.float32 and case.R_net.dtype == np.float32
    R, t, info = C.iter_oracle(case)
    if n < 4:
        assert info == (0, -1) and np.array_equal(R, case.R_net) and np.array_equal(t, case.t_net)
    else:
        assert _iter_precondition(case)[1] in (0, 1) and info[1] < 100
        assert np.abs(t - case.t_true).max() < 0.05


def test_iter_pack_fills_the_unused_rows_with_nan():
    cases = [C.iter_count_case(n) for n in C.ITER_COUNTS]
    img, mdl, count, K, R_net, t_net = C.iter_pack(cases, C.ITER_STRIDE)
    assert C.ITER_COUNTS == (0, 3, 4, 5, 63, 64, 65, 129, 256) and count.tolist() == list(C.ITER_COUNTS)
    for i, n in enumerate(C.ITER_COUNTS):
        assert np.isfinite(img[i, :n]).all() and np.isnan(img[i, n:]).all() and np.isnan(mdl[i, n:]).all()


@pytest.mark.parametrize("name", list(C.ITER_RNET))
def test_iter_rnet_cases_take_the_branch_they_are_named_for(name):
    case = C.iter_rnet_case(name)
    R = C.ITER_RNET[name]
    assert R.dtype == np.float32 and np.array_equal(case.R_net, R)
    small_s, c_pos = C.rodrigues_log_path(R)[:2]
    r = P.rodrigues_log(R)
    if name == "identity":
        assert small_s and c_pos and not r.any()
    else:
        assert small_s and not c_pos and abs(np.linalg.norm(r) - np.pi) < 1e-6
        assert np.abs(P.rodrigues_exp(r) - R).max() < 1e-6                   # the signs came out right: it is the same rotation
    assert _iter_precondition(case)[1] in (0, 1)


def test_iter_oblique_pi_matrices_differ_in_the_sign_tests_that_fire():
    paths = {name: C.rodrigues_log_path(C.ITER_RNET[name])[2:] for name in C.ITER_RNET_OBLIQUE}
    assert len(set(paths.values())) == len(paths), paths
    fired = np.array(list(paths.values()))
    assert fired.any(0).all() and not fired.all(0).any(), paths     # every decision (ry sign, rz sign, rx smallest, flip) goes both ways
    assert paths["pi_0_1_-1"][3] and not paths["pi_0.2_-1_-1"][3] and paths["pi_0.2_-1_-1"][2]


def test_iter_far_fallback_is_not_marginal():
    for which, fires in (("far", True), ("near", False)):
        case = C.iter_far_case(which)
        info = _iter_precondition(case)
        rt, _ = C.lm_oracle(C.iter_as_lm(case))
        d = np.linalg.norm(rt[3:] - case.t_net.astype(np.float64))
        assert abs(d - 1) > 0.01 and (d > 1) == fires, (which, d)
        assert abs(case.t_true[2] - 0.9) < 1e-12 and abs(float(case.t_net[2]) - (2.5 if fires else 1.85)) < 1e-6
        R, t, oinfo = C.iter_oracle(case)
        assert oinfo == (info[0], info[1] + 100 * fires) and info[1] in (0, 1)
        assert np.array_equal(t, case.t_net) == fires
        assert np.abs(rt[3:] - case.t_true).max() < 0.01                      # the LM found the pose from either start


def test_iter_clamp_case_would_show_an_unclamped_count():
    case, img, mdl = C.iter_clamp_case()
    assert img.shape == (C.ITER_CLAMP["rows"], 2) and mdl.shape == (C.ITER_CLAMP["rows"], 3) and np.isfinite(img).all()
    assert C.ITER_CLAMP["stride"] == 64 < C.ITER_CLAMP["count"] == 100 <= C.ITER_CLAMP["rows"] == 128
    assert _iter_precondition(case)[1] in (0, 1)
    R64, t64 = P.net_iter_pnp(img[:64], mdl[:64], C.K32, case.R_net, case.t_net)
    R100, t100 = P.net_iter_pnp(img[:100], mdl[:100], C.K32, case.R_net, case.t_net)
    assert max(np.abs(R64 - R100).max(), np.abs(t64 - t100).max()) > 100 * C.ITER_ATOL


# ------------------------------------------------------------------------------------------------------------ epnp_ransac
def _agrees_with_the_oracle(case, tr, res):
    ok, R, t, mask = res
    assert ok == (tr["best"] is not None)
    if ok:
        assert int(mask.sum()) == tr["counts"][tr["best"]]


def test_ransac_no_model_case():
    case = C.ransac_case("no_model")
    assert len(case.img) == 40 and (case.img >= 0).all() and (case.img[:, 0] <= 640).all() and (case.img[:, 1] <= 480).all()
    tr, res = C.ransac_trace(case), C.ransac_oracle(case)
    _agrees_with_the_oracle(case, tr, res)
    assert not res[0] and not res[3].any() and tr["best"] is None
    assert tr["used"] == case.iters == len(tr["counts"]) and 0 < max(tr["counts"]) <= 3      # models exist, none reaches five inliers


def test_ransac_early_stop_case_cuts_off_a_better_hypothesis():
    case = C.ransac_case("early_stop")
    tr, res = C.ransac_trace(case), C.ransac_oracle(case)
    full_tr, full = C.ransac_trace(case, 1.0), C.ransac_oracle(case, 1.0)
    _agrees_with_the_oracle(case, tr, res)
    _agrees_with_the_oracle(case, full_tr, full)
    assert case.confidence == 0.99 and res[0] and full[0]
    assert full_tr["used"] == case.iters                     # confidence 1.0 (clamped to 1 - tiny) does not cut this run
    assert tr["used"] < 10 and max(tr["counts"][tr["used"]:]) > tr["counts"][tr["best"]]
    assert full_tr["best"] >= tr["used"] and not np.array_equal(res[3], full[3])
    assert tr["margin"] > C.RANSAC_MARGIN


def test_ransac_repeats_case_needs_many_words():
    case = C.ransac_case("repeats")
    tr, res = C.ransac_trace(case), C.ransac_oracle(case)
    _agrees_with_the_oracle(case, tr, res)
    assert len(case.img) == 6 and res[0] and max(tr["words"]) >= 8 and np.mean(tr["words"]) > 6
    assert len(case.words) >= 5 * case.iters and tr["margin"] > C.RANSAC_MARGIN


def test_ransac_short_streams_run_dry():
    case = C.ransac_case("short7")
    tr, res = C.ransac_trace(case), C.ransac_oracle(case)
    _agrees_with_the_oracle(case, tr, res)
    assert len(case.words) == 5 * case.iters == 40                           # as many words as the C ABI asks for
    assert len(tr["counts"]) == 7 and tr["used"] == 7 and tr["niters"] == 8  # the stream, not the confidence, ended the run
    assert res[0] and tr["best"] == 6 and tr["margin"] > C.RANSAC_MARGIN      # the last set made is the winner
    case = C.ransac_case("short0")
    tr, res = C.ransac_trace(case), C.ransac_oracle(case)
    assert len(case.words) == 40 and tr["counts"] == [] and not res[0] and not res[3].any()


def test_get_subset_returns_none_when_the_words_run_out():
    src = C.word_source([3, 9, 3, 3, 4, 1, 7])                  # indices 3 3 3 3 4 1 1: three distinct ones, then nothing
    assert E.get_subset(src, 6, 5) is None
    src = C.word_source([0, 1, 2, 3, 4, 0, 0, 0])
    assert E.get_subset(src, 6, 5) == [0, 1, 2, 3, 4] and E.get_subset(src, 6, 5) is None
