"""-m gpu: the LM and RANSAC pose solvers (csrc/uncertainty_pnp.hip, csrc/epnp_ransac.hip) on every branch they can take, against
the CPU oracles, on the cases of tests/pose_solver_cases.py (whose preconditions tests/test_pose_solver_cases_cpu.py asserts).
The bars are the ones the kernels already carry: uncertainty_pnp_batched — (iterations, code) identical, parameters within 1e-9;
pnp_iter_from_correspondences — R, t within 1e-5, (iterations, code) identical; epnp_ransac — status, inlier mask and count
identical, pose within 1e-4.  Every test prints what it measured before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import pose_solver_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # a copy: the builders' arrays are read-only


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ uncertainty_pnp_batched
_LM_ALONE = {}


def _lm_alone(hip, name):
    """The device's (parameters, (iterations, code)) for one case launched alone; computed once."""
    if name not in _LM_ALONE:
        out, info = hip.uncertainty_pnp_batched(*(T(a) for a in C.lm_batch((name,))), return_info=True)
        _LM_ALONE[name] = (out.cpu().numpy()[0], tuple(int(v) for v in info.cpu().numpy()[0]))
    return _LM_ALONE[name]


@pytest.mark.parametrize("name", C.LM_NAMES)
def test_upnp_case_vs_oracle(hip, name):
    case = C.lm_case(name)
    want, want_info = C.lm_oracle(case)
    got, got_info = _lm_alone(hip, name)
    dev = np.abs(got - want).max()
    print(f"upnp {name}: pn={len(case.p2)} device {got_info} oracle {want_info} max deviation {dev:.3e}")
    assert got_info == want_info
    assert np.isfinite(got).all() and dev <= C.LM_ATOL
    if name in C.LM_START_KEPT:
        assert np.array_equal(_bits(got), _bits(case.init))                   # nothing accepted: the start, bit for bit


def test_upnp_rows_of_one_launch_are_independent(hip):
    """Every 64-point case (iteration counts 0 to 50, all termination codes reached) in one launch: each row equals the same problem
    launched alone, bit for bit — a wave that ends early or late does not disturb its neighbours."""
    names = C.lm_names_with(64)
    out, info = hip.uncertainty_pnp_batched(*(T(a) for a in C.lm_batch(names)), return_info=True)
    out, info = out.cpu().numpy(), info.cpu().numpy()
    alone = [_lm_alone(hip, n) for n in names]
    print("upnp batch of", len(names), "infos", [tuple(r) for r in info.tolist()],
          "rows differing from the single launches:", sum(not np.array_equal(_bits(out[i]), _bits(a[0])) for i, a in enumerate(alone)))
    assert len(names) >= 8 and {0, 50} <= {a[1][0] for a in alone}
    for i, (name, (o, inf)) in enumerate(zip(names, alone)):
        assert tuple(info[i]) == inf, name
        assert np.array_equal(_bits(out[i]), _bits(o)), name


@pytest.mark.parametrize("pn", [1, 65])
def test_upnp_host_symbol_equals_the_batched_row(hip, pn):
    lib = hip.load()
    case = C.lm_case(f"pn{pn}")
    p2, p3, w, K, init = (np.array(case[k]) for k in ("p2", "p3", "w", "K", "init"))     # writable copies for the double* ABI
    res = np.zeros(6)
    vp = ctypes.c_void_p
    lib.uncertainty_pnp(p2.ctypes.data_as(vp), p3.ctypes.data_as(vp), w.ctypes.data_as(vp), K.ctypes.data_as(vp),
                        init.ctypes.data_as(vp), res.ctypes.data_as(vp), pn)
    got, info = _lm_alone(hip, f"pn{pn}")
    print(f"upnp host symbol pn={pn}: batched {info}, max deviation from the batched row {np.abs(res - got).max():.3e}")
    assert np.array_equal(_bits(res), _bits(got))


# ------------------------------------------------------------------------------------------ pnp_iter_from_correspondences
def _iter_launch(hip, cases, stride):
    img, mdl, count, K, R_net, t_net = C.iter_pack(cases, stride)
    R, t, info = hip.pnp_iter_from_correspondences(T(img), T(mdl), T(count), T(K), T(R_net), T(t_net), return_info=True)
    return R.cpu().numpy(), t.cpu().numpy(), [tuple(r) for r in info.cpu().numpy().tolist()]


def _iter_compare(label, case, R, t, info):
    oR, ot, oinfo = C.iter_oracle(case)
    dR, dt = np.abs(R - oR).max(), np.abs(t - ot).max()
    print(f"pnp_iter {label}: n={len(case.img)} device {info} oracle {oinfo} max deviation R {dR:.3e} t {dt:.3e}")
    assert info == oinfo, label
    assert np.isfinite(R).all() and np.isfinite(t).all() and dR <= C.ITER_ATOL and dt <= C.ITER_ATOL, label


def test_pnp_iter_counts_around_the_lane_stride(hip):
    cases = [C.iter_count_case(n) for n in C.ITER_COUNTS]
    R, t, info = _iter_launch(hip, cases, C.ITER_STRIDE)
    for i, (n, case) in enumerate(zip(C.ITER_COUNTS, cases)):
        _iter_compare(f"count {n}", case, R[i], t[i], info[i])
        if n < 4:
            assert np.array_equal(_bits(R[i]), _bits(case.R_net)) and np.array_equal(_bits(t[i]), _bits(case.t_net))


def test_pnp_iter_starts_at_zero_and_pi_rotations(hip):
    names = list(C.ITER_RNET)
    cases = [C.iter_rnet_case(n) for n in names]
    R, t, info = _iter_launch(hip, cases, 64)
    for i, (name, case) in enumerate(zip(names, cases)):
        _iter_compare(f"R_net {name}", case, R[i], t[i], info[i])


def test_pnp_iter_far_fallback(hip):
    cases = [C.iter_far_case("far"), C.iter_far_case("near")]
    R, t, info = _iter_launch(hip, cases, 64)
    for i, (which, case) in enumerate(zip(("far", "near"), cases)):
        _iter_compare(f"fallback {which}", case, R[i], t[i], info[i])
    assert info[0][1] >= 100 and np.array_equal(_bits(t[0]), _bits(cases[0].t_net))     # the network translation, bit for bit ...
    assert np.abs(R[0] - cases[0].R_net).max() > 1e-4                                   # ... with the rotation of the LM
    assert info[1][1] < 100 and np.abs(t[1] - cases[1].t_true).max() < 0.01


def test_pnp_iter_clamps_count_to_stride(hip):
    """C ABI: one problem in buffers of 128 rows, stride 64, count 100 — every row either kernel could read is allocated.  The
    result is the oracle's on the first 64 rows."""
    lib = hip.load()
    case, img, mdl = C.iter_clamp_case()
    d_img, d_mdl = T(img), T(mdl)
    assert d_img.shape[0] == C.ITER_CLAMP["rows"] >= C.ITER_CLAMP["count"]
    count, K, R_net, t_net = T(np.array([C.ITER_CLAMP["count"]], np.int32)), T(case.K), T(case.R_net.reshape(9)), T(case.t_net)
    R = torch.zeros(9, device=DEV)
    t = torch.zeros(3, device=DEV)
    info = torch.zeros(2, dtype=torch.int32, device=DEV)
    rc = lib.gdrnpp_pnp_iter_from_correspondences(d_img.data_ptr(), d_mdl.data_ptr(), count.data_ptr(), C.ITER_CLAMP["stride"],
                                                  K.data_ptr(), R_net.data_ptr(), t_net.data_ptr(), R.data_ptr(), t.data_ptr(),
                                                  info.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    _iter_compare("count 100 > stride 64", case, R.cpu().numpy().reshape(3, 3), t.cpu().numpy(), tuple(info.cpu().numpy().tolist()))


# ------------------------------------------------------------------------------------------------------------ epnp_ransac
def _ransac_compare(hip, name):
    case = C.ransac_case(name)
    n = len(case.img)
    R, t, n_inl, status, mask = hip.epnp_ransac(T(case.img[None]), T(case.mdl[None]), T(np.array([n], np.int32)), T(C.K32.reshape(1, 9)),
                                                iters=case.iters, reproj_err=case.reproj_err, confidence=case.confidence,
                                                draws=T(case.words.astype(np.int32)[None]))
    R, t, n_inl, status, mask = (x.cpu().numpy()[0] for x in (R, t, n_inl, status, mask))
    ok, Ro, to, mo = C.ransac_oracle(case)
    dev = max(np.abs(R - Ro).max(), np.abs(t - to).max())
    print(f"ransac {name}: n={n} device status {status} inliers {n_inl} oracle ok {ok} inliers {int(mo.sum())} mask mismatches "
          f"{int((mask.astype(bool) != mo).sum())} max pose deviation {dev:.3e}")
    assert bool(status) == ok
    assert np.array_equal(mask.astype(bool), mo) and n_inl == mo.sum()
    assert dev <= C.RANSAC_ATOL
    return R, t, n_inl, status, mask


def test_ransac_without_a_model(hip):
    R, t, n_inl, status, mask = _ransac_compare(hip, "no_model")
    assert status == 0 and n_inl == 0 and not mask.any()
    assert np.array_equal(R, np.eye(3, dtype=np.float32)) and not t.any()


def test_ransac_confidence_stop_ignores_later_better_hypotheses(hip):
    R, t, n_inl, status, mask = _ransac_compare(hip, "early_stop")
    tr = C.ransac_trace(C.ransac_case("early_stop"))
    assert status == 1 and n_inl == tr["counts"][tr["best"]] < max(tr["counts"])


def test_ransac_with_repeating_draws(hip):
    assert _ransac_compare(hip, "repeats")[3] == 1


def test_ransac_with_a_short_word_stream(hip):
    assert _ransac_compare(hip, "short7")[3] == 1
    R, t, n_inl, status, mask = _ransac_compare(hip, "short0")
    assert status == 0 and n_inl == 0 and not mask.any() and np.array_equal(R, np.eye(3, dtype=np.float32)) and not t.any()
