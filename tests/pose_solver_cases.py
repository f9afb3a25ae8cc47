"""Case builders for the pose solvers on the branches they can take, shared by tests/test_gpu_pose_solver_edges.py (HIP kernels
against the CPU oracles) and tests/test_pose_solver_cases_cpu.py (the preconditions that make each case prove something).  Plain
helper module: no fixtures; builders are cached and their arrays are read-only.  Every seed below was picked by search
(``PYTHONPATH=. python tests/pose_solver_cases.py`` prints the candidates) and is frozen; the CPU test fails when one of them is replaced by a
case the oracle itself is not sure about.

Internal boundaries the cases are placed on:

    evaluate()            64 lanes stride over the correspondences, then a 6-step butterfly: counts 1, 3, 4, 5, 63, 64, 65, 127,
                          128, 129, 700 (fewer points than lanes, one full pass, one point in the next pass, eleven passes)
    lm_minimise           termination 0 (parameter), 1 (function), 2 (gradient: at entry with noise-free data, with all-zero
                          weights, with a non-finite cost), 3 (50 iterations), 5 (five invalid steps in a row); runs of 15 to 50
                          iterations in which steps are rejected, the radius shrinks and the LM diagonal is reused.  Termination 4
                          (radius below 1e-32) needs about 15 rejected steps in a row without the function tolerance firing; it
                          was not reached in a search over thousands of draws, and no input is contorted for it: code 4 stays
                          untested.
    rotation_and_derivs   theta^2 <= 2^-52: start rotation exactly zero (the first evaluation is first-order, the rest general);
                          optimum at 1e-9 rad, started 0.1 mm away with zero rotation (every evaluation of the run is first-order),
                          and the same at 1.2e-8 rad, the far end of the branch: there the rotation the run has to find exceeds
                          the 1e-9 bar, so a wrong first-order Jacobian cannot hide; |rotation| = pi
    weights               off-diagonal terms, the same scaled by 1e6, all zero, 1e160 (J^T J overflows)
    non-finite data       a NaN and a +Inf image point: cost -> DBL_MAX, gradient NaN -> fmax(0, NaN) = 0 -> termination 2
    rodrigues_log         s < 1e-5 with c > 0 (identity) and c <= 0 (pi about x, y, z and four oblique axes: each sign test of
                          ry, rz and the rz flip fires in one and not in another)
    pnp_iter_kernel       count < 4 keeps the network pose, count > stride is clamped, |t - t_net| > 1 m keeps t_net (info + 100)
    epnp_ransac           no hypothesis with 5 inliers; the confidence stop cutting off a better hypothesis; minimal sets that
                          need many words (6 points); a word stream that runs dry after 7 sets and before the first one

A case of the LM kernels is only usable if the oracle's own answer does not depend on what the device does differently (lane-strided
partial sums and a butterfly instead of a serial sum; an analytic Jacobian instead of jets): ``lm_robustness`` reruns the oracle on
permuted correspondences and on image points moved by a relative 2^-50 and reports whether (iterations, code) stayed the same and how
far the parameters moved.
"""
from functools import lru_cache

import numpy as np

from oracle import epnp as E
from oracle import postproc as P

K64 = np.array([[1066.778, 0.0, 312.9869], [0.0, 1067.487, 241.3109], [0.0, 0.0, 1.0]], np.float32).astype(np.float64)   # YCB-V
K32 = K64.astype(np.float32)
IDENTITY_W = (1.0, 0.0, 1.0)
ROBUST_PERMUTATIONS = 8
ROBUST_JITTERS = 4
ROBUST_TOL = 1e-10          # a tenth of the device bar
LM_ATOL = 1e-9              # test_upnp_batched_vs_oracle's bar
ITER_ATOL = 1e-5            # test_net_iter_pnp_from_correspondences' bar
RANSAC_ATOL = 1e-4          # test_ransac_matches_oracle_with_identical_draws' bar


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def project(p3, rt, K=K64):
    cam = np.asarray(p3, np.float64) @ P.rodrigues_exp(rt[:3]).T + rt[3:]
    return cam[:, :2] / cam[:, 2:] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]


def random_pose(rng, angle=None):
    """Rotation vector with a uniform axis and an angle in [0.2, 2.8] (or ``angle``), translation in the YCB-V working volume."""
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.2, 2.8) if angle is None else angle
    t = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), rng.uniform(0.4, 1.4)])
    return np.concatenate([axis * ang, t])


# ------------------------------------------------------------------------------------------------ uncertainty_pnp_batched
class LmCase(dict):
    """p2 f64[pn,2], p3 f64[pn,3], w f64[pn,3], K f64[9], init f64[6], truth f64[6]"""
    __getattr__ = dict.__getitem__


def _lm_case(p2, p3, w, init, truth):
    return LmCase(p2=_frozen(np.ascontiguousarray(p2, np.float64)), p3=_frozen(np.ascontiguousarray(p3, np.float64)),
                  w=_frozen(np.ascontiguousarray(w, np.float64)), K=_frozen(K64.reshape(9).copy()),
                  init=_frozen(np.ascontiguousarray(init, np.float64)), truth=_frozen(np.ascontiguousarray(truth, np.float64)))


def lm_problem(seed, pn, noise=0.5, start_sigma=0.03, truth_rot=None, start_rot=None, rot_offset=0.0, weights=IDENTITY_W):
    """Model points in +-0.1 m, a pose in the working volume, image points with ``noise`` pixels of Gaussian noise, start =
    truth + N(0, start_sigma) (rotation moved by a further ``rot_offset`` rad about a random axis).  ``truth_rot`` / ``start_rot``
    replace the rotation vectors."""
    rng = np.random.default_rng([77, seed, pn])
    p3 = rng.uniform(-0.1, 0.1, (pn, 3))
    truth = random_pose(rng)
    if truth_rot is not None:
        truth[:3] = truth_rot
    p2 = project(p3, truth) + rng.normal(0, noise, (pn, 2)) * (noise > 0)
    init = truth + rng.normal(0, start_sigma, 6)
    off = rng.standard_normal(3)
    init[:3] += rot_offset * off / np.linalg.norm(off)
    if start_rot is not None:
        init[:3] = start_rot
    w = np.tile(np.asarray(weights, np.float64), (pn, 1))
    return _lm_case(p2, p3, w, init, truth)


def lm_oracle(case):
    out, info = P.uncertainty_pnp(case.p2, case.p3, case.w, case.K, case.init, return_info=True)
    return out, (int(info[0]), int(info[1]))


def lm_robustness(case):
    """-> (infos, moved): the set of (iterations, code) the oracle returns over the case itself, ROBUST_PERMUTATIONS random orders of
    its correspondences and ROBUST_JITTERS copies whose image points are moved by a relative 2^-50, and the largest change of a
    parameter among them (NaN counts as infinite)."""
    base, info = lm_oracle(case)
    infos, moved = {info}, 0.0
    rng = np.random.default_rng(2024)
    pn = len(case.p2)
    for k in range(ROBUST_PERMUTATIONS + ROBUST_JITTERS):
        if k < ROBUST_PERMUTATIONS:
            o = rng.permutation(pn)
            p2, p3, w = case.p2[o], case.p3[o], case.w[o]
        else:
            p2, p3, w = case.p2 * (1.0 + 2.0 ** -50 * rng.choice([-1.0, 1.0], case.p2.shape)), case.p3, case.w
        out, inf = P.uncertainty_pnp(p2, p3, w, case.K, case.init, return_info=True)
        infos.add((int(inf[0]), int(inf[1])))
        d = np.abs(out - base).max()
        moved = max(moved, d if np.isfinite(d) else np.inf)
    return infos, moved


def lm_is_robust(case):
    infos, moved = lm_robustness(case)
    return len(infos) == 1 and moved <= ROBUST_TOL


def _chol_solve6(A, b):
    L = np.zeros((6, 6))
    for i in range(6):
        for j in range(i + 1):
            s = A[i, j]
            for k in range(j):
                s -= L[i, k] * L[j, k]
            if i == j:
                if not s > 0.0:
                    return None
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    z, y = np.zeros(6), np.zeros(6)
    for i in range(6):
        s = b[i]
        for k in range(i):
            s -= L[i, k] * z[k]
        z[i] = s / L[i, i]
    for i in range(5, -1, -1):
        s = z[i]
        for k in range(i + 1, 6):
            s -= L[k, i] * y[k]
        y[i] = s / L[i, i]
    return y if np.isfinite(y).all() else None


def lm_trace(case):
    """The schedule of oracle/upnp_oracle.c walked in NumPy over the oracle's own residuals and Jacobians, to see what a run is made of
    -> dict(info, accepted, rejected, invalid, reused_diag: iterations entered with the LM diagonal of the one before, first_order /
    general: evaluations in either rotation branch, failed_evals: evaluations with a non-finite cost).  Not a reference: the CPU test
    requires its (iterations, code) to be the oracle's."""
    pn = len(case.p2)
    n = dict(accepted=0, rejected=0, invalid=0, reused_diag=0, first_order=0, general=0, failed_evals=0)

    def evaluate(x):
        n["general" if x[0] * x[0] + x[1] * x[1] + x[2] * x[2] > 2.220446049250313e-16 else "first_order"] += 1
        H, g, cost = np.zeros((6, 6)), np.zeros(6), 0.0
        for i in range(pn):
            r, J = P.upnp_residual(x, case.p2[i], case.p3[i], case.w[i], case.K)
            cost += r[0] * r[0] + r[1] * r[1]
            g += J[0] * r[0] + J[1] * r[1]
            H += np.outer(J[0], J[0]) + np.outer(J[1], J[1])
        cost *= 0.5
        if not np.isfinite(cost):
            n["failed_evals"] += 1
            cost = np.finfo(np.float64).max
        return cost, H, g

    with np.errstate(all="ignore"):
        x = case.init.copy()
        radius, decrease, invalid, it, term, reuse = 1e4, 2.0, 0, 0, 3, False
        cost, H, g = evaluate(x)
        scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))
        gmax = np.fmax.reduce(np.abs(g), initial=0.0)
        diag = np.zeros(6)
        while True:
            if it >= 50:
                term = 3
                break
            if gmax <= 1e-10:
                term = 2
                break
            if radius < 1e-32:
                term = 4
                break
            it += 1
            n["reused_diag"] += int(reuse)
            Hs, gs = scale[:, None] * H * scale[None, :], scale * g
            if not reuse:
                diag = np.fmin(np.fmax(np.diag(Hs), 1e-6), 1e32)
            reuse = True
            y = _chol_solve6(Hs + np.diag(diag / radius), gs)
            change = 0.0
            if y is not None:
                step = -y
                sg = sum(step[a] * gs[a] for a in range(6))
                sHs = sum(step[a] * sum(Hs[a, b] * step[b] for b in range(6)) for a in range(6))
                change = -sg - 0.5 * sHs
            if y is None or not change > 0.0:
                n["invalid"] += 1
                invalid += 1
                if invalid >= 5:
                    term = 5
                    break
                radius *= 0.5
                reuse = False
                continue
            invalid = 0
            cand = x + step * scale
            delta, xn = np.sqrt(sum((x - cand) ** 2)), np.sqrt(sum(x * x))
            ccost, Hc, gc = evaluate(cand)
            if delta <= 1e-8 * (xn + 1e-8):
                term = 0
                break
            if abs(cost - ccost) <= 1e-6 * cost:
                term = 1
                break
            rel = (cost - ccost) / change
            if rel > 1e-3:
                n["accepted"] += 1
                x, H, g, cost = cand, Hc, gc, ccost
                gmax = np.fmax.reduce(np.abs(g), initial=0.0)
                t = 2.0 * rel - 1.0
                radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - t * t * t))
                decrease, reuse = 2.0, False
            else:
                n["rejected"] += 1
                radius /= decrease
                decrease *= 2.0
                reuse = True
    n["info"] = (it, term)
    return n


LM_COUNTS = (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 700)
LM_COUNT_SEEDS = {pn: 0 for pn in LM_COUNTS}

# name -> builder keywords.  The long runs start with the rotation 2 to 2.5 rad off (in front of the camera all the same: a start
# behind it makes the oracle itself chaotic).  "code2_entry" carries weights of 0.01 (a standard deviation of 100 pixels): with unit
# weights a last-bit change of an image point already lifts the gradient of a noise-free problem above 1e-10.
LM_SPECS = {
    "code0":         dict(seed=1, pn=64),
    "code1":         dict(seed=0, pn=64),
    "code2_entry":   dict(seed=0, pn=64, noise=0.0, start_sigma=0.0, weights=(0.01, 0.0, 0.01)),
    "code3":         dict(seed=164, pn=5, rot_offset=2.0),
    "code3_pn64":    dict(seed=20, pn=64, rot_offset=2.5),
    "code5":         dict(seed=0, pn=64, weights=(1e160, 0.0, 1e160)),
    "long15_code0":  dict(seed=1, pn=64, rot_offset=2.5),
    "long30_code0":  dict(seed=144, pn=6, rot_offset=2.5),
    "long15_code1":  dict(seed=28, pn=64, rot_offset=2.5),
    "long30_code1":  dict(seed=73, pn=64, rot_offset=2.5),
    "it50_code1":    dict(seed=88, pn=5, rot_offset=2.0),
    "start_rot0":    dict(seed=0, pn=64, truth_rot=(0.04, -0.03, 0.05), start_rot=(0.0, 0.0, 0.0)),
    "truth_rot1e-9": dict(seed=0, pn=64, noise=0.0, truth_rot=(6e-10, -5e-10, 6e-10), start_rot=(0.0, 0.0, 0.0), start_sigma=1e-4),
    "truth_rot1e-8": dict(seed=0, pn=64, noise=0.0, truth_rot=(7e-9, -6e-9, 7e-9), start_rot=(0.0, 0.0, 0.0), start_sigma=1e-4),
    "truth_rot_pi":  dict(seed=0, pn=64, truth_rot=(np.pi, 0.0, 0.0)),
    "zero_weights":  dict(seed=0, pn=64, weights=(0.0, 0.0, 0.0)),
}
# what the oracle must return: an exact (iterations, code), (at least so many iterations, code), a code, or convergence (0 or 1)
LM_EXPECT = {
    "code0": ("code", 0), "code1": ("code", 1), "code2_entry": ("exact", (0, 2)), "code3": ("exact", (50, 3)),
    "code3_pn64": ("exact", (50, 3)), "code5": ("exact", (5, 5)), "long15_code0": ("min", (15, 0)), "long30_code0": ("min", (30, 0)),
    "long15_code1": ("min", (15, 1)), "long30_code1": ("min", (30, 1)), "it50_code1": ("exact", (50, 1)),
    "start_rot0": ("converged", None), "truth_rot1e-9": ("converged", None), "truth_rot1e-8": ("converged", None),
    "truth_rot_pi": ("converged", None), "zero_weights": ("exact", (0, 2)), "aniso": ("converged", None), "aniso_1e6": ("converged", None), "nonfinite": ("exact", (0, 2)),
}
LM_REJECTING = ("code3", "code3_pn64", "long15_code0", "long30_code0", "long15_code1", "long30_code1", "it50_code1")
LM_START_KEPT = ("code5", "zero_weights", "nonfinite")        # the result is the start, bit for bit
ANISO_SEED = 0
NONFINITE_SEED = 0
NONFINITE_ROWS = (37, 150)        # NaN, +Inf: lane 37 of pass 0, lane 22 of pass 2


def lm_expectation_holds(name, info):
    kind, want = LM_EXPECT.get(name, ("converged", None))
    if kind == "exact":
        return info == want
    if kind == "min":
        return info[0] >= want[0] and info[1] == want[1]
    if kind == "code":
        return info[1] == want
    return info[1] in (0, 1)


def _aniso_weights(rng, pn):
    """W = sqrt of a random 2 x 2 information matrix: wxx, wyy in [0.3, 2], |wxy| up to 0.6 of their geometric mean."""
    wxx, wyy = rng.uniform(0.3, 2.0, pn), rng.uniform(0.3, 2.0, pn)
    wxy = rng.uniform(-0.6, 0.6, pn) * np.sqrt(wxx * wyy)
    return np.stack([wxx, wxy, wyy], 1)


@lru_cache(maxsize=None)
def lm_case(name):
    if name.startswith("pn"):
        pn = int(name[2:])
        return lm_problem(LM_COUNT_SEEDS[pn], pn)
    if name in ("aniso", "aniso_1e6"):
        c = lm_problem(ANISO_SEED, 9)
        w = _aniso_weights(np.random.default_rng([78, ANISO_SEED]), 9) * (1e6 if name == "aniso_1e6" else 1.0)
        return _lm_case(c.p2, c.p3, w, c.init, c.truth)
    if name == "nonfinite":
        c = lm_problem(NONFINITE_SEED, 200)
        p2 = c.p2.copy()
        p2[NONFINITE_ROWS[0], 0] = np.nan
        p2[NONFINITE_ROWS[1], 1] = np.inf
        return _lm_case(p2, c.p3, c.w, c.init, c.truth)
    return lm_problem(**LM_SPECS[name])


LM_COUNT_NAMES = tuple(f"pn{pn}" for pn in LM_COUNTS)
LM_NAMES = LM_COUNT_NAMES + tuple(LM_SPECS) + ("aniso", "aniso_1e6", "nonfinite")


def lm_names_with(pn):
    return tuple(n for n in LM_NAMES if len(lm_case(n).p2) == pn)


def lm_batch(names):
    """-> (P2, P3, W, Kb, inits) stacked over ``names`` (all of one point count)."""
    cs = [lm_case(n) for n in names]
    return tuple(np.stack([c[k] for c in cs]) for k in ("p2", "p3", "w", "K", "init"))


# ------------------------------------------------------------------------------------------ pnp_iter_from_correspondences
class IterCase(dict):
    """img f32[n,2], mdl f32[n,3], K f32[9], R_net f32[3,3], t_net f32[3], t_true f64[3]"""
    __getattr__ = dict.__getitem__


def iter_problem(seed, n, R_net=None, noise=0.5):
    """Truth pose -> float32 correspondences with ``noise`` pixels; the network pose is the truth turned by 0.03 rad and moved by
    1 cm.  With ``R_net`` given the truth rotation is R_net turned by 0.03 rad instead."""
    rng = np.random.default_rng([79, seed, n])
    truth = random_pose(rng)
    dR = P.rodrigues_exp(rng.normal(0, 0.03, 3))
    if R_net is None:
        R_true = P.rodrigues_exp(truth[:3])
        R_net = (R_true @ dR).astype(np.float32)
    else:
        R_net = np.asarray(R_net, np.float32)
        R_true = R_net.astype(np.float64) @ dR
    mdl = rng.uniform(-0.1, 0.1, (max(n, 1), 3)).astype(np.float32)[:n]
    cam = mdl.astype(np.float64) @ R_true.T + truth[3:]
    uv = cam[:, :2] / cam[:, 2:] * [K64[0, 0], K64[1, 1]] + [K64[0, 2], K64[1, 2]]
    img = (uv + rng.normal(0, noise, uv.shape)).astype(np.float32)
    t_net = (truth[3:] + rng.normal(0, 0.01, 3)).astype(np.float32)
    return IterCase(img=_frozen(img), mdl=_frozen(mdl), K=_frozen(K32.reshape(9).copy()), R_net=_frozen(np.ascontiguousarray(R_net)),
                    t_net=_frozen(t_net), t_true=_frozen(truth[3:].copy()))


def iter_as_lm(case):
    """The LM problem the oracle solves for this case (identity weights, start = rodrigues_log(R_net), t_net)."""
    n = len(case.img)
    init = np.concatenate([P.rodrigues_log(case.R_net), case.t_net.astype(np.float64)])
    c = _lm_case(case.img.astype(np.float64), case.mdl.astype(np.float64), np.tile(IDENTITY_W, (n, 1)), init, init)
    c["K"] = _frozen(case.K.astype(np.float64))
    return c


def iter_oracle(case):
    """-> (R f32[3,3], t f32[3], (iterations, code)); code + 100 when the far fallback fires, (0, -1) below four points."""
    R, t = P.net_iter_pnp(case.img, case.mdl, case.K.reshape(3, 3), case.R_net, case.t_net)
    if len(case.img) < 4:
        return R, t, (0, -1)
    rt, (it, code) = lm_oracle(iter_as_lm(case))
    far = np.linalg.norm(rt[3:] - case.t_net.astype(np.float64)) > 1
    return R, t, (it, code + 100 * int(far))


ITER_STRIDE = 256
ITER_COUNTS = (0, 3, 4, 5, 63, 64, 65, 129, 256)
ITER_COUNT_SEEDS = {n: 0 for n in ITER_COUNTS}


@lru_cache(maxsize=None)
def iter_count_case(n):
    return iter_problem(ITER_COUNT_SEEDS[n], n)


def iter_pack(cases, stride):
    """-> (img f32[b,stride,2], mdl f32[b,stride,3], count i32[b], K f32[b,9], R_net f32[b,9], t_net f32[b,3]); rows at and beyond
    each count are NaN."""
    b = len(cases)
    img = np.full((b, stride, 2), np.nan, np.float32)
    mdl = np.full((b, stride, 3), np.nan, np.float32)
    for i, c in enumerate(cases):
        img[i, :len(c.img)], mdl[i, :len(c.mdl)] = c.img, c.mdl
    return (img, mdl, np.array([len(c.img) for c in cases], np.int32), np.stack([c.K for c in cases]),
            np.stack([c.R_net.reshape(9) for c in cases]), np.stack([c.t_net for c in cases]))


def _pi_about(axis):
    u = np.asarray(axis, np.float64)
    u = u / np.linalg.norm(u)
    return (2.0 * np.outer(u, u) - np.eye(3)).astype(np.float32)


# name -> float32 matrix.  The first seven are the ones the issue lists; "pi_0_1_-1" is added because it is the one in which the rz
# flip fires (rx = 0 leaves the signs of ry and rz to R[1] = R[2] = 0, and R[5] < 0 contradicts them).
ITER_RNET = {
    "identity": np.eye(3, dtype=np.float32),
    "pi_x": _pi_about((1, 0, 0)), "pi_y": _pi_about((0, 1, 0)), "pi_z": _pi_about((0, 0, 1)),
    "pi_1_1_0": _pi_about((1, 1, 0)), "pi_-1_1_1": _pi_about((-1, 1, 1)), "pi_0.2_-1_-1": _pi_about((0.2, -1, -1)),
    "pi_0_1_-1": _pi_about((0, 1, -1)),
}
ITER_RNET_OBLIQUE = ("pi_1_1_0", "pi_-1_1_1", "pi_0.2_-1_-1", "pi_0_1_-1")
ITER_RNET_SEEDS = {name: 0 for name in ITER_RNET}


def rodrigues_log_path(R):
    """The decisions rodrigues_log takes on R -> (s < 1e-5, c > 0, R[1] < 0, R[2] < 0, rx strictly smallest, rz flipped)."""
    R = np.asarray(R, np.float64).reshape(9)
    rx, ry, rz = R[7] - R[5], R[2] - R[6], R[3] - R[1]
    s = np.sqrt((rx * rx + ry * ry + rz * rz) * 0.25)
    c = min(max((R[0] + R[4] + R[8] - 1) * 0.5, -1.0), 1.0)
    if not s < 1e-5 or c > 0:
        return (bool(s < 1e-5), bool(c > 0), False, False, False, False)
    rx = np.sqrt(max((R[0] + 1) * 0.5, 0.0))
    ry = np.sqrt(max((R[4] + 1) * 0.5, 0.0)) * (-1.0 if R[1] < 0 else 1.0)
    rz = np.sqrt(max((R[8] + 1) * 0.5, 0.0)) * (-1.0 if R[2] < 0 else 1.0)
    smallest = abs(rx) < abs(ry) and abs(rx) < abs(rz)
    return (True, False, bool(R[1] < 0), bool(R[2] < 0), bool(smallest), bool(smallest and (R[5] > 0) != (ry * rz > 0)))


@lru_cache(maxsize=None)
def iter_rnet_case(name):
    return iter_problem(ITER_RNET_SEEDS[name], 64, R_net=ITER_RNET[name])


ITER_FAR_SEED = 0
ITER_FAR_OFFSETS = {"far": 1.6, "near": 0.95}       # t_net z = 2.5 and 1.85 with the truth at z = 0.9


@lru_cache(maxsize=None)
def iter_far_case(which):
    c = iter_problem(ITER_FAR_SEED, 64)
    t_true = np.array([c.t_true[0], c.t_true[1], 0.9])
    R_true = c.R_net.astype(np.float64)
    cam = c.mdl.astype(np.float64) @ R_true.T + t_true
    uv = cam[:, :2] / cam[:, 2:] * [K64[0, 0], K64[1, 1]] + [K64[0, 2], K64[1, 2]]
    rng = np.random.default_rng([80, ITER_FAR_SEED])
    img = (uv + rng.normal(0, 0.5, uv.shape)).astype(np.float32)
    t_net = (t_true + [0.0, 0.0, ITER_FAR_OFFSETS[which]]).astype(np.float32)
    return IterCase(img=_frozen(img), mdl=c.mdl, K=c.K, R_net=c.R_net, t_net=_frozen(t_net), t_true=_frozen(t_true))


ITER_CLAMP = dict(rows=128, stride=64, count=100)
ITER_CLAMP_SEED = 0


@lru_cache(maxsize=None)
def iter_clamp_case():
    """-> (case on the first 64 rows, img f32[128,2], mdl f32[128,3]): rows 64..127 are correspondences of the same model under a pose
    5 cm and 0.3 rad away, so a kernel that believed count = 100 would land somewhere else."""
    c = iter_problem(ITER_CLAMP_SEED, 64)
    rng = np.random.default_rng([81, ITER_CLAMP_SEED])
    mdl2 = rng.uniform(-0.1, 0.1, (64, 3)).astype(np.float32)
    other = np.concatenate([P.rodrigues_log(c.R_net) + [0.3, 0.0, 0.0], c.t_true + [0.05, 0.0, 0.0]])
    img2 = project(mdl2, other).astype(np.float32)
    return c, _frozen(np.concatenate([c.img, img2])), _frozen(np.concatenate([c.mdl, mdl2]))


# ------------------------------------------------------------------------------------------------------------ epnp_ransac
class RansacCase(dict):
    """img f32[n,2], mdl f32[n,3], words u32[n_words], iters, reproj_err, confidence"""
    __getattr__ = dict.__getitem__


def ransac_points(rng, n, noise, outliers):
    """test_gpu_epnp's ``_problem``: a pose in the working volume, ``noise`` pixels, a fraction of gross outliers."""
    truth = random_pose(rng)
    mdl = rng.uniform(-0.1, 0.1, (n, 3)).astype(np.float32)
    uv = project(mdl, truth) + rng.normal(0, noise, (n, 2)) * (noise > 0)
    bad = rng.uniform(0, 1, n) < outliers
    uv[bad] += rng.uniform(20, 100, (int(bad.sum()), 2))
    return mdl, uv.astype(np.float32), bad


def word_source(words):
    """The oracle's ``rng_next`` over a finite stream; running dry raises StopIteration, which ``get_subset`` turns into None."""
    it = iter(np.asarray(words).astype(np.uint32).tolist())
    return lambda: next(it)


def ransac_oracle(case, confidence=None):
    return E.solve_pnp_ransac_epnp(case.mdl, case.img, K64, case.reproj_err, case.iters,
                                   case.confidence if confidence is None else confidence, rng_next=word_source(case.words))


def ransac_trace(case, confidence=None):
    """Replays RANSACPointSetRegistrator::run with the oracle's own pieces -> dict(counts: inliers of every hypothesis made (-1: no
    model), used: hypotheses the loop looked at, best: index of the winner or None, words: words each minimal set took, margin:
    the smallest |err^2 - thr^2| over the hypotheses looked at)."""
    conf = case.confidence if confidence is None else confidence
    n = len(case.img)
    thr2 = np.float32(case.reproj_err) * np.float32(case.reproj_err)
    taken = [0]

    def nxt(src=word_source(case.words)):
        taken[0] += 1
        return src()

    counts, errs, words = [], [], []
    while len(counts) < case.iters:                     # every minimal set the stream can fill, like subsets_kernel
        before = taken[0]
        idx = E.get_subset(nxt, n, 5)
        if idx is None:
            break
        words.append(taken[0] - before)
        sol = E.epnp(case.mdl[idx], case.img[idx], K64)
        e2 = None if sol is None else E.reproj_err2_f32(case.mdl, case.img, K64, sol[0], sol[1])
        errs.append(e2)
        counts.append(-1 if e2 is None else int((e2 <= thr2).sum()))
    best, best_count, niters, it, margin = None, 0, case.iters, 0, np.inf
    while it < niters and it < len(counts):             # the sequential part, like final_kernel
        if errs[it] is not None:
            margin = min(margin, float(np.abs(errs[it].astype(np.float64) - float(thr2)).min()))
        if counts[it] > max(best_count, 4):
            best, best_count = it, counts[it]
            niters = E.update_num_iters(conf, (n - counts[it]) / n, 5, niters)
        it += 1
    return dict(counts=counts, used=it, best=best, words=words, margin=margin, niters=niters)


RANSAC_SEEDS = {"no_model": 8, "early_stop": 1, "repeats": 0, "short7": 1}
RANSAC_MARGIN = 0.02        # px^2: no squared error a compared run looks at lies this close to the threshold (poses agree to ~1e-6,
                            # about 1e-3 pixels at these depths, 6e-3 px^2 at the 3-pixel threshold)


def _ransac_case(mdl, img, words, iters, confidence=0.99):
    return RansacCase(mdl=_frozen(mdl), img=_frozen(img), words=_frozen(np.asarray(words, np.uint32)), iters=iters, reproj_err=3.0,
                      confidence=confidence)


@lru_cache(maxsize=None)
def ransac_case(name):
    rng = np.random.default_rng([82, RANSAC_SEEDS.get(name, 0), sorted(RANSAC_BUILDERS).index(name)])
    return RANSAC_BUILDERS[name](rng)


def _no_model(rng):
    """40 model points against image points uniform over the 640 x 480 image: nothing to find."""
    mdl = rng.uniform(-0.1, 0.1, (40, 3)).astype(np.float32)
    img = np.stack([rng.uniform(0, 640, 40), rng.uniform(0, 480, 40)], 1).astype(np.float32)
    return _ransac_case(mdl, img, rng.integers(0, 2 ** 31 - 1, 40 * 8), 40)


def _early_stop(rng):
    """60 points, 1.2 pixels of noise, no gross outliers: hypotheses gather between half and all of the points, so the first good one
    pulls the iteration limit down to a handful while better ones follow."""
    mdl, img, _ = ransac_points(rng, 60, 1.2, 0.0)
    return _ransac_case(mdl, img, rng.integers(0, 2 ** 31 - 1, 100 * 8), 100)


def _repeats(rng):
    """6 points: a word repeats an index already chosen with probability up to 4/6."""
    mdl, img, _ = ransac_points(rng, 6, 0.3, 0.0)
    return _ransac_case(mdl, img, rng.integers(0, 2 ** 31 - 1, 30 * 16), 30)


def _short_words(rng, n, sets):
    """``sets`` minimal sets of distinct indices (5 words each), then the same index until the stream of 8 * 5 words ends."""
    words = [int(i) + n * int(k) for _ in range(sets) for i, k in zip(rng.permutation(n)[:5], rng.integers(0, 1000, 5))]
    return words + [7 + n * 3] * (40 - len(words))


def _short7(rng):
    """40 points with 30 % outliers, 8 iterations asked for, words for 7 minimal sets."""
    mdl, img, _ = ransac_points(rng, 40, 0.4, 0.3)
    return _ransac_case(mdl, img, _short_words(rng, 40, 7), 8)


def _short0(rng):
    mdl, img, _ = ransac_points(rng, 40, 0.4, 0.3)
    return _ransac_case(mdl, img, _short_words(rng, 40, 0), 8)


RANSAC_BUILDERS = {"no_model": _no_model, "early_stop": _early_stop, "repeats": _repeats, "short7": _short7, "short0": _short0}


# ----------------------------------------------------------------------------------------------------------------- search
def _search():
    """Prints, for every frozen seed, the first candidates that satisfy the case's preconditions."""
    def first(make, ok, seeds=range(400), want=3):
        found = []
        for s in seeds:
            c = make(s)
            r = ok(c)
            if r:
                found.append((s, r))
                if len(found) == want:
                    break
        return found

    for pn in LM_COUNTS:
        print("pn", pn, first(lambda s: lm_problem(s, pn), lambda c: lm_is_robust(c) and lm_oracle(c)[1], want=1))
    for name, spec in LM_SPECS.items():
        kw = {k: v for k, v in spec.items() if k != "seed"}
        print(name, first(lambda s: lm_problem(s, **kw),
                          lambda c: lm_expectation_holds(name, lm_oracle(c)[1]) and lm_is_robust(c) and lm_oracle(c)[1], seeds=range(3000)))
    g = globals()

    def with_seed(var, key, s, build, *args):
        old = g[var] if key is None else g[var][key]
        if key is None:
            g[var] = s
        else:
            g[var][key] = s
        build.cache_clear()
        try:
            return build(*args)
        finally:
            if key is None:
                g[var] = old
            else:
                g[var][key] = old
            build.cache_clear()

    def lm_ok(name):
        return lambda c: lm_expectation_holds(name, lm_oracle(c)[1]) and lm_is_robust(c) and lm_oracle(c)[1]

    for name in ("aniso", "aniso_1e6"):
        print(name, first(lambda s: with_seed("ANISO_SEED", None, s, lm_case, name), lm_ok(name)))
    print("nonfinite", first(lambda s: with_seed("NONFINITE_SEED", None, s, lm_case, "nonfinite"), lm_ok("nonfinite")))

    def iter_ok(c):
        return len(c.img) < 4 or (lm_is_robust(iter_as_lm(c)) and iter_oracle(c)[2])

    for cnt in ITER_COUNTS:
        print("iter count", cnt, first(lambda s: with_seed("ITER_COUNT_SEEDS", cnt, s, iter_count_case, cnt), iter_ok, want=1))
    for name in ITER_RNET:
        print("iter R_net", name, first(lambda s: with_seed("ITER_RNET_SEEDS", name, s, iter_rnet_case, name), iter_ok, want=1))

    def far_ok(s):
        res = []
        for which in ITER_FAR_OFFSETS:
            c = with_seed("ITER_FAR_SEED", None, s, iter_far_case, which)
            if not lm_is_robust(iter_as_lm(c)):
                return False
            rt, info = lm_oracle(iter_as_lm(c))
            res.append((info, round(float(np.linalg.norm(rt[3:] - c.t_net.astype(np.float64))), 3)))
        return res if res[0][1] > 1.01 and res[1][1] < 0.99 and res[0][0][1] in (0, 1) and res[1][0][1] in (0, 1) else False

    print("iter far", [(s, far_ok(s)) for s in range(40) if far_ok(s)][:3])
    print("iter clamp", first(lambda s: with_seed("ITER_CLAMP_SEED", None, s, iter_clamp_case), lambda c: iter_ok(c[0]), want=1))

    def ransac_ok(name):
        def ok(c):
            tr = ransac_trace(c)
            res = ransac_oracle(c)
            if name == "no_model":
                return not res[0] and tr["best"] is None and max(tr["counts"]) <= 3 and max(tr["counts"])
            if name == "early_stop":
                full = ransac_oracle(c, 1.0)
                return (res[0] and full[0] and not np.array_equal(res[3], full[3]) and tr["margin"] > 0.05
                        and (tr["used"], tr["counts"][tr["best"]], max(tr["counts"]), tr["margin"]))
            if name == "repeats":
                return res[0] and max(tr["words"]) >= 8 and tr["margin"] > 0.05 and (tr["used"], max(tr["words"]))
            return res[0] and tr["used"] == 7 and tr["niters"] > 7 and tr["margin"] > 0.05 and (tr["counts"], tr["niters"])
        return ok

    for name in RANSAC_SEEDS:
        print("ransac", name, first(lambda s: with_seed("RANSAC_SEEDS", name, s, ransac_case, name), ransac_ok(name), want=2))
    for name in LM_REJECTING:
        print(name, lm_trace(lm_case(name)))


if __name__ == "__main__":
    _search()
