"""The multi-tensor Ranger kernel (csrc/ranger.hip through ``solver.Ranger``) on the GPU against tests/ranger_ref.py in fp64, with the bars
of tests/golden/ranger_golden.npz: per tensor and quantity twice the reference's own fp32 error plus one fp32 unit in the last place of the
tensor's largest value.  The kernel may differ from the reference's fp32 run only in the order of the row mean (fp64 here) and in
contraction (none here).

Measured on an MI355X, worst error over bar per quantity (p, m, v, slow) over every variant, step and tensor (the tests print them, ``-s``):
    single step from the reference's state, kernel            0.49  0.56  0.60  0.49
    single step from the reference's state, torch operators   0.32  0.68  0.77  0.32
    13-step trajectory at steps 5, 6, 12, 13, kernel          0.58  0.65  0.60  0.58
    shapes at the tile and item limits, kernel                0.33  0.34  0.38  0.33
The factor 2 is not needed anywhere: every figure is below 1 with the bar as stated, none needed more.

``step()`` issues no host synchronisation: checked by running it under ``torch.cuda.set_sync_debug_mode("error")`` from the second
iteration on (the first allocates the state and the pinned staging buffers) in the end-to-end test."""
import copy
import gc

import numpy as np
import pytest
import torch

from tests import ranger_ref as R
from tests.test_ranger_cpu import build, read, set_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WORST = {}


@pytest.fixture(scope="module")
def golden():
    return R.Golden()


@pytest.fixture(autouse=True)
def _collect_what_the_test_leaves():
    """An optimiser is cyclic garbage (torch wraps its ``step``), and here it holds device state, pinned staging buffers, events and, in the
    model tests, an autograd graph.  Collect it when the test ends, with the device idle, instead of leaving it to the collector in the
    middle of a later test's multi-stream step or graph capture.  A precaution of this file for the tests behind it: no failure has been
    traced to such a free.  Code that drops an optimiser before capturing a graph has ``Ranger.close()`` for the same purpose."""
    yield
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def up(st):
    return dict(st, **{q: st[q].astype(np.float64) for q in R.QUANTITIES})


def hold(got, want, bars, where, key):
    """|got - want| <= bars per quantity; the worst error / bar is kept per (key, quantity) and printed by the caller."""
    for q in R.QUANTITIES:
        err = float(np.abs(got[q].astype(np.float64) - want[q]).max())
        WORST[(key, q)] = max(WORST.get((key, q), 0.0), err / bars[q])
        assert err <= bars[q], (where, q, err, bars[q])


@pytest.mark.parametrize("use_kernel", [None, False], ids=["kernel", "torch_ops"])
@pytest.mark.parametrize("variant", R.VARIANTS)
def test_single_step_from_the_recorded_state(golden, variant, use_kernel):
    """Every step t of every variant, started from the reference's fp32 state after step t-1: the kernel, and the class's torch-operator
    path on the GPU, each against the fp64 step from that state (not against each other)."""
    from gdrnpp_bop2022_amd.gdrn_modeling import solver

    counted = solver.torch_path_tensors()
    key = "kernel" if use_kernel is None else "torch_ops"
    for t in range(1, R.STEPS + 1):
        prev = golden.state32(variant, t - 1)
        opt, params = build(variant, prev, DEV, use_kernel=use_kernel)
        set_grads(params, golden.grads[t])
        opt.step()
        got = read(opt, params)
        want = R.step_all({n: up(st) for n, st in prev.items()}, golden.grads[t], variant)
        for n in golden.grads[t]:
            e = golden.err("step32_err", variant, t, n)
            hold(got[n], want[n], {q: 2 * e[q] + R.ulp_of_max(want[n][q]) for q in R.QUANTITIES}, (variant, t, n), key)
            assert got[n]["step"] == want[n]["step"]
    assert solver.torch_path_tensors() == counted        # fp32 contiguous tensors: nothing was counted as foreign on either path
    print(f"{variant} {key}: worst error / bar so far " + ", ".join(f"{q} {WORST[(key, q)]:.3f}" for q in R.QUANTITIES))


def run_trajectory(golden, variant, place=None):
    """13 steps on the kernel -> [state after step t].  ``place``: how a host array becomes a device tensor (default: a fresh allocation)."""
    from gdrnpp_bop2022_amd.gdrn_modeling.solver import Ranger

    preset = place is not None        # a placed run sets the state a first step would create, placed like the parameter
    place = place or (lambda a: torch.from_numpy(a.copy()).to(DEV))

    params = {n: torch.nn.Parameter(place(p)) for n, p in golden.params.items()}
    groups = [dict(params=[params[n] for n, (_, g) in R.TENSORS.items() if g == gi], **grp) for gi, grp in enumerate(R.GROUPS)]
    opt = Ranger(groups, **R.VARIANTS[variant])
    if preset:
        for n, p in params.items():
            if n != "never":
                opt.state[p] = dict(step=0, exp_avg=place(np.zeros_like(golden.params[n])), exp_avg_sq=place(np.zeros_like(golden.params[n])),
                                    slow_buffer=place(golden.params[n]))
    traj = []
    for t in range(1, R.STEPS + 1):
        for n, p in params.items():
            p.grad = place(golden.grads[t][n]) if n in golden.grads[t] else None
        opt.step()
        traj.append(read(opt, params))
    return traj, params


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_trajectory_and_bookkeeping(golden, variant):
    traj, params = run_trajectory(golden, variant)
    states = {n: R.fresh_state(p) for n, p in golden.params.items()}
    for t in range(1, R.STEPS + 1):
        states = R.step_all(states, golden.grads[t], variant)        # the fp64 run (held to the fixture's by tests/test_ranger_cpu.py)
        got = traj[t - 1]
        steps = golden.steps(variant, t)
        for n in R.TENSORS:
            if n == "never":
                continue
            assert got[n]["step"] == steps[n]
            if t in R.CHECK_STEPS:
                e = golden.err("traj32_err", variant, t, n)
                hold(got[n], states[n], {q: 2 * e[q] + R.ulp_of_max(states[n][q]) for q in R.QUANTITIES}, (variant, t, n), "trajectory")
    # the tensor without a gradient: untouched bit for bit, no state; the one that skipped step 4 is one step behind
    assert np.array_equal(params["never"].detach().cpu().numpy(), golden.params["never"])
    assert all(step["never"] is None for step in traj)
    assert traj[-1]["skip4"]["step"] == 12 and traj[-1]["fc"]["step"] == 13
    print(f"{variant} trajectory: worst error / bar so far " + ", ".join(f"{q} {WORST[('trajectory', q)]:.3f}" for q in R.QUANTITIES))


def misplaced(a):
    """The array inside a larger device buffer, 4 bytes behind a 16-byte boundary."""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[1:1 + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a.copy()))
    assert t.data_ptr() % 16 == 4
    return t


def test_runs_repeat_bit_for_bit_aligned_or_not(golden):
    a, _ = run_trajectory(golden, "default")
    b, _ = run_trajectory(golden, "default")
    c, params = run_trajectory(golden, "default", place=misplaced)
    assert all(p.data_ptr() % 16 == 4 for p in params.values())
    for t in range(R.STEPS):
        for n in R.TENSORS:
            if n == "never":
                continue
            for q in R.QUANTITIES:
                assert np.array_equal(a[t][n][q], b[t][n][q]), (t, n, q)
                assert np.array_equal(a[t][n][q], c[t][n][q]), ("misaligned", t, n, q)


def edge_shapes():
    from gdrnpp_bop2022_amd.hip_lib import RANGER_TILE as TILE

    return [(TILE - 1,), (TILE,), (TILE + 1,), (2, TILE - 1), (2, TILE), (2, TILE + 1), (5, 4099), (250, 49), (2, 4100), (3, 2 * TILE + 5), (2, 3, 5, 7)]


@pytest.mark.parametrize("place", [None, misplaced], ids=["aligned", "misaligned"])
def test_shapes_at_the_tile_and_item_limits(place):
    """Shapes the fixture is too small for: one element below, at and above the tile, as a plain vector and as a row; rows cut into items of
    2 (4099 elements: items start off a 16-byte boundary) and of 248 rows; rows longer than a tile, whose mean comes from the pre-pass.  A
    first step and a rectified Lookahead step (6) from a seeded state.  Yardstick: ranger_ref in fp64; bar: twice the distance of ranger_ref's
    own fp32 step from it (the number format's error for this arithmetic) plus one unit in the last place of the largest value."""
    from gdrnpp_bop2022_amd.gdrn_modeling.solver import Ranger

    put = place or (lambda a: torch.from_numpy(a.copy()).to(DEV))
    rng = np.random.default_rng(R.SEED + 99)
    shapes = edge_shapes()
    for step in (1, 6):
        host, params = [], []
        for s in shapes:
            p = (rng.standard_normal(s) * 0.5).astype(np.float32)
            g = (rng.standard_normal(s) * 0.05 + 0.02).astype(np.float32)
            m = (rng.standard_normal(s) * 0.01).astype(np.float32) if step > 1 else np.zeros(s, np.float32)
            v = (rng.random(s) * 1e-4).astype(np.float32) if step > 1 else np.zeros(s, np.float32)
            slow = (p + rng.standard_normal(s).astype(np.float32) * 0.01).astype(np.float32) if step > 1 else p.copy()
            host.append(dict(p=p, m=m, v=v, slow=slow, g=g))
            params.append(torch.nn.Parameter(put(p)))
        opt = Ranger([dict(params=params, **R.GROUPS[0])])
        for h, p in zip(host, params):
            opt.state[p] = dict(step=step - 1, exp_avg=put(h["m"]), exp_avg_sq=put(h["v"]), slow_buffer=put(h["slow"]))
            p.grad = put(h["g"])
        opt.step()
        torch.cuda.synchronize()
        for s, h, p in zip(shapes, host, params):
            st = opt.state[p]
            got = dict(p=p.detach().cpu().numpy(), m=st["exp_avg"].cpu().numpy(), v=st["exp_avg_sq"].cpu().numpy(), slow=st["slow_buffer"].cpu().numpy())
            args = (h["p"], h["m"], h["v"], h["slow"], h["g"], step, R.GROUPS[0]["lr"], R.GROUPS[0]["weight_decay"])
            w64 = dict(zip(R.QUANTITIES, R.ranger_step_ref(*args)))
            w32 = dict(zip(R.QUANTITIES, R.ranger_step_ref(*args, dtype=np.float32)))
            bars = {q: 2 * float(np.abs(w32[q].astype(np.float64) - w64[q]).max()) + R.ulp_of_max(w64[q]) for q in R.QUANTITIES}
            hold(got, w64, bars, (s, step), "edges")
    print("edge shapes: worst error / bar " + ", ".join(f"{q} {WORST[('edges', q)]:.3f}" for q in R.QUANTITIES))


def test_nan_to_num_in_the_step_equals_nan_to_num_before_it():
    from gdrnpp_bop2022_amd.gdrn_modeling.solver import Ranger
    from gdrnpp_bop2022_amd.hip_lib import RANGER_TILE as TILE

    rng = np.random.default_rng(R.SEED + 5)
    shapes = [(7,), (6, 1, 7, 7), (8, 130), (2, TILE + 1)]
    p0 = [(rng.standard_normal(s) * 0.5).astype(np.float32) for s in shapes]
    g0 = [(rng.standard_normal(s) * 0.05 + 0.02).astype(np.float32) for s in shapes]
    for g in g0:
        flat = g.reshape(-1)
        flat[0], flat[flat.size // 2], flat[-1] = np.nan, np.inf, -np.inf
    results = []
    for flag in (True, False):
        params = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(DEV)) for p in p0]
        opt = Ranger(params, lr=8e-4, weight_decay=0.01, nan_to_num=flag)
        for p, g in zip(params, g0):
            p.grad = torch.from_numpy(g.copy()).to(DEV)
            if not flag:
                torch.nan_to_num(p.grad, nan=0, posinf=1e5, neginf=-1e5, out=p.grad)
        opt.step()
        results.append([(p.detach().cpu(), p.grad.cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()) for p in params])
    for s, on, off, g in zip(shapes, results[0], results[1], g0):
        assert all(torch.equal(a, b) for a, b in zip(on, off)), s
        assert torch.equal(on[1], torch.nan_to_num(torch.from_numpy(g), nan=0, posinf=1e5, neginf=-1e5)) and torch.isfinite(on[0]).all()


def clear_caches(model):
    for mod in model.modules():
        mod.__dict__.pop("_gdrnpp_cache", None)


def tiny_training_setup(extra=()):
    from gdrnpp_bop2022_amd.gdrn_modeling import GDRN
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
    from tests.test_gpu_losses import _training_batch

    cfg = get_cfg("lmo_resnet34_ape", ["MODEL.POSE_NET.LOSS_CFG.PM_LOSS_SYM=True", "SOLVER.OPTIMIZER_CFG={'type': 'Ranger', 'lr': 8e-4, 'weight_decay': 0.01}",
                                       "SOLVER.LR_SCHEDULER_NAME=flat_and_anneal", "SOLVER.ANNEAL_METHOD=cosine", "SOLVER.WARMUP_ITERS=10",
                                       "SOLVER.WARMUP_FACTOR=0.1", "SOLVER.TARGET_LR_FACTOR=0.05", "MODEL.POSE_NET.PNP_NET.LR_MULT=0.5", *extra])
    torch.manual_seed(11)
    model, opt = GDRN.build_model_optimizer(cfg, is_test=False)
    x, batch, tables, _ = _training_batch(cfg, 2, np.random.default_rng(R.SEED + 17), DEV)
    infer = {k: batch[k] for k in ("roi_classes", "roi_cams", "roi_whs", "roi_centers", "resize_ratios", "roi_coord_2d", "roi_extents")}
    return cfg, model, opt, x, batch, tables, infer


def test_a_kernel_step_advances_versions_and_the_weight_caches_follow():
    from gdrnpp_bop2022_amd.gdrn_modeling import solver, weight_cache

    cfg, model, opt, x, batch, tables, infer = tiny_training_setup()
    assert isinstance(opt, solver.Ranger) and model.training
    model.eval()
    with torch.no_grad():
        model(x, **infer)                      # fills the derived-weight caches from the initial weights
    model.train()
    layer = next(m for m in model.geo_head_net.modules() if isinstance(m, torch.nn.Conv2d))
    tag = weight_cache.weight_tag(layer.weight)
    versions = {n: p._version for n, p in model.named_parameters()}
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    counted = solver.torch_path_tensors()
    _, loss = model(x, do_loss=True, gt_tables=tables, **batch)
    sum(loss.values()).backward()
    opt.step()
    assert solver.torch_path_tensors() == counted, solver.last_torch_path()      # every tensor of the model went through the kernel
    for n, p in model.named_parameters():
        assert p.grad is not None and p._version > versions[n], n
    assert not torch.equal(layer.weight.detach(), before[next(n for n, p in model.named_parameters() if p is layer.weight)])
    assert weight_cache.weight_tag(layer.weight) != tag
    model.eval()
    fresh = copy.deepcopy(model)
    clear_caches(fresh)
    with torch.no_grad():
        out, want = model(x, **infer), fresh(x, **infer)
    for k in want:           # the bar of tests/test_gpu_losses.py for a repeated inference forward
        diff = (out[k] - want[k]).abs().max().item()
        print(f"eval forward after the step, {k}: max |cached model - fresh copy| {diff:.3g} of max {want[k].abs().max().item():.3g}")
        assert diff <= 2e-5 * want[k].abs().max().item(), k


def test_twenty_training_iterations_end_to_end(golden):
    from gdrnpp_bop2022_amd.gdrn_modeling import solver

    cfg, model, opt, x, batch, tables, _ = tiny_training_setup()
    sched = solver.build_lr_scheduler(cfg, opt, total_iters=golden.meta["sched"]["kwargs"]["total_iters"])
    sc = golden.meta["sched"]
    factors = golden.z["sched"][sc["warmups"].index("linear"), sc["anneals"].index("cosine"), 0]
    base = [8e-4, 8e-4, 8e-4 * 0.5]
    totals = []
    for it in range(20):
        assert [g["lr"] for g in opt.param_groups] == [b * float(factors[it]) for b in base], it
        _, loss = model(x, do_loss=True, gt_tables=tables, **batch)
        total = sum(loss.values())
        total.backward()
        if it:                  # from the second iteration on nothing in step() may wait for the device or read from it
            torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        sched.step()
        opt.zero_grad(set_to_none=True)
        totals.append(total.detach())
    totals = [float(t) for t in totals]
    print("total loss per iteration:", " ".join(f"{t:.4f}" for t in totals))
    assert all(np.isfinite(totals)) and totals[19] < totals[0]
    tables_ = next(iter(opt._tables.values()))
    assert tables_.uploads == 20 and len(tables_.plans) == 1       # one table copy per step, one layout


def test_what_the_kernel_cannot_take_runs_on_torch_operators_and_is_counted():
    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.gdrn_modeling import solver

    rng = np.random.default_rng(R.SEED + 3)
    a, g = (rng.standard_normal((130, 8)) * 0.5).astype(np.float32), (rng.standard_normal((130, 8)) * 0.05 + 0.02).astype(np.float32)
    strided = torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV).t())            # [8, 130], not contiguous
    half = torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV).half())
    plain = torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV))
    opt = solver.Ranger([strided, half, plain], **R.GROUPS[0])
    strided.grad, half.grad, plain.grad = torch.from_numpy(g.copy()).to(DEV).t(), torch.from_numpy(g.copy()).to(DEV).half(), torch.from_numpy(g.copy()).to(DEV)
    from gdrnpp_bop2022_amd.gdrn_modeling import weight_cache

    counted = solver.torch_path_tensors()
    tags = [(weight_cache.weight_tag(p), p._version) for p in (strided, half, plain)]
    opt.step()
    assert solver.torch_path_tensors() == counted + 2 and "torch operators" in solver.last_torch_path()
    for p, (tag, version) in zip((strided, half, plain), tags):        # either path moves the key of the derived-weight caches
        assert p._version > version and weight_cache.weight_tag(p) != tag
    # use_kernel=False: torch operators by request — not counted, and the versions advance all the same
    asked = torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV))
    asked.grad = torch.from_numpy(g.copy()).to(DEV)
    tag, version, n_counted = weight_cache.weight_tag(asked), asked._version, solver.torch_path_tensors()
    solver.Ranger([asked], use_kernel=False, **R.GROUPS[0]).step()
    assert asked._version > version and weight_cache.weight_tag(asked) != tag and solver.torch_path_tensors() == n_counted
    assert half.dtype == torch.float16 and opt.state[half]["exp_avg"].dtype == torch.float32
    z = np.zeros_like(a.T)
    w64 = R.ranger_step_ref(a.T, z, z, a.T, g.T, 1, R.GROUPS[0]["lr"], R.GROUPS[0]["weight_decay"])
    w32 = R.ranger_step_ref(a.T, z, z, a.T, g.T, 1, R.GROUPS[0]["lr"], R.GROUPS[0]["weight_decay"], dtype=np.float32)
    assert np.abs(strided.detach().cpu().numpy() - w64[0]).max() <= 2 * np.abs(w32[0] - w64[0]).max() + R.ulp_of_max(w64[0])
    # the binding itself refuses them
    tables = hip_lib.RangerTables(DEV)
    ok = [torch.zeros(8, 130, device=DEV) for _ in range(5)]
    coefs = [(0.95, 0.999, 0.05, 0.001, 1e-5, 0.5, 0.0, -1e-3)]
    for bad in (torch.zeros(8, 130), torch.zeros(130, 8, device=DEV).t(), torch.zeros(8, 130, device=DEV, dtype=torch.float64), torch.zeros(8, 131, device=DEV)):
        for slot in (0, 1, 4):
            args = list(ok)
            args[slot] = bad
            with pytest.raises(RuntimeError, match="ranger_step"):
                hip_lib.ranger_step(tables, *[[t] for t in args], [130], [0], coefs)
    with pytest.raises(RuntimeError, match="differ in length"):
        hip_lib.ranger_step(tables, ok[:1], ok[:1], ok[:1], ok[:1], ok[:1], [130, 130], [0], coefs)
    hip_lib.ranger_step(tables, *[[t] for t in ok], [130], [0], coefs)           # and takes the well-formed call
    assert all(float(t.abs().max()) == 0 for t in ok)


def test_channels_last_parameters_run_on_the_kernel():
    """The models' 4-D weights are channels_last: a row (all dimensions but the first) is one run of memory as in a contiguous tensor.  A
    [C,1,7,7] weight is both at once and torch reports either set of strides for it and its gradient: still one layout."""
    from gdrnpp_bop2022_amd.gdrn_modeling import solver

    rng = np.random.default_rng(R.SEED + 4)
    shapes = [(8, 6, 3, 3), (16, 1, 7, 7), (4, 5, 1, 1)]
    host = [((rng.standard_normal(s) * 0.5).astype(np.float32), (rng.standard_normal(s) * 0.05 + 0.02).astype(np.float32)) for s in shapes]
    def nhwc(a):        # channels_last strides spelled out: .contiguous(memory_format=...) leaves a tensor that already qualifies as it is
        n, c, h, w = a.shape
        return torch.empty_strided(a.shape, (h * w * c, 1, w * c, c), dtype=torch.float32, device=DEV).copy_(torch.from_numpy(a.copy()))

    params = [torch.nn.Parameter(nhwc(a)) for a, _ in host]
    opt = solver.Ranger(params, **R.GROUPS[0])
    for p, (_, g) in zip(params, host):
        p.grad = nhwc(g) if p.shape[1] > 1 and p.shape[2] > 1 else torch.from_numpy(g.copy()).to(DEV)
    assert params[0].stride() != torch.empty(shapes[0]).stride() and params[1].grad.stride() != params[1].stride()
    counted = solver.torch_path_tensors()
    opt.step()
    assert solver.torch_path_tensors() == counted, solver.last_torch_path()
    for p, (a, g) in zip(params, host):
        z = np.zeros_like(a)
        args = (a, z, z, a, g, 1, R.GROUPS[0]["lr"], R.GROUPS[0]["weight_decay"])
        w64, w32 = R.ranger_step_ref(*args), R.ranger_step_ref(*args, dtype=np.float32)
        st = opt.state[p]
        got = dict(p=p.detach().cpu().numpy(), m=st["exp_avg"].cpu().numpy(), v=st["exp_avg_sq"].cpu().numpy(), slow=st["slow_buffer"].cpu().numpy())
        hold(got, dict(zip(R.QUANTITIES, w64)),
             {q: 2 * float(np.abs(w32[j].astype(np.float64) - w64[j]).max()) + R.ulp_of_max(w64[j]) for j, q in enumerate(R.QUANTITIES)}, tuple(a.shape), "nhwc")


def test_resumed_state_is_laid_out_like_its_parameter_once_and_close_releases_the_tables():
    """A reference checkpoint's optimiser state is contiguous; the models' 4-D weights are channels_last.  The first step copies such a
    state into the parameter's layout, so the tensor runs on the kernel from then on instead of on torch operators for ever."""
    from gdrnpp_bop2022_amd.gdrn_modeling import solver

    rng = np.random.default_rng(R.SEED + 6)
    s = (8, 6, 3, 3)
    h = {k: (rng.standard_normal(s) * 0.1).astype(np.float32) for k in ("p", "m", "g", "slow")}
    h["v"] = (rng.random(s) * 1e-4).astype(np.float32)
    p = torch.nn.Parameter(torch.from_numpy(h["p"].copy()).to(DEV).contiguous(memory_format=torch.channels_last))
    opt = solver.Ranger([p], **R.GROUPS[0])
    opt.state[p] = dict(step=5, exp_avg=torch.from_numpy(h["m"].copy()).to(DEV), exp_avg_sq=torch.from_numpy(h["v"].copy()).to(DEV),
                        slow_buffer=torch.from_numpy(h["slow"].copy()).to(DEV))
    assert opt.state[p]["exp_avg"].stride() != p.stride()
    p.grad = torch.from_numpy(h["g"].copy()).to(DEV).contiguous(memory_format=torch.channels_last)
    counted = solver.torch_path_tensors()
    opt.step()
    assert solver.torch_path_tensors() == counted, solver.last_torch_path()
    st = opt.state[p]
    assert all(st[k].stride() == p.stride() for k in ("exp_avg", "exp_avg_sq", "slow_buffer"))
    args = (h["p"], h["m"], h["v"], h["slow"], h["g"], 6, R.GROUPS[0]["lr"], R.GROUPS[0]["weight_decay"])
    w64, w32 = R.ranger_step_ref(*args), R.ranger_step_ref(*args, dtype=np.float32)
    got = dict(p=p.detach().cpu().numpy(), m=st["exp_avg"].cpu().numpy(), v=st["exp_avg_sq"].cpu().numpy(), slow=st["slow_buffer"].cpu().numpy())
    hold(got, dict(zip(R.QUANTITIES, w64)),
         {q: 2 * float(np.abs(w32[j].astype(np.float64) - w64[j]).max()) + R.ulp_of_max(w64[j]) for j, q in enumerate(R.QUANTITIES)}, s, "resumed")
    tables = opt._tables[p.device]
    assert tables.staging and tables.plans
    opt.close()
    assert not tables.staging and not tables.plans and tables.table is None and not opt._tables
    opt.step()                       # and the next step builds them again
    assert opt._tables[p.device].uploads == 1 and opt.state[p]["step"] == 7
