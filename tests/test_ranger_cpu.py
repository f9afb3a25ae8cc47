"""gdrn_modeling/solver.py without a GPU: the torch-operator path of ``Ranger`` and the ``flat_and_anneal`` schedule against values recorded
from the reference's own code (tests/golden/ranger_golden.npz, written by tests/golden/make_golden_ranger.py), tests/ranger_ref.py — the
yardstick of the GPU tests — against the reference's fp64 run, the builders, and the C ABI of the kernel.  CPU only."""
import copy
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

from tests import ranger_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return R.Golden()


def same_torch_as_recorded(golden):
    """The installed torch is the build, on the CPU capability, whose kernels produced the fixture's fp32 run: then the torch-operator path
    must reproduce that run bit for bit.  On any other build the order of a reduction or a contraction may differ in the last place, and the
    bar of twice the reference's own fp32 error plus one unit in the last place is what holds."""
    return golden.meta["torch_version"] == torch.__version__ and golden.meta["cpu_capability"] == torch.backends.cpu.get_cpu_capability()


def build(variant, states, device="cpu", **kw):
    """``solver.Ranger`` over the fixture's tensors in its two groups, with the per-tensor state of ``states`` set."""
    from gdrnpp_bop2022_amd.gdrn_modeling.solver import Ranger

    params = {n: torch.nn.Parameter(torch.from_numpy(states[n]["p"].copy()).to(device)) for n in R.TENSORS}
    groups = [dict(params=[params[n] for n, (_, g) in R.TENSORS.items() if g == gi], **grp) for gi, grp in enumerate(R.GROUPS)]
    opt = Ranger(groups, **R.VARIANTS[variant], **kw)
    for n, st in states.items():
        if st["step"] > 0:
            opt.state[params[n]] = dict(step=st["step"], exp_avg=torch.from_numpy(st["m"].copy()).to(device),
                                        exp_avg_sq=torch.from_numpy(st["v"].copy()).to(device), slow_buffer=torch.from_numpy(st["slow"].copy()).to(device))
    return opt, params


def set_grads(params, grads_t):
    for n, p in params.items():
        p.grad = torch.from_numpy(grads_t[n].copy()).to(p.device) if n in grads_t else None


def read(opt, params):
    out = {}
    for n, p in params.items():
        st = opt.state.get(p, {})
        out[n] = dict(p=p.detach().cpu().numpy(), m=st["exp_avg"].cpu().numpy(), v=st["exp_avg_sq"].cpu().numpy(), slow=st["slow_buffer"].cpu().numpy(),
                      step=int(st["step"])) if st else None
    return out


def test_fixture_holds_the_cases(golden):
    meta = golden.meta
    assert meta["variants"] == list(R.VARIANTS) and meta["steps"] == R.STEPS == 13
    assert {n: tuple(s) for n, s in meta["tensors"].items()} == {n: s for n, (s, _) in R.TENSORS.items()}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ranger_golden.npz")) < 1 << 20
    # the inputs are the seeded ones
    assert all(np.array_equal(golden.params[n], p) for n, p in R.seeded_params().items())
    grads = R.seeded_grads()
    assert all(sorted(grads[t]) == sorted(golden.grads[t]) and all(np.array_equal(golden.grads[t][n], g) for n, g in grads[t].items()) for t in grads)
    # the rectification starts at step 6 with the default betas, at step 5 with the threshold at 4
    n_sma = golden.z["default/radam"][:, 0]
    assert abs(n_sma[4] - 4.996) < 1e-3 and abs(n_sma[5] - 5.994) < 1e-3 and n_sma[3] < 4 < n_sma[4] < 5 < n_sma[5]
    # step counts diverge inside one optimiser
    s13 = golden.steps("default", 13)
    assert s13["never"] == -1 and s13["skip4"] == 12 and s13["fc"] == 13


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_restatement_matches_the_recorded_fp64_run(golden, variant):
    """ranger_ref in fp64 against the reference's fp64 run: 1e-12 of the tensor's largest value on the states recorded in full, and on the
    sum and the sum of squares of every quantity at every step."""
    states = {n: R.fresh_state(p) for n, p in golden.params.items()}
    for t in range(1, R.STEPS + 1):
        states = R.step_all(states, golden.grads[t], variant)
        kw = dict(R.DEFAULTS, **{k: v for k, v in R.VARIANTS[variant].items() if k in R.DEFAULTS})
        assert R.radam(t, *kw["betas"], kw["N_sma_threshhold"]) == tuple(golden.z[f"{variant}/radam"][t - 1])
        for n, st in states.items():
            sums = golden.sums64(variant, t, n)
            for j, q in enumerate(R.QUANTITIES):
                a = st[q]
                scale = max(float(np.abs(a).max()), 1e-300)
                assert abs(a.sum() - sums[j, 0]) <= 1e-12 * scale * a.size, (t, n, q)
                assert abs((a ** 2).sum() - sums[j, 1]) <= 1e-12 * scale * scale * a.size, (t, n, q)
            if t in golden.meta["full64_steps"][variant]:
                full = golden.full64(variant, t, n)
                for q in ("p", "m", "v"):
                    assert np.abs(st[q] - full[q]).max() <= 1e-12 * max(np.abs(full[q]).max(), 1e-300), (t, n, q)


def test_fp32_restatement_is_the_formats_own_error(golden):
    """The fp32 mode of ranger_ref (the bar of the GPU tests on shapes the fixture does not hold) errs like the reference's fp32 step."""
    for t in (1, 6, 13):
        prev = golden.state32("default", t - 1)
        s32 = R.step_all(prev, golden.grads[t], "default", dtype=np.float32)
        s64 = R.step_all({n: dict(st, **{q: st[q].astype(np.float64) for q in R.QUANTITIES}) for n, st in prev.items()}, golden.grads[t], "default")
        for n in golden.grads[t]:
            for q in R.QUANTITIES:
                ours = np.abs(s32[n][q].astype(np.float64) - s64[n][q]).max()
                assert ours <= 2 * golden.err("step32_err", "default", t, n)[q] + R.ulp_of_max(s64[n][q]), (t, n, q)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_torch_path_follows_the_recorded_fp32_run(golden, variant):
    """13 steps of ``solver.Ranger`` on CPU tensors against the reference's fp32 states.  The installed torch reproduces the fixture bit for
    bit, so equality is asserted wherever torch is the recorded build on the recorded CPU capability (``same_torch_as_recorded``); on
    another build: within twice the reference's own distance from its fp64 run plus one fp32 unit in the last place of the largest value."""
    opt, params = build(variant, golden.state32(variant, 0))
    exact, must_equal = True, same_torch_as_recorded(golden)
    for t in range(1, R.STEPS + 1):
        set_grads(params, golden.grads[t])
        opt.step()
        got, want = read(opt, params), golden.state32(variant, t)
        assert got["never"] is None and np.array_equal(params["never"].detach().numpy(), golden.params["never"])
        for n, st in got.items():
            if st is None:
                continue
            assert st["step"] == want[n]["step"] == golden.steps(variant, t)[n]
            for q in R.QUANTITIES:
                bar = 2 * golden.err("traj32_err", variant, t, n)[q] + R.ulp_of_max(want[n][q])
                assert np.abs(st[q].astype(np.float64) - want[n][q]).max() <= bar, (t, n, q)
                exact = exact and np.array_equal(st[q], want[n][q])
                assert exact or not must_equal, (t, n, q, "not bit-equal to the reference's fp32 run on the torch build that recorded it")
    print(f"{variant}: torch-operator path bit-equal to the reference's fp32 run: {exact}")


def test_state_dict_has_the_references_keys_and_resumes_its_state(golden):
    opt, params = build("default", golden.state32("default", 7))
    sd = opt.state_dict()
    ref_groups = json.loads(str(golden.z["state7/param_groups"]))
    assert [sorted(g) for g in sd["param_groups"]] == [sorted(g) for g in ref_groups]
    for g, r in zip(sd["param_groups"], ref_groups):
        assert {k: (list(v) if isinstance(v, tuple) else v) for k, v in g.items()} == r
    assert sorted(sd["state"]) == [int(i) for i in golden.z["state7/ids"]]
    assert all(sorted(st) == ["exp_avg", "exp_avg_sq", "slow_buffer", "step"] for st in sd["state"].values())
    # the state goes into a fresh optimiser through torch's own load_state_dict and continues to the recorded step 8
    fresh, params2 = build("default", {n: dict(R.fresh_state(st["p"], np.float32)) for n, st in golden.state32("default", 7).items()})
    fresh.load_state_dict(copy.deepcopy(sd))
    assert fresh.state_dict()["param_groups"] == sd["param_groups"]
    set_grads(params2, golden.grads[8])
    fresh.step()
    got, want = read(fresh, params2), golden.state32("default", 8)
    for n, st in got.items():
        if st is None:
            assert n == "never"
            continue
        assert st["step"] == want[n]["step"]
        for q in R.QUANTITIES:
            bar = 2 * golden.err("step32_err", "default", 8, n)[q] + R.ulp_of_max(want[n][q])
            assert np.abs(st[q].astype(np.float64) - want[n][q]).max() <= bar, (n, q)
            assert np.array_equal(st[q], want[n][q]) or not same_torch_as_recorded(golden), (n, q)       # bit for bit on the recorded build


def test_torch_path_advances_the_parameters_version():
    """``weight_cache.weight_tag`` keys derived weights on (data_ptr, _version): a step on torch operators must move it as a kernel step does."""
    from gdrnpp_bop2022_amd.gdrn_modeling import weight_cache
    from gdrnpp_bop2022_amd.gdrn_modeling.solver import Ranger

    p, q = torch.nn.Parameter(torch.ones(4, 3)), torch.nn.Parameter(torch.ones(2))
    opt = Ranger([p, q], lr=0.1)
    p.grad = torch.arange(12.0).reshape(4, 3)
    tag, vp, vq = weight_cache.weight_tag(p), p._version, q._version
    opt.step()
    assert p._version > vp and weight_cache.weight_tag(p) != tag and q._version == vq       # q had no gradient: untouched


def test_constructor_checks_and_sparse_gradients_raise():
    from gdrnpp_bop2022_amd.gdrn_modeling.solver import Ranger

    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw, text in ((dict(alpha=1.5), "Invalid slow update rate"), (dict(alpha=-0.1), "Invalid slow update rate"), (dict(k=0), "Invalid lookahead steps"),
                     (dict(lr=0), "Invalid Learning Rate"), (dict(lr=-1.0), "Invalid Learning Rate"), (dict(eps=0), "Invalid eps")):
        with pytest.raises(ValueError, match=text):
            Ranger(p, **kw)
    opt = Ranger(p)
    assert opt.defaults == dict(lr=1e-3, alpha=0.5, k=6, step_counter=0, betas=(0.95, 0.999), N_sma_threshhold=5, eps=1e-5, weight_decay=0)
    emb = torch.nn.Embedding(4, 3, sparse=True)
    emb(torch.tensor([1])).sum().backward()
    with pytest.raises(RuntimeError, match="sparse"):
        Ranger(emb.parameters()).step()
    # other dtypes run the same step in fp32 and keep their own type
    h = torch.nn.Parameter(torch.ones(2, 4, dtype=torch.float64))
    o = Ranger([h], lr=0.1)
    h.grad = torch.arange(8, dtype=torch.float64).reshape(2, 4)
    o.step()
    assert h.dtype == torch.float64 and o.state[h]["exp_avg"].dtype == torch.float32 and o.state[h]["slow_buffer"].dtype == torch.float64
    want = R.ranger_step_ref(np.ones((2, 4), np.float32), np.zeros((2, 4)), np.zeros((2, 4)), np.ones((2, 4)), np.arange(8.0).reshape(2, 4), 1, 0.1, 0,
                             dtype=np.float32)
    assert np.allclose(h.detach().numpy(), want[0], rtol=0, atol=1e-6)


def test_schedule_equals_the_recorded_factors(golden):
    from gdrnpp_bop2022_amd.gdrn_modeling.solver import flat_and_anneal_lr_scheduler

    sc = golden.meta["sched"]
    table = golden.z["sched"]
    for a, wm in enumerate(sc["warmups"]):
        for b, am in enumerate(sc["anneals"]):
            for cyclic in (False, True):
                opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    sched, f = flat_and_anneal_lr_scheduler(opt, warmup_method=wm, anneal_method=am, cyclic=cyclic, return_function=True, **sc["kwargs"])
                assert isinstance(sched, torch.optim.lr_scheduler.LambdaLR)
                for x in range(sc["iters"]):
                    assert float(f(x)) == float(table[a, b, int(cyclic), x]), (wm, am, cyclic, x)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    for kw, text in ((dict(warmup_method="cubic"), "warmup_method"), (dict(anneal_method="sine"), "anneal_method"), (dict(anneal_point=1.5), "anneal_point"),
                     (dict(anneal_method="step", steps=[0.8, 0.6]), "ascending"), (dict(anneal_method="step", steps=[0.5, 1.5]), "error in steps")):
        with pytest.raises(ValueError, match=text), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            flat_and_anneal_lr_scheduler(opt, 50, **kw)
    assert isinstance(flat_and_anneal_lr_scheduler(opt, 50), torch.optim.lr_scheduler.LambdaLR)


def test_builders_read_the_solver_block():
    from gdrnpp_bop2022_amd.gdrn_modeling import solver
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg

    cfg = get_cfg("ycbv_convnext_a6")
    assert dict(cfg.SOLVER.OPTIMIZER_CFG) == dict(type="Ranger", lr=8e-4, weight_decay=0.01)
    assert (cfg.SOLVER.LR_SCHEDULER_NAME, cfg.SOLVER.ANNEAL_METHOD, cfg.SOLVER.ANNEAL_POINT) == ("flat_and_anneal", "cosine", 0.72)
    p = [dict(params=[torch.nn.Parameter(torch.zeros(2))], lr=1e-4)]
    opt = solver.build_optimizer_with_params(cfg, p)
    assert isinstance(opt, solver.Ranger) and opt.param_groups[0]["lr"] == 1e-4 and opt.param_groups[0]["weight_decay"] == 0.01 and not opt.nan_to_num
    assert solver.build_optimizer_with_params(get_cfg("ycbv_convnext_a6", ["SOLVER.SET_NAN_GRAD_TO_ZERO=True"]), p).nan_to_num
    cfg.SOLVER.OPTIMIZER_CFG = "dict(type='AdamW', lr=1e-3, weight_decay=0.05)"
    assert isinstance(solver.build_optimizer_with_params(cfg, p), torch.optim.AdamW)
    assert isinstance(solver.build_optimizer_with_params(get_cfg("lmo_resnet34_ape"), p), torch.optim.RMSprop)       # the base file's block
    cfg.SOLVER.OPTIMIZER_CFG = dict(type="Lion", lr=1e-3)
    with pytest.raises(ValueError, match="Lion"):
        solver.build_optimizer_with_params(cfg, p)
    cfg.SOLVER.OPTIMIZER_CFG = ""
    with pytest.raises(RuntimeError, match="OPTIMIZER_CFG"):
        solver.build_optimizer_with_params(cfg, p)
    with pytest.raises(NotImplementedError, match="CLIP_GRADIENTS"):
        solver.build_optimizer_with_params(get_cfg("ycbv_convnext_a6", ["SOLVER.CLIP_GRADIENTS.ENABLED=True"]), p)
    # the scheduler of the shipped block: 1000 warm-up iterations from 0.001, flat, cosine from 72 %
    cfg = get_cfg("ycbv_convnext_a6")
    opt = solver.build_optimizer_with_params(cfg, p)
    sched, f = solver.build_lr_scheduler(cfg, opt, total_iters=10000, return_function=True)
    assert f(0) == 0.001 and f(1000) == 1 and f(7199) == 1 and 0 < f(9999) < 1e-3 and f(10000) == 0
    assert opt.param_groups[0]["lr"] == 1e-4 * 0.001
    with pytest.raises(ValueError, match="WarmupMultiStepLR"):
        solver.build_lr_scheduler(get_cfg("lmo_resnet34_ape"), opt, 100)


SMALL = ["MODEL.DEVICE=cpu", "MODEL.POSE_NET.BACKBONE.INIT_CFG.pretrained=False"]


@pytest.mark.parametrize("name", ["lmo_resnet34_ape", "ycbv_convnext_a6"])
def test_build_model_optimizer_for_training(name):
    from gdrnpp_bop2022_amd.gdrn_modeling import GDRN, GDRN_double_mask, solver
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg

    ranger = "SOLVER.OPTIMIZER_CFG={'type': 'Ranger', 'lr': 8e-4, 'weight_decay': 0.01}"

    def make(opts, is_test=False):
        cfg = get_cfg(name, SMALL + [ranger] + opts)
        builder = GDRN.build_model_optimizer if cfg.MODEL.POSE_NET.NAME == "GDRN" else GDRN_double_mask.build_model_optimizer
        torch.manual_seed(3)
        return builder(cfg, is_test=is_test)

    model, opt = make(["MODEL.POSE_NET.GEO_HEAD.LR_MULT=0.5", "MODEL.POSE_NET.PNP_NET.LR_MULT=2.0"])
    assert isinstance(opt, solver.Ranger) and model.training
    assert [g["lr"] for g in opt.param_groups] == [8e-4, 8e-4 * 0.5, 8e-4 * 2.0] and all(g["weight_decay"] == 0.01 for g in opt.param_groups)
    parts = (model.backbone, model.geo_head_net, model.pnp_net)
    for g, part in zip(opt.param_groups, parts):
        assert [id(p) for p in g["params"]] == [id(p) for p in part.parameters() if p.requires_grad]
    ids = [id(p) for g in opt.param_groups for p in g["params"]]
    assert len(ids) == len(set(ids)) and set(ids) == {id(p) for p in model.parameters() if p.requires_grad}
    # a frozen backbone: no group, no gradients
    model, opt = make(["MODEL.POSE_NET.BACKBONE.FREEZE=True", "MODEL.POSE_NET.PNP_NET.LR_MULT=2.0"])
    assert [g["lr"] for g in opt.param_groups] == [8e-4, 8e-4 * 2.0]
    assert not any(p.requires_grad for p in model.backbone.parameters()) and all(p.requires_grad for p in model.pnp_net.parameters())
    ids = [id(p) for g in opt.param_groups for p in g["params"]]
    assert set(ids) == {id(p) for p in model.parameters() if p.requires_grad} and len(ids) == len(set(ids))
    # the inference build is what it was: eval mode, no optimiser, every parameter as built
    test_model, none = make([], is_test=True)
    train_model, _ = make([])
    assert none is None and not test_model.training
    a, b = test_model.state_dict(), train_model.state_dict()
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert all(p.requires_grad for p in test_model.parameters())


def test_header_signatures_and_exports_name_the_kernel():
    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.hip_lib import abi, net

    header = open(os.path.join(ROOT, "include", "gdrnpp_hip.h")).read()
    assert re.search(r"\bint gdrnpp_ranger_step\(const gdrnpp_ranger_tensor\* tensors, int n_tensors, const gdrnpp_ranger_work\* work, int n_work,", header)
    res, args = abi.SIGNATURES["gdrnpp_ranger_step"]
    assert res is abi.c_int and len(args) == 8 and args[-1] is abi.c_void_p
    for name in ("ranger_step", "ranger_plan", "RangerTables", "ranger_tensor_ok", "RANGER_TILE"):
        assert getattr(hip_lib, name) is getattr(net, name)
    # the Python side's constants and table layouts are the header's
    consts = dict(re.findall(r"#define GDRNPP_RANGER_(\w+) (\d+)", header))
    assert {k: int(v) for k, v in consts.items()} == dict(TILE=net.RANGER_TILE, RECTIFIED=net.RANGER_RECTIFIED, LOOKAHEAD=net.RANGER_LOOKAHEAD,
                                                          NAN_TO_NUM=net.RANGER_NAN_TO_NUM)
    assert (net.RANGER_TENSOR.itemsize, net.RANGER_WORK.itemsize, net.RANGER_LONG_ROW.itemsize) == (96, 24, 16)
    for struct, dtype in (("gdrnpp_ranger_tensor", net.RANGER_TENSOR), ("gdrnpp_ranger_work", net.RANGER_WORK), ("gdrnpp_ranger_long_row", net.RANGER_LONG_ROW)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        fields = [f.strip().lstrip("*") for decl in body.split(";") if decl.strip() for f in decl.strip().split(" ", 1)[1].replace("long ", "").split(",")]
        assert [re.sub(r"\[\d+\]", "", f) for f in fields] == list(dtype.names), struct
    assert os.path.exists(os.path.join(ROOT, "gdrnpp_bop2022_amd", "csrc", "ranger.hip"))


def test_plan_cuts_tensors_into_items_inside_them():
    from gdrnpp_bop2022_amd.hip_lib import RANGER_TILE as TILE, ranger_plan

    shapes = [(5, 0), (TILE, 0), (TILE + 1, 0), (6 * 49, 49), (250 * 49, 49), (5 * 4099, 4099), (2 * TILE, TILE), (2 * (TILE + 1), TILE + 1), (0, 0),
              (3 * (2 * TILE + 5), 2 * TILE + 5), (7, 1)]
    work, long_rows = ranger_plan([n for n, _ in shapes], [L for _, L in shapes])
    covered = {}
    for w in work:
        n, L = shapes[w["tensor"]]
        assert 0 < w["count"] <= TILE and 0 <= w["start"] and w["start"] + w["count"] <= n
        if 0 < L <= TILE:
            assert w["start"] % L == 0 and w["count"] % L == 0 and w["mean_slot"] == -1
            if TILE // L >= 4:
                assert w["start"] % 4 == 0
        elif L > TILE:
            row = long_rows[w["mean_slot"]]
            assert row["tensor"] == w["tensor"] and row["row"] * L <= w["start"] and w["start"] + w["count"] <= (row["row"] + 1) * L
        else:
            assert w["mean_slot"] == -1
        covered.setdefault(int(w["tensor"]), []).append((int(w["start"]), int(w["count"])))
    for t, (n, _) in enumerate(shapes):
        spans = sorted(covered.get(t, []))
        assert sum(c for _, c in spans) == n and all(a + c == b for (a, c), (b, _) in zip(spans, spans[1:])), t
    assert len(long_rows) == 2 + 3 and [int(w["count"]) for w in work if w["tensor"] == 7] == [TILE, 1, TILE, 1]
    assert [int(w["count"]) for w in work if w["tensor"] == 4] == [248 * 49, 2 * 49] and [int(w["start"]) for w in work if w["tensor"] == 5] == [0, 8198, 16396]
    with pytest.raises(RuntimeError, match="does not divide"):
        ranger_plan([10], [3])
