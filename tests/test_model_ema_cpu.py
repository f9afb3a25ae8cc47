"""``ModelEMA`` (det/yolox/utils/ema.py and the lib/torch_utils shim), ``build_model_ema`` and the YOLOX training step's builders on the CPU.

The torch-operator path is held to tests/golden/model_ema_golden.npz, recorded from the reference's own two classes: equality of the bits at
every recorded update, which is what the two statements give on any torch build (no reduction, no contraction: a product, a product and
a sum per element, each its own operator)."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT
from tests import model_ema_ref as R


@pytest.fixture(scope="module")
def golden():
    return R.Golden()


def ema_class(cls):
    if cls == "yolox":
        from gdrnpp_bop2022_amd.det.yolox.utils.ema import ModelEMA
    else:
        from gdrnpp_bop2022_amd.lib.torch_utils.torch_utils import ModelEMA
    return ModelEMA


def follow(golden, ema, model, cls, decay, run):
    """Every recorded update of ``run``: the model takes the recorded state, the EMA must arrive at the recorded one, bit for bit."""
    for t in range(1, R.RUNS[run]["steps"] + 1):
        R.load_state(getattr(model, "module", model), golden.model(run, t))
        ema.update(model)
        assert ema.updates == R.RUNS[run]["updates"] + t
        assert ema.decay(ema.updates) == golden.d(cls, decay, run, t)
        want = golden.ema(cls, decay, run, t)
        for k, v in ema.ema.state_dict().items():
            assert v.dtype == torch.from_numpy(want[k]).dtype, k
            assert R.same_bits(v, torch.from_numpy(want[k])), (cls, decay, run, t, k)


@pytest.mark.parametrize("run", list(R.RUNS))
@pytest.mark.parametrize("decay", R.DECAYS)
@pytest.mark.parametrize("cls", R.CLASSES)
@pytest.mark.parametrize("use_kernel", [None, False], ids=["default", "torch_ops"])
def test_torch_path_reproduces_the_references_run(golden, cls, decay, run, use_kernel):
    from gdrnpp_bop2022_amd.det.yolox.utils import ema as E

    counted = E.torch_path_tensors()
    model = R.build_tiny()
    ema = ema_class(cls)(model, decay, updates=R.RUNS[run]["updates"], use_kernel=use_kernel)
    follow(golden, ema, model, cls, decay, run)
    sd = ema.ema.state_dict()
    assert int(sd["bn.num_batches_tracked"]) == R.TRACKED_AT_COPY != int(model.bn.num_batches_tracked)      # the copy's value, not the model's
    assert sd["scale64"].dtype == torch.float64
    # fp64 all the way: the fp64 buffer of the last update is the two statements in fp64, not in fp32
    t = R.RUNS[run]["steps"]
    prev = golden.ema(cls, decay, run, t - 1)["scale64"] if t > 1 else None
    if prev is not None:
        d = golden.d(cls, decay, run, t)
        want = prev * d + (1.0 - d) * golden.model(run, t)["scale64"]
        assert np.array_equal(sd["scale64"].numpy(), want)
        assert not np.array_equal(want, want.astype(np.float32).astype(np.float64))
    assert E.torch_path_tensors() == counted          # CPU tensors: no kernel was passed over, nothing is counted


def test_the_fixture_is_what_the_docstring_says(golden):
    assert set(golden.keys) == set(R.build_tiny().state_dict())
    for cls in R.CLASSES:
        for decay in R.DECAYS:
            assert golden.d(cls, decay, "fresh", 1) == decay * (1 - math.exp(-1 / 2000))
            assert golden.d(cls, decay, "resume", 1) == decay * (1 - math.exp(-2000 / 2000))
    a, b = golden.ema("yolox", 0.9998, "fresh", 5), golden.ema("gdrn", 0.9998, "fresh", 5)
    assert all(np.array_equal(a[k], b[k]) for k in golden.keys)          # the reference's two classes are one computation
    assert not np.array_equal(a["conv.weight"], golden.ema("yolox", 0.9999, "fresh", 5)["conv.weight"])
    assert os.path.getsize(R.GOLDEN) < 100 * 1024


@pytest.mark.parametrize("cls", R.CLASSES)
def test_the_copy_is_an_eval_mode_copy_without_gradients_or_caches(cls):
    from gdrnpp_bop2022_amd.gdrn_modeling import weight_cache

    model = R.build_tiny().train()
    stale = torch.zeros(3)
    weight_cache.module_cache(model.conv)["w"] = (weight_cache.weight_tag(model.conv.weight), stale)
    model.__dict__["_gdrnpp_yolox_buffers"] = {"plan": stale}
    ema = ema_class(cls)(model)
    assert ema.updates == 0 and ema.decay(2000) == 0.9999 * (1 - math.exp(-1.0))
    assert model.training and not ema.ema.training and all(not m.training for m in ema.ema.modules())
    assert all(p.requires_grad for p in model.parameters()) and not any(p.requires_grad for p in ema.ema.parameters())
    assert all(not any(k.startswith("_gdrnpp_") for k in m.__dict__) for m in ema.ema.modules())
    assert model.conv.__dict__["_gdrnpp_cache"]["w"][1] is stale and "_gdrnpp_yolox_buffers" in model.__dict__      # the model keeps its own
    for (k, a), b in zip(model.state_dict().items(), ema.ema.state_dict().values()):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr(), k


@pytest.mark.parametrize("cls", R.CLASSES)
def test_a_data_parallel_model_is_unwrapped(cls, golden):
    from gdrnpp_bop2022_amd.det.yolox.utils.ema import is_parallel
    from gdrnpp_bop2022_amd.lib.torch_utils import torch_utils as TU

    model = R.build_tiny()
    wrapped = nn.DataParallel(model)
    assert is_parallel(wrapped) and TU.is_parallel(wrapped) and not is_parallel(model) and TU.is_parallel is is_parallel
    ema = ema_class(cls)(wrapped, 0.9998)
    assert isinstance(ema.ema, R.Tiny) and list(ema.ema.state_dict()) == list(model.state_dict())      # no "module." prefix
    follow(golden, ema, wrapped, cls, 0.9998, "fresh")


def test_update_attr_and_copy_attr_honour_include_and_exclude():
    from gdrnpp_bop2022_amd.lib.torch_utils.torch_utils import ModelEMA, copy_attr

    class A:
        pass

    src, dst = A(), A()
    src.names, src.stride, src.reducer, src._hidden, src.hyp = ["a"], 32, object(), 1, {"lr": 1}
    copy_attr(dst, src)
    assert vars(dst) == dict(names=["a"], stride=32, reducer=src.reducer, hyp={"lr": 1})          # everything public; nothing is excluded by default
    dst = A()
    copy_attr(dst, src, include=("names", "_hidden"), exclude=("stride",))
    assert vars(dst) == dict(names=["a"])
    dst = A()
    copy_attr(dst, src, exclude=("names", "hyp"))
    assert sorted(vars(dst)) == ["reducer", "stride"]

    model = R.build_tiny()
    ema = ModelEMA(model)
    model.names, model.process_group, model.reducer, model.stride = ["obj"], "pg", "red", 8
    ema.update_attr(model)
    assert ema.ema.names == ["obj"] and ema.ema.stride == 8 and not hasattr(ema.ema, "process_group") and not hasattr(ema.ema, "reducer")
    fresh = ModelEMA(model)
    del fresh.ema.names
    fresh.update_attr(model, include=("names",), exclude=())
    assert fresh.ema.names == ["obj"]


def test_build_model_ema_reads_the_block_with_defaults():
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
    from gdrnpp_bop2022_amd.gdrn_modeling.solver import build_model_ema
    from gdrnpp_bop2022_amd.lib.torch_utils.torch_utils import ModelEMA

    model = R.build_tiny()
    cfg = get_cfg("ycbv_convnext_a6")
    assert build_model_ema(cfg, model) is None                      # no MODEL.EMA block
    cfg.MODEL.EMA = dict(ENABLED=False, INIT_CFG=dict(decay=0.999, updates=0))
    assert build_model_ema(cfg, model) is None
    cfg.MODEL.EMA = dict(ENABLED=True, INIT_CFG=dict(decay=0.999, updates=40))
    ema = build_model_ema(cfg, model)
    assert isinstance(ema, ModelEMA) and ema.updates == 40 and ema.decay(2000) == 0.999 * (1 - math.exp(-1.0)) and hasattr(ema, "update_attr")
    cfg.MODEL.EMA = dict(ENABLED=True)
    ema = build_model_ema(cfg, model)
    assert ema.updates == 0 and ema.decay(2000) == 0.9999 * (1 - math.exp(-1.0))


def _sgd():
    return torch.optim.SGD([nn.Parameter(torch.zeros(1))], lr=1.0)


def test_yolox_lr_scheduler_moves_the_anneal_point_behind_the_warm_up():
    from gdrnpp_bop2022_amd.det.yolox.engine.train_step import yolox_lr_scheduler
    from gdrnpp_bop2022_amd.gdrn_modeling.solver import flat_and_anneal_lr_scheduler

    # the shipped ycbv numbers: 30 epochs, the last 15 without augmentation, 5 of warm-up -> annealing starts at 1/3 of the 15 that count
    epoch = 10
    lr_config = dict(warmup_method="pow", warmup_pow=2, warmup_factor=0.0, anneal_method="cosine", target_lr_factor=0.05)
    train = dict(total_epochs=30, no_aug_epochs=15, warmup_epochs=5, anneal_after_warmup=True, max_iter=30 * epoch, no_aug_iters=15 * epoch,
                 warmup_iters=5 * epoch)
    opt = _sgd()
    sched = yolox_lr_scheduler(opt, lr_config, train)
    _, want = flat_and_anneal_lr_scheduler(_sgd(), total_iters=15 * epoch, warmup_iters=5 * epoch, anneal_point=5 / 15, return_function=True,
                                           **lr_config)
    got = []
    for _ in range(30 * epoch):
        got.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert got == [want(x) for x in range(30 * epoch)]
    assert got[0] == 0.0 and got[25] == 0.25 and got[5 * epoch] == pytest.approx(1.0, abs=1e-12)      # pow-2 warm-up, flat for zero iterations:
    assert got[5 * epoch + 1] < 1.0                                             # the anneal point IS the end of the warm-up
    assert got[15 * epoch] == 0.05 and got[-1] == 0.05                          # the no-augmentation epochs run at the target rate
    # the clamp: a warm-up longer than what is left of the cycle
    train2 = dict(train, warmup_epochs=12, warmup_iters=12 * epoch)
    _, f = flat_and_anneal_lr_scheduler(_sgd(), total_iters=15 * epoch, warmup_iters=12 * epoch, anneal_point=1.0, return_function=True, **lr_config)
    opt2 = _sgd()
    sched2 = yolox_lr_scheduler(opt2, dict(lr_config, anneal_point=0.5), train2)      # 0.5 + 12 / 15 > 1
    seen = []
    for _ in range(16 * epoch):
        seen.append(opt2.param_groups[0]["lr"])
        opt2.step()
        sched2.step()
    assert seen == [f(x) for x in range(16 * epoch)] and seen[15 * epoch - 1] == 1.0 and seen[15 * epoch] == 0.05
    # without the flag the configured point stands
    opt3 = _sgd()
    sched3 = yolox_lr_scheduler(opt3, dict(lr_config, anneal_point=0.5), dict(train, anneal_after_warmup=False))
    _, g = flat_and_anneal_lr_scheduler(_sgd(), total_iters=15 * epoch, warmup_iters=5 * epoch, anneal_point=0.5, return_function=True, **lr_config)
    for x in range(77):
        assert opt3.param_groups[0]["lr"] == g(x), x
        opt3.step()
        sched3.step()
    assert g(74) == 1 and g(76) < 1


def test_yolox_param_groups_list_every_parameter_once_with_its_decay():
    from gdrnpp_bop2022_amd.det.yolox.engine.train_step import yolox_param_groups
    from gdrnpp_bop2022_amd.det.yolox.models import build_yolox

    model = build_yolox(0.33, 0.25, 3)
    groups = yolox_param_groups(model, 5e-4)
    listed = [p for g in groups for p in g["params"]]
    assert len(listed) == len({id(p) for p in listed}) == len(list(model.parameters()))
    assert {id(p) for p in listed} == {id(p) for p in model.parameters()}
    decay_of = {id(p): g["weight_decay"] for g in groups for p in g["params"]}
    assert sorted(g["weight_decay"] for g in groups) == [0.0, 5e-4]
    for mod in model.modules():
        for name, p in mod.named_parameters(recurse=False):
            want = 0.0 if isinstance(mod, nn.BatchNorm2d) or name == "bias" else 5e-4
            assert decay_of[id(p)] == want, (type(mod).__name__, name)
    n_bn = sum(isinstance(m, nn.BatchNorm2d) for m in model.modules())
    n_bias = sum(name == "bias" and not isinstance(m, nn.BatchNorm2d) for m in model.modules() for name, _ in m.named_parameters(recurse=False))
    assert n_bn > 0 and n_bias > 0 and sum(len(g["params"]) for g in groups if g["weight_decay"] == 0.0) == 2 * n_bn + n_bias
    # the three rates apart, a frozen parameter left out, and the result is what an optimiser takes
    model.head.stems[0].conv.weight.requires_grad_(False)
    groups = yolox_param_groups(model, 1e-2, weight_decay_norm=1e-3, weight_decay_bias=1e-4)
    assert sorted(g["weight_decay"] for g in groups) == [1e-4, 1e-3, 1e-2]
    by = {g["weight_decay"]: g["params"] for g in groups}
    assert len(by[1e-3]) == n_bn and len(by[1e-4]) == n_bn + n_bias           # a norm layer's bias takes the bias rate
    assert sum(len(g["params"]) for g in groups) == len(list(model.parameters())) - 1
    torch.optim.SGD(groups, lr=0.1)


def test_header_signature_and_namespace_name_the_kernel():
    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.hip_lib import abi, net

    header = open(os.path.join(ROOT, "include", "gdrnpp_hip.h")).read()
    assert re.search(r"\bint gdrnpp_model_ema_update\(const void\* tensors, int n_tensors, const void\* work, int n_work, float decay, "
                     r"float one_minus_decay,\s+void\* stream\);", header)
    res, args = abi.SIGNATURES["gdrnpp_model_ema_update"]
    assert res is abi.c_int and args == [abi.c_void_p, abi.c_int, abi.c_void_p, abi.c_int, abi.c_float, abi.c_float, abi.c_void_p]
    for name in ("ema_update", "ema_plan", "EmaTables", "ema_tensor_ok", "EMA_TILE", "EMA_TENSOR", "EMA_WORK"):
        assert getattr(hip_lib, name) is getattr(net, name), name
    # the header declares the tables as bytes (its struct and define lists are pinned by older tests): the kernel's source is where the
    # tile and the record layouts are stated, and the Python side's must be the same numbers
    kernel = open(os.path.join(ROOT, "gdrnpp_bop2022_amd", "csrc", "model_ema.hip")).read()
    assert net.EMA_TILE == int(re.search(r"^#define GDRNPP_EMA_TILE (\d+)$", kernel, re.M).group(1)) and net.EMA_TILE % 4 == 0
    for dtype, struct in ((net.EMA_TENSOR, "EmaTensor"), (net.EMA_WORK, "EmaWork")):
        said = re.search(r"static_assert\(sizeof\(%s\) == (\d+)((?: && offsetof\(%s, \w+\) == \d+)+)," % (struct, struct), kernel)
        offsets = {k: int(v) for k, v in re.findall(r"offsetof\(\w+, (\w+)\) == (\d+)", said.group(2))}
        assert dtype.itemsize == int(said.group(1)) and {k: dtype.fields[k][1] for k in dtype.names} == offsets, struct
        members = re.search(r"struct %s \{(.*?)\};" % struct, kernel, re.S).group(1)
        assert tuple(re.findall(r"(\w+);", members)) == dtype.names
    assert [net.EMA_TENSOR[k].itemsize for k in net.EMA_TENSOR.names] == [8, 8, 8] and [net.EMA_WORK[k].itemsize for k in net.EMA_WORK.names] == [8, 4, 4]
    assert f"{net.EMA_TENSOR.itemsize} bytes per pair" in header and f"{net.EMA_WORK.itemsize} bytes per item" in header and f"{net.EMA_TILE} elements" in header


def test_ema_plan_cuts_every_tensor_into_tiles_inside_it():
    from gdrnpp_bop2022_amd.hip_lib import EMA_TILE as T, ema_plan

    numels = [1, 0, T - 1, T, T + 1, 2 * T + 3, 5]
    w = ema_plan(numels)
    assert w["tensor"].tolist() == [0, 2, 3, 4, 4, 5, 5, 5, 6]
    assert w["start"].tolist() == [0, 0, 0, 0, T, 0, T, 2 * T, 0]
    assert w["count"].tolist() == [1, T - 1, T, T, 1, T, T, 3, 5]
    covered = np.zeros(len(numels), np.int64)
    np.add.at(covered, w["tensor"], w["count"])
    assert covered.tolist() == numels and (w["count"] > 0).all() and (w["start"] % 4 == 0).all()
    assert len(ema_plan([])) == 0 and len(ema_plan([0, 0])) == 0
    big = ema_plan([(1 << 31) + 5])          # starts are 64-bit
    assert int(big["start"][-1]) == (1 << 31) and int(big["count"][-1]) == 5 and big["start"].dtype == np.int64
