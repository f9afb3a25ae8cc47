"""The multi-tensor ModelEMA kernel (csrc/model_ema.hip through ``hip_lib.ema_update`` and ``ModelEMA``) on the GPU.

Every comparison is equality of the bits (any NaN equals any NaN).  The oracle is the reference's two statements, ``v *= d; v += (1.0 - d)
* m``, run by torch on CPU copies of the same inputs (tests/model_ema_ref.py ``reference_update``): on fp32 tensors that is
``fadd(fmul(v, float32(d)), fmul(float32(1.0 - d), m))``, which the kernel computes with no contraction.

Cache invalidation (``test_an_updated_ema_is_evaluated_with_its_new_weights``): tried once on an MI355X with the version bump behind the
launch disabled.  The test failed at ``cache_fills() > fills`` (157 > 157: no folded or packed weight was rebuilt).  The second output
did differ from the first even so, because the forward reads some tensors live (not through a cached form), so the assertion that
the outputs differ alone would not have caught it; the fill count did (the comparison with PyTorch's operators behind it was not reached
in that run)."""
import gc
import math

import pytest
import torch
import torch.nn as nn

from tests import model_ema_ref as R

from gdrnpp_bop2022_amd import hip_lib
from gdrnpp_bop2022_amd.det.yolox.utils import ema as E
from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = hip_lib.EMA_TILE
UPDATES = (1, 2000, 10 ** 6)


def decay_at(updates, decay=0.9998):
    return decay * (1 - math.exp(-updates / 2000))


@pytest.fixture(autouse=True)
def _collect_what_the_test_leaves():
    """As tests/test_gpu_ranger.py: pinned staging buffers and device tables go back with the device idle, not in a later test."""
    yield
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def golden():
    return R.Golden()


def randn(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def check_pairs(es, ms, want, where):
    torch.cuda.synchronize()
    for i, (e, w) in enumerate(zip(es, want)):
        assert R.same_bits(e, w), (where, i, tuple(e.shape))


def test_every_size_around_the_tile_and_a_second_call_on_the_same_tables(hip):
    numels = [T + 1, 3, 2 * T + 3, 1, T, 5, T - 1, 4]
    es = [randn(n, 10 + i).to(DEV) for i, n in enumerate(numels)]
    ms = [randn(n, 50 + i).to(DEV) for i, n in enumerate(numels)]
    kept = [m.clone() for m in ms]
    tables = hip.EmaTables(DEV)
    for call, u in enumerate(UPDATES):
        d = decay_at(u)
        want = [R.reference_update(e, m, d) for e, m in zip(es, ms)]
        hip.ema_update(tables, es, ms, d, 1.0 - d)
        check_pairs(es, ms, want, f"updates {u}")
        # the tables went up with the first call; other coefficients are arguments of the launch
        assert (tables.builds, tables.uploads) == (1, 2), (call, tables.builds, tables.uploads)
    assert tables.n_tensors == len(numels) and tables.n_work == sum(-(-n // T) for n in numels)
    assert all(torch.equal(m, k) for m, k in zip(ms, kept))
    tables.close()


@pytest.mark.parametrize("e_off,m_off", [(1, 3), (2, 2), (4, 8)], ids=["4_and_12_bytes_off", "both_8_bytes_off", "views_on_16_bytes"])
def test_views_are_updated_inside_their_bounds(hip, e_off, m_off):
    """``ema = base[e_off:e_off + n]``, ``model = other[m_off:m_off + n]``: the dword path where either is off a 16-byte boundary, the
    16-byte path with a dword tail where both are on one.  Guards in front of and behind the EMA view and the whole model buffer keep
    their bits."""
    sizes = list(range(1, 10)) + [T + 2]
    pad = 16
    bases = [torch.full((n + 2 * pad,), float(100 + n)) for n in sizes]
    others = [torch.full((n + 2 * pad,), float(-100 - n)) for n in sizes]
    for i, n in enumerate(sizes):
        bases[i][e_off:e_off + n] = randn(n, 200 + i)
        others[i][m_off:m_off + n] = randn(n, 300 + i)
    dev_b, dev_o = [b.to(DEV) for b in bases], [o.to(DEV) for o in others]
    assert all(b.data_ptr() % 16 == 0 for b in dev_b + dev_o)
    es = [b[e_off:e_off + n] for b, n in zip(dev_b, sizes)]
    ms = [o[m_off:m_off + n] for o, n in zip(dev_o, sizes)]
    assert all(hip.ema_tensor_ok(e, m) for e, m in zip(es, ms))
    d = decay_at(2000)
    want = [R.reference_update(e, m, d) for e, m in zip(es, ms)]
    tables = hip.EmaTables(DEV)
    hip.ema_update(tables, es, ms, d, 1.0 - d)
    check_pairs(es, ms, want, (e_off, m_off))
    for b, o, b0, o0, n in zip(dev_b, dev_o, bases, others, sizes):
        got = b.cpu()
        assert torch.equal(got[:e_off], b0[:e_off]) and torch.equal(got[e_off + n:], b0[e_off + n:]), n      # the guards
        assert torch.equal(o.cpu(), o0), n                                                                     # the model's buffer
    tables.close()


def test_special_values_in_both_operands(hip):
    """NaN, +-inf, +-0 and 3e38 against each other, on the 16-byte path and, as a view one float off, on the dword path.  No denormals:
    whether torch's CPU kernels flush them is the build's business."""
    vals = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 3e38, -3e38, 1.0, -2.5])
    e0 = vals.repeat_interleave(len(vals))
    m0 = vals.repeat(len(vals))
    for u in UPDATES:
        d = decay_at(u)
        e, m = e0.to(DEV), m0.to(DEV)
        buf_e, buf_m = torch.zeros(len(e0) + 1, device=DEV), torch.zeros(len(e0) + 1, device=DEV)
        buf_e[1:], buf_m[1:] = e0.to(DEV), m0.to(DEV)
        es, ms = [e, buf_e[1:]], [m, buf_m[1:]]
        want = [R.reference_update(x, y, d) for x, y in zip(es, ms)]
        assert torch.isnan(want[0]).any() and torch.isinf(want[0]).any() and (want[0] == 0).any()
        tables = hip.EmaTables(DEV)
        hip.ema_update(tables, es, ms, d, 1.0 - d)
        check_pairs(es, ms, want, f"updates {u}")
        assert R.same_bits(es[0], es[1])
        tables.close()
    # the sign of zero is part of the bits that were compared: -0 d + omd (-0) = -0
    assert math.copysign(1.0, float(R.reference_update(torch.tensor([-0.0]), torch.tensor([-0.0]), 0.5))) == -1.0


def test_many_small_tensors_take_one_launch(hip):
    """300 tensors of 1..40 elements and one of three tiles: one launch, seen by the ``LaunchTimer`` that ``abi.launch`` reports to."""
    numels = [1 + (7 * i) % 40 for i in range(300)] + [3 * T]
    assert set(numels[:300]) == set(range(1, 41))
    es = [randn(n, 1000 + i).to(DEV) for i, n in enumerate(numels)]
    ms = [randn(n, 2000 + i).to(DEV) for i, n in enumerate(numels)]
    d = decay_at(7)
    want = [R.reference_update(e, m, d) for e, m in zip(es, ms)]
    tables = hip.EmaTables(DEV)
    timer = hip.LaunchTimer()
    hip.set_launch_timer(timer)
    try:
        hip.ema_update(tables, es, ms, d, 1.0 - d)
    finally:
        hip.set_launch_timer(None)
    check_pairs(es, ms, want, "many")
    assert [(r[0], r[4]) for r in timer.records] == [("hbm:model_ema", 12.0 * sum(numels))]
    assert tables.n_work == 300 + 3
    tables.close()


def test_arguments_are_checked_before_anything_is_launched(hip):
    e, m = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    tables = hip.EmaTables(DEV)
    hip.ema_update(tables, [], [], 0.5, 0.5)                    # nothing to do
    assert tables.builds == 0
    with pytest.raises(RuntimeError, match="differ in length"):
        hip.ema_update(tables, [e], [], 0.5, 0.5)
    for bad in (m.double(), m.cpu(), torch.ones(16, device=DEV)[::2], torch.ones(4, device=DEV)):
        assert not hip.ema_tensor_ok(e, bad)
        with pytest.raises(RuntimeError, match="pair 0 must be two dense float32 tensors"):
            hip.ema_update(tables, [e], [bad], 0.5, 0.5)
    assert tables.builds == 0 and torch.equal(e.cpu(), torch.zeros(8))
    assert hip.load().gdrnpp_model_ema_update(None, 0, None, 0, 0.5, 0.5, None) == 0          # n_work == 0: success without a launch
    assert hip.load().gdrnpp_model_ema_update(None, 0, None, 3, 0.5, 0.5, None) != 0 and b"work without tables" in hip.load().gdrnpp_last_error()
    assert hip.load().gdrnpp_model_ema_update(None, -1, None, 0, 0.5, 0.5, None) != 0 and b"negative count" in hip.load().gdrnpp_last_error()
    tables.close()


@pytest.mark.parametrize("run", list(R.RUNS))
@pytest.mark.parametrize("decay", R.DECAYS)
@pytest.mark.parametrize("cls", R.CLASSES)
def test_kernel_path_reproduces_the_references_run(hip, golden, cls, decay, run):
    from test_model_ema_cpu import ema_class, follow

    model = R.build_tiny().to(DEV)
    ema = ema_class(cls)(model, decay, updates=R.RUNS[run]["updates"])
    counted = E.torch_path_tensors()
    with torch.cuda.device(DEV):
        follow(golden, ema, model, cls, decay, run)
    steps = R.RUNS[run]["steps"]
    assert E.torch_path_tensors() == counted + steps and "scale64" in E.last_torch_path()        # the fp64 buffer, once per update
    tables = ema._tables[DEV]
    assert (tables.builds, tables.uploads) == (1, 2) and tables.n_tensors == len(R.float_keys(model)) - 1
    assert int(ema.ema.bn.num_batches_tracked) == R.TRACKED_AT_COPY != int(model.bn.num_batches_tracked)
    ema.close()


def test_channels_last_pairs_stay_on_the_kernel_and_differing_layouts_do_not(hip):
    model = nn.Sequential(nn.Conv2d(6, 4, 3)).to(DEV).to(memory_format=torch.channels_last)
    assert not model[0].weight.is_contiguous() and model[0].weight.is_contiguous(memory_format=torch.channels_last)
    ema = E.ModelEMA(model, 0.9998)
    assert ema.ema[0].weight.stride() == model[0].weight.stride() and hip.ema_tensor_ok(ema.ema[0].weight, model[0].weight)
    counted = E.torch_path_tensors()
    with torch.no_grad():
        model[0].weight.add_(randn(model[0].weight.numel(), 5).view_as(model[0].weight).to(DEV))
    want = R.reference_update(ema.ema[0].weight, model[0].weight, ema.decay(1))
    ema.update(model)
    torch.cuda.synchronize()
    assert E.torch_path_tensors() == counted and R.same_bits(ema.ema[0].weight, want)
    assert ema.ema[0].weight.is_contiguous(memory_format=torch.channels_last)
    # the model's weight re-laid out: element i of one is no longer element i of the other in memory, so the torch operators take the pair
    model[0].weight.data = model[0].weight.data.contiguous()
    assert not hip.ema_tensor_ok(ema.ema[0].weight, model[0].weight)
    want = R.reference_update(ema.ema[0].weight, model[0].weight, ema.decay(2))
    want_bias = R.reference_update(ema.ema[0].bias, model[0].bias, ema.decay(2))
    ema.update(model)
    torch.cuda.synchronize()
    assert E.torch_path_tensors() == counted + 1 and "0.weight" in E.last_torch_path()
    assert R.same_bits(ema.ema[0].weight, want) and R.same_bits(ema.ema[0].bias, want_bias)
    ema.close()


def test_a_replaced_parameter_rebuilds_the_tables(hip):
    model = nn.Linear(33, 9).to(DEV)
    ema = E.ModelEMA(model, 0.9998)
    ema.update(model)
    tables = ema._tables[DEV]
    ema.update(model)
    assert (tables.builds, tables.uploads) == (1, 2)
    old = model.weight.data
    model.weight.data = randn(33 * 9, 77).view(9, 33).to(DEV)          # what load_state_dict(assign=True) or a move does
    assert model.weight.data_ptr() != old.data_ptr()
    kept_old = old.clone()
    want = R.reference_update(ema.ema.weight, model.weight, ema.decay(3))
    ema.update(model)
    torch.cuda.synchronize()
    assert (tables.builds, tables.uploads) == (2, 4)
    assert R.same_bits(ema.ema.weight, want) and torch.equal(old, kept_old)
    ema.close()
    assert ema._tables == {}


def _perturb_parameters(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_((1.0 + 0.1 * torch.randn(p.shape, generator=gen)).to(p.device))


@pytest.fixture(scope="module")
def tiny_yolox():
    from tests import conv_bn_bwd_ref as CB

    return CB


def test_model_level_kernel_and_torch_operators_agree_on_every_entry(hip, tiny_yolox):
    model = tiny_yolox.build_model(100).to(DEV)
    on_kernel, on_torch = E.ModelEMA(model, 0.9998), E.ModelEMA(model, 0.9998, use_kernel=False)
    counted = E.torch_path_tensors()
    for step in range(3):
        _perturb_parameters(model, 40 + step)
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.running_mean.add_(0.01 * (step + 1)), m.running_var.mul_(1.0 + 0.01 * (step + 1)), m.num_batches_tracked.add_(1)
        on_kernel.update(model)
        on_torch.update(model)
    torch.cuda.synchronize()
    assert E.torch_path_tensors() == counted          # every floating entry of the detector is the kernel's; use_kernel=False counts nothing
    a, b, src = on_kernel.ema.state_dict(), on_torch.ema.state_dict(), model.state_dict()
    n_float = 0
    for k in a:
        assert R.same_bits(a[k], b[k]), k
        if a[k].dtype.is_floating_point:
            n_float += 1
            assert not torch.equal(a[k], src[k]) or not src[k].any(), k          # an average, not a copy
        else:
            assert int(a[k]) == 0 and int(src[k]) == 3, k
    tables = on_kernel._tables[DEV]
    assert tables.n_tensors == n_float and (tables.builds, tables.uploads) == (1, 2) and on_torch._tables == {}
    on_kernel.close()


def test_an_updated_ema_is_evaluated_with_its_new_weights(hip, tiny_yolox):
    """The kernel writes through raw pointers; ``weight_cache.weight_tag`` keys the folded and packed weights of the HIP forward on the
    tensors' version counters.  ``ModelEMA.update`` advances them behind the launch: without that the second forward serves the weights
    of before the update."""
    model = tiny_yolox.build_model(100).to(DEV)
    ema = E.ModelEMA(model, 0.9998)
    x = randn(3 * 64 * 96, 9).view(1, 3, 64, 96).to(DEV)
    assert hip_layers.is_enabled()
    foreign = hip_layers.fallback_launches()
    with torch.no_grad():
        first = ema.ema(x)["det_preds"].clone()
    fills = hip_layers.cache_fills()
    assert fills > 0 and hip_layers.fallback_launches() == foreign, hip_layers.last_fallback()
    _perturb_parameters(model, 3)
    ema.update(model)          # d = 0.9998 (1 - exp(-1 / 2000)): the average all but takes the perturbed weights
    with torch.no_grad():
        second = ema.ema(x)["det_preds"].clone()
    torch.cuda.synchronize()
    assert not torch.equal(first, second), "the forward after the update is the forward before it: stale derived weights"
    assert hip_layers.cache_fills() > fills and hip_layers.fallback_launches() == foreign
    hip_layers.set_enabled(False)
    try:
        with torch.no_grad():
            want = ema.ema(x)["det_preds"]
    finally:
        hip_layers.set_enabled(True)
    # the bar of tests/test_gpu_yolox_net.py::test_disabled_hip_layers_take_the_operator_path_and_agree
    err_scores, err_boxes = float((second[..., 4:] - want[..., 4:]).abs().max()), float((second[..., :4] - want[..., :4]).abs().max())
    moved = float((first[..., 4:] - want[..., 4:]).abs().max())
    print(f"EMA forward after the update against PyTorch's operators: scores {err_scores:.3e} boxes {err_boxes:.3e}; the update moved the scores by {moved:.3e}")
    assert torch.isfinite(second).all() and err_scores < 1e-4 and err_boxes < 1e-2
    assert moved > 1e-3, "the perturbation is too small for the bar to tell the two sets of weights apart"
    ema.close()


def _train_once(CB, seed):
    from gdrnpp_bop2022_amd.det.yolox.engine.train_step import YoloxTrainStep, yolox_param_groups
    from gdrnpp_bop2022_amd.gdrn_modeling.solver import Ranger

    model = CB.build_model(seed).to(DEV)
    x, targets = CB.model_inputs(seed)
    opt = Ranger(yolox_param_groups(model, 0), lr=1e-3)
    step = YoloxTrainStep(model, opt, ema_decay=0.9998)
    e0 = {k: v.detach().clone() for k, v in step.ema.ema.state_dict().items()}
    p0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    _, loss_dict = step.run_step(x.to(DEV), targets.to(DEV))
    torch.cuda.synchronize()
    return step, e0, p0, {k: float(v.detach()) for k, v in loss_dict.items()}


def test_training_step_updates_the_ema_behind_the_optimiser_and_repeats(hip, tiny_yolox):
    CB = tiny_yolox
    assert CB.MODEL_INPUT == (2, 3, 64, 96)
    hip_layers.set_train_kernels(True)
    try:
        step, e0, p0, losses = _train_once(CB, 100)
        again, _, _, losses2 = _train_once(CB, 100)
    finally:
        hip_layers.set_train_kernels(False)
    assert all(math.isfinite(v) for v in losses.values()) and losses == losses2
    assert step.ema.updates == 1 and step.iter == 1 and step.eval_model is step.ema.ema and not step.eval_model.training
    d = step.ema.decay(1)
    after, ema = step.model.state_dict(), step.ema.ema.state_dict()
    moved = 0
    for k, v in ema.items():
        if v.dtype.is_floating_point:
            assert R.same_bits(v, R.reference_update(e0[k], after[k], d)), k                          # the state BEHIND the optimiser's step
            if not torch.equal(after[k], p0[k]):
                moved += 1
                assert not R.same_bits(v, R.reference_update(e0[k], p0[k], d)) or not after[k].any(), k      # ... not the one in front of it
        else:
            assert torch.equal(v, e0[k]) and int(after[k]) == int(p0[k]) + 1, k
    assert moved >= len(list(step.model.parameters())) // 2, moved
    for k, v in again.model.state_dict().items():
        assert R.same_bits(v, after[k]), k
    for k, v in again.ema.ema.state_dict().items():
        assert R.same_bits(v, ema[k]), k
    assert not hip_layers.train_kernels()
