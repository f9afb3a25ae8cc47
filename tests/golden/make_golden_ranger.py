"""Golden Ranger steps and ``flat_and_anneal`` factors from the reference's OWN code (authoring container only: needs /root/reference).

``lib/torch_utils/solver/ranger.py`` and ``lib/torch_utils/solver/lr_scheduler.py`` are executed from their path, unmodified; both import
only the standard library and torch at module level.  The fp64 run needs one shim: the reference's ``step()`` casts parameter and gradient
with ``.float()``, so during that run ``torch.Tensor.float`` is replaced by ``.double()`` — the same statements then carry fp64.

The cases are tests/ranger_ref.py's tables: ten small tensors in two parameter groups, 13 steps of seeded gradients (steps 1-5 unrectified,
6 the first rectified step and first Lookahead, 12 the second Lookahead, 13 the step behind it), one tensor that never has a gradient and
one that misses step 4, five variants.  Recorded in ranger_golden.npz:

    param f32[N], grad f32[13, N]                 the seeded fp32 inputs, the tensors flattened one behind the other in table order (N = all elements)
    <variant>/d32 i32[13, 4, N]                   the reference's fp32 state after step t (p, m, v, slow) as the integer distance, in units of the
                                                  last place, from ranger_ref's bit-reproducible fp32 step taken from the reference's fp32 state
                                                  after step t-1 (mostly zeros); <variant>/sum32 i64[13, tensors, 4]: a checksum of every state
    <variant>/s64 f64[steps, 3, N]                the fp64 run's p, m, v in full (default: steps 5, 6, 12, 13; other variants: step 13)
    <variant>/sum64 f64[13, tensors, 4, 2]        every step: per quantity the sum and the sum of squares of the fp64 state
    <variant>/traj32_err f64[13, tensors, 4]      max |fp32 run - fp64 run|: the reference's own fp32 distance from fp64
    <variant>/step32_err f64[13, tensors, 4]      max |one fp32 step - one fp64 step|, both from the fp32 state after step t-1
    <variant>/steps i64[13, tensors]              state["step"] per tensor (-1: no state)
    <variant>/radam f64[13, 2]                    N_sma and step_size per step
    sched f64[4 warm-ups, 6 anneals, plain | cyclic, 60]   the factor of every iteration of a 50-iteration schedule with 10 warm-up iterations
    state7/param_groups, state7/ids               the reference's ``state_dict()`` after step 7 of the default variant: its groups and state keys
                                                  (the tensors are the fp32 state of step 7)

meta records the torch version and CPU capability (``torch.backends.cpu.get_cpu_capability()``) of the fp32 run: where both are the
installed ones, tests/test_ranger_cpu.py holds the torch-operator path to the fp32 states bit for bit.

The full fp64 and fp32 states of every step would be some 6 MB; the distances and checksums keep the file at a few hundred KB."""
import contextlib
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from tests import ranger_ref as R  # noqa: E402

REF = "/root/reference"
SCHED_TOTAL, SCHED_WARMUP, SCHED_ITERS = 50, 10, 60
WARMUPS = ("constant", "linear", "pow", "exp")
ANNEALS = ("cosine", "linear", "poly", "exp", "step", "none")


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@contextlib.contextmanager
def float_is_double():
    orig = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        yield
    finally:
        torch.Tensor.float = orig


def build(Ranger, variant, dtype, states=None):
    """The reference's optimiser over the tensors (two groups, in table order inside each), optionally with the per-tensor state set."""
    params = {n: torch.nn.Parameter(torch.from_numpy(np.array((states[n]["p"] if states else R.seeded_params()[n]), dtype=dtype))) for n in R.TENSORS}
    groups = [dict(params=[params[n] for n, (_, g) in R.TENSORS.items() if g == gi], **grp) for gi, grp in enumerate(R.GROUPS)]
    opt = Ranger(groups, **R.VARIANTS[variant])
    if states:
        for n, st in states.items():
            if st["step"] > 0:
                opt.state[params[n]] = dict(step=st["step"], exp_avg=torch.from_numpy(np.array(st["m"], dtype=dtype)),
                                            exp_avg_sq=torch.from_numpy(np.array(st["v"], dtype=dtype)),
                                            slow_buffer=torch.from_numpy(np.array(st["slow"], dtype=dtype)))
    return opt, params


def snapshot(opt, params):
    out = {}
    for n, p in params.items():
        st = opt.state.get(p, {})
        if st:
            out[n] = dict(p=p.detach().numpy().copy(), m=st["exp_avg"].numpy().copy(), v=st["exp_avg_sq"].numpy().copy(),
                          slow=st["slow_buffer"].numpy().copy(), step=int(st["step"]))
        else:
            out[n] = dict(R.fresh_state(p.detach().numpy(), p.detach().numpy().dtype))
    return out


def one_step(opt, params, grads_t, dtype):
    for n, p in params.items():
        p.grad = torch.from_numpy(np.array(grads_t[n], dtype=dtype)) if n in grads_t else None
    if dtype == np.float64:
        with float_is_double():
            opt.step()
    else:
        opt.step()


def run(Ranger, variant, dtype, grads):
    opt, params = build(Ranger, variant, dtype)
    traj = [snapshot(opt, params)]
    for t in range(1, R.STEPS + 1):
        one_step(opt, params, grads[t], dtype)
        traj.append(snapshot(opt, params))
        for n, st in traj[-1].items():
            assert all(st[q].dtype == dtype for q in R.QUANTITIES), (n, dtype)
    return traj, opt


def main():
    ranger = load("lib/torch_utils/solver/ranger.py", "ref_ranger")
    sched = load("lib/torch_utils/solver/lr_scheduler.py", "ref_lr_scheduler")
    grads, params0 = R.seeded_grads(), R.seeded_params()
    names, nq, T = list(R.TENSORS), len(R.QUANTITIES), R.STEPS

    def flat(per_name, dtype):          # {name: array} -> one vector in table order, zeros where a tensor is absent
        return np.concatenate([np.asarray(per_name[n], dtype=dtype).reshape(-1) if n in per_name else np.zeros(R.numel(n), dtype) for n in names])

    out = {"param": flat(params0, np.float32), "grad": np.stack([flat(grads[t], np.float32) for t in range(1, T + 1)])}
    nonzero = total = 0
    for variant in R.VARIANTS:
        t32, _ = run(ranger.Ranger, variant, np.float32, grads)
        t64, _ = run(ranger.Ranger, variant, np.float64, grads)
        kw = dict(R.DEFAULTS, **{k: v for k, v in R.VARIANTS[variant].items() if k in R.DEFAULTS})
        out[f"{variant}/radam"] = np.array([R.radam(t, *kw["betas"], kw["N_sma_threshhold"]) for t in range(1, T + 1)])
        d32 = np.zeros((T, nq, R.TOTAL), np.int32)
        sum32 = np.zeros((T, len(names), nq), np.int64)
        sum64 = np.zeros((T, len(names), nq, 2))
        traj_err, step_err = np.zeros((T, len(names), nq)), np.zeros((T, len(names), nq))
        steps = np.zeros((T, len(names)), np.int64)
        full_steps = R.FULL64_STEPS.get(variant, (T,))
        s64 = np.zeros((len(full_steps), 3, R.TOTAL))
        for t in range(1, T + 1):
            pred = R.step_all(t32[t - 1], grads[t], variant, dtype=np.float32)
            opt1, params1 = build(ranger.Ranger, variant, np.float64, states=t32[t - 1])       # one fp64 step from the fp32 state
            one_step(opt1, params1, grads[t], np.float64)
            s1 = snapshot(opt1, params1)
            for i, n in enumerate(names):
                a32, a64 = t32[t][n], t64[t][n]
                assert a32["step"] == a64["step"] == s1[n]["step"]
                steps[t - 1, i] = a32["step"] if a32["step"] else -1
                for j, q in enumerate(R.QUANTITIES):
                    sum64[t - 1, i, j] = a64[q].sum(), (a64[q] ** 2).sum()
                    traj_err[t - 1, i, j] = np.abs(a32[q].astype(np.float64) - a64[q]).max()
                    step_err[t - 1, i, j] = np.abs(a32[q].astype(np.float64) - s1[n][q]).max()
                    sum32[t - 1, i, j] = R.checksum(a32[q])
                    if n in grads[t]:
                        d = a32[q].view(np.int32).astype(np.int64) - pred[n][q].view(np.int32).astype(np.int64)
                        assert np.abs(d).max() < 2 ** 31
                        nonzero, total = nonzero + int((d != 0).sum()), total + d.size
                        d32[t - 1, j, R.span(n)] = d.reshape(-1)
                    else:
                        assert np.array_equal(a32[q], pred[n][q])
            if t in full_steps:
                for j, q in enumerate(("p", "m", "v")):
                    s64[full_steps.index(t), j] = flat({n: t64[t][n][q] for n in names}, np.float64)
        out.update({f"{variant}/d32": d32, f"{variant}/sum32": sum32, f"{variant}/sum64": sum64, f"{variant}/traj32_err": traj_err,
                    f"{variant}/step32_err": step_err, f"{variant}/steps": steps, f"{variant}/s64": s64})
        if variant == "default":          # the reference-side state_dict after step 7: load_state_dict of it must continue to step 8
            opt, params = build(ranger.Ranger, variant, np.float32, states=t32[7])
            sd = opt.state_dict()
            out["state7/param_groups"] = np.array(json.dumps([{k: (list(v) if isinstance(v, tuple) else v) for k, v in g.items()} for g in sd["param_groups"]]))
            out["state7/ids"] = np.array(sorted(sd["state"]), np.int64)
    # the schedule
    table = np.zeros((len(WARMUPS), len(ANNEALS), 2, SCHED_ITERS))
    for a, wm in enumerate(WARMUPS):
        for b, am in enumerate(ANNEALS):
            for cyclic in (False, True):
                p = torch.nn.Parameter(torch.zeros(1))
                o = torch.optim.SGD([p], lr=1.0)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    _, f = sched.flat_and_anneal_lr_scheduler(o, total_iters=SCHED_TOTAL, warmup_iters=SCHED_WARMUP, warmup_factor=0.1, warmup_method=wm,
                                                              anneal_method=am, anneal_point=0.72, target_lr_factor=0.05, poly_power=0.9,
                                                              step_gamma=0.1, steps=[0.5, 0.75], cyclic=cyclic, return_function=True)
                table[a, b, int(cyclic)] = [float(f(x)) for x in range(SCHED_ITERS)]
    out["sched"] = table
    out["meta"] = np.array(json.dumps(dict(variants=list(R.VARIANTS), tensors={n: list(s) for n, (s, _) in R.TENSORS.items()}, steps=T, seed=R.SEED,
                                            full64_steps={v: list(R.FULL64_STEPS.get(v, (T,))) for v in R.VARIANTS},
                                            sched=dict(warmups=WARMUPS, anneals=ANNEALS, iters=SCHED_ITERS,
                                                       kwargs=dict(total_iters=SCHED_TOTAL, warmup_iters=SCHED_WARMUP, warmup_factor=0.1, anneal_point=0.72,
                                                                   target_lr_factor=0.05, poly_power=0.9, step_gamma=0.1, steps=[0.5, 0.75])),
                                            d32_nonzero=nonzero, d32_total=total,
                                            torch_version=torch.__version__, cpu_capability=torch.backends.cpu.get_cpu_capability())))
    path = os.path.join(HERE, "ranger_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", nonzero, "of", total, "fp32 values differ from the restatement's fp32 step")


if __name__ == "__main__":
    main()
