"""The Ranger step restated in NumPy (fp64 the yardstick of the GPU tests, fp32 the format's own error), the case tables shared with
tests/golden/make_golden_ranger.py, and the loader of tests/golden/ranger_golden.npz.

Per tensor with a gradient g, step count t (after the increment), group lr / weight_decay, betas (b1, b2), eps, alpha, k:
    g   -= mean of g over all dimensions but the first          where g.ndim > 1 (> 3 with gc_conv_only)
    v    = v b2 + ((1 - b2) g) g;     m = m b1 + (1 - b1) g
    p   += (-weight_decay lr) p                                 where weight_decay != 0
    N_sma, step_size = radam(t);  p += (-step_size lr) (m / (sqrt(v) + eps)) where N_sma > threshold, else p += (-step_size lr) m
    slow += alpha (p - slow), p = slow                          where t % k == 0
Scalars are formed in Python floats and then rounded to the working type, as a torch kernel receives them.

The fp32 mode is bit-reproducible: the elementwise operations are single IEEE roundings and a row mean is the correctly rounded sum
(``math.fsum``) divided in fp64 and rounded once.  The fixture stores the reference's fp32 states as integer distances (in units of the last
place) from this restatement's fp32 step taken from the reference's previous fp32 state, which are almost all zero and so cost nothing
to store; ``Golden`` adds them back and checks a recorded checksum of every decoded array."""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20221020
STEPS = 13
GROUPS = (dict(lr=8e-4, weight_decay=0.01), dict(lr=4e-4, weight_decay=0))
# name -> (shape, group)
TENSORS = {
    "v1": ((1,), 1), "v3": ((3,), 0), "v5": ((5,), 1),                    # no centralisation, tails shorter than a vector
    "dw": ((6, 1, 7, 7), 0),                                              # 49-element rows at odd offsets
    "fc": ((8, 130), 0), "one_row": ((1, 257), 1), "conv": ((5, 3, 3, 3), 0),
    "col": ((7, 1), 1),                                                   # rows of one element: the centralised gradient is zero
    "never": ((4, 6), 0),                                                 # never receives a gradient
    "skip4": ((3, 7), 1),                                                 # misses its gradient at step 4 only
}
VARIANTS = {
    "default": {},
    "gc_conv_only": dict(gc_conv_only=True),
    "no_gc": dict(use_gc=False),
    "k1": dict(k=1, alpha=0.3),
    "thr4": dict(N_sma_threshhold=4),
}
DEFAULTS = dict(alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999), eps=1e-5, gc_conv_only=False)
QUANTITIES = ("p", "m", "v", "slow")
FULL64_STEPS = {"default": (5, 6, 12, 13)}        # steps whose fp64 p, m, v are recorded in full; the other variants: step 13
CHECK_STEPS = (5, 6, 12, 13)


def numel(name):
    return int(np.prod(TENSORS[name][0]))


TOTAL = sum(int(np.prod(s)) for s, _ in TENSORS.values())


def span(name):
    """Where ``name``'s elements sit in the fixture's flat vectors (the tensors one behind the other in table order)."""
    names = list(TENSORS)
    start = sum(numel(n) for n in names[:names.index(name)])
    return slice(start, start + numel(name))


def has_grad(name, step):
    return name != "never" and not (name == "skip4" and step == 4)


def seeded_params():
    rng = np.random.default_rng([SEED, 0])
    return {n: (rng.standard_normal(shape) * 0.5).astype(np.float32) for n, (shape, _) in TENSORS.items()}


def seeded_grads():
    """{step: {name: f32 gradient}}: a common offset and a per-row offset, so that centralisation matters, on noise of a few scales."""
    out = {}
    for t in range(1, STEPS + 1):
        rng = np.random.default_rng([SEED, t])
        out[t] = {}
        for n, (shape, _) in TENSORS.items():
            g = rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, -1) + 0.02
            g += rng.standard_normal((shape[0],) + (1,) * (len(shape) - 1)) * 0.01
            if has_grad(n, t):
                out[t][n] = g.astype(np.float32)
    return out


def radam(step, beta1, beta2, threshold):
    beta2_t = beta2 ** step
    n_max = 2 / (1 - beta2) - 1
    n_sma = n_max - 2 * step * beta2_t / (1 - beta2_t)
    if n_sma > threshold:
        size = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - beta1 ** step)
    else:
        size = 1.0 / (1 - beta1 ** step)
    return n_sma, size


def row_means(g, dtype):
    rows = g.reshape(g.shape[0], -1)
    if dtype == np.float64:
        return rows.mean(axis=1).reshape((g.shape[0],) + (1,) * (g.ndim - 1))
    mu = np.array([math.fsum(float(x) for x in r) / rows.shape[1] for r in rows], dtype=np.float64).astype(dtype)
    return mu.reshape((g.shape[0],) + (1,) * (g.ndim - 1))


def ranger_step_ref(p, m, v, slow, g, step, lr, weight_decay, dtype=np.float64, nan_to_num=False, **kw):
    """One step of one tensor in ``dtype`` -> (p, m, v, slow), new arrays.  ``step`` is the count after the increment."""
    o = dict(DEFAULTS, **{k: x for k, x in kw.items() if k in DEFAULTS})
    T = np.dtype(dtype).type
    p, m, v, slow, g = (np.array(a, dtype=dtype) for a in (p, m, v, slow, g))
    if nan_to_num:
        g = np.nan_to_num(g, nan=0.0, posinf=1e5, neginf=-1e5).astype(dtype)
    b1, b2 = o["betas"]
    if g.ndim > (3 if o["gc_conv_only"] else 1):
        g = g - row_means(g, dtype)
    v = v * T(b2) + (T(1 - b2) * g) * g
    m = m * T(b1) + T(1 - b1) * g
    n_sma, size = radam(step, b1, b2, o["N_sma_threshhold"])
    if weight_decay != 0:
        p = p + T(-weight_decay * lr) * p
    if n_sma > o["N_sma_threshhold"]:
        p = p + T(-size * lr) * (m / (np.sqrt(v) + T(o["eps"])))
    else:
        p = p + T(-size * lr) * m
    if step % o["k"] == 0:
        slow = slow + T(o["alpha"]) * (p - slow)
        p = slow.copy()
    assert p.dtype == m.dtype == v.dtype == slow.dtype == np.dtype(dtype)
    return p, m, v, slow


def fresh_state(p, dtype=np.float64):
    p = np.array(p, dtype=dtype)
    return dict(p=p, m=np.zeros_like(p), v=np.zeros_like(p), slow=p.copy(), step=0)


def step_all(states, grads_t, variant, dtype=np.float64, nan_to_num=False):
    """One optimiser step over {name: state dict} with the gradients {name: g} of one iteration -> new {name: state}.  A tensor without a
    gradient keeps its state object (and ``None`` while it never had one)."""
    out = {}
    for n, st in states.items():
        g = grads_t.get(n)
        if g is None:
            out[n] = st
            continue
        grp = GROUPS[TENSORS[n][1]] if n in TENSORS else GROUPS[0]
        p, m, v, slow = ranger_step_ref(st["p"], st["m"], st["v"], st["slow"], g, st["step"] + 1, grp["lr"], grp["weight_decay"], dtype=dtype,
                                        nan_to_num=nan_to_num, **VARIANTS.get(variant, {}))
        out[n] = dict(p=p, m=m, v=v, slow=slow, step=st["step"] + 1)
    return out


def trajectory64(variant):
    """[state after step t for t in 0..STEPS] of the fp64 restatement on the seeded inputs cast up."""
    grads = seeded_grads()
    states = [{n: fresh_state(p) for n, p in seeded_params().items()}]
    for t in range(1, STEPS + 1):
        states.append(step_all(states[-1], grads[t], variant))
    return states


def ulp_of_max(a):
    """One fp32 unit in the last place at the largest magnitude of ``a``."""
    return float(np.spacing(np.float32(np.abs(np.asarray(a, dtype=np.float64)).max())))


def checksum(a):
    return int(np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64).sum())


class Golden:
    """tests/golden/ranger_golden.npz.  ``state32(variant, t)`` -> {name: state dict} of the reference's fp32 run after step t (t = 0: the
    seeded parameters, no moments); ``err(kind, variant, t, name)`` -> {quantity: float} for kind in ("traj32_err", "step32_err")."""

    def __init__(self, path=None):
        self.z = np.load(path or os.path.join(HERE, "golden", "ranger_golden.npz"))
        self.meta = json.loads(str(self.z["meta"]))
        self.params = {n: self.z["param"][span(n)].reshape(TENSORS[n][0]) for n in TENSORS}
        self.grads = {t: {n: self.z["grad"][t - 1][span(n)].reshape(TENSORS[n][0]) for n in TENSORS if has_grad(n, t)} for t in range(1, STEPS + 1)}
        self._s32 = {}

    def state32(self, variant, t):
        key = (variant, t)
        if key not in self._s32:
            if t == 0:
                self._s32[key] = {n: dict(fresh_state(p, np.float32)) for n, p in self.params.items()}
            else:
                pred = step_all(self.state32(variant, t - 1), self.grads[t], variant, dtype=np.float32)
                out = {}
                for i, (n, st) in enumerate(pred.items()):
                    new = dict(step=st["step"])
                    for j, q in enumerate(QUANTITIES):
                        d = self.z[f"{variant}/d32"][t - 1, j][span(n)].reshape(st[q].shape)
                        new[q] = (st[q].view(np.int32) + d).view(np.float32)
                        if checksum(new[q]) != int(self.z[f"{variant}/sum32"][t - 1, i, j]):
                            raise AssertionError(f"ranger_golden.npz: fp32 state {variant} step {t} {n}.{q} does not decode to its checksum")
                    out[n] = new
                self._s32[key] = out
        return self._s32[key]

    def err(self, kind, variant, t, name):
        return dict(zip(QUANTITIES, (float(x) for x in self.z[f"{variant}/{kind}"][t - 1, list(TENSORS).index(name)])))

    def full64(self, variant, t, name):
        k = self.meta["full64_steps"][variant].index(t)
        return {q: self.z[f"{variant}/s64"][k, j][span(name)].reshape(TENSORS[name][0]) for j, q in enumerate(("p", "m", "v"))}

    def sums64(self, variant, t, name):
        """f64[4, 2]: per quantity the sum and the sum of squares of the reference's fp64 state."""
        return self.z[f"{variant}/sum64"][t - 1, list(TENSORS).index(name)]

    def steps(self, variant, t):
        return dict(zip(TENSORS, (int(x) for x in self.z[f"{variant}/steps"][t - 1])))
