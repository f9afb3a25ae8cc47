"""Host-side oracle of the split GEMMs with NO tolerance (pure torch on the CPU; tests/test_split_lattice_cpu.py checks it
where there is no GPU, tests/test_gpu_split_exact.py compares the kernels with it through torch.equal).

The three-product scheme (csrc/gemm_split2_pipe.hip) writes x = h + l with h = rn_f16(x), l = rn_f16(x - h), scales the weight by
2^e (max|w| * 2^e in [2^13, 2^14), split2_common.hpp: weight_exp) and accumulates hA*lW + lA*hW + hA*hW in fp32; lA*lW is
dropped.  On the lattices below every partial product and every partial sum of that scheme is an integer multiple of one
granularity g with magnitude below 2^24 g, i.e. exactly representable in fp32: the result is ONE bit pattern whatever order the
MFMAs add in.  A dropped, doubled or stale k-tile, a swapped h / l plane, a wrong LDS slot or a row of the wrong image changes
integers in the output.

  int_lattice   small integers: l = 0 on both sides, three and six products are exact, the expected value is the plain product;
  hl_lattice    p + q 2^-12, p in {+-2, +-3}, q in {-2 .. 2} (and exact zeros): h = p, l = q 2^-12 (a NORMAL fp16 number), the
                weight scale is exactly 2^12, so the l planes of BOTH operands are non-zero.  (p = +-1 would not do: 1 - 2^-11 is
                an fp16 number, h would absorb the fraction.)  Rows have rms >= 2: no range word;
  fine_lattice  +-(1 + c 2^-9 + d 2^-17): fills the m and l planes of the SIX-product (bf16 x 3) split of one operand.

The fused ConvNeXt MLP (csrc/gemm_mlp_fused.hip; tests/test_gpu_mlp_fused_exact.py) is two such GEMMs around a GELU: its section at
the end of this file says on which inputs the GELU is exact as well, and builds them.

Every ``*_expected`` function asserts its exactness precondition on the actual operands before it returns (AssertionError: the
inputs are no lattice for this K), so a test built on it cannot pass or fail by rounding."""
import functools
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
LIMIT = 2.0 ** 24


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


# ---- lattices ----------------------------------------------------------------------------------------------------------------
def int_lattice(shape, vmax, zero_frac, gen):
    """f32 integers in [-vmax, vmax], a fraction ``zero_frac`` of them forced to zero."""
    v = torch.randint(-vmax, vmax + 1, tuple(shape), generator=gen).float()
    v[torch.rand(tuple(shape), generator=gen) < zero_frac] = 0.0
    return v


def hl_lattice(shape, gen, zero_frac=0.125):
    """f32 values p + q 2^-12 with p in {+-2, +-3}, q in {-2 .. 2}; a fraction ``zero_frac`` of exact zeros."""
    shape = tuple(shape)
    p = torch.randint(2, 4, shape, generator=gen).double() * (torch.randint(0, 2, shape, generator=gen).double() * 2 - 1)
    q = torch.randint(-2, 3, shape, generator=gen).double()
    v = p + q * 2.0 ** -12
    v[torch.rand(shape, generator=gen) < zero_frac] = 0.0
    return v.float()


def fine_lattice(shape, gen):
    """f32 values +-(1 + c 2^-9 + d 2^-17), c, d in {0, 1}: 18 significant bits, more than two bf16 planes hold."""
    shape = tuple(shape)
    s = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    c, d = (torch.randint(0, 2, shape, generator=gen).double() for _ in range(2))
    return (s * (1 + c * 2.0 ** -9 + d * 2.0 ** -17)).float()


def lattice(kind, shape, gen, zero_frac=None):
    if kind == "hl":
        return hl_lattice(shape, gen, 0.125 if zero_frac is None else zero_frac)
    assert kind == "int", kind
    return int_lattice(shape, 5, 0.25 if zero_frac is None else zero_frac, gen)


# ---- the scheme on the host ----------------------------------------------------------------------------------------------------
def granularity(*tensors):
    """The largest power of two of which every element of every tensor is an integer multiple (inf when all are zero)."""
    g = math.inf
    for t in tensors:
        t = t.double().reshape(-1)
        t = t[t != 0]
        if t.numel():
            m, e = torch.frexp(t)
            mi = (m.abs() * 2.0 ** 53).long()
            g = min(g, torch.ldexp((mi & -mi).double(), e - 53).min().item())
    return g


def weight_exp(w):
    """e of split2_common.hpp: max|w| * 2^e in [2^13, 2^14)."""
    amax = float(w.abs().max())
    if amax == 0.0:
        return 0
    return max(-110, min(110, 13 - (math.frexp(amax)[1] - 1)))


def split_f16(x):
    """(h, l) in float64 of an f32-representable tensor: h = rn_f16(x), l = rn_f16(x - h)."""
    x32 = x.float()
    assert torch.equal(x32.double(), x.double()), "operand is not an fp32 tensor"
    h = x32.half()
    assert torch.isfinite(h).all(), "operand beyond the fp16 range"
    l = (x32 - h.float()).half()
    return h.double(), l.double()


def _f32_exact(t, what):
    assert torch.equal(t.float().double(), t), f"{what} does not round-trip through float32"


def _assert_sums_exact(terms, op, what):
    """terms: (a, w) plane pairs whose op(a, w) the kernel accumulates in one fp32 accumulator, in any order."""
    g, bound = math.inf, 0.0
    for a, w in terms:
        ga, gw = granularity(a), granularity(w)
        if math.isinf(ga) or math.isinf(gw):
            continue
        g = min(g, ga * gw)
        bound = bound + op(a.abs(), w.abs())
    if math.isinf(g):
        return
    worst = float(bound.max()) / g
    assert worst * (1 + 2.0 ** -6) < LIMIT, f"{what}: partial sums reach {worst:.4g} units of the finest term, 2^24 = {LIMIT:.4g} is the end of exact fp32"


def _epilogue(v, bias, gamma, resid, bias_dim):
    if bias is not None:
        shape = [1] * v.dim()
        shape[bias_dim] = -1
        v = v + bias.double().reshape(shape)
    _f32_exact(v, "accumulator * 2^-e + bias")
    if gamma is not None:
        gv = gamma.double() * v
        _f32_exact(gv, "gamma * v")
        v = resid.double() + gv
    _f32_exact(v, "result")
    return v


def _linear(a, w):
    return a @ w.t()


def three_product_planes(A, W):
    """((hA, lA), (hW, lW), e): the fp16 planes of A and of W * 2^e in float64, reconstruction asserted."""
    e = weight_exp(W)
    ws = W.double() * 2.0 ** e
    hA, lA = split_f16(A)
    hW, lW = split_f16(ws)
    assert torch.equal(hA + lA, A.double()), "A is not h + l: outside the lattice"
    assert torch.equal(hW + lW, ws), "W * 2^e is not h + l: outside the lattice"
    return (hA, lA), (hW, lW), e


def three_product_op(A, W, op, bias=None, gamma=None, resid=None, bias_dim=-1):
    """What the three-product kernels must store for the bilinear ``op`` (matmul, convolution, transposed convolution), float64.
    Differs from op(A, W) in float64 by the dropped lA * lW term: that is the scheme, not an error."""
    (hA, lA), (hW, lW), e = three_product_planes(A, W)
    _assert_sums_exact([(hA, lW), (lA, hW), (hA, hW)], op, "three products")
    acc = op(hA, lW) + op(lA, hW) + op(hA, hW)
    _f32_exact(acc, "accumulator")
    return _epilogue(acc * 2.0 ** -e, bias, gamma, resid, bias_dim)


def three_product_expected(A, W, bias=None, gamma=None, resid=None):
    """Linear form: A f32[M, K], W f32[N, K] -> float64[M, N] = resid + gamma * ((hA lW^T + lA hW^T + hA hW^T) 2^-e + bias)."""
    return three_product_op(A, W, _linear, bias, gamma, resid)


def dropped_ll_term(A, W, op=_linear):
    """lA * lW (unscaled): op(A, W) in float64 minus the three-product value."""
    (_, lA), (_, lW), e = three_product_planes(A, W)
    return op(lA, lW) * 2.0 ** -e


def conv_op(stride, pad):
    return lambda x, w: F.conv2d(x, w, None, stride=stride, padding=pad)


def deconv_op(stride, pad, out_pad):
    return lambda x, w: F.conv_transpose2d(x, w, None, stride=stride, padding=pad, output_padding=out_pad)


def three_product_conv_expected(x, w, bias, stride, pad):
    """x f32[n, Cin, H, W], w f32[Cout, Cin, KH, KW] -> float64 NCHW, three F.conv2d calls on the emulated planes."""
    return three_product_op(x, w, conv_op(stride, pad), bias, bias_dim=1)


def three_product_deconv_expected(x, w, bias, stride, pad, out_pad):
    """w f32[Cin, Cout, KS, KS] (nn.ConvTranspose2d): GEMM + col2im, every sum of the gather exact as well."""
    return three_product_op(x, w, deconv_op(stride, pad, out_pad), bias, bias_dim=1)


def exact_product_expected(A, W, op=_linear, bias=None, gamma=None, resid=None, bias_dim=-1):
    """op(A, W) in float64 for operands on which the SIX-product (bf16 x 3) kernels are exact: every plane of x = h + m + l is
    a multiple of x's granularity, so every partial product is a multiple of gA * gW and every partial sum — of any plane pair, of
    a split-K chunk, of the fixed-order reduce — is bounded by |A| |W|."""
    _assert_sums_exact([(A.double(), W.double())], op, "six products")
    acc = op(A.double(), W.double())
    _f32_exact(acc, "accumulator")
    return _epilogue(acc, bias, gamma, resid, bias_dim)


def fine_product_expected(A, W):
    """One-sided six-product case: one operand on fine_lattice (granularity 2^-17), the other in {-1, 0, 1}; K * 2^17 <= 2^24."""
    assert A.shape[1] * 2 ** 17 <= 2 ** 24, "K too long for the 2^-17 lattice"
    return exact_product_expected(A, W)


# ---- one-hot probe ---------------------------------------------------------------------------------------------------------------
ONEHOT_MOD = 61


def onehot_k(m, K):
    """k(m): starts at the LAST k and walks down through all of K."""
    return (K - 1 - m) % K


def onehot_probe(M, K, N):
    """A[m] = 2 e_k(m); W[n, k] = 1 + (n mod 61) K + k, a distinct code per (n mod 61, k) -> C[m, n] = 2 W[n, k(m)]."""
    A = torch.zeros(M, K)
    A[torch.arange(M), onehot_k(torch.arange(M), K)] = 2.0
    W = (1 + (torch.arange(N) % ONEHOT_MOD)[:, None] * K + torch.arange(K)[None, :]).float()
    want = three_product_expected(A, W)
    assert torch.equal(want, 2.0 * W.double()[:, onehot_k(torch.arange(M), K)].t())
    return A, W, want


def onehot_decode(C, K):
    """(n mod 61, k) the kernel used per element of C (both -1 where the value is no code: a dropped or mixed k-tile)."""
    code = C.double() / 2.0 - 1.0
    ok = (code == code.round()) & (code >= 0) & (code < ONEHOT_MOD * K)
    code = torch.where(ok, code, torch.zeros_like(code)).long()
    nmod = torch.where(ok, code // K, torch.full_like(code, -1))
    k = torch.where(ok, code % K, torch.full_like(code, -1))
    return nmod, k


def onehot_report(C, want, K, limit=8):
    """Lines "(m, n): kernel used k = .. of column class .., expected k = .." of the first mismatches."""
    bad = (C.double() != want).nonzero()
    nmod, k = onehot_decode(C, K)
    lines = [f"{bad.shape[0]} of {want.numel()} elements differ"]
    for m, n in bad[:limit].tolist():
        lines.append(f"  (m={m}, n={n}): got {float(C[m, n])} = code of k {int(k[m, n])}, column class {int(nmod[m, n])}; "
                     f"expected k {int(onehot_k(m, K))}, column class {n % ONEHOT_MOD}")
    return "\n".join(lines)


def mismatch_report(got, want, limit=8):
    """First mismatching indices of an exact comparison, with the rows / columns (first two dims) they fall in."""
    bad = (got.double() != want).nonzero()
    lines = [f"{bad.shape[0]} of {want.numel()} elements differ; dim-0 indices {sorted(set(bad[:, 0].tolist()))[:16]}, "
             f"dim-1 indices {sorted(set(bad[:, 1].tolist()))[:16]}"]
    for idx in bad[:limit].tolist():
        lines.append(f"  {tuple(idx)}: got {float(got[tuple(idx)])!r}, expected {float(want[tuple(idx)])!r}")
    return "\n".join(lines)


# ---- the cases of tests/test_gpu_split_exact.py (built once per process, on the CPU) ---------------------------------------------
# The builders are cached and hand every caller the SAME tensors: treat them as read-only (the GPU tests only copy them to the
# device); a test that needs to write takes a .clone().
M_ALL, K_ALL = (1, 63, 255, 256, 257, 513), (32, 96, 160, 448)
# every M at K = 32 (nk = 2: every prologue / k-tile clamp active) and K = 96 (nk = 6: A stages and weight slots out of phase),
# every K at M = 257, both N
LINEAR_SHAPES = [(m, 32, 128) for m in M_ALL] + [(m, 96, 384) for m in M_ALL] + [(257, 160, 128), (257, 448, 384), (257, 32, 384), (257, 96, 128)]
EPILOGUES = ("none", "bias", "scale_res")
GAMMAS = (1.0, -1.0, 2.0, -2.0, 0.5)


def _small_ints(shape, gen, vmax=8):
    return torch.randint(-vmax, vmax + 1, tuple(shape), generator=gen).float()


def _gammas(n, gen):
    return torch.tensor(GAMMAS)[torch.randint(0, len(GAMMAS), (n,), generator=gen)]


@functools.lru_cache(maxsize=None)
def linear_case(m, k, n, kind, seed=0, w_zero_frac=None, w_vmax=None):
    """dict(A, W, bias, gamma, resid, want = {epilogue: float64[M, N]}) of one linear launch shape on one lattice."""
    gen = _gen(1000 * m + 10 * k + n + seed + (7 if kind == "hl" else 0))
    A = lattice(kind, (m, k), gen)
    W = lattice(kind, (n, k), gen, w_zero_frac) if w_vmax is None else int_lattice((n, k), w_vmax, w_zero_frac or 0.25, gen)
    bias, gamma, resid = _small_ints((n,), gen), _gammas(n, gen), _small_ints((m, n), gen)
    want = {"none": three_product_expected(A, W), "bias": three_product_expected(A, W, bias),
            "scale_res": three_product_expected(A, W, bias, gamma, resid)}
    return dict(A=A, W=W, bias=bias, gamma=gamma, resid=resid, want=want)


def rows_of(x):
    """Host restatement of the "f16x2 rows" layout (split2_common.hpp): per 8 elements of a row, 8 h halves then 8 l halves."""
    h = x.float().half()
    l = (x.float() - h.float()).half()
    k = x.shape[-1]
    packed = torch.stack([h.view(*x.shape[:-1], k // 8, 8), l.view(*x.shape[:-1], k // 8, 8)], dim=-2).contiguous()
    return packed.view(torch.float32).view(x.shape)


@functools.lru_cache(maxsize=None)
def rows_chain_case(m, k2):
    """Two launches: hl_lattice [m, 32] x [k2, 32] -> "f16x2 rows" (epilogue none), then rows x {-1, 0, 1} [128, k2] with the
    scale + residual epilogue.  The first result has at most 22 significant bits (|x| < 2^10 on a 2^-12 grid), so its h + l is
    exact; its l is non-zero, and the second expected value comes from the first through the same helper."""
    first = linear_case(m, 32, k2, "hl", seed=3, w_zero_frac=0.5)
    x = first["want"]["bias"]
    assert float(x.abs().max()) < 2.0 ** 10 and granularity(x) >= 2.0 ** -12, "first result has more than 22 significant bits"
    h, l = split_f16(x)
    assert torch.equal(h + l, x) and bool((l != 0).any())
    gen = _gen(m + k2)
    W2 = int_lattice((128, k2), 1, 0.8, gen)
    gamma, resid = _gammas(128, gen), _small_ints((m, 128), gen)
    want = three_product_expected(x.float(), W2, None, gamma, resid)
    return dict(first=first, x=x, h=h, l=l, W2=W2, gamma=gamma, resid=resid, want=want)


# 3x3 / 1 / 1 (CONV == 1): (n, Cin, H, W, Cout).  105 rows; 585 rows (tiles span images); stencils wider than the image;
# exactly one tile (Cin = 64: hl_lattice with more zeros, K = 576 would leave the exact range otherwise)
CONV3_SHAPES = [(3, 32, 5, 7, 128), (5, 32, 9, 13, 128), (2, 32, 1, 9, 128), (2, 32, 9, 1, 128), (1, 64, 16, 16, 128), (3, 32, 5, 7, 256)]
# general form (CONV == 2) on (n = 3, 11 x 7): (Cin, ks, stride, pad, lattice); 25 taps on int_lattice; Cin = 64: cpt = 4 chunks per tap
CONV2_CASES = [(32, 2, 2, 0, "hl"), (32, 2, 2, 0, "int"), (32, 3, 2, 1, "hl"), (32, 3, 2, 1, "int"), (32, 3, 1, 0, "hl"), (32, 3, 1, 0, "int"),
               (32, 5, 2, 2, "int"), (64, 2, 2, 0, "hl"), (64, 3, 2, 1, "int")]
DECONV_CASES = [(3, 1, 1), (4, 1, 0), (2, 0, 0)]     # (ks, pad, out_pad), stride 2, input (2, 64, 5, 7) -> Cout 128


@functools.lru_cache(maxsize=None)
def conv_case(n, cin, h, w, cout, ks, stride, pad, kind):
    """dict(x NCHW, w, bias, want = {False: without bias, True: with}) of one convolution on one lattice."""
    gen = _gen(n * 7919 + cin * 31 + h * 17 + w * 13 + cout + ks * 101 + stride + (7 if kind == "hl" else 0))
    zf = 0.4 if (kind == "hl" and ks * ks * cin > 448) else None
    x = lattice(kind, (n, cin, h, w), gen, zf)
    wt = lattice(kind, (cout, cin, ks, ks), gen, zf)
    bias = _small_ints((cout,), gen)
    want = {False: three_product_conv_expected(x, wt, None, stride, pad), True: three_product_conv_expected(x, wt, bias, stride, pad)}
    return dict(x=x, w=wt, bias=bias, want=want)


@functools.lru_cache(maxsize=None)
def deconv_case(ks, pad, out_pad):
    gen = _gen(ks * 100 + pad * 10 + out_pad)
    x = int_lattice((2, 64, 5, 7), 5, 0.25, gen)
    wt = int_lattice((64, 128, ks, ks), 5, 0.25, gen)
    bias = _small_ints((128,), gen)
    want = three_product_deconv_expected(x, wt, bias, 2, pad, out_pad)
    assert torch.equal(want, exact_product_expected(x, wt, deconv_op(2, pad, out_pad), bias, bias_dim=1))
    return dict(x=x, w=wt, bias=bias, want=want)


@functools.lru_cache(maxsize=None)
def int_case(m, k, n, seed=0):
    """int_lattice operands whose expected tensors hold for three AND six products, every epilogue."""
    c = linear_case(m, k, n, "int", seed)
    for epi, args in (("none", ()), ("bias", (c["bias"],)), ("scale_res", (c["bias"], c["gamma"], c["resid"]))):
        assert torch.equal(c["want"][epi], exact_product_expected(c["A"], c["W"], _linear, *args)), epi
    assert torch.equal(c["want"]["none"], (c["A"].long() @ c["W"].long().t()).double())
    return c


@functools.lru_cache(maxsize=None)
def fine_case(k, side):
    """side "A": A on fine_lattice, W in {-1, 0, 1}; side "W": the mirror.  M = 257, N = 128."""
    gen = _gen(k + (1 if side == "A" else 2))
    fine, tern = (257, k), (128, k)
    if side == "W":
        fine, tern = tern, fine
    f, t = fine_lattice(fine, gen), int_lattice(tern, 1, 0.3, gen)
    A, W = (f, t) if side == "A" else (t, f)
    return dict(A=A, W=W, want=fine_product_expected(A, W))


# ---- the fused ConvNeXt MLP (csrc/gemm_mlp_fused.hip; tests/test_gpu_mlp_fused_exact.py) ------------------------------------------
# gelu_erf (csrc/common.hpp) is max(x, 0) - u 2^q(u) with u = min(|x|, 5.9): for |x| >= 5.9 the subtracted term is 9.6e-9.  It
# vanishes in the rounding of any x >= 6 (half an ulp there is 2.4e-7), and for x <= -6 the result -9.6e-9 is below half the
# smallest fp16 subnormal (2.98e-8): both halves of fc2's operand are +-0.  On inputs with NO pre-activation in (-6, 6) the fused
# MLP is therefore resid + gamma * (W2 . max(W1 x + b1, 0) + b2) under the three-product scheme, twice — one bit pattern.
GELU_EXACT_FROM = 6.0
GELU_DEAD_BELOW = 2.0 ** -25        # half the smallest fp16 subnormal: rn_f16 of anything smaller is +-0
MLPF_M = (1, 31, 32, 33, 127, 128, 129, 255, 257, 513)      # one wave (32 pixels), one workgroup (128), a second one, a fifth
MLPF_C = (128, 256)
MLPF_KINDS = ("int", "xl", "w2l", "ll")


def mlp_fused_preact(x, W1, b1):
    """fc1(x) + b1 as the kernel has it in front of the GELU: float64[M, hidden], every stage asserted exact."""
    return three_product_op(x, W1, _linear, b1)


def mlp_fused_hidden(pre):
    """The activation model: gelu_erf == max(., 0) for fc2's fp16 operand when no pre-activation lies in (-6, 6).  EVERY element
    is held to that (AssertionError otherwise): the model is a condition on the inputs, not a tolerance."""
    assert bool((pre.abs() >= GELU_EXACT_FROM).all()), \
        f"pre-activation {float(pre[pre.abs() < GELU_EXACT_FROM][0])} inside (-6, 6): gelu_erf is not max(x, 0) there"
    return pre.clamp_min(0.0)


def mlp_fused_expected(x, W1, b1, W2, b2, gamma, resid):
    """What gdrnpp_convnext_mlp_f32_fused must store: x f32[M, C], W1 f32[4C, C], W2 f32[C, 4C] -> float64[M, C] =
    resid + gamma * ((hH lW2^T + lH hW2^T + hH hW2^T) 2^-e2 + b2), H = max((hx lW1^T + lx hW1^T + hx hW1^T) 2^-e1 + b1, 0) = hH + lH.
    Each GEMM with its own weight scale, the l * l term dropped in both."""
    hidden = mlp_fused_hidden(mlp_fused_preact(x, W1, b1))
    return three_product_op(hidden.float(), W2, _linear, b2, gamma, resid)


def _nonzero_ints(shape, vmax, gen):
    shape = tuple(shape)
    return (torch.randint(1, vmax + 1, shape, generator=gen) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).float()


def sparse_rows(rows, cols, nnz, values, gen):
    """f32[rows, cols] with ``values`` [rows, nnz] (all non-zero) on exactly nnz columns per row.  Row r sits on columns
    perm[(r mod S) + S i], S = cols / nnz, i < nnz, of one random permutation: with rows >= S every column is used."""
    s = cols // nnz
    assert s * nnz == cols and rows >= s and bool((values != 0).all())
    perm = torch.randperm(cols, generator=gen)
    col = perm[(torch.arange(rows) % s)[:, None] + s * torch.arange(nnz)[None, :]]
    w = torch.zeros(rows, cols)
    w[torch.arange(rows)[:, None], col] = values
    return w


def x_rows_in_range(x):
    """The kernel's verdict on fc1's A rows: the sum of squares of the h halves of every NON-ZERO row is at least C / 256."""
    ss = x.float().half().double().pow(2).sum(dim=1)
    return bool(((ss == 0) | (ss >= x.shape[1] / 256.0)).all())


@functools.lru_cache(maxsize=None)
def mlp_fused_case(m, c, kind, seed=0):
    """dict(x, W1, b1, W2, b2, gamma, resid, pre, want) of one fused-MLP launch, hidden = 4 c.  b1 comes from the data: unit j gets a
    sign s_j and b1[j] = s_j (ceil(max_m |three-product(x, W1)[m, j]|) + 6) (ll: + 32) — about half the units are active (>= 6) for every
    pixel, the others dead (<= -6) for every pixel.
      int   x, W1, W2 dense small integers: l planes zero, the dense stress of indexing, weight ring and row tails;
      xl    x and W1 on hl_lattice (W1: two non-zeros per row, so that the hidden values stay below 64 and are h + l), W2 integer
            with 16 non-zeros per row: l planes of x, of W1 and of the hidden operand in use;
      w2l   x integer, W1 integer with two non-zeros per row, W2 on hl_lattice with 8 non-zeros per row: l plane of W2 in use
            (the hidden values are integers: l . l of fc2 is zero);
      ll    x and W1 as in xl, W2 as in w2l: the l planes of the hidden operand AND of W2 in use, fc2's dropped l . l term is
            non-zero — a kernel that adds it is wrong here and nowhere above."""
    assert kind in MLPF_KINDS, kind
    h = 4 * c
    gen = _gen(100003 * m + 11 * c + seed + 1 + MLPF_KINDS.index(kind))
    if kind == "int":
        x, W1, W2 = (int_lattice(s, 5, 0.25, gen) for s in ((m, c), (h, c), (c, h)))
    else:
        if kind in ("xl", "ll"):
            x = hl_lattice((m, c), gen)
            W1 = sparse_rows(h, c, 2, hl_lattice((h, 2), gen, 0.0), gen)
        else:
            x = int_lattice((m, c), 5, 0.25, gen)
            W1 = sparse_rows(h, c, 2, _nonzero_ints((h, 2), 5, gen), gen)
        if kind == "xl":
            W2 = sparse_rows(c, h, 16, _nonzero_ints((c, 16), 5, gen), gen)
        else:
            W2 = sparse_rows(c, h, 8, hl_lattice((c, 8), gen, 0.0), gen)
    assert bool((W2 != 0).any(dim=0).all()), "a hidden unit no row of W2 reads"
    assert x_rows_in_range(x), "a non-zero x row below the range of fc1's A operand"
    sign = torch.randint(0, 2, (h,), generator=gen).float() * 2 - 1
    # ll: active values from 32 on, where an fp16 ulp (2^-5) is above the lattice's fractions (< 2^-7) — the h halves of the
    # hidden operand are integers, or h . l_W2 would need units of 2^-8 and the sums would leave 2^24
    margin = 32.0 if kind == "ll" else GELU_EXACT_FROM
    b1 = sign * (three_product_expected(x, W1).abs().amax(dim=0).ceil().float() + margin)
    b2, gamma, resid = _small_ints((c,), gen), _gammas(c, gen), _small_ints((m, c), gen)
    pre = mlp_fused_preact(x, W1, b1)
    assert torch.equal(pre >= GELU_EXACT_FROM, (sign > 0).expand(m, h)) and 0 < int((sign > 0).sum()) < h      # every hidden row >= 36: in range
    want = mlp_fused_expected(x, W1, b1, W2, b2, gamma, resid)
    return dict(x=x, W1=W1, b1=b1, W2=W2, b2=b2, gamma=gamma, resid=resid, pre=pre, want=want)


# ---- probes of the fused MLP: one launch per block q of C hidden units, gamma = 1, b2 = resid = 0 -------------------------------
FC1_PROBE_B1 = 6.0                  # every unit active
FC2_PROBE_T, FC2_PROBE_B = 7.0, 6.0    # the one live unit of a pixel holds 2 T - B = 8, all others -B


def _codes(rows, cols):
    """f32[rows, cols]: 1 + (row mod 61) cols + col, a distinct code per (row mod 61, col)."""
    return (1 + (torch.arange(rows) % ONEHOT_MOD)[:, None] * cols + torch.arange(cols)[None, :]).float()


def _decode(code, cols):
    """(row class, col) per element of a tensor of codes (both -1 where the value is no code: a dropped or mixed term)."""
    code = code - 1.0
    ok = (code == code.round()) & (code >= 0) & (code < ONEHOT_MOD * cols)
    code = torch.where(ok, code, torch.zeros_like(code)).long()
    return torch.where(ok, code // cols, torch.full_like(code, -1)), torch.where(ok, code % cols, torch.full_like(code, -1))


def _probe_x(M, C):
    x = torch.zeros(M, C)
    x[torch.arange(M), onehot_k(torch.arange(M), C)] = 2.0
    return x


def mlp_fc1_probe(M, C, q):
    """Pixel m = 2 e_k(m) (row 0 needs the LAST k-step); W1[j, k] a code of (j mod 61, k); W2 selects hidden block q
    (W2[o, C q + o] = 1) -> y[m, o] = 2 W1[C q + o, k(m)] + 6: an element names the hidden unit and the k the first GEMM used for
    it — the x swizzle, the W1 fragment order and the accumulator-to-hidden map."""
    H = 4 * C
    x, W1, b1 = _probe_x(M, C), _codes(H, C), torch.full((H,), FC1_PROBE_B1)
    W2 = torch.zeros(C, H)
    W2[torch.arange(C), C * q + torch.arange(C)] = 1.0
    b2, gamma, resid = torch.zeros(C), torch.ones(C), torch.zeros(M, C)
    want = mlp_fused_expected(x, W1, b1, W2, b2, gamma, resid)
    assert torch.equal(want, 2.0 * W1.double()[C * q:C * (q + 1), onehot_k(torch.arange(M), C)].t() + FC1_PROBE_B1)
    return dict(x=x, W1=W1, b1=b1, W2=W2, b2=b2, gamma=gamma, resid=resid, want=want)


def mlp_fc1_probe_decode(y, C):
    """(hidden unit mod 61, k) the kernel used per element of y."""
    return _decode((y.double() - FC1_PROBE_B1) / 2.0, C)


def mlp_fc1_probe_report(y, want, C, q, limit=8):
    bad = (y.double() != want).nonzero()
    jmod, k = mlp_fc1_probe_decode(y, C)
    lines = [f"{bad.shape[0]} of {want.numel()} elements differ"]
    for m, o in bad[:limit].tolist():
        lines.append(f"  (m={m}, o={o}): got {float(y[m, o])} = code of k {int(k[m, o])}, hidden class {int(jmod[m, o])}; "
                     f"expected k {int(onehot_k(m, C))}, hidden unit {C * q + o} (class {(C * q + o) % ONEHOT_MOD})")
    return "\n".join(lines)


def mlp_fc2_probe(M, C, q):
    """Pixel m has exactly ONE live hidden unit j(m) = C q + k(m) (W1[C q + k, k] = T, b1 = -B: 2 T - B = 8 there, -B <= -6
    elsewhere); W2[o, j] a code of (o mod 61, j) -> y[m, o] = 8 W2[o, j(m)]: an element names the hidden unit the second GEMM
    paired with that column of W2 — the W2 pack order against the accumulator order."""
    H = 4 * C
    x = _probe_x(M, C)
    W1 = torch.zeros(H, C)
    W1[C * q + torch.arange(C), torch.arange(C)] = FC2_PROBE_T
    b1, W2 = torch.full((H,), -FC2_PROBE_B), _codes(C, H)
    b2, gamma, resid = torch.zeros(C), torch.ones(C), torch.zeros(M, C)
    want = mlp_fused_expected(x, W1, b1, W2, b2, gamma, resid)
    live = 2.0 * FC2_PROBE_T - FC2_PROBE_B
    assert torch.equal(want, live * W2.double()[:, mlp_fc2_probe_unit(torch.arange(M), C, q)].t())
    return dict(x=x, W1=W1, b1=b1, W2=W2, b2=b2, gamma=gamma, resid=resid, want=want)


def mlp_fc2_probe_unit(m, C, q):
    return C * q + onehot_k(m, C)


def mlp_fc2_probe_decode(y, C):
    """(output channel mod 61, hidden unit) the kernel used per element of y."""
    return _decode(y.double() / (2.0 * FC2_PROBE_T - FC2_PROBE_B), 4 * C)


def mlp_fc2_probe_report(y, want, C, q, limit=8):
    bad = (y.double() != want).nonzero()
    omod, j = mlp_fc2_probe_decode(y, C)
    lines = [f"{bad.shape[0]} of {want.numel()} elements differ"]
    for m, o in bad[:limit].tolist():
        lines.append(f"  (m={m}, o={o}): got {float(y[m, o])} = code of hidden unit {int(j[m, o])}, output class {int(omod[m, o])}; "
                     f"expected hidden unit {int(mlp_fc2_probe_unit(m, C, q))}, output class {o % ONEHOT_MOD}")
    return "\n".join(lines)
