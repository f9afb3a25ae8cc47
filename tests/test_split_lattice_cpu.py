"""tests/split_lattice.py checked where there is no GPU: the zero-tolerance oracle of tests/test_gpu_split_exact.py is itself exact
— the lattices reconstruct from their fp16 planes, every term is an integer of the scaled domain, an fp32 accumulation of the
three products gives the same bits in any order, the expected value differs from the fp64 product by exactly the dropped l * l
term, and the precondition refuses operands for which none of this holds.  The same for the oracle of the fused ConvNeXt MLP
(tests/test_gpu_mlp_fused_exact.py): its activation model against gelu_erf restated in fp32, its probes, and mutations of its
restatement (swapped hidden units, a stale W2 tile, a dropped plane pair, no GELU) that must each change the expected output."""
import pytest
import torch

from tests import split_lattice as SL


def _f32_accumulate(A, W, perm):
    """fp32 accumulation of the 3 K rank-one terms (plane pair, k) of the scheme in the order ``perm`` -> f32[M, N] (scaled domain)."""
    (hA, lA), (hW, lW), _ = SL.three_product_planes(A, W)
    pairs = [(hA.float(), lW.float()), (lA.float(), hW.float()), (hA.float(), hW.float())]
    K = A.shape[1]
    acc = torch.zeros(A.shape[0], W.shape[0], dtype=torch.float32)
    for i in perm.tolist():
        a, w = pairs[i // K]
        k = i % K
        term = a[:, k, None] * w[None, :, k]          # fp16 x fp16: exact in fp32
        assert torch.equal(term.double(), a[:, k, None].double() * w[None, :, k].double())
        acc += term
    return acc


@pytest.mark.parametrize("k", SL.K_ALL)
def test_hl_lattice_planes_and_any_order_fp32_sum(k):
    gen = torch.Generator().manual_seed(k)
    A, W = SL.hl_lattice((300, k), gen), SL.hl_lattice((128, k), gen)
    bias = torch.randint(-8, 9, (128,), generator=gen).float()
    (hA, lA), (hW, lW), e = SL.three_product_planes(A, W)
    assert e == 12                                                   # pack_weight_f16x2 scales by exactly 2^12
    nz = A != 0
    assert torch.equal(hA[nz].abs().clamp(2, 3), hA[nz].abs()) and torch.equal(hA, hA.round())      # h = p
    assert float(lA.abs().max()) == 2.0 ** -11 and float(lA[lA != 0].abs().min()) == 2.0 ** -12        # l = q 2^-12: normal fp16
    assert bool((lA != 0).any()) and bool((lW != 0).any())
    for t in (hA @ lW.t(), lA @ hW.t(), hA @ hW.t()):                 # integers of the scaled domain
        assert torch.equal(t, t.round())
    assert 9 * k * 2 ** 12 + 6 * k * 2 + 8 * 2 ** 12 < 2 ** 24        # worst case of the lattice at this K
    assert float((A.double() ** 2).mean(dim=1).min()) >= 4.0 * 0.7    # rows far above the 2^-4 rms of the range check
    want = SL.three_product_expected(A, W, bias)
    for seed in (1, 2):
        perm = torch.randperm(3 * k, generator=torch.Generator().manual_seed(seed))
        acc = _f32_accumulate(A, W, perm)
        got = acc * 2.0 ** -e + bias
        assert torch.equal(got.double(), want), seed
    # against the fp64 product: exactly the dropped l * l term
    full = A.double() @ W.double().t() + bias.double()
    ll = SL.dropped_ll_term(A, W)
    assert bool((ll != 0).any()) and torch.equal(full - want, ll)
    assert float(ll.abs().max()) <= k * 2.0 ** -22


@pytest.mark.parametrize("k", (32, 96, 512, 1024))
def test_int_lattice_expected_is_the_int64_product(k):
    gen = torch.Generator().manual_seed(k)
    A, W = SL.int_lattice((300, k), 5, 0.25, gen), SL.int_lattice((128, k), 5, 0.25, gen)
    want = (A.long() @ W.long().t()).double()
    assert torch.equal(SL.three_product_expected(A, W), want)
    assert torch.equal(SL.exact_product_expected(A, W), want)
    (hA, lA), (hW, lW), _ = SL.three_product_planes(A, W)
    assert not lA.any() and not lW.any()
    assert torch.equal(_f32_accumulate(A[:16], W, torch.randperm(3 * k, generator=gen)).double() * 2.0 ** -SL.weight_exp(W), want[:16])


def test_weight_exp_and_granularity():
    assert SL.weight_exp(torch.tensor([3.0 + 2.0 ** -11])) == 12 and SL.weight_exp(torch.tensor([5.0])) == 11
    assert SL.weight_exp(torch.tensor([1.0])) == 13 and SL.weight_exp(torch.tensor([0.7])) == 14 and SL.weight_exp(torch.zeros(3)) == 0
    assert SL.granularity(torch.tensor([6.0, 0.0, 2.0 + 2.0 ** -12])) == 2.0 ** -12
    assert SL.granularity(torch.tensor([8.0, -24.0])) == 8.0 and SL.granularity(torch.zeros(4)) == float("inf")


def test_precondition_refuses_what_is_not_exact():
    gen = torch.Generator().manual_seed(0)
    A, W = SL.hl_lattice((8, 4096), gen), SL.hl_lattice((128, 4096), gen)
    with pytest.raises(AssertionError, match="2\\^24"):
        SL.three_product_expected(A, W)                              # K = 4096: sums beyond 2^24 units
    with pytest.raises(AssertionError, match="h \\+ l"):
        SL.three_product_expected(torch.full((4, 32), 1.0 + 2.0 ** -11 + 2.0 ** -23), SL.hl_lattice((128, 32), gen))     # 24 bits do not fit two halves
    with pytest.raises(AssertionError, match="K too long"):
        SL.fine_product_expected(SL.fine_lattice((4, 160), gen), SL.int_lattice((128, 160), 1, 0.3, gen))
    with pytest.raises(AssertionError, match="round-trip"):
        SL.three_product_expected(SL.hl_lattice((4, 448), gen, 0.0).abs(), SL.hl_lattice((128, 448), gen, 0.0).abs(),
                                  torch.full((128,), 2.0 ** 13))     # sum ~ 2800 on a 2^-12 grid + 8192: 26 bits


def test_onehot_probe_decodes():
    for m, k, n in ((257, 96, 384), (1, 32, 128)):
        A, W, want = SL.onehot_probe(m, k, n)
        assert float(A.double().pow(2).sum(dim=1).min()) == 4.0 and len(set(SL.onehot_k(torch.arange(m), k).tolist())) == min(m, k)
        assert SL.onehot_k(0, k) == k - 1                               # row 0 needs the LAST k-tile
        nmod, kk = SL.onehot_decode(want.float(), k)
        assert torch.equal(kk, SL.onehot_k(torch.arange(m), k)[:, None].expand(m, n))
        assert torch.equal(nmod, (torch.arange(n) % SL.ONEHOT_MOD)[None, :].expand(m, n))
        codes = W[:SL.ONEHOT_MOD].reshape(-1)
        assert codes.unique().numel() == codes.numel()
        broken = want.float().clone()
        broken[0, 5] = 0.0                                              # a dropped k-tile
        broken[0, 6] = 2.0 * W[6, 3]                                    # a stale one
        nmod, kk = SL.onehot_decode(broken, k)
        assert int(kk[0, 5]) == -1 and int(kk[0, 6]) == 3 and "(m=0, n=6)" in SL.onehot_report(broken, want, k)


def test_fine_lattice_fills_the_lower_bf16_planes():
    gen = torch.Generator().manual_seed(4)
    x = SL.fine_lattice((64, 64), gen)
    h = x.bfloat16().float()
    m = (x - h).bfloat16().float()
    l = x - h - m
    assert bool((m != 0).any()) and bool((l != 0).any()) and torch.equal(h.abs(), torch.ones_like(h))
    for k in (32, 64):
        for side in ("A", "W"):
            c = SL.fine_case(k, side)
            assert k * 2 ** 17 <= 2 ** 24 and torch.equal(c["want"], c["A"].double() @ c["W"].double().t())


@pytest.mark.parametrize("kind", ("int", "hl"))
def test_every_gpu_case_meets_its_precondition(kind):
    """Building a case asserts reconstruction, the 2^24 bound on the actual operands and the float32 round trip of every epilogue
    stage: every (K, taps) pair of tests/test_gpu_split_exact.py, built here once."""
    for m, k, n in SL.LINEAR_SHAPES + [(300, 96, 256)]:
        c = SL.linear_case(m, k, n, kind)
        assert set(c["want"]) == set(SL.EPILOGUES) and c["want"]["none"].shape == (m, n)
        if kind == "hl":
            assert bool(SL.dropped_ll_term(c["A"], c["W"]).any())
    for n, cin, h, w, cout in SL.CONV3_SHAPES:
        assert SL.conv_case(n, cin, h, w, cout, 3, 1, 1, kind)["want"][True].shape == (n, cout, h, w)
    for cin, ks, stride, pad, lat in SL.CONV2_CASES:
        if lat == kind:
            SL.conv_case(3, cin, 11, 7, 128, ks, stride, pad, kind)
    if kind == "int":
        for m, k, n in ((300, 512, 1024), (1300, 512, 1152), (257, 96, 384), (63, 32, 128), (5, 1024, 256), (300, 1024, 256), (512, 96, 256)):
            SL.int_case(m, k, n)
        for case in SL.DECONV_CASES:
            SL.deconv_case(*case)
        SL.conv_case(1, 32, 16, 16, 256, 3, 1, 1, "int")
        SL.conv_case(3, 32, 16, 16, 256, 3, 1, 1, "int")
    else:
        for m in (300, 1):
            for k2 in (128, 384):
                c = SL.rows_chain_case(m, k2)
                assert c["want"].shape == (m, 128)
                assert torch.equal(SL.rows_of(c["x"]).view(torch.float16).view(m, k2 // 8, 2, 8)[:, :, 1].double().reshape(m, k2), c["l"])


# ---- the fused ConvNeXt MLP: oracle of tests/test_gpu_mlp_fused_exact.py ------------------------------------------------------------
MLPF_CASES = [(c, kind) for c in SL.MLPF_C for kind in SL.MLPF_KINDS]
_GELU_Q = (-2.7721912374545354e-06, 3.862218727590516e-05, -0.00018255332543049008, -0.000145858692121692, 0.007075459696352482,
           -0.052505023777484894, -0.45920491218566895, -1.1511057615280151, -1.0)      # csrc/common.hpp: gelu_erf


def _fmaf(a, b, c):
    """fp32 fma of f32 tensors: the product of two floats is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def _gelu_erf_f32(x):
    """gelu_erf of csrc/common.hpp restated in fp32: max(x, 0) - u 2^q(u), u = min(|x|, 5.9)."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    u = torch.minimum(x.abs(), f32(5.9))
    q = torch.full_like(u, _GELU_Q[0])
    for coef in _GELU_Q[1:]:
        q = _fmaf(q, u, f32(coef))
    return _fmaf(-u, torch.exp2(q), x.clamp_min(0.0))


def _fused_restated(c, W2=None, act=lambda pre: pre.clamp_min(0.0), fc2_terms=("hl", "lh", "hh")):
    """The second half of SL.mlp_fused_expected without its asserts, open to mutation: another W2, another activation, a dropped
    plane pair ("hl" = h of the hidden operand x l of W2, ...)."""
    W2 = c["W2"] if W2 is None else W2
    e2 = SL.weight_exp(W2)
    hH, lH = SL.split_f16(act(c["pre"]).float())
    hW, lW = SL.split_f16(W2.double() * 2.0 ** e2)
    pairs = {"hl": (hH, lW), "lh": (lH, hW), "hh": (hH, hW), "ll": (lH, lW)}
    acc = sum(pairs[t][0] @ pairs[t][1].t() for t in fc2_terms)
    return c["resid"].double() + c["gamma"].double() * (acc * 2.0 ** -e2 + c["b2"].double())


@pytest.mark.parametrize("c,kind", MLPF_CASES)
def test_every_fused_mlp_case_meets_its_precondition(c, kind):
    """Building a case asserts, on the actual operands: reconstruction of x, W1, the hidden tensor and W2 from their halves, the 2^24
    bound of both GEMMs, the float32 round trip of every stage, |pre-activation| >= 6 for EVERY element, x rows in range, every
    hidden unit read by W2.  Every (M, C, kind) of tests/test_gpu_mlp_fused_exact.py, built here once."""
    h = 4 * c
    for m in SL.MLPF_M:
        cs = SL.mlp_fused_case(m, c, kind)
        assert cs["want"].shape == (m, c) and cs["pre"].shape == (m, h)
        hidden = cs["pre"].clamp_min(0.0)
        active = (cs["pre"] > 0).sum(dim=1)
        assert int(active.min()) == int(active.max()) and h // 4 < int(active[0]) < 3 * h // 4      # about half, the same for every pixel
        assert float(hidden.pow(2).sum(dim=1).min()) >= 36.0 and float(hidden.max()) < 2048.0         # fc2's A rows in range, far from 65504
        assert torch.equal(_fused_restated(cs), cs["want"])
        (hx, lx), (hW1, lW1), _ = SL.three_product_planes(cs["x"], cs["W1"])
        (hH, lH), (hW2, lW2), _ = SL.three_product_planes(hidden.float(), cs["W2"])
        if kind == "int":
            want = cs["resid"].long() + cs["gamma"].double() * (torch.relu(cs["x"].long() @ cs["W1"].long().t() + cs["b1"].long()) @ cs["W2"].long().t()
                                                                + cs["b2"].long()).double()
            assert torch.equal(cs["want"], want)
            assert not lx.any() and not lW1.any() and not lH.any() and not lW2.any()
        elif kind == "xl":
            assert bool(lx.any()) and bool(lW1.any()) and bool(lH.any()) and not lW2.any()
            assert bool(SL.dropped_ll_term(cs["x"], cs["W1"]).any())        # the scheme, not the plain product
            assert bool((lH @ hW2.t()).any())
        elif kind == "w2l":                                               # integer hidden values: l . l of fc2 is zero by construction
            assert bool(lW2.any()) and bool((hH @ lW2.t()).any()) and not lx.any() and not lH.any()
        else:                                                             # every plane of both GEMMs, both dropped terms
            assert bool(lx.any()) and bool(lW1.any()) and bool(lH.any()) and bool(lW2.any())
            assert bool(SL.dropped_ll_term(cs["x"], cs["W1"]).any()) and bool(SL.dropped_ll_term(hidden.float(), cs["W2"]).any())
            assert torch.equal(hH, hH.round()) and float(hidden[hidden > 0].min()) >= 32.0


@pytest.mark.parametrize("c,kind", MLPF_CASES)
def test_fused_mlp_activation_model_is_gelu_erf_in_fp32(c, kind):
    """Over the pre-activations of every case: the active units pass gelu_erf bit for bit, the dead ones come out below half the
    smallest fp16 subnormal (both halves of fc2's operand +-0).  A retuned gelu_erf that breaks the model fails here."""
    for m in SL.MLPF_M:
        pre = SL.mlp_fused_case(m, c, kind)["pre"].float()
        g = _gelu_erf_f32(pre)
        act = pre > 0
        assert torch.equal(g[act], pre[act])
        assert float(g[~act].abs().max()) < SL.GELU_DEAD_BELOW and not g[~act].half().any()
    edge = torch.tensor([6.0, -6.0, 6.0 + 2.0 ** -21, 8.0, 65504.0])
    g = _gelu_erf_f32(edge)
    assert torch.equal(g[[0, 2, 3, 4]], edge[[0, 2, 3, 4]]) and 0 < -float(g[1]) < SL.GELU_DEAD_BELOW
    assert float(_gelu_erf_f32(torch.tensor([3.0]))) != 3.0                 # inside (-6, 6) the model does not hold


def test_fused_mlp_precondition_refuses_what_is_not_exact():
    cs = SL.mlp_fused_case(33, 128, "int")
    args = lambda **kw: [kw.get(k, cs[k]) for k in ("x", "W1", "b1", "W2", "b2", "gamma", "resid")]
    assert torch.equal(SL.mlp_fused_expected(*args()), cs["want"])
    b1 = cs["b1"].clone()
    b1[7] += 3.0 - cs["pre"][5, 7].float()                                  # ONE pre-activation of 3.0 among 33 x 512
    with pytest.raises(AssertionError, match="inside \\(-6, 6\\)"):
        SL.mlp_fused_expected(*args(b1=b1))
    xl = SL.mlp_fused_case(33, 128, "xl")
    dense = SL.int_lattice((128, 512), 5, 0.25, torch.Generator().manual_seed(1))
    with pytest.raises(AssertionError, match="2\\^24"):
        SL.mlp_fused_expected(xl["x"], xl["W1"], xl["b1"], dense, xl["b2"], xl["gamma"], xl["resid"])
    with pytest.raises(AssertionError):                                     # sparse_rows: fewer rows than columns per non-zero
        SL.sparse_rows(4, 128, 2, torch.ones(4, 2), torch.Generator().manual_seed(1))
    small = cs["x"].clone()
    small[3] *= 2.0 ** -12
    assert SL.x_rows_in_range(cs["x"]) and not SL.x_rows_in_range(small)


@pytest.mark.parametrize("c", SL.MLPF_C)
def test_fused_mlp_probes_decode(c):
    h = 4 * c
    for m in (257, 1):
        units = set()
        for q in range(4):
            p1, p2 = SL.mlp_fc1_probe(m, c, q), SL.mlp_fc2_probe(m, c, q)
            ks = SL.onehot_k(torch.arange(m), c)
            assert SL.onehot_k(0, c) == c - 1 and float(p1["x"].pow(2).sum(dim=1).min()) == 4.0
            jmod, k = SL.mlp_fc1_probe_decode(p1["want"].float(), c)
            assert torch.equal(k, ks[:, None].expand(m, c))
            assert torch.equal(jmod, ((c * q + torch.arange(c)) % SL.ONEHOT_MOD)[None, :].expand(m, c))
            omod, j = SL.mlp_fc2_probe_decode(p2["want"].float(), c)
            assert torch.equal(j, (c * q + ks)[:, None].expand(m, c))
            assert torch.equal(omod, (torch.arange(c) % SL.ONEHOT_MOD)[None, :].expand(m, c))
            pre = SL.mlp_fused_preact(p2["x"], p2["W1"], p2["b1"])
            assert torch.equal((pre > 0).sum(dim=1), torch.ones(m, dtype=torch.long))       # exactly one live unit per pixel
            units |= set((pre > 0).nonzero()[:, 1].tolist())
            for codes in (p1["W1"][:SL.ONEHOT_MOD], p2["W2"][:SL.ONEHOT_MOD]):
                assert codes.unique().numel() == codes.numel()
            # a dropped unit and a stale one, named with the right indices
            b1 = p1["want"].float().clone()
            b1[0, 5] = SL.FC1_PROBE_B1
            b1[0, 6] = 2.0 * p1["W1"][c * q + 9, 3] + SL.FC1_PROBE_B1
            jmod, k = SL.mlp_fc1_probe_decode(b1, c)
            assert int(k[0, 5]) == -1 and int(k[0, 6]) == 3 and int(jmod[0, 6]) == (c * q + 9) % SL.ONEHOT_MOD
            rep = SL.mlp_fc1_probe_report(b1, p1["want"], c, q)
            assert rep.startswith("2 of") and "(m=0, o=6)" in rep and f"hidden unit {c * q + 6} " in rep
            b2 = p2["want"].float().clone()
            b2[0, 5] = 0.0
            b2[0, 6] = 8.0 * p2["W2"][6, 77]
            omod, j = SL.mlp_fc2_probe_decode(b2, c)
            assert int(j[0, 5]) == -1 and int(j[0, 6]) == 77 and int(omod[0, 6]) == 6
            rep = SL.mlp_fc2_probe_report(b2, p2["want"], c, q)
            assert rep.startswith("2 of") and "(m=0, o=6)" in rep and f"expected hidden unit {c * q + c - 1}," in rep
        if m >= c:
            assert units == set(range(h))                                   # the four launches cover every hidden unit


@pytest.mark.parametrize("c", SL.MLPF_C)
def test_fused_mlp_oracle_sees_the_errors_it_is_for(c):
    """Mutations of the restatement, each of which must change the expected output: two hidden units swapped inside one 32-tile
    of the W2 order, a tile's W2 taken from two tiles earlier (a stale ring slot), fc2's h_w . l_x term dropped, the dead units let
    through (no GELU); and the l . l term that the scheme drops added to fc2."""
    changed = {name: [] for name in ("swap", "stale tile", "h_w . l_x", "dead units", "l . l")}
    for kind in SL.MLPF_KINDS:
        cs = SL.mlp_fused_case(257, c, kind)
        want = cs["want"]
        t = 5
        tile = cs["b1"][32 * t:32 * t + 32]
        a, b = 32 * t + int((tile > 0).nonzero()[0]), 32 * t + int((tile < 0).nonzero()[0])     # an active and a dead unit
        W2 = cs["W2"].clone()
        W2[:, [a, b]] = W2[:, [b, a]]
        changed["swap"].append(not torch.equal(_fused_restated(cs, W2=W2), want))
        W2 = cs["W2"].clone()
        W2[:, 32 * t:32 * t + 32] = W2[:, 32 * (t - 2):32 * (t - 2) + 32]
        changed["stale tile"].append(not torch.equal(_fused_restated(cs, W2=W2), want))
        changed["h_w . l_x"].append(not torch.equal(_fused_restated(cs, fc2_terms=("hl", "hh")), want))
        changed["dead units"].append(not torch.equal(_fused_restated(cs, act=lambda pre: pre), want))
        changed["l . l"].append(not torch.equal(_fused_restated(cs, fc2_terms=("hl", "lh", "hh", "ll")), want))
    assert all(changed["swap"]) and all(changed["stale tile"]) and all(changed["dead units"]), changed
    assert changed["h_w . l_x"] == [False, True, False, True], changed      # the hidden operand's l plane: xl and ll
    assert changed["l . l"] == [False, False, False, True], changed         # both l planes of fc2 at once: ll alone
