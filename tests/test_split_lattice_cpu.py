"""tests/split_lattice.py checked where there is no GPU: the zero-tolerance oracle of tests/test_gpu_split_exact.py is itself exact
— the lattices reconstruct from their fp16 planes, every term is an integer of the scaled domain, an fp32 accumulation of the
three products gives the same bits in any order, the expected value differs from the fp64 product by exactly the dropped l * l
term, and the precondition refuses operands for which none of this holds."""
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
