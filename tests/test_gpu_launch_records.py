"""-m gpu: what a ``LaunchTimer`` receives from every timed wrapper of ``hip_lib``, at the smallest shape its entry point accepts.
The records (kind, fp32-equivalent flops, algorithmic bytes) are pinned to the literal table below, printed on an MI355X by commit
cfac865 ("Pin the split GEMMs bit-exactly on lattice inputs at their edge shapes") — the last one with all wrappers in one
file — so that moving the wrappers or their launch path changes no record, no three-product launch count and no result
bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (kind, flops, nbytes) in call order
EXPECTED = [
    ("linear", 2097152.0, 188416.0),
    ("linear", 2097152.0, 319488.0),
    ("linear_x3", 2097152.0, 180224.0),
    ("linear_x3", 2097152.0, 311296.0),
    ("linear_splitk", 2097152.0, 188416.0),
    ("linear_splitk", 2097152.0, 319488.0),
    ("linear_grouped", 2097152.0, 188416.0),
    ("conv_splitk", 18874368.0, 385024.0),
    ("conv_x3", 18874368.0, 311296.0),
    ("conv", 2097152.0, 163840.0),
    ("conv_x3", 2097152.0, 131072.0),
    ("conv3x3", 18874368.0, 385024.0),
    ("hbm:groupnorm_apply", 0.0, 262144.0),
    ("conv3x3_x3", 18874368.0, 311296.0),
    ("hbm:groupnorm_apply", 0.0, 262144.0),
    ("deconv", 524288.0, 65536.0),
    ("hbm:groupnorm_apply", 0.0, 65536.0),
    ("mlp_fused_x3", 67108864.0, 917504.0),
    ("hbm:dwconv7_ln", 0.0, 65536.0),
    ("hbm:layernorm", 0.0, 65536.0),
    ("hbm:upsample2x", 0.0, 163840.0),
    ("hbm:groupnorm", 0.0, 98304.0),
    ("mfma_f32:point_pnp_pool", 38010880.0, 0.0),
    ("mfma_f32:conv_bias_act", 8192.0, 4352.0),
]


def _calls(hip):
    """[(label, thunk)]: every timed wrapper once, on inputs fixed by the seed; a thunk returns a tensor or a tuple of them."""
    g = torch.Generator(device=DEV).manual_seed(1234)

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, device=DEV, generator=g) * scale

    def cl(*shape):
        return rn(*shape).contiguous(memory_format=torch.channels_last)

    calls = []
    m, n, k = 256, 128, 32
    x, w, bias, gamma, resid = rn(m, k), rn(n, k, scale=k ** -0.5), rn(n), rn(n), rn(m, n)
    pk6, pk3 = hip.pack_weight_bf16x3(w), hip.pack_weight_f16x2(w)
    for tag, pk in (("bf16x3", pk6), ("f16x2", pk3)):
        calls.append((f"linear_f32_split {tag} none", lambda pk=pk: hip.linear_f32_split(x, pk, bias)))
        calls.append((f"linear_f32_split {tag} scale_res", lambda pk=pk: hip.linear_f32_split(x, pk, bias, "scale_res", gamma, resid)))
    calls.append(("linear_f32_splitk none", lambda: hip.linear_f32_splitk(x, pk6, bias)))
    calls.append(("linear_f32_splitk scale_res", lambda: hip.linear_f32_splitk(x, pk6, bias, "scale_res", gamma, resid)))
    pk_stack, bias_stack = hip.pack_weight_bf16x3(rn(2 * n, k, scale=k ** -0.5)), rn(2, n)
    sel = torch.ones((1,), dtype=torch.int32, device=DEV)
    calls.append(("linear_f32_split_grouped", lambda: hip.linear_f32_split_grouped(x, pk_stack, bias_stack, sel, 256)))

    xc, cb = cl(1, 32, 16, 16), rn(128)
    for kh, stride, pad in ((3, 1, 1), (2, 2, 0)):
        wc = rn(128, 32, kh, kh, scale=(32 * kh * kh) ** -0.5)
        for tag, pack in (("bf16x3", hip.pack_conv_weight_bf16x3), ("f16x2", hip.pack_conv_weight_f16x2)):
            calls.append((f"conv2d_f32_split {kh}x{kh}/{stride}/{pad} {tag}",
                          lambda p=pack(wc), a=(kh, kh, stride, pad): hip.conv2d_f32_split(xc, p, cb, *a)))
    w3, gw, gb = rn(128, 32, 3, 3, scale=288 ** -0.5), rn(128), rn(128)
    for tag, pack in (("bf16x3", hip.pack_conv_weight_bf16x3), ("f16x2", hip.pack_conv_weight_f16x2)):
        calls.append((f"conv3x3_groupnorm_act {tag}",
                      lambda p=pack(w3): hip.conv3x3_groupnorm_act(xc, p, cb, gw, gb, 16, gelu=True, _min_tiles=1)))
    xd, wd = cl(1, 32, 8, 8), rn(32, 32, 2, 2, scale=32 ** -0.5)
    pkd, dg, db = hip.pack_deconv_weight_bf16x3(wd), rn(32), rn(32)
    calls.append(("conv_transpose2d_groupnorm_act", lambda: hip.conv_transpose2d_groupnorm_act(xd, pkd, None, 2, 2, 0, 0, dg, db, 4)))

    c, hidden = 128, 512
    pkm = hip.pack_mlp_fused_f16x2(rn(hidden, c, scale=c ** -0.5), rn(c, hidden, scale=hidden ** -0.5))
    xm, b1, b2, mg, mres = rn(m, c), rn(hidden), rn(c), rn(c), rn(m, c)
    calls.append(("convnext_mlp_f32_fused", lambda: hip.convnext_mlp_f32_fused(xm, pkm, b1, b2, mg, mres)))

    xn, w49c, nb, lw, lb = cl(1, 128, 8, 8), rn(49, 128, scale=1 / 7), rn(128), rn(128), rn(128)
    calls.append(("dwconv7x7_ln", lambda: hip.dwconv7x7_ln(xn, w49c, nb, lw, lb)))
    calls.append(("layernorm_nhwc", lambda: hip.layernorm_nhwc(xn, lw, lb)))
    calls.append(("upsample_bilinear2x", lambda: hip.upsample_bilinear2x(xn)))
    calls.append(("groupnorm_act", lambda: hip.groupnorm_act(xn, lw, lb, 16)))

    xp, p1, p2, p3 = rn(128, 32), rn(128, 8), rn(128, 128, scale=128 ** -0.5), rn(1024, 128, scale=128 ** -0.5)
    pb1, pb2, pb3 = rn(128), rn(128), rn(1024)
    calls.append(("point_pnp_pool", lambda: hip.point_pnp_pool(xp, 8, p1, pb1, p2, pb2, p3, pb3, 1, 128)[0]))     # pooled; the workspace has padding

    a, wk, kb = rn(1, 8, 8, 8), hip.pack_conv_weight_kmajor(rn(8, 8, 1, 1)), rn(8)
    calls.append(("conv_bias_act_f32", lambda: hip.conv_bias_act_f32(a, 0, 8, wk, kb, torch.empty((1, 8, 8, 8), device=DEV), 0, 8, 1, 1, "silu")))
    return calls


def _run(calls):
    out = []
    for label, thunk in calls:
        res = thunk()
        assert res is not None, label
        out.append([t for t in (res if isinstance(res, tuple) else (res,)) if t is not None])
    torch.cuda.synchronize()
    return out


def test_launch_records_counts_and_results_are_the_parents(hip):
    calls = _calls(hip)
    timer, before = hip.LaunchTimer(), hip.x3_launch_count()
    hip.set_launch_timer(timer)
    try:
        timed = _run(calls)
    finally:
        hip.set_launch_timer(None)
    records = [(kind, flops, nbytes) for kind, flops, _, _, nbytes in timer.records]
    for rec in records:
        print(f"    {rec!r},")
    assert hip.x3_launch_count() - before == sum(kind.endswith(hip.X3) for kind, _, _ in records)
    assert all(e0.elapsed_time(e1) >= 0.0 for _, _, e0, e1, _ in timer.records)       # both events were recorded, in order
    plain = _run(calls)
    assert len(timer.records) == len(records)                                           # the timer is out: nothing more arrives
    for (label, _), got, want in zip(calls, plain, timed):
        assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want)), label
    assert hip.split2_range_words() == {}
    assert records == EXPECTED
