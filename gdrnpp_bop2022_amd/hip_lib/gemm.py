"""The split-GEMM family: weight packing, linear / convolution / transposed-convolution launches in the six-product (bf16x3) and
three-product (fp16x2) forms, the fused ConvNeXt MLP, the GEMM + GroupNorm pairs, and the ConvNeXt MLP tail for training (forward
under autograd and its backward: csrc/mlp_bwd.hip beside the six-product linear)."""
from __future__ import annotations

import torch

from . import dispatch
from .abi import DEFINES, channels_last_f32, current_stream, dev_ptr, f32_ptr, launch, load, opt_f32_ptr
from .range_words import count_x3, x3_flag_ptr

X3 = "_x3"   # LaunchTimer kind suffix of the three-product (fp16x2) kernels: 3 instead of 6 MFMA flops per fp32-equivalent flop
A_F16X2_ROWS, C_F16X2_ROWS = DEFINES["GDRNPP_A_F16X2_ROWS"], DEFINES["GDRNPP_C_F16X2_ROWS"]
_EPILOGUES = {"none": 0, "gelu": 1, "scale_res": 2}


def f16x2_rows_decode(t: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(h, l) as float16 tensors of ``t``'s shape from an "f16x2 rows" tensor (tests / debugging): x ~ h + l."""
    k = t.shape[-1]
    v = t.contiguous().view(torch.float16).view(*t.shape[:-1], k // 8, 2, 8)
    return v[..., 0, :].reshape(t.shape), v[..., 1, :].reshape(t.shape)


def pack_weight_bf16x3(weight):
    """nn.Linear weight f32[N,K] -> bf16[N/128, K/16, 3, 2, 128, 8]: exact 3-way bf16 split (w == h + m + l) of every
    128x16 tile, laid out as gdrnpp_linear_f32_split stages it (split, k-block, row, 8 k)."""
    n, k = weight.shape
    packed = torch.empty((n // 128, k // 16, 3, 2, 128, 8), dtype=torch.bfloat16, device=weight.device)
    launch("gdrnpp_pack_weight_bf16x3", f32_ptr(weight, "weight"), packed.data_ptr(), n, k)
    return packed


def pack_weight_f16x2(weight):
    """nn.Linear weight f32[N,K] -> fp16[N/128, K/16, 2, 2, 128, 8]: two-way fp16 split (w * 2^e ~ h + l, 22 significant bits) of
    every 128x16 tile for the three-product kernels (csrc/gemm_split2_pipe.hip).  The returned tensor is a VIEW of a buffer that
    also carries the 16-byte trailer with the power-of-two scale behind the tiles: pass it on as it is (a copy loses the trailer)."""
    n, k = weight.shape
    nbytes = load().gdrnpp_pack_weight_f16x2_bytes(n, k)
    buf = torch.empty((nbytes,), dtype=torch.uint8, device=weight.device)
    launch("gdrnpp_pack_weight_f16x2", f32_ptr(weight, "weight"), buf.data_ptr(), n, k)
    packed = buf[:n * k * 4].view(torch.float16).view(n // 128, k // 16, 2, 2, 128, 8)
    packed._gdrnpp_base = buf
    return packed


def mlp_fused_supported(c: int, hidden: int) -> bool:
    return load().gdrnpp_pack_mlp_fused_f16x2_bytes(int(c), int(hidden)) > 0


def pack_mlp_fused_f16x2(w1, w2):
    """fc1.weight f32[hidden,C], fc2.weight f32[C,hidden] -> the packed image of ``convnext_mlp_f32_fused`` (u8 buffer: per hidden
    tile of 32 the fp16 h / l fragments of both layers in LDS order + a 32-byte trailer with the two power-of-two scales)."""
    hidden, c = w1.shape
    if tuple(w2.shape) != (c, hidden):
        raise ValueError("pack_mlp_fused_f16x2: fc2.weight must be [C, hidden] for fc1.weight [hidden, C]")
    nbytes = load().gdrnpp_pack_mlp_fused_f16x2_bytes(c, hidden)
    if nbytes == 0:
        raise ValueError(f"the fused MLP exists for C = 128, hidden = 512, not {c} / {hidden}")
    buf = torch.empty((nbytes,), dtype=torch.uint8, device=w1.device)
    launch("gdrnpp_pack_mlp_fused_f16x2", f32_ptr(w1, "w1"), f32_ptr(w2, "w2"), buf.data_ptr(), c, hidden)
    return buf


def mlp_fused_rows_in_range(packed_buf) -> tuple:
    """(fc1 ok, fc2 ok): False when the pack kernel found a non-zero weight row of that layer below the three-product range."""
    tr = packed_buf[-32:].view(torch.int32).cpu()
    return int(tr[3]) == 0, int(tr[7]) == 0


def convnext_mlp_f32_fused(x2d, packed_buf, b1, b2, gamma, resid, slot_fc1: int = 0, slot_fc2: int = 0):
    """y = resid + gamma * fc2(gelu(fc1(x))) in one launch (``gdrnpp_convnext_mlp_f32_fused``, three-product form, C = 128)."""
    m, c = x2d.shape
    hidden = b1.shape[0]
    y = torch.empty((m, c), dtype=torch.float32, device=x2d.device)
    count_x3()
    launch("gdrnpp_convnext_mlp_f32_fused", f32_ptr(x2d, "x"), packed_buf.data_ptr(), f32_ptr(b1, "b1"), f32_ptr(b2, "b2"),
           f32_ptr(gamma, "gamma"), f32_ptr(resid, "resid"), y.data_ptr(), m, c, hidden, x3_flag_ptr(slot_fc1), x3_flag_ptr(slot_fc2),
           timed=("mlp_fused" + X3, 4.0 * m * c * hidden, 4.0 * m * c * 3 + 8.0 * c * hidden))    # bytes: x + residual + y, both weights once
    return y


def packed_rows_in_range(packed) -> bool:
    """False when gdrnpp_pack_weight_f16x2 found a non-zero weight row whose scaled rms is below 2^-4 (trailer word 3): the layer
    belongs on the six-product kernels.  One 16-byte read-back, done once per packed weight (x3_policy caches it)."""
    trailer = packed._gdrnpp_base[packed.numel() * 2:].view(torch.int32)
    return int(trailer[3].item()) == 0


def unpack_weight_f16x2(packed):
    """For tests: (fp16[2, N, K] planes h / l of the SCALED weight, 2^-e) of a pack_weight_f16x2 result."""
    tn, tk = packed.shape[:2]
    planes = packed.permute(2, 0, 4, 1, 3, 5).reshape(2, tn * 128, tk * 16)
    trailer = packed._gdrnpp_base[packed.numel() * 2:].view(torch.float32)
    return planes, float(trailer[1])


def unpack_weight_bf16x3(packed):
    """Inverse view of pack_weight_bf16x3 for tests: bf16[3, N, K] planes."""
    tn, tk = packed.shape[:2]
    return packed.permute(2, 0, 4, 1, 3, 5).reshape(3, tn * 128, tk * 16)


def pack_conv_weight_bf16x3(weight):
    """nn.Conv2d weight f32[Cout,Cin,KH,KW] -> packed split image of the [Cout, (ky,kx,Cin)] GEMM weight."""
    cout, cin, kh, kw = weight.shape
    return pack_weight_bf16x3(weight.permute(0, 2, 3, 1).reshape(cout, kh * kw * cin).contiguous())


pack_conv3x3_weight_bf16x3 = pack_conv_weight_bf16x3


def pack_conv_weight_f16x2(weight):
    """nn.Conv2d weight [Cout, Cin, KH, KW] -> pack_weight_f16x2 of the (tap, channel)-ordered [Cout, KH*KW*Cin] matrix."""
    cout, cin, kh, kw = weight.shape
    return pack_weight_f16x2(weight.detach().permute(0, 2, 3, 1).reshape(cout, kh * kw * cin).contiguous())


def pack_deconv_weight_bf16x3(weight):
    """nn.ConvTranspose2d weight [Cin, Cout, KS, KS] -> packed GEMM weight with rows (ky, kx, co), K = Cin."""
    cin, cout, kh, kw = weight.shape
    return pack_weight_bf16x3(weight.detach().permute(2, 3, 1, 0).reshape(kh * kw * cout, cin).contiguous())


def pack_deconv_weight_f16x2(weight):
    """pack_deconv_weight_bf16x3 in the three-product format."""
    cin, cout, kh, kw = weight.shape
    return pack_weight_f16x2(weight.detach().permute(2, 3, 1, 0).reshape(kh * kw * cout, cin).contiguous())


def pack_upconv_weight_bf16x3(weight):
    """nn.Conv2d weight [Cout, Cin, 3, 3] -> packed tap-GEMM weight with rows (ky, kx, co), K = Cin (``upsample2x_conv3x3_groupnorm_act``)."""
    cout, cin, kh, kw = weight.shape
    return pack_weight_bf16x3(weight.detach().permute(2, 3, 0, 1).reshape(kh * kw * cout, cin).contiguous())


def pack_upconv_weight_f16x2(weight):
    """pack_upconv_weight_bf16x3 in the three-product format."""
    cout, cin, kh, kw = weight.shape
    return pack_weight_f16x2(weight.detach().permute(2, 3, 0, 1).reshape(kh * kw * cout, cin).contiguous())


def _packed_weight(weight_packed, k: int, what: str, contiguous: bool = False):
    """Validate a packed split-GEMM weight with GEMM depth ``k`` (``contiguous``: and that it is contiguous); returns
    (N, True for the three-product fp16x2 format).  ``what`` is the caller's message."""
    fp16x2 = weight_packed.dtype == torch.float16     # pack_weight_f16x2: the three-product kernel
    if weight_packed.dtype not in (torch.bfloat16, torch.float16) or weight_packed.dim() != 6 \
            or (contiguous and not weight_packed.is_contiguous()) \
            or weight_packed.shape[1] * 16 != k or weight_packed.shape[2] != (2 if fp16x2 else 3):
        raise ValueError(what)
    return weight_packed.shape[0] * 128, fp16x2


def linear_f32_split(x2d, weight_packed, bias, epilogue: str = "none", gamma=None, resid=None, _kind: str = "linear", x3_slot: int = 0,
                     a_rows: bool = False, c_rows: bool = False):
    """out = epilogue(x2d @ W^T + bias) with the weight given as pack_weight_bf16x3(weight); runs on the bf16 matrix cores
    with six partial products per fp32 product (fp32-accurate, see csrc/gemm_split.hip).  With a pack_weight_f16x2 weight: the
    three-product kernel; there ``a_rows`` = x2d is an "f16x2 rows" tensor (epilogues gelu / scale_res), ``c_rows`` = write the
    result as one (epilogues none / gelu) — gdrnpp_linear_f32_split2_rows, bit-identical to the fp32 hand-over."""
    m, k = x2d.shape
    n, fp16x2 = _packed_weight(weight_packed, k, "weight_packed must be the contiguous tensor from pack_weight_bf16x3 / pack_weight_f16x2 with matching K",
                               contiguous=True)
    out = torch.empty((m, n), dtype=torch.float32, device=x2d.device)
    args = (f32_ptr(x2d, "x"), weight_packed.data_ptr(), opt_f32_ptr(bias, "bias"), opt_f32_ptr(gamma, "gamma"), opt_f32_ptr(resid, "resid"),
            out.data_ptr(), m, n, k, _EPILOGUES[epilogue])
    if (a_rows or c_rows) and not fp16x2:
        raise ValueError("f16x2-rows tensors exist for the three-product kernel (pack_weight_f16x2) only")
    nbytes = 4.0 * m * k + (4.0 if fp16x2 else 6.0) * n * k + 4.0 * m * n * (2 if epilogue == "scale_res" else 1)
    if fp16x2:
        count_x3()
        launch("gdrnpp_linear_f32_split2_rows", *args, (A_F16X2_ROWS if a_rows else 0) | (C_F16X2_ROWS if c_rows else 0), x3_flag_ptr(x3_slot),
               timed=(_kind + X3, 2.0 * m * n * k, nbytes))
    else:
        launch("gdrnpp_linear_f32_split", *args, timed=(_kind, 2.0 * m * n * k, nbytes))
    return out


def linear_f32_split_grouped(x2d, weight_packed_stack, bias_stack, group_sel, rows_per_group: int, n_store: int | None = None):
    """out[m] = x2d[m] @ W[sel[m // rows_per_group]]^T + bias[sel[...]]: the class-sliced output layer of the geometry head.
    ``weight_packed_stack`` = pack_weight_bf16x3 of the slices stacked along N ([groups * N, K]), ``bias_stack`` f32[groups, N],
    ``group_sel`` i32[M / rows_per_group].  Returns f32[M, N]; columns >= n_store are left unwritten.  Rows whose selector is
    outside [0, groups) come back as NaN (nothing is read out of bounds)."""
    m, k = x2d.shape
    n = bias_stack.shape[1]
    if weight_packed_stack.dtype != torch.bfloat16 or weight_packed_stack.dim() != 6 or weight_packed_stack.shape[1] * 16 != k \
            or (weight_packed_stack.shape[0] * 128) % n:
        raise ValueError("weight_packed_stack must come from pack_weight_bf16x3 of the stacked [groups*N, K] weight")
    out = torch.empty((m, n), dtype=torch.float32, device=x2d.device)
    launch("gdrnpp_linear_f32_split_grouped", f32_ptr(x2d, "x"), weight_packed_stack.data_ptr(), f32_ptr(bias_stack, "bias_stack"),
           dev_ptr(group_sel, torch.int32, "group_sel"), int(bias_stack.shape[0]), int(rows_per_group), out.data_ptr(), m, n, k,
           int(n_store if n_store is not None else n),
           timed=("linear_grouped", 2.0 * m * n * k, 4.0 * m * k + 6.0 * n * k * group_sel.numel() + 4.0 * m * (n_store or n)))
    return out


def _grouped_grad_shapes(what: str, d_out, n_out: int, group_sel, rows_per_group: int):
    m, pitch = d_out.shape
    if rows_per_group <= 0 or m % rows_per_group or group_sel.numel() != m // rows_per_group or not 0 < n_out <= pitch:
        raise RuntimeError(f"{what}: d_out {tuple(d_out.shape)}, n_out={n_out}, {group_sel.numel()} selectors, rows_per_group={rows_per_group} do not fit")
    return m, pitch


def grouped_linear_dinput(d_out, weight_slices, group_sel, rows_per_group: int):
    """Data gradient of ``linear_f32_split_grouped`` (``gdrnpp_grouped_linear_dinput_f32``): dfeat[m] = d_out[m, :n_out] @
    W[sel[m // rows_per_group]] -> f32[M, K], for ``weight_slices`` f32[slices, n_out, K] (the sliced weight itself, nothing packed)
    and ``d_out`` f32[M, pitch], whose columns from n_out on are never used.  One fp32 chain in column order on the exact-f32 matrix
    instruction.  Rows whose selector is outside [0, slices) come back as NaN."""
    n_slices, n_out, k = weight_slices.shape
    m, pitch = _grouped_grad_shapes("grouped_linear_dinput", d_out, n_out, group_sel, rows_per_group)
    dfeat = torch.empty((m, k), dtype=torch.float32, device=d_out.device)
    launch("gdrnpp_grouped_linear_dinput_f32", f32_ptr(d_out, "d_out"), pitch, n_out, f32_ptr(weight_slices, "weight_slices"),
           dev_ptr(group_sel, torch.int32, "group_sel"), n_slices, int(rows_per_group), dfeat.data_ptr(), m, k,
           timed=("mfma_f32:grouped_dinput", 2.0 * m * n_out * k, 4.0 * m * (72 + k) + 4.0 * n_out * k * group_sel.numel()))
    return dfeat


def grouped_linear_wgrad(d_out, feat2d, group_sel, cls_rows, n_slices: int, out_rows: int, rows_per_group: int, want=(True, True)):
    """Weight and bias gradient of ``linear_f32_split_grouped`` by slice (``gdrnpp_grouped_linear_wgrad_f32``) -> (dW f32[out_rows, K],
    db f32[out_rows]), shaped like the layer's own parameters: row cls_rows[c, j] holds channel j of slice c, summed over the groups
    with selector c in index order (fp64, fixed slots, one rounding).  ``cls_rows`` i64[slices, n_out] on the device.  Rows of a slice
    no group selects are 0, as are rows ``cls_rows`` does not name; groups with a selector outside [0, slices) are left out.
    ``want`` = (dW, db): an entry is None where its flag is false, the other keeps its bits; with neither nothing is launched."""
    want_w, want_b = bool(want[0]), bool(want[1])
    if not (want_w or want_b):
        return None, None
    n_out = cls_rows.shape[1]
    m, pitch = _grouped_grad_shapes("grouped_linear_wgrad", d_out, n_out, group_sel, rows_per_group)
    k = feat2d.shape[1]
    b = m // rows_per_group
    if feat2d.shape[0] != m or tuple(cls_rows.shape) != (n_slices, n_out):
        raise RuntimeError(f"grouped_linear_wgrad: feat {tuple(feat2d.shape)} / cls_rows {tuple(cls_rows.shape)} do not fit d_out {tuple(d_out.shape)}")
    nbytes = load().gdrnpp_grouped_linear_wgrad_f32_workspace_bytes(b, int(rows_per_group), k, n_out)
    if nbytes == 0:
        raise RuntimeError(f"grouped_linear_wgrad: rows_per_group={rows_per_group} must be a multiple of 256, K={k} of 128, n_out={n_out} <= 72")
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=d_out.device)
    # rows the table does not name stay 0 (a table over all rows, as the class-aware and the class-agnostic heads have, leaves none)
    alloc = torch.empty if cls_rows.numel() == out_rows else torch.zeros
    dw = alloc((out_rows, k), dtype=torch.float32, device=d_out.device) if want_w else None
    db = alloc((out_rows,), dtype=torch.float32, device=d_out.device) if want_b else None
    launch("gdrnpp_grouped_linear_wgrad_f32", f32_ptr(d_out, "d_out"), pitch, n_out, f32_ptr(feat2d, "feat"),
           dev_ptr(group_sel, torch.int32, "group_sel"), int(n_slices), dev_ptr(cls_rows, torch.int64, "cls_rows"), int(out_rows),
           dw.data_ptr() if want_w else None, db.data_ptr() if want_b else None, b, int(rows_per_group), k, ws.data_ptr(), nbytes,
           timed=("mfma_f32:grouped_wgrad", 2.0 * m * 128 * k if want_w else 0.0, 4.0 * m * (72 + (k if want_w else 0)) + 2.0 * nbytes))
    return dw, db


def linear_f32_splitk(x2d, weight_packed, bias, epilogue: str = "none", gamma=None, resid=None):
    """Same contract as linear_f32_split for problems with few output tiles: split-K with a deterministic reduction that
    also applies bias and epilogue."""
    m, k = x2d.shape
    if weight_packed.dtype != torch.bfloat16 or weight_packed.dim() != 6 or weight_packed.shape[1] * 16 != k:   # six-product only
        raise ValueError("weight_packed must be the contiguous bf16 tensor from pack_weight_bf16x3 with matching K")
    n = weight_packed.shape[0] * 128
    out = torch.empty((m, n), dtype=torch.float32, device=x2d.device)
    nbytes = load().gdrnpp_linear_f32_splitk_workspace_bytes(m, n, k)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x2d.device)
    launch("gdrnpp_linear_f32_splitk", f32_ptr(x2d, "x"), weight_packed.data_ptr(), opt_f32_ptr(bias, "bias"), opt_f32_ptr(gamma, "gamma"),
           opt_f32_ptr(resid, "resid"), out.data_ptr(), m, n, k, _EPILOGUES[epilogue], ws.data_ptr(), nbytes,
           timed=("linear_splitk", 2.0 * m * n * k, 4.0 * m * k + 6.0 * n * k + 4.0 * m * n * (2 if epilogue == "scale_res" else 1)))
    return out


def conv2d_f32_split(x_cl, weight_packed, bias, kh: int, kw: int, stride: int, pad: int, gelu: bool = False, _kind: str = "conv",
                     x3_slot: int = 0):
    """KHxKW / stride / zero-pad convolution of a channels_last tensor [N,Cin,H,W] on the bf16 matrix cores (fp32-accurate
    split GEMM, implicit im2col) -> channels_last [N,Cout,OH,OW]."""
    n, cin, h, w = channels_last_f32(x_cl, "conv2d_f32_split")
    cout, fp16x2 = _packed_weight(weight_packed, kh * kw * cin, "weight_packed must come from pack_conv_weight_bf16x3 / pack_conv_weight_f16x2 with matching Cin and kernel size")
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    out = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=x_cl.device, memory_format=torch.channels_last)
    if fp16x2 and kh * kw > 32:
        raise ValueError("the three-product convolution takes at most 32 taps")
    args = (x_cl.data_ptr(), weight_packed.data_ptr(), opt_f32_ptr(bias, "bias"),
            out.data_ptr(), n, h, w, cin, cout, kh, kw, stride, pad, 1 if gelu else 0)
    flops = 2.0 * n * oh * ow * cout * kh * kw * cin
    nbytes = 4.0 * n * (h * w * cin + oh * ow * cout) + (4.0 if fp16x2 else 6.0) * cout * kh * kw * cin
    if fp16x2:
        count_x3()
        launch("gdrnpp_conv2d_f32_split2", *args, x3_flag_ptr(x3_slot), timed=(_kind + X3, flops, nbytes))
        return out
    ws_bytes = load().gdrnpp_conv2d_f32_splitk_workspace_bytes(n, oh, ow, cin, cout, kh, kw) if dispatch._CONV_SPLITK else 0
    if ws_bytes:    # few output tiles (small ROI batches): K in chunks, partial sums through a workspace
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=x_cl.device)
        launch("gdrnpp_conv2d_f32_splitk", *args, ws.data_ptr(), ws_bytes, timed=("conv_splitk", flops, nbytes))
    else:
        launch("gdrnpp_conv2d_f32_split", *args, timed=(_kind, flops, nbytes))
    return out


def conv3x3_f32_split(x_cl, weight_packed, bias, gelu: bool = False, x3_slot: int = 0):
    """3x3 / stride 1 / pad 1 convolution of a channels_last tensor [N,Cin,H,W] on the bf16 matrix cores (fp32-accurate
    split GEMM, implicit im2col) -> channels_last [N,Cout,H,W] (gdrnpp_conv3x3_f32_split = the general entry with 3, 3, 1, 1)."""
    return conv2d_f32_split(x_cl, weight_packed, bias, 3, 3, 1, 1, gelu, _kind="conv3x3", x3_slot=x3_slot)


def _deconv_cols(x_cl, weight_packed, ks: int, stride: int, pad: int, out_pad: int, x3_slot: int, what: str):
    """First half of a transposed convolution: the GEMM into ``cols`` [N*H*W, KS*KS*Cout] and the empty channels_last result
    the col2im gather fills; returns (cols, y, cout, oh, ow)."""
    n, cin, h, w = channels_last_f32(x_cl, what)
    cout = weight_packed.shape[0] * 128 // (ks * ks)
    cols = linear_f32_split(x_cl.permute(0, 2, 3, 1).reshape(n * h * w, cin), weight_packed, None, _kind="deconv", x3_slot=x3_slot)
    oh, ow = (h - 1) * stride - 2 * pad + ks + out_pad, (w - 1) * stride - 2 * pad + ks + out_pad
    y = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=x_cl.device, memory_format=torch.channels_last)
    return cols, y, cout, oh, ow


def conv_transpose2d_f32_split(x_cl, weight_packed, bias, ks: int, stride: int, pad: int, out_pad: int, x3_slot: int = 0):
    """nn.ConvTranspose2d of a channels_last tensor [N,Cin,H,W] as split GEMM + col2im gather -> channels_last
    [N,Cout,OH,OW] (``weight_packed`` from pack_deconv_weight_bf16x3)."""
    n, _, h, w = x_cl.shape
    cols, y, cout, _, _ = _deconv_cols(x_cl, weight_packed, ks, stride, pad, out_pad, x3_slot, "conv_transpose2d_f32_split")
    launch("gdrnpp_deconv_col2im_nhwc", cols.data_ptr(), opt_f32_ptr(bias, "bias"), y.data_ptr(), n, h, w, cout, ks, stride, pad, out_pad)
    return y


def _groupnorm_apply(y, part, P: int, gamma, beta, n: int, hw: int, cout: int, groups: int, eps: float, gelu: bool):
    """Second half of a GEMM + GroupNorm pair: normalise ``y`` with the partial sums the GEMM's epilogue / gather left in ``part``."""
    out = torch.empty_like(y)
    launch("gdrnpp_groupnorm_apply_nhwc", y.data_ptr(), part.data_ptr(), P, f32_ptr(gamma, "gamma"), f32_ptr(beta, "beta"),
           out.data_ptr(), n, hw, cout, groups, float(eps), 1 if gelu else 0, timed=("hbm:groupnorm_apply", 0.0, 8.0 * y.numel()))
    return out


def conv_transpose2d_groupnorm_act(x_cl, weight_packed, bias, ks: int, stride: int, pad: int, out_pad: int, gamma, beta, groups: int,
                                   eps: float = 1e-5, gelu: bool = False, x3_slot: int = 0):
    """nn.ConvTranspose2d -> GroupNorm(groups) [-> GELU] of a channels_last tensor: split GEMM, then the col2im gather leaves the
    GroupNorm partial sums (``gdrnpp_deconv_col2im_gn_nhwc``) and the norm is one more pass (``gdrnpp_groupnorm_apply_nhwc``) —
    bitwise the result of conv_transpose2d_f32_split + groupnorm_act, one launch fewer."""
    n, _, h, w = x_cl.shape
    cols, y, cout, oh, ow = _deconv_cols(x_cl, weight_packed, ks, stride, pad, out_pad, x3_slot, "conv_transpose2d_groupnorm_act")
    nbytes = load().gdrnpp_groupnorm_workspace_bytes(n, oh * ow, groups)
    P = nbytes // (16 * n * groups)
    part = torch.empty((n, P, groups, 2), dtype=torch.float64, device=x_cl.device)
    launch("gdrnpp_deconv_col2im_gn_nhwc", cols.data_ptr(), opt_f32_ptr(bias, "bias"), y.data_ptr(), part.data_ptr(), n, h, w, cout, ks, stride,
           pad, out_pad, groups)
    return _groupnorm_apply(y, part, P, gamma, beta, n, oh * ow, cout, groups, eps, gelu)


def conv3x3_groupnorm_act(x_cl, weight_packed, bias, gamma, beta, groups: int, eps: float = 1e-5, gelu: bool = False, x3_slot: int = 0,
                          _min_tiles: int = 256):
    """conv3x3 (stride 1, pad 1) -> GroupNorm(groups) [-> GELU] of a channels_last tensor: the convolution's epilogue
    leaves the GroupNorm partial sums, the norm is one more pass (``gdrnpp_conv3x3_f32_split_gnstats`` +
    ``gdrnpp_groupnorm_apply_nhwc``).  Returns None when the shape is outside the fused form (H*W % 256, 8 channels
    per group) or the launch has fewer than 256 tiles of 256 x 128 (a dispatch rule, not a limit of the kernels; ``_min_tiles`` is a
    test / A-B knob like ``_kind``, not a tuning parameter: tests lower it to reach the kernels' smallest shape): the caller then runs the two layers separately."""
    n, cin, h, w = channels_last_f32(x_cl, "conv3x3_groupnorm_act")
    cout, fp16x2 = _packed_weight(weight_packed, 9 * cin, "weight_packed must come from pack_conv_weight_bf16x3 / pack_conv_weight_f16x2 with matching Cin")
    P = load().gdrnpp_conv3x3_gnstats_partials(h, w)
    if P <= 0 or cout != 8 * groups or (n * h * w // 256) * (cout // 128) < _min_tiles:   # below: the 128x128-tile kernels are faster
        return None
    y = torch.empty((n, cout, h, w), dtype=torch.float32, device=x_cl.device, memory_format=torch.channels_last)
    part = torch.empty((n, P, groups, 2), dtype=torch.float64, device=x_cl.device)
    args = (x_cl.data_ptr(), weight_packed.data_ptr(), opt_f32_ptr(bias, "bias"), y.data_ptr(), part.data_ptr(), n, h, w, cin, cout, groups)
    flops = 2.0 * n * h * w * cout * 9 * cin
    nbytes = 4.0 * n * h * w * (cin + cout) + (4.0 if fp16x2 else 6.0) * cout * 9 * cin
    if fp16x2:
        count_x3()
        launch("gdrnpp_conv3x3_f32_split2", *args, 0, x3_flag_ptr(x3_slot), timed=("conv3x3" + X3, flops, nbytes))
    else:
        launch("gdrnpp_conv3x3_f32_split_gnstats", *args, timed=("conv3x3", flops, nbytes))
    return _groupnorm_apply(y, part, P, gamma, beta, n, h * w, cout, groups, eps, gelu)


def upsample2x_conv3x3_raw(x_cl, weight_packed, bias, groups: int, x3_slot: int = 0, chunk: int = 0):
    """nn.UpsamplingBilinear2d(2) -> conv3x3 (stride 1, zero pad 1) of a channels_last tensor [N,Cin,H,W] without forming the
    upsampled tensor: per chunk of ``chunk`` images (0 = all at once) the tap GEMM of the LOW-resolution pixels into
    [n*H*W, 9*Cout] (``weight_packed`` from pack_upconv_weight_f16x2 / _bf16x3; a quarter of the convolution's matrix work), then
    ``gdrnpp_upconv_gather_gn_nhwc`` interpolates and sums the nine tap planes -> (raw convolution output, channels_last
    [N,Cout,2H,2W]; GroupNorm(groups) partial sums f64[N,P,groups,2]; P).  Bitwise independent of ``chunk``."""
    n, cin, h, w = channels_last_f32(x_cl, "upsample2x_conv3x3_raw")
    cols, _ = _packed_weight(weight_packed, cin, "weight_packed must come from pack_upconv_weight_bf16x3 / pack_upconv_weight_f16x2 with matching Cin",
                             contiguous=True)
    if cols % 9:
        raise ValueError("weight_packed must hold the nine taps of a 3x3 kernel")
    cout = cols // 9
    P = load().gdrnpp_upconv_gather_partials(h, w, cout)
    if P <= 0:
        raise ValueError(f"upsample2x_conv3x3_raw: shape H={h} W={w} Cout={cout} is outside the gather kernel")
    y = torch.empty((n, cout, 2 * h, 2 * w), dtype=torch.float32, device=x_cl.device, memory_format=torch.channels_last)
    part = torch.empty((n, P, groups, 2), dtype=torch.float64, device=x_cl.device)
    x2d = x_cl.permute(0, 2, 3, 1).reshape(n * h * w, cin)      # a view of the NHWC memory
    y_nhwc = y.permute(0, 2, 3, 1)
    step = n if chunk <= 0 else min(int(chunk), n)
    for n0 in range(0, n, step):
        n1 = min(n, n0 + step)
        taps = linear_f32_split(x2d[n0 * h * w:n1 * h * w], weight_packed, None, _kind="upconv_taps", x3_slot=x3_slot)
        launch("gdrnpp_upconv_gather_gn_nhwc", taps.data_ptr(), opt_f32_ptr(bias, "bias"), y_nhwc[n0:n1].data_ptr(), part[n0:n1].data_ptr(),
               n1 - n0, h, w, cout, groups, timed=("hbm:upconv_gather", 0.0, 4.0 * (n1 - n0) * h * w * cout * (9 + 4)))
    return y, part, P


def upsample2x_conv3x3_groupnorm_act(x_cl, weight_packed, bias, gamma, beta, groups: int, eps: float = 1e-5, gelu: bool = False,
                                     x3_slot: int = 0, chunk: int = 0):
    """nn.UpsamplingBilinear2d(2) -> conv3x3 (stride 1, pad 1) -> GroupNorm(groups) [-> GELU] of a channels_last tensor at the low
    resolution (``upsample2x_conv3x3_raw``) + ``gdrnpp_groupnorm_apply_nhwc``."""
    y, part, P = upsample2x_conv3x3_raw(x_cl, weight_packed, bias, groups, x3_slot, chunk)
    n, cout, oh, ow = y.shape
    return _groupnorm_apply(y, part, P, gamma, beta, n, oh * ow, cout, groups, eps, gelu)


# ---- training: the ConvNeXt MLP tail under autograd (csrc/mlp_bwd.hip) ----------------------------------------------------------
def pack_weight_bf16x3_t(weight, row_scale=None):
    """``pack_weight_bf16x3((weight * row_scale[:, None]).t().contiguous())`` read straight from ``weight`` f32[R,K] (``row_scale``
    f32[R] or None) -> bf16[K/128, R/16, 3, 2, 128, 8]: the operand of a data-gradient product, without a transpose or a multiply
    kernel.  Byte for byte that composition."""
    r, k = weight.shape
    if row_scale is not None and row_scale.numel() != r:
        raise RuntimeError(f"pack_weight_bf16x3_t: row_scale must be f32[{r}]")
    packed = torch.empty((k // 128, r // 16, 3, 2, 128, 8), dtype=torch.bfloat16, device=weight.device)
    launch("gdrnpp_pack_weight_bf16x3_t", f32_ptr(weight, "weight"), opt_f32_ptr(row_scale, "row_scale"), packed.data_ptr(), r, k)
    return packed


def gelu_f32(pre):
    """h = gelu(pre) (exact-erf form) with the function of the split GEMMs' GELU epilogue (``gdrnpp_gelu_f32``)."""
    h = torch.empty_like(pre)
    launch("gdrnpp_gelu_f32", f32_ptr(pre, "pre"), h.data_ptr(), pre.numel(), timed=("hbm:gelu", 0.0, 8.0 * pre.numel()))
    return h


def _colsum_ws(m: int, cols: int, device):
    nbytes = load().gdrnpp_colsum_workspace_bytes(m, cols)
    return torch.empty((max(nbytes, 16) // 8,), dtype=torch.float64, device=device), nbytes


def colsum_f32(x2d, scale=None, want32: bool = True):
    """Column sums of x2d f32[M,cols] in fp64, fixed order -> (sum64 f64[cols], fl(scale * sum) f32[cols] or None)."""
    m, cols = x2d.shape
    ws, nbytes = _colsum_ws(m, cols, x2d.device)
    s64 = torch.empty((cols,), dtype=torch.float64, device=x2d.device)
    s32 = torch.empty((cols,), dtype=torch.float32, device=x2d.device) if want32 else None
    launch("gdrnpp_colsum_f32", f32_ptr(x2d, "x"), opt_f32_ptr(scale, "scale"), s64.data_ptr(), s32.data_ptr() if want32 else None, m, cols,
           ws.data_ptr(), nbytes, timed=("hbm:colsum", 0.0, 4.0 * x2d.numel()))
    return s64, s32


def mlp_bwd_act_(pre, dh, want_h: bool = True, want_db1: bool = True):
    """``gdrnpp_mlp_bwd_act``: dh f32[M,H] becomes dpre = dh * gelu'(pre) IN PLACE -> (h = gelu(pre) or None, db1 = colsum(dpre) or None)."""
    m, cols = pre.shape
    if tuple(dh.shape) != (m, cols):
        raise RuntimeError(f"mlp_bwd_act_: dh must be f32[{m},{cols}] as pre is, got {tuple(dh.shape)}")
    ws, nbytes = _colsum_ws(m, cols, pre.device)
    h = torch.empty_like(pre) if want_h else None
    db1 = torch.empty((cols,), dtype=torch.float32, device=pre.device) if want_db1 else None
    launch("gdrnpp_mlp_bwd_act", f32_ptr(pre, "pre"), f32_ptr(dh, "dh"), h.data_ptr() if want_h else None, db1.data_ptr() if want_db1 else None,
           m, cols, ws.data_ptr(), nbytes, timed=("hbm:mlp_bwd_act", 0.0, 4.0 * pre.numel() * (3 + want_h)))
    return h, db1


def gemm_tn_f32(a, b, row_scale=None, w=None, bias=None, sg=None, want_g: bool = True, persistent_ws: bool = False):
    """G[N1,N2] = a^T b for a f32[M,N1], b f32[M,N2] (N1, N2 multiples of 128, any M >= 1) on the exact-f32 matrix instruction
    (``gdrnpp_gemm_tn_f32``): the weight-gradient product.  Deterministic: fixed slots, fp64 finalize, one rounding.
    ``row_scale`` f32[N1]: G[c,:] = fl(row_scale[c] * sum).  With ``w`` f32[N1,N2], ``bias`` f32[N1] and ``sg`` f64[N1] the result is
    (G, drow) with drow[c] = fl(sum_k w[c,k] sum[c,k] + bias[c] sg[c]), the layer-scale gradient, taken before G is rounded;
    ``want_g`` False leaves G out (None).  ``persistent_ws``: the slot tiles live in ``workspace`` (kept per device and stream) instead
    of a tensor of this call."""
    m, n1 = a.shape
    if b.dim() != 2 or b.shape[0] != m:
        raise RuntimeError(f"gemm_tn_f32: b must have the {m} rows of a, got {tuple(b.shape)}")
    n2 = b.shape[1]
    layer_scale = w is not None
    if layer_scale and (bias is None or sg is None or tuple(w.shape) != (n1, n2) or bias.numel() != n1 or sg.numel() != n1):
        raise RuntimeError(f"gemm_tn_f32: the layer-scale form takes w f32[{n1},{n2}], bias f32[{n1}] and sg f64[{n1}]")
    if not (want_g or layer_scale):
        raise RuntimeError("gemm_tn_f32: nothing asked for")
    nbytes = load().gdrnpp_gemm_tn_f32_workspace_bytes(m, n1, n2)
    if nbytes == 0:
        raise RuntimeError(f"gemm_tn_f32: N1={n1} N2={n2} must be multiples of 128 (M={m} >= 1)")
    ws = workspace(a.device, nbytes) if persistent_ws else torch.empty((nbytes // 8,), dtype=torch.float64, device=a.device)
    g = torch.empty((n1, n2), dtype=torch.float32, device=a.device) if want_g else None
    drow = torch.empty((n1,), dtype=torch.float32, device=a.device) if layer_scale else None
    launch("gdrnpp_gemm_tn_f32", f32_ptr(a, "a"), f32_ptr(b, "b"), g.data_ptr() if want_g else None, m, n1, n2, opt_f32_ptr(row_scale, "row_scale"),
           opt_f32_ptr(w, "w"), opt_f32_ptr(bias, "bias"), dev_ptr(sg, torch.float64, "sg") if layer_scale else None,
           drow.data_ptr() if layer_scale else None, ws.data_ptr(), nbytes, timed=("gemm_tn", 2.0 * m * n1 * n2, 4.0 * m * (n1 + n2) + 4.0 * n1 * n2))
    return (g, drow) if layer_scale else g


def linear_f32_exact(x2d, weight, bias=None, gamma=None, resid=None, weight_kn: bool = False, row_scale=None):
    """out = x2d @ weight^T + bias (``weight`` f32[N,K], as nn.Linear holds it) or, ``weight_kn``, x2d @ (row_scale[:, None] * weight)
    for a weight f32[K,N]; with ``gamma`` and ``resid``: resid + gamma * (that).  ``gdrnpp_linear_f32_exact``: the exact-f32 matrix
    instruction, fp32 chains of 128 carried in fp64, one rounding — for products too deep for the six-product kernel's accuracy."""
    m, k = x2d.shape
    n = weight.shape[1] if weight_kn else weight.shape[0]
    if tuple(weight.shape) != ((k, n) if weight_kn else (n, k)):
        raise RuntimeError(f"linear_f32_exact: weight {tuple(weight.shape)} does not fit x [{m},{k}]")
    if (gamma is None) != (resid is None) or (row_scale is not None and not weight_kn):
        raise RuntimeError("linear_f32_exact: gamma and resid come together; row_scale goes with weight_kn")
    out = torch.empty((m, n), dtype=torch.float32, device=x2d.device)
    nbytes = load().gdrnpp_linear_f32_exact_workspace_bytes(m, n, k)      # 0: one depth slot, no workspace
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x2d.device) if nbytes else None
    launch("gdrnpp_linear_f32_exact", f32_ptr(x2d, "x"), f32_ptr(weight, "weight"), 0 if weight_kn else 1, opt_f32_ptr(row_scale, "row_scale"),
           opt_f32_ptr(bias, "bias"), opt_f32_ptr(gamma, "gamma"), opt_f32_ptr(resid, "resid"), out.data_ptr(), m, n, k,
           ws.data_ptr() if nbytes else None, nbytes,
           timed=("linear_exact", 2.0 * m * n * k, 4.0 * (m * k + n * k + m * n * (2 if gamma is not None else 1))))
    return out


# Deepest product of the training tail that runs on the six-product kernel.  Measured on an MI355X against fp64 on the same operands,
# beside a CPU sgemm: gdrnpp_linear_f32_split 1.3 - 1.6e-6 at K = 128 (CPU 1.7 - 2.0e-6), 2.5e-6 at 256 (1.8e-6), 2.5 - 3.0e-6 at 512
# (1.4 - 1.7e-6), 3.5 - 3.7e-6 at 1024 (1.1 - 1.4e-6): from 512 on it is at or past the factor 2 the gradient tests' bar allows, so
# those products take linear_f32_exact.  Inference is not concerned.
_SIX_PRODUCT_MAX_DEPTH = 256


def _tail_product(a, w, bias=None, epilogue="none", gamma=None, resid=None, weight_kn=False, row_scale=None):
    """One forward-shaped product of the training tail: a @ w^T (w [N,K]) or, ``weight_kn``, a @ (row_scale[:, None] * w) (w [K,N])."""
    if a.shape[1] > _SIX_PRODUCT_MAX_DEPTH:
        return linear_f32_exact(a, w, bias, gamma, resid, weight_kn, row_scale)
    packed = pack_weight_bf16x3_t(w, row_scale) if weight_kn else pack_weight_bf16x3(w)
    return linear_f32_split(a, packed, bias, epilogue, gamma, resid)


def convnext_mlp_forward_train(x2d, w1, b1, w2, b2, gamma, resid):
    """The ConvNeXt MLP tail for autograd -> (y, pre): pre = x2d W1^T + b1 (kept for the backward), y = resid + gamma * (gelu(pre)
    W2^T + b2).  Products up to a depth of 256 on the six-product split GEMM with the weights packed per call (they change every
    step), deeper ones on ``linear_f32_exact``; h is not kept."""
    pre = _tail_product(x2d, w1, b1)
    y = _tail_product(gelu_f32(pre), w2, b2, "scale_res", gamma, resid)
    return y, pre


def convnext_mlp_backward(x2d, pre, w1, w2, b2, gamma, grad_y, want=(True,) * 6):
    """Gradients of ``convnext_mlp_forward_train`` for grad_y = dL/dy f32[M,C] -> (dx, dw1, db1, dw2, db2, dgamma); the shortcut's
    gradient is grad_y itself.  ``want``: six flags in that order — an entry is None where its flag is false and the kernels only it
    needs are not launched; the others keep their bits.  Saved from the forward: x2d and pre only (h is recomputed, z never formed:
    dgamma = rowsum(W2 * G) + b2 * colsum(g) with G = g^T h).  Fixed summation order: two calls give the same bits."""
    what = "convnext_mlp_backward"
    want = tuple(bool(f) for f in want)
    if len(want) != 6 or not any(want):
        raise RuntimeError(f"{what}: want must hold six flags, at least one of them set")
    m, c = x2d.shape
    hid = w1.shape[0]
    if tuple(pre.shape) != (m, hid) or tuple(w1.shape) != (hid, c) or tuple(w2.shape) != (c, hid) or tuple(grad_y.shape) != (m, c) \
            or b2.numel() != c or gamma.numel() != c:
        raise RuntimeError(f"{what}: shapes x [{m},{c}], pre {tuple(pre.shape)}, w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)}, grad_y {tuple(grad_y.shape)} do not fit")
    w_dx, w_dw1, w_db1, w_dw2, w_db2, w_dg = want
    need_dpre, need_g = w_dx or w_dw1 or w_db1, w_dw2 or w_dg
    dx = dw1 = db1 = dw2 = db2 = dgamma = h = None
    if need_dpre:
        dpre = _tail_product(grad_y, w2, weight_kn=True, row_scale=gamma)        # dh = g (diag(gamma) W2), then in place
        h, db1 = mlp_bwd_act_(pre, dpre, want_h=need_g, want_db1=w_db1)
        if w_dx:
            dx = _tail_product(dpre, w1, weight_kn=True)
        if w_dw1:
            dw1 = gemm_tn_f32(dpre, x2d)
    elif need_g:
        h = gelu_f32(pre)
    if need_g or w_db2:
        sg, db2 = colsum_f32(grad_y, gamma, want32=w_db2)
    if need_g:
        dw2, dgamma = gemm_tn_f32(grad_y, h, gamma, w2, b2, sg, want_g=w_dw2)
        if not w_dg:
            dgamma = None
    return dx, dw1, db1, dw2, db2, dgamma


# ---- training: the geometry head's [conv3x3, GroupNorm(, GELU)] under autograd (csrc/conv_gn_bwd.hip) ----------------------------
# The two forward-shaped convolutions (z, and dx = conv3x3(dz, W')) have a depth of 9 Cin = 1152 - 2304.  Measured on an MI355X, error
# over the gradient tests' bar at depths 1152 / 2304 / 2304 (tools/head_bwd_microbench.py --engine-errors, profiles/head_bwd_microbench.json):
#   six-product conv3x3 on its 256-row tiles (what a training batch runs)   1.87 / 2.49 / 2.37     1.01 ms per 48-ROI layer
#   six-product conv3x3 as dispatched at those small sizes (K cut in chunks) 0.34 / 0.40 / 0.42
#   gdrnpp_conv_bias_act_f32 (fp32 MFMA, two-level fp32 sums)                0.42 / 0.40 / 0.42     2.59 ms
#   an implicit GEMM with gemm_rows' fp64 carries, written for this and not kept  0.39 / 0.39 / 0.32   2.50 ms
# So both run on gdrnpp_conv_bias_act_f32 as it is: inside the bar whatever the launch size, and within 5 % of the kernel not kept.
_ACT_NONE = DEFINES["GDRNPP_ACT_NONE"]


def conv3x3_weight_kn(weight):
    """nn.Conv2d weight [Cout,Cin,3,3] -> the forward operand of ``conv3x3_f32_mfma``: f32[9 Cin, Cout], row (ky 3 + kx) Cin + ci."""
    cout, cin = weight.shape[:2]
    return weight.detach().permute(2, 3, 1, 0).reshape(9 * cin, cout).contiguous()


def conv3x3_weight_kn_flipped(weight):
    """nn.Conv2d weight [Cout,Cin,3,3] -> the data-gradient operand W'[(ky 3 + kx) Cout + co][ci] = W[co][ci][2-ky][2-kx], f32[9 Cout, Cin]."""
    cout, cin = weight.shape[:2]
    return weight.detach().flip(2, 3).permute(2, 3, 0, 1).reshape(9 * cout, cin).contiguous()


def conv3x3_f32_mfma(x_cl, weight_kn, bias=None):
    """3x3 / stride 1 / zero pad 1 convolution of a channels_last tensor [N,Cin,H,W] with ``weight_kn`` f32[9 Cin, Cout]
    (``conv3x3_weight_kn``) on the exact-f32 matrix instruction (``gdrnpp_conv_bias_act_f32`` without activation or residual: fp32
    sums in a fixed two-level order, bit-reproducible) -> channels_last [N,Cout,H,W].  Cin % 4 == 0, Cout % 4 == 0."""
    n, cin, h, w = channels_last_f32(x_cl, "conv3x3_f32_mfma")
    if weight_kn.dim() != 2 or weight_kn.shape[0] != 9 * cin:
        raise RuntimeError(f"conv3x3_f32_mfma: weight_kn must be f32[{9 * cin},Cout], got {tuple(weight_kn.shape)}")
    cout = weight_kn.shape[1]
    if cin % 4 or cout % 4:
        raise RuntimeError(f"conv3x3_f32_mfma: Cin={cin} and Cout={cout} must be multiples of 4")
    out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x_cl.device, memory_format=torch.channels_last)
    launch("gdrnpp_conv_bias_act_f32", x_cl.data_ptr(), cin, 0, f32_ptr(weight_kn, "weight_kn"), cout, opt_f32_ptr(bias, "bias"), None, 0, 0,
           out.data_ptr(), cout, 0, 0, 0, n, h, w, cin, cout, 3, 1, _ACT_NONE, 0.0,
           timed=("mfma_f32:conv3x3", 2.0 * n * h * w * cout * 9 * cin, 4.0 * n * h * w * (cin + cout) + 36.0 * cin * cout))
    return out


def conv3x3_wgrad_f32(dz_cl, x_cl):
    """dW f32[Cout,Cin,3,3] = the weight gradient of a 3x3 / stride 1 / zero pad 1 convolution for dz [N,Cout,H,W] and its input x
    [N,Cin,H,W], both channels_last (``gdrnpp_conv3x3_wgrad_f32``: implicit TN GEMM on the exact-f32 matrix instruction, fixed slots,
    fp64 finalize, one rounding).  Cin % 128 == 0, Cout % 128 == 0."""
    n, cout, h, w = channels_last_f32(dz_cl, "conv3x3_wgrad_f32")
    xn, cin, xh, xw = channels_last_f32(x_cl, "conv3x3_wgrad_f32")
    if (xn, xh, xw) != (n, h, w):
        raise RuntimeError(f"conv3x3_wgrad_f32: x {tuple(x_cl.shape)} does not fit dz {tuple(dz_cl.shape)}")
    nbytes = load().gdrnpp_conv3x3_wgrad_f32_workspace_bytes(n, h, w, cin, cout)
    if nbytes == 0:
        raise RuntimeError(f"conv3x3_wgrad_f32: Cin={cin} and Cout={cout} must be multiples of 128")
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x_cl.device)
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=x_cl.device)
    launch("gdrnpp_conv3x3_wgrad_f32", dz_cl.data_ptr(), x_cl.data_ptr(), dw.data_ptr(), n, h, w, cin, cout, ws.data_ptr(), nbytes,
           timed=("conv3x3_wgrad", 2.0 * n * h * w * cout * 9 * cin, 4.0 * n * h * w * (cin + cout) + 36.0 * cin * cout))
    return dw


def conv3x3_backward(x_cl, weight, dz_cl, want=(True, True, True)):
    """Gradients of z = conv3x3(x, weight) + bias for dz = dL/dz -> (dx, dweight, dbias).  ``want``: three flags in that order — an
    entry is None where its flag is false and its launches are left out; the others keep their bits.  dx = conv3x3(dz, W') on
    ``conv3x3_f32_mfma`` with the flipped, transposed weight formed here (the weight changes every step), dweight =
    ``conv3x3_wgrad_f32``, dbias = ``colsum_f32(dz)``."""
    want = tuple(bool(f) for f in want)
    if len(want) != 3 or not any(want):
        raise RuntimeError("conv3x3_backward: want must hold three flags, at least one of them set")
    n, cout, h, w = dz_cl.shape
    dx = conv3x3_f32_mfma(dz_cl, conv3x3_weight_kn_flipped(weight)) if want[0] else None
    dw = conv3x3_wgrad_f32(dz_cl, x_cl) if want[1] else None
    db = colsum_f32(dz_cl.permute(0, 2, 3, 1).reshape(n * h * w, cout))[1] if want[2] else None
    return dx, dw, db


def deconv_weight_kn(weight):
    """nn.ConvTranspose2d weight [Cin,Cout,KS,KS] -> Wmat f32[KS KS Cout, Cin], rows (ky, kx, co): nn.Linear's [N,K] form of the
    forward product cols = x Wmat^T and the [K,N] form of the data gradient dx = dcols Wmat."""
    cin, cout, kh, kw = weight.shape
    return weight.detach().permute(2, 3, 1, 0).reshape(kh * kw * cout, cin).contiguous()


def deconv_im2col(dy_cl, h: int, w: int, ks: int, stride: int, pad: int, out_pad: int):
    """``gdrnpp_deconv_im2col_nhwc``: dcols f32[N h w, ks ks Cout] from dy [N,Cout,OH,OW] channels_last, the adjoint of the col2im gather
    of ``conv_transpose2d_f32_split`` (values copied, zero where a tap leaves dy)."""
    n, cout, oh, ow = channels_last_f32(dy_cl, "deconv_im2col")
    if (oh, ow) != ((h - 1) * stride - 2 * pad + ks + out_pad, (w - 1) * stride - 2 * pad + ks + out_pad):
        raise RuntimeError(f"deconv_im2col: dy {tuple(dy_cl.shape)} is not the output of a {h} x {w} input with k={ks} s={stride} p={pad} op={out_pad}")
    dcols = torch.empty((n * h * w, ks * ks * cout), dtype=torch.float32, device=dy_cl.device)
    launch("gdrnpp_deconv_im2col_nhwc", dy_cl.data_ptr(), dcols.data_ptr(), n, h, w, cout, ks, stride, pad, out_pad,
           timed=("hbm:deconv_im2col", 0.0, 4.0 * (dy_cl.numel() + dcols.numel())))
    return dcols


def conv_transpose2d_train(x_cl, weight, bias, ks: int, stride: int, pad: int, out_pad: int, groups: int):
    """nn.ConvTranspose2d of a channels_last tensor for training -> (z channels_last [N,Cout,OH,OW], GroupNorm(groups) partial sums
    f64[N,P,groups,2]): cols = x Wmat^T through ``_tail_product`` (six products up to a depth of 256, exact-f32 beyond), then the
    col2im gather that also leaves the statistics (``gdrnpp_deconv_col2im_gn_nhwc``)."""
    n, cin, h, w = channels_last_f32(x_cl, "conv_transpose2d_train")
    cout = weight.shape[1]
    cols = _tail_product(x_cl.permute(0, 2, 3, 1).reshape(n * h * w, cin), deconv_weight_kn(weight))
    oh, ow = (h - 1) * stride - 2 * pad + ks + out_pad, (w - 1) * stride - 2 * pad + ks + out_pad
    z = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=x_cl.device, memory_format=torch.channels_last)
    P = load().gdrnpp_groupnorm_workspace_bytes(n, oh * ow, groups) // (16 * n * groups)
    part = torch.empty((n, P, groups, 2), dtype=torch.float64, device=x_cl.device)
    launch("gdrnpp_deconv_col2im_gn_nhwc", cols.data_ptr(), opt_f32_ptr(bias, "bias"), z.data_ptr(), part.data_ptr(), n, h, w, cout, ks, stride,
           pad, out_pad, groups)
    return z, part


def conv_transpose2d_backward(x_cl, weight, dz_cl, ks: int, stride: int, pad: int, out_pad: int, want=(True, True, True)):
    """Gradients of z = conv_transpose2d(x, weight) + bias for dz = dL/dz -> (dx, dweight [Cin,Cout,ks,ks], dbias): the im2col gather,
    then dx = ``linear_f32_exact(dcols, Wmat)`` and dweight = ``gemm_tn_f32(x, dcols)``; dbias = ``colsum_f32(dz)``.  ``want``: three
    flags in that order — an entry is None where its flag is false and its launches are left out.  Cin % 128 == 0 and
    ks ks Cout % 128 == 0."""
    want = tuple(bool(f) for f in want)
    if len(want) != 3 or not any(want):
        raise RuntimeError("conv_transpose2d_backward: want must hold three flags, at least one of them set")
    n, cin, h, w = channels_last_f32(x_cl, "conv_transpose2d_backward")
    cout = weight.shape[1]
    if tuple(weight.shape) != (cin, cout, ks, ks) or cin % 128 or (ks * ks * cout) % 128:
        raise RuntimeError(f"conv_transpose2d_backward: weight {tuple(weight.shape)} for Cin={cin}, ks={ks}: Cin and ks ks Cout must be multiples of 128")
    dx = dw = db = None
    if want[0] or want[1]:
        dcols = deconv_im2col(dz_cl, h, w, ks, stride, pad, out_pad)
        if want[0]:
            dx2d = linear_f32_exact(dcols, deconv_weight_kn(weight), weight_kn=True)
            dx = dx2d.view(n, h, w, cin).permute(0, 3, 1, 2)
        if want[1]:
            g = gemm_tn_f32(x_cl.permute(0, 2, 3, 1).reshape(n * h * w, cin), dcols)
            dw = g.view(cin, ks, ks, cout).permute(0, 3, 1, 2).contiguous()
    if want[2]:
        oh, ow = dz_cl.shape[2:]
        db = colsum_f32(dz_cl.permute(0, 2, 3, 1).reshape(n * oh * ow, cout))[1]
    return dx, dw, db


def groupnorm_apply(z_cl, part, gamma, beta, groups: int, eps: float = 1e-5, gelu: bool = False):
    """y = GroupNorm(groups)(z) [-> GELU] from the partial sums f64[N,P,groups,2] a GEMM's epilogue or gather left (``gdrnpp_groupnorm_apply_nhwc``)."""
    n, c, h, w = channels_last_f32(z_cl, "groupnorm_apply")
    return _groupnorm_apply(z_cl, part, int(part.shape[1]), gamma, beta, n, h * w, c, groups, eps, gelu)


# ---- training: Patch-PnP under autograd (csrc/pnp_bwd.hip) ------------------------------------------------------------------------
# The forward convolutions run on gdrnpp_conv_bias_act_f32 (ks 3, stride 2) like the head's; the first layer reads the 96-pitch
# prepared input with Cin rounded up to 72 and zero weight rows for the channels 69..71.
_WORKSPACES = {}


def workspace(device, nbytes: int):
    """A float64 device buffer of at least ``nbytes`` bytes kept per (device, stream) and grown on demand: the slot tiles of a large
    weight-gradient product (64 MB for Patch-PnP's fc1) are taken once, not once per step.  Its contents mean nothing between calls."""
    key = (torch.device(device).index, current_stream())
    buf = _WORKSPACES.get(key)
    if buf is None or buf.numel() * 8 < nbytes:
        buf = torch.empty(((max(nbytes, 16) + 7) // 8,), dtype=torch.float64, device=device)
        _WORKSPACES[key] = buf
    return buf


def _s2_input(x_cl, cin: int, what: str):
    n, ld, h, w = channels_last_f32(x_cl, what)
    if not 0 < cin <= ld:
        raise RuntimeError(f"{what}: cin={cin} outside the {ld} channels of x")
    return n, ld, h, w


def conv3x3s2_weight_kn(weight, cin_pad: int | None = None):
    """nn.Conv2d weight [Cout,Cin,3,3] -> the forward operand of ``conv3x3s2_f32_mfma``: f32[9 cin_pad, Cout], row (ky 3 + kx) cin_pad
    + ci, zero rows for ci >= Cin (``cin_pad``: Cin rounded up to a multiple of 4 unless given)."""
    cout, cin = weight.shape[:2]
    cin_pad = (cin + 3) // 4 * 4 if cin_pad is None else cin_pad
    w = weight.detach().permute(2, 3, 1, 0)
    if cin_pad == cin:
        return w.reshape(9 * cin, cout).contiguous()
    out = torch.zeros((3, 3, cin_pad, cout), dtype=weight.dtype, device=weight.device)
    out[:, :, :cin] = w
    return out.view(9 * cin_pad, cout)


def conv3x3s2_f32_mfma(x_cl, weight_kn):
    """3x3 / stride 2 / zero pad 1 convolution of the first ``weight_kn.shape[0] / 9`` channels of a channels_last tensor [N,ld,H,W]
    with ``weight_kn`` (``conv3x3s2_weight_kn``) on ``gdrnpp_conv_bias_act_f32`` -> channels_last [N,Cout,H/2,W/2]."""
    cin = weight_kn.shape[0] // 9
    n, ld, h, w = _s2_input(x_cl, cin, "conv3x3s2_f32_mfma")
    cout = weight_kn.shape[1]
    if weight_kn.dim() != 2 or weight_kn.shape[0] != 9 * cin or cin % 4 or cout % 4 or ld % 4 or h % 2 or w % 2:
        raise RuntimeError(f"conv3x3s2_f32_mfma: weight_kn {tuple(weight_kn.shape)} for x {tuple(x_cl.shape)}: channel counts multiples of 4, H and W even")
    out = torch.empty((n, cout, h // 2, w // 2), dtype=torch.float32, device=x_cl.device, memory_format=torch.channels_last)
    launch("gdrnpp_conv_bias_act_f32", x_cl.data_ptr(), ld, 0, f32_ptr(weight_kn, "weight_kn"), cout, None, None, 0, 0, out.data_ptr(), cout, 0, 0, 0,
           n, h, w, cin, cout, 3, 2, _ACT_NONE, 0.0,
           timed=("mfma_f32:conv3x3s2", 2.0 * n * (h // 2) * (w // 2) * cout * 9 * cin, 4.0 * n * (h * w * cin + (h // 2) * (w // 2) * cout) + 36.0 * cin * cout))
    return out


def conv3x3s2_wgrad_f32(dz_cl, x_cl, cin: int):
    """dW f32[Cout,cin,3,3] of a 3x3 / stride 2 / zero pad 1 convolution for dz [N,Cout,H/2,W/2] and the first ``cin`` channels of its
    input x [N,ld,H,W], both channels_last (``gdrnpp_conv3x3s2_wgrad_f32``).  What x holds in the channels from ``cin`` on does not matter."""
    what = "conv3x3s2_wgrad_f32"
    n, ld, h, w = _s2_input(x_cl, cin, what)
    dn, cout, oh, ow = channels_last_f32(dz_cl, what)
    if (dn, 2 * oh, 2 * ow) != (n, h, w):
        raise RuntimeError(f"{what}: dz {tuple(dz_cl.shape)} does not fit x {tuple(x_cl.shape)}")
    nbytes = load().gdrnpp_conv3x3s2_wgrad_f32_workspace_bytes(n, h, w, cin, ld, cout)      # 0: the entry point refuses the shape, in its words
    ws = torch.empty((max(nbytes, 16) // 8,), dtype=torch.float64, device=x_cl.device)
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=x_cl.device)
    launch("gdrnpp_conv3x3s2_wgrad_f32", dz_cl.data_ptr(), x_cl.data_ptr(), ld, dw.data_ptr(), n, h, w, cin, cout, ws.data_ptr(), nbytes,
           timed=("mfma_f32:conv3x3s2_wgrad", 2.0 * n * oh * ow * cout * 9 * cin, 4.0 * n * (h * w * cin + oh * ow * cout) + 36.0 * cin * cout))
    return dw


def conv3x3s2_dinput_weight(weight):
    """nn.Conv2d weight [Cout,Cin,3,3] -> the operand of ``conv3x3s2_dinput_f32``: f32[9 Cout, ldw], row (ky 3 + kx) Cout + co, column
    ci, ldw = Cin rounded up to a multiple of 4 (the columns from Cin on are not read as values)."""
    cout, cin = weight.shape[:2]
    w = weight.detach().permute(2, 3, 0, 1)
    if cin % 4 == 0:
        return w.reshape(9 * cout, cin).contiguous()
    out = torch.zeros((3, 3, cout, (cin + 3) // 4 * 4), dtype=weight.dtype, device=weight.device)
    out[..., :cin] = w
    return out.view(9 * cout, -1)


def conv3x3s2_dinput_f32(dz_cl, w_op, cin: int, ld: int | None = None):
    """dx [N,ld,H,W] channels_last of a 3x3 / stride 2 / zero pad 1 convolution for dz [N,Cout,H/2,W/2] channels_last and ``w_op``
    (``conv3x3s2_dinput_weight``): channels [0, cin) the gradient, [cin, ld) zero (``gdrnpp_conv3x3s2_dinput_f32``, by parity class)."""
    what = "conv3x3s2_dinput_f32"
    n, cout, oh, ow = channels_last_f32(dz_cl, what)
    ld = cin if ld is None else ld
    if w_op.dim() != 2 or w_op.shape[0] != 9 * cout or w_op.shape[1] < cin:
        raise RuntimeError(f"{what}: w_op must be f32[{9 * cout}, >= {cin}], got {tuple(w_op.shape)}")
    dx = torch.empty((n, ld, 2 * oh, 2 * ow), dtype=torch.float32, device=dz_cl.device, memory_format=torch.channels_last)
    launch("gdrnpp_conv3x3s2_dinput_f32", dz_cl.data_ptr(), f32_ptr(w_op, "w_op"), w_op.shape[1], dx.data_ptr(), ld, n, 2 * oh, 2 * ow, cin, cout,
           timed=("mfma_f32:conv3x3s2_dinput", 2.0 * n * oh * ow * cout * 9 * cin, 4.0 * n * oh * ow * (4 * ld + 4 * cout) + 36.0 * cin * cout))
    return dx


def conv3x3s2_backward(x_cl, cin: int, weight, dz_cl, want=(True, True)):
    """Gradients of z = conv3x3 / stride 2 (x[:, :cin], weight) for dz = dL/dz -> (dx, dweight).  ``want``: two flags in that order — an
    entry is None where its flag is false and its launches are left out; the other keeps its bits.  dx has the channels and the pitch
    of x (zero from ``cin`` on); the data-gradient operand is formed here, per call (the weight changes every step)."""
    want = tuple(bool(f) for f in want)
    if len(want) != 2 or not any(want):
        raise RuntimeError("conv3x3s2_backward: want must hold two flags, at least one of them set")
    if weight.shape[1] != cin:
        raise RuntimeError(f"conv3x3s2_backward: weight {tuple(weight.shape)} for cin={cin}")
    dx = conv3x3s2_dinput_f32(dz_cl, conv3x3s2_dinput_weight(weight), cin, x_cl.shape[1]) if want[0] else None
    dw = conv3x3s2_wgrad_f32(dz_cl, x_cl, cin) if want[1] else None
    return dx, dw


def nhwc_flatten_nchw(x_cl):
    """``x.flatten(1)`` of a channels_last tensor [B,C,H,W] -> f32[B, C H W] in NCHW order (``gdrnpp_nhwc_flatten_nchw``)."""
    b, c, h, w = channels_last_f32(x_cl, "nhwc_flatten_nchw")
    out = torch.empty((b, c * h * w), dtype=torch.float32, device=x_cl.device)
    launch("gdrnpp_nhwc_flatten_nchw", x_cl.data_ptr(), out.data_ptr(), b, h * w, c, 0, timed=("hbm:flatten_nchw", 0.0, 8.0 * out.numel()))
    return out


def nhwc_unflatten_nchw(x2d, c: int, h: int, w: int):
    """The inverse of ``nhwc_flatten_nchw``: f32[B, c h w] in NCHW order -> channels_last [B,c,h,w]."""
    b = x2d.shape[0]
    if x2d.dim() != 2 or x2d.shape[1] != c * h * w:
        raise RuntimeError(f"nhwc_unflatten_nchw: x must be f32[B,{c * h * w}], got {tuple(x2d.shape)}")
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=x2d.device, memory_format=torch.channels_last)
    launch("gdrnpp_nhwc_flatten_nchw", f32_ptr(x2d, "x"), out.data_ptr(), b, h * w, c, 1, timed=("hbm:flatten_nchw", 0.0, 8.0 * out.numel()))
    return out


def pnp_fc_heads_backward(g_r, g_t, feat, w_r, w_t, want=(True,) * 5):
    """Gradients of ``pnp_fc_heads`` (``gdrnpp_pnp_fc_heads_backward``) for g_r f32[B,rot_dim] and g_t f32[B,3], either of which may be
    None (no gradient from that head) -> (dfeat, dw_r, db_r, dw_t, db_t).  ``want``: five flags in that order — an entry is None where
    its flag is false, and a launch nothing asks for is left out."""
    want = tuple(bool(f) for f in want)
    if len(want) != 5:
        raise RuntimeError("pnp_fc_heads_backward: want must hold five flags")
    b, k = feat.shape
    rd = w_r.shape[0]
    for name, g, n in (("g_r", g_r, rd), ("g_t", g_t, 3)):
        if g is not None and tuple(g.shape) != (b, n):
            raise RuntimeError(f"pnp_fc_heads_backward: {name} must be f32[{b},{n}], got {tuple(g.shape)}")
    dev = feat.device
    shapes = ((b, k), (rd, k), (rd,), (3, k), (3,))
    dfeat, dw_r, db_r, dw_t, db_t = (torch.empty(s, dtype=torch.float32, device=dev) if f else None for s, f in zip(shapes, want))
    if any(want):
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        launch("gdrnpp_pnp_fc_heads_backward", opt_f32_ptr(g_r, "g_r"), opt_f32_ptr(g_t, "g_t"), f32_ptr(feat, "feat"), f32_ptr(w_r, "w_r"),
               f32_ptr(w_t, "w_t"), ptr(dfeat), ptr(dw_r), ptr(dw_t), ptr(db_r), ptr(db_t), b, k, rd,
               timed=("pnp_heads_bwd", 2.0 * b * k * (rd + 3) * (want[0] + (want[1] or want[3])), 4.0 * (2 * b * k + 2 * (rd + 3) * k)))
    return dfeat, dw_r, db_r, dw_t, db_t
