"""tests/backbone_bwd_ref.py checked on the CPU: the fp64 restatements of the stem and downsample backwards agree with fp64 autograd, the
integer lattices are exact in every summation order, the slot formulas behave, and wrong restatements (ky / kx transposed, the patch
order swapped, the mean term of the LayerNorm backward dropped) are caught by the lattice, locator and autograd checks that the GPU tests
apply to the kernels."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backbone_bwd_ref as R  # noqa: E402

STEM_SMALL = tuple(c for c in R.STEM_CASES if c != (1, 4, 1024)) + ((1, 4, 1024),)


def _close(a, b, tol=1e-11):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("case", STEM_SMALL, ids=R.case_id)
def test_stem_restatement_agrees_with_fp64_autograd(case):
    t = R.stem_inputs(case)
    ref64, _ = R.stem_references(case)
    got = R.stem_restated(*t)
    for name in ("y",) + R.STEM_NAMES:
        assert _close(got[name], ref64[name]), name


@pytest.mark.parametrize("case", R.DOWN_CASES, ids=R.case_id)
def test_downsample_restatement_agrees_with_fp64_autograd(case):
    t = R.down_inputs(case)
    ref64, _ = R.down_references(case)
    got = R.down_restated(*t)
    for name in ("z",) + R.DOWN_NAMES:
        assert _close(got[name], ref64[name]), name
    n, h, w, c, _ = case
    assert torch.equal(R.unpatch2x2(R.patch2x2(R.rows_of(t[0]).reshape(n, h, w, c)), n, h, w, c).permute(0, 3, 1, 2), t[0])


@pytest.mark.parametrize("case", R.STEM_CASES + (R.STEM_DEEP,), ids=R.case_id)
def test_stem_lattice_is_exact_in_fp32_and_fp64(case):
    x, g, dw, db = R.stem_lattice(case)
    m = g.numel() // R.STEM_C
    assert R.lattice_ok(m, R.STEM_CHAIN) and float(x.abs().max()) <= R.LATTICE and float(g.abs().max()) <= R.LATTICE
    assert int(dw.abs().max()) < 2 ** 24 and int(db.abs().max()) < 2 ** 24
    assert torch.equal(dw.float().long(), dw) and torch.equal(db.float().long(), db)      # the rounded result is the result
    if m <= 4096:      # the fp32 product in whatever order the CPU takes equals the integers
        P, g2 = R.patches4x4(x), R.rows_of(g)
        assert torch.equal((g2.t() @ P).reshape(dw.shape).long(), dw)
        assert torch.equal(R.stem_restated(x, torch.zeros(128, 3, 4, 4), torch.zeros(128), None, None, g)["dW"].long(), dw)


@pytest.mark.parametrize("case", R.DOWN_CASES, ids=R.case_id)
def test_downsample_lattice_is_exact_in_fp32_and_fp64(case):
    x, weight, g, want = R.down_lattice(case)
    n, h, w, c, cout = case
    for name in ("z", "dA", "dW", "db", "dx"):
        v = want[name]
        assert float(v.abs().max()) < 2 ** 24 and torch.equal(v, v.round()), name
    dz, Wp = R.rows_of(g), weight.permute(0, 2, 3, 1).reshape(cout, 4 * c)
    assert torch.equal((dz @ Wp).double(), want["dA"]) and torch.equal((dz.t() @ want["A"].float()).double().reshape(cout, 2, 2, c).permute(0, 3, 1, 2), want["dW"])


def test_slot_formulas():
    assert R.stem_slots(4) == (1, 256) and R.stem_slots(256) == (1, 256) and R.stem_slots(260) == (2, 256)
    assert R.stem_slots(48 * 64 * 64) == (256, 768) and R.stem_slots(8 * 64 * 64) == (128, 256) and R.stem_slots(66560) == (130, 512)
    for m in (4, 124, 128, 132, 252, 256, 260, 65536, 65540, 66560, 196608, 10 ** 7):
        slots, rows = R.stem_slots(m)
        assert slots <= R.STEM_SLOT_CAP and rows % R.STEM_SLOT_ROWS == 0 and (slots - 1) * rows < m <= slots * rows
    assert R.ln_patch_slots(4, 128) == 1 and R.ln_patch_slots(33, 128) == 2 and R.ln_patch_slots(4, 1024) == 1 and R.ln_patch_slots(5, 1024) == 2
    assert R.ln_patch_slots(10 ** 6, 256) == R.LN_SLOT_CAP and R.ln_patch_slots(48 * 48, 1024) == R.LN_SLOT_CAP < 48 * 48 // 4
    n, h, w, c, _ = R.DOWN_GRID_STRIDE
    assert -(-n * h * w // ((256 // (c // 4)) * R.LN_PIX)) > 4096      # more groups than the forward kernels' workgroups
    assert R.stem_workspace_bytes(1, 4, 16) == R.STEM_PART * 8 and R.ln_patch_workspace_bytes(1, 2, 2, 128) == 2 * 128 * 8


def test_probes_cover_the_kernels_edges():
    probes = R.stem_probes((5, 32, 32))
    assert {p for p, _ in probes} >= {0, 7, 8, 31, 32, 127, 128, 255, 256, 319} and len({c for _, c in probes}) >= 6
    assert R.stem_probes((1, 4, 16)) == [(0, 0), (2, 31), (3, 32)]


# ---- wrong restatements are caught ---------------------------------------------------------------------------------------------------
def test_transposed_ky_kx_is_caught():
    case = (3, 8, 16)
    x, g, dw, _ = R.stem_lattice(case)
    zw, zb = torch.zeros(128, 3, 4, 4), torch.zeros(128)
    assert torch.equal(R.stem_restated(x, zw, zb, None, None, g)["dW"].long(), dw)
    assert not torch.equal(R.stem_restated(x, zw, zb, None, None, g, mutate="kykx")["dW"].long(), dw)
    cx = R.stem_coded_x(case)
    for probe in R.stem_probes(case):
        oh = R.stem_onehot(case, probe)
        good, bad = (R.stem_restated(cx, zw, zb, None, None, oh, mutate=m)["dW"] for m in (None, "kykx"))
        patch = R.stem_probe_patch(case, cx, probe).double()
        assert torch.equal(good[probe[1]], patch) and not torch.equal(bad[probe[1]], patch) and torch.equal(bad[probe[1]], patch.transpose(1, 2))
        assert not good[torch.arange(128) != probe[1]].any()


def test_swapped_patch_order_is_caught():
    case = (3, 2, 6, 128, 256)
    n, h, w, c, cout = case
    cx = R.down_coded_x(case)
    good, bad = (R.patch2x2(R.rows_of(cx).reshape(n, h, w, c), m) for m in (None, "order"))
    for row in range(good.shape[0]):
        b, rem = divmod(row, (h // 2) * (w // 2))
        oy, ox = divmod(rem, w // 2)
        for ky in range(2):
            for kx in range(2):
                want = cx[b, :, 2 * oy + ky, 2 * ox + kx]
                assert torch.equal(good[row, (2 * ky + kx) * c:(2 * ky + kx + 1) * c], want)
                if ky != kx:
                    assert not torch.equal(bad[row, (2 * ky + kx) * c:(2 * ky + kx + 1) * c], want)
    x, weight, g, want = R.down_lattice(case)
    assert not torch.equal(R.down_restated(x, None, None, weight, torch.zeros(cout), g, mutate="order")["dW"], want["dW"])


def test_dropped_mean_term_is_caught():
    case = (3, 8, 16)
    ref64, ref32 = R.stem_references(case)
    bad = R.stem_restated(*R.stem_inputs(case), mutate="no_mean")
    assert R.ratio_to_bar(bad["dW"], ref64["dW"], ref32["dW"]) > 100.0 and R.ratio_to_bar(bad["db"], ref64["db"], ref32["db"]) > 100.0
    assert R.ratio_to_bar(R.stem_restated(*R.stem_inputs(case))["dW"], ref64["dW"], ref32["dW"]) < 1.0
    dcase = (3, 2, 6, 128, 256)
    d64, d32 = R.down_references(dcase)
    assert R.ratio_to_bar(R.down_restated(*R.down_inputs(dcase), mutate="no_mean")["dx"], d64["dx"], d32["dx"]) > 100.0
    assert R.ratio_to_bar(R.down_restated(*R.down_inputs(dcase))["dx"], d64["dx"], d32["dx"]) < 1.0
