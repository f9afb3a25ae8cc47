"""``gdrn_modeling/hip_layers.py`` is the namespace of four modules with a strict import order; the three-product policy has
one owner (``x3_policy``).  CPU only: no device, no library call."""
import ast
import importlib
import os
import threading
from unittest import mock

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "gdrnpp_bop2022_amd.gdrn_modeling"

# table order = dependency order: a module imports only from those in front of it
MODULES = ("weight_cache", "x3_policy", "hip_layers", "slice_layers")

# every name somebody read as ``hip_layers.<name>`` before the split (package, bench.py, tests, tools, oracle), without the
# deleted aliases (_packed, reset_x3_calibration), the names that became public elsewhere (_packed_weight, _use_x3) and the
# slice layers (slice_layers): name -> (owner, the owner's name for it)
NAMESPACE = {
    "weight_cache": {"weight_tag": "weight_tag", "cached": "cached", "cache_fills": "cache_fills"},
    "x3_policy": {"set_gemm_products": "set_gemm_products", "gemm_products": "gemm_products", "forced_gemm_products": "forced_gemm_products",
                  "x3_demoted": "demoted", "demote_x3": "demote", "x3_launch_order": "launch_order", "x3_slot": "slot", "x3_for": "weight_for",
                  "reset_x3_demotions": "reset"},
    "hip_layers": {n: n for n in (
        "set_enabled", "is_enabled", "enabled_for", "note_foreign_launch", "fallback_launches", "last_fallback", "foreign", "upsample2x",
        "groupnorm_act", "layernorm2d", "stem", "dwconv_ln", "mlp_gemm", "set_mlp_gemm", "set_library_below_tiles", "set_fused_mlp_x3",
        "set_f16x2_rows", "mlp_takes_rows", "convnext_mlp", "set_conv_split", "conv2d", "folded_conv_bn", "folded_conv", "conv_bn_act",
        "conv_transpose2d", "conv_transpose2d_groupnorm_act", "set_conv_gn_fused", "conv3x3_groupnorm_act", "linear", "pnp_fc_heads",
        "point_pnp")},
}


def _mod(name):
    return importlib.import_module(f"{PKG}.{name}")


def _tree(name):
    return ast.parse(open(os.path.join(ROOT, "gdrnpp_bop2022_amd", "gdrn_modeling", name + ".py")).read())


def test_hip_layers_resolves_every_name_as_the_owners_object():
    hip_layers = _mod("hip_layers")
    for owner, names in NAMESPACE.items():
        for name, owners_name in names.items():
            obj = getattr(hip_layers, name)
            assert obj is getattr(_mod(owner), owners_name), name
            assert obj.__module__ == f"{PKG}.{owner}", name
    assert sum(len(v) for v in NAMESPACE.values()) == 43
    # state somebody might assign stays with its owner: a re-exported int or dict would be a stale copy
    for private in ("_GEMM_PRODUCTS", "_TLS", "_X3_NEXT_SLOT", "_X3_EPOCH", "_X3_DEMOTED", "_X3_LAUNCH_SEQ", "_X3_LAUNCH_COUNTER", "_CACHE_FILLS"):
        assert not hasattr(hip_layers, private), private
    for gone in ("_packed", "_packed_weight", "_use_x3", "reset_x3_calibration", "set_fused_mlp", "NhwcSlice", "conv_bn_act_slice"):
        assert not hasattr(hip_layers, gone), gone


@pytest.mark.parametrize("index", range(len(MODULES)), ids=MODULES)
def test_modules_import_in_table_order(index):
    """Besides hip_lib, torch and the standard library a module imports only modules in front of it in the table."""
    allowed = set(MODULES[:index])
    for node in ast.walk(_tree(MODULES[index])):
        if isinstance(node, ast.ImportFrom) and node.level == 1:
            names = {node.module.split(".")[0]} if node.module else {a.name for a in node.names}
            assert names <= allowed, ast.dump(node)
        elif isinstance(node, ast.ImportFrom):
            assert node.level == 0 or (node.level == 2 and node.module is None and [a.name for a in node.names] == ["hip_lib"]), ast.dump(node)
        elif isinstance(node, ast.Import):
            assert all("gdrn_modeling" not in a.name for a in node.names), ast.dump(node)


@pytest.mark.parametrize("name", MODULES)
def test_no_top_level_function_is_defined_twice(name):
    defs = [n.name for n in _tree(name).body if isinstance(n, (ast.FunctionDef, ast.ClassDef))]
    assert len(defs) == len(set(defs)), sorted(d for d in set(defs) if defs.count(d) > 1)
    if name == "hip_layers":
        assert defs.count("mlp_gemm") == 1


def test_products_set_through_the_namespace_are_the_owners():
    hip_layers, x3_policy = _mod("hip_layers"), _mod("x3_policy")
    before = x3_policy.gemm_products()
    try:
        hip_layers.set_gemm_products(6)
        assert x3_policy.gemm_products() == 6 and hip_layers.gemm_products() == 6
        x3_policy.set_gemm_products(3)
        assert hip_layers.gemm_products() == 3
        seen = []
        with hip_layers.forced_gemm_products(6):
            t = threading.Thread(target=lambda: seen.append(x3_policy.gemm_products()))
            t.start()
            t.join()
            assert x3_policy.gemm_products() == 6        # the calling thread
        assert seen == [3]                               # ... and no other
        assert x3_policy.gemm_products() == 3
    finally:
        x3_policy.set_gemm_products(before)


def test_demotions_and_reset_through_the_namespace_are_the_owners():
    hip_layers, x3_policy = _mod("hip_layers"), _mod("x3_policy")
    x3_policy.reset()
    try:
        hip_layers.demote_x3({3: 2})
        assert x3_policy.is_demoted(3) and not x3_policy.is_demoted(2)
        assert hip_layers.x3_demoted() == {3: 2} == x3_policy.demoted()
        cache, other = {}, {}
        assert x3_policy.slot(cache, "fc1") == 1 and hip_layers.x3_slot(other, "fc1") == 2 and x3_policy.slot(cache, "fc1") == 1
        epoch = x3_policy._X3_EPOCH
        x3_policy.reset()
        assert x3_policy._X3_EPOCH == epoch + 1 and x3_policy.demoted() == {} and not x3_policy.is_demoted(3)
        assert x3_policy.slot(other, "fc1") == 1        # numbering restarts at 1 ...
        assert x3_policy.slot(cache, "fc1") == 2        # ... and the dict that held slot 1 before the reset gets a fresh one
    finally:
        x3_policy.reset()


# (m, n, k_linear, demoted?, rows in range?, allow3) -> (packed weight, slot, pack3 ran, launch noted).  256 tiles of 256 x 128
# make a launch eligible: m = 65536 x n = 128 is, m = 65280 is one tile short, n = 192 is no multiple of the tile;
# m * k_linear * 4 must stay below 2^32.  The layer under test is the second of the model: slot 2.
P3, P6 = ("pack3", "w"), ("pack6", "w")
SPLIT_WEIGHT_CASES = [
    ((65536, 128, 0, False, True, True), (P3, 2, True, True)),
    ((65536, 128, 512, False, True, True), (P3, 2, True, True)),
    ((65536, 128, 0, False, True, False), (P6, 0, False, False)),       # allow3 off: no slot taken, nothing packed for x3
    ((65280, 128, 0, False, True, True), (P6, 0, False, False)),        # too few tiles
    ((65536, 192, 0, False, True, True), (P6, 0, False, False)),        # n % 128
    ((65536, 128, 16384, False, True, True), (P6, 0, False, False)),    # 65536 * 16384 * 4 = 2^32: beyond 32-bit lane offsets
    ((65536, 128, 0, True, True, True), (P6, 2, False, False)),         # demoted: keeps its slot, six products
    ((65536, 128, 0, False, False, True), (P6, 2, True, False)),        # weight rows below the range: packed once, never launched
]


@pytest.mark.parametrize("case,want", SPLIT_WEIGHT_CASES)
def test_split_weight_returns_what_the_inline_form_returned(case, want):
    import torch

    from gdrnpp_bop2022_amd import hip_lib

    x3_policy = _mod("x3_policy")
    m, n, k_linear, is_demoted, in_range, allow3 = case
    weight, calls = torch.zeros(2, 2), []

    def pack3(w):
        calls.append("pack3")
        return P3

    x3_policy.reset()
    try:
        with mock.patch.object(hip_lib, "packed_rows_in_range", lambda packed: in_range), mock.patch.object(hip_lib.dispatch, "SPLIT2_MIN_TILES", 256):
            cache = {}
            assert x3_policy.slot({}, "conv") == 1           # another layer launched first
            if is_demoted:
                x3_policy.demote({2: hip_lib.X3_SMALL_ROWS})
            got = x3_policy.split_weight(cache, "conv", "w_pk", weight, pack3, lambda w: P6, m, n, k_linear, allow3=allow3)
        assert got == want[:2]
        assert ("pack3" in calls) == want[2]
        assert (2 in x3_policy._X3_LAUNCH_SEQ) == want[3]
        assert ("w_pk" in cache) == (want[0] is P6) and ("conv_pk_x3" in cache) == want[2]
    finally:
        x3_policy.reset()
