"""``gdrnpp_bop2022_amd/hip_lib`` is the namespace of nine modules with a strict import order, one launch path (``abi.launch``) and
state that lives with its owner.  CPU only: the package is imported, the shared library is never loaded."""
import ast
import importlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "gdrnpp_bop2022_amd.hip_lib"
PKG_DIR = os.path.join(ROOT, "gdrnpp_bop2022_amd", "hip_lib")

# table order = dependency order: a module imports only from those in front of it.  The names are every one that the package,
# bench.py, __graft_entry__.py, tests/, tools/ or oracle/ read as ``hip_lib.<name>`` while hip_lib was one file (an ast search of
# that tree), with the four helpers other modules used under underscore names listed under their public ones.
NAMESPACE = {
    "abi": ["LIB_PATH", "LaunchTimer", "SIGNATURES", "copy_d2d", "load", "set_launch_timer", "set_option", "spin",
            "check", "current_stream", "dev_ptr"],
    "dispatch": ["SPLIT2_MIN_TILES", "SPLIT2_SHARED_MIN_ROWS", "SPLIT2_SHARED_MIN_TILES", "set_conv_splitk", "shared_min_tiles",
                 "shared_min_tiles_scope", "split2_tiles_ok", "split_gemm_tiles"],
    "range_words": ["X3_NONFINITE", "X3_SLOTS", "X3_SMALL_ROWS", "range_words_of", "split2_nonfinite", "split2_range_words", "x3_flag_scope",
                    "x3_flags", "x3_launch_count", "x3_flag_ptr"],
    "cv_resize": ["RESIZE_MODES", "cv_round", "resize_request"],      # the request of cv2.resize: one owner for roi's and yolox's tables
    "gemm": ["X3", "conv2d_f32_split", "conv3x3_f32_split", "conv3x3_groupnorm_act", "conv_transpose2d_f32_split",
             "conv_transpose2d_groupnorm_act", "convnext_mlp_f32_fused", "f16x2_rows_decode", "linear_f32_split", "linear_f32_split_grouped",
             "linear_f32_splitk", "mlp_fused_rows_in_range", "mlp_fused_supported", "pack_conv3x3_weight_bf16x3", "pack_conv_weight_bf16x3",
             "pack_conv_weight_f16x2", "pack_deconv_weight_bf16x3", "pack_deconv_weight_f16x2", "pack_mlp_fused_f16x2", "pack_weight_bf16x3",
             "pack_weight_f16x2", "packed_rows_in_range", "unpack_weight_bf16x3", "unpack_weight_f16x2"],
    "net": ["POINT_PNP_TILE", "ROT_DIMS", "bias_act_nhwc_", "dwconv7x7_ln", "groupnorm_act", "head_tail_nhwc", "layernorm_nhwc", "pnp_fc_heads",
            "pnp_fc_heads_pose", "point_pnp_fc", "point_pnp_pool", "stem_conv4x4_ln", "upsample_bilinear2x"],
    "pose": ["MeshSet", "decode_correspondences", "depth_refine", "epnp_batched", "epnp_ransac", "flow_forward", "fps", "nnd_backward",
             "nnd_forward", "pack_pose_records", "paste_masks_rle", "pnp_iter_from_correspondences", "pose_from_pred",
             "pose_from_pred_centroid_z", "refine_kernel_name", "refine_to_records", "render_depth", "set_refine_event_sink",
             "uncertainty_pnp_batched", "zoom_K"],
    "roi": ["ROI_TABLE_COLUMNS", "crop_resize_roi", "roi_align", "roi_pool", "roi_table", "rois_from_dets"],
    "yolox": ["conv_bias_act_f32", "letterbox_sizes", "pack_conv_weight_kmajor", "spp_maxpool_5_9_13", "upsample_nearest2x_slice", "yolox_focus",
              "yolox_letterbox", "yolox_postprocess"],
}
MODULES = tuple(NAMESPACE)
THRESHOLDS = ("SPLIT2_MIN_TILES", "SPLIT2_SHARED_MIN_TILES", "SPLIT2_SHARED_MIN_ROWS")


def _mod(name=None):
    return importlib.import_module(f"{PKG}.{name}" if name else PKG)


def _tree(path):
    return ast.parse(open(path).read(), path)


def _module_tree(name):
    return _tree(os.path.join(PKG_DIR, name + ".py"))


def test_hip_lib_resolves_every_name_as_the_owners_object():
    hip_lib = _mod()
    for owner, names in NAMESPACE.items():
        for name in names:
            obj = getattr(hip_lib, name)
            assert obj is getattr(_mod(owner), name), name
            if callable(obj):
                assert obj.__module__ == f"{PKG}.{owner}", name
    assert sum(len(v) for v in NAMESPACE.values()) == 103
    assert sorted(os.listdir(PKG_DIR)) == sorted(["__init__.py"] + [m + ".py" for m in MODULES] + (["__pycache__"] if os.path.isdir(os.path.join(PKG_DIR, "__pycache__")) else []))


def test_state_stays_with_its_owner_and_removed_names_are_gone():
    hip_lib = _mod()
    for m in MODULES:
        _mod(m)
    # a re-exported int, dict or None would be a stale copy of what the owner's setters rebind
    for private in ("_lib", "_LAUNCH_TIMER", "_REFINE_EVENT_SINK", "_X3_FLAG_OVERRIDE", "_X3_FLAGS", "_X3_LAUNCHES", "_CONV_SPLITK", "_SHARED_TLS"):
        assert not hasattr(hip_lib, private), private
    for gone in ("_nhwc_buf", "_dev", "_check", "_stream", "_x3_flag_ptr", "_f32", "_opt_f32", "_nhwc", "_channels_last_f32", "_timed", "_count_x3"):
        assert not hasattr(hip_lib, gone), gone
    for name in THRESHOLDS:
        assert name not in vars(hip_lib), name
    with pytest.raises(AttributeError, match="no attribute 'SPLIT2_NOTHING'"):
        hip_lib.SPLIT2_NOTHING


def test_thresholds_read_on_the_namespace_are_the_owners_current_values():
    hip_lib, dispatch = _mod(), _mod("dispatch")
    old = dispatch.SPLIT2_MIN_TILES, dispatch.SPLIT2_SHARED_MIN_TILES, dispatch.SPLIT2_SHARED_MIN_ROWS
    try:
        dispatch.SPLIT2_MIN_TILES, dispatch.SPLIT2_SHARED_MIN_TILES, dispatch.SPLIT2_SHARED_MIN_ROWS = 7, 0, 4096
        assert hip_lib.SPLIT2_MIN_TILES == 7
        assert hip_lib.split2_tiles_ok(256, 128 * 7) and not hip_lib.split2_tiles_ok(256, 128 * 6)
        dispatch.SPLIT2_SHARED_MIN_TILES, dispatch.SPLIT2_SHARED_MIN_ROWS = 3, 512
        assert (hip_lib.SPLIT2_SHARED_MIN_TILES, hip_lib.SPLIT2_SHARED_MIN_ROWS) == (3, 512) == (hip_lib.shared_min_tiles(), hip_lib.shared_min_rows())
        assert hip_lib.split2_tiles_ok(512, 128 * 2) and not hip_lib.split2_tiles_ok(256, 128 * 6)      # 4 tiles of 512 rows; 256 rows are too few
    finally:
        dispatch.SPLIT2_MIN_TILES, dispatch.SPLIT2_SHARED_MIN_TILES, dispatch.SPLIT2_SHARED_MIN_ROWS = old
    assert all(name not in vars(hip_lib) for name in THRESHOLDS)


@pytest.mark.parametrize("index", range(len(MODULES)), ids=MODULES)
def test_modules_import_in_table_order(index):
    """Besides torch, numpy and the standard library a module imports only package modules in front of it in the table; ctypes is
    abi's (pose and roi use it for byref and the c_double arrays), and so is re, for reading the header."""
    name, allowed = MODULES[index], set(MODULES[:index])
    outside = set()
    for node in ast.walk(_module_tree(name)):
        if isinstance(node, ast.ImportFrom) and node.level:
            assert node.level == 1, ast.dump(node)
            assert ({node.module.split(".")[0]} if node.module else {a.name for a in node.names}) <= allowed, ast.dump(node)
        elif isinstance(node, ast.ImportFrom):
            outside.add(node.module.split(".")[0])
        elif isinstance(node, ast.Import):
            outside.update(a.name.split(".")[0] for a in node.names)
    own = ({"ctypes"} if name in ("abi", "pose", "roi") else set()) | ({"re"} if name == "abi" else set())
    assert outside <= {"__future__", "torch", "numpy", "os", "threading"} | own, outside


def test_init_is_the_namespace_and_nothing_else():
    body = _module_tree("__init__").body
    assert isinstance(body[0], ast.Expr) and isinstance(body[0].value, ast.Constant)      # the docstring
    for node in body[1:]:
        if isinstance(node, ast.FunctionDef):
            assert node.name == "__getattr__"
        elif isinstance(node, (ast.Assign, ast.AnnAssign)):
            assert [t.id for t in node.targets] == ["__all__"]
        else:
            assert isinstance(node, ast.ImportFrom) and node.level == 1 and all(a.name != "*" for a in node.names), ast.dump(node)


def _is_bound_call(node):
    """``load().gdrnpp_x(...)`` / ``lib.gdrnpp_x(...)``: a call of a bound ctypes function."""
    return isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("gdrnpp_")


@pytest.mark.parametrize("name", MODULES[1:])
def test_every_status_returning_entry_point_goes_through_launch(name):
    """Outside abi only the size queries (``*_bytes``, ``*_partials``) are called on the library object."""
    calls = [n.func.attr for n in ast.walk(_module_tree(name)) if _is_bound_call(n)]
    assert all(c.endswith(("_bytes", "_partials")) for c in calls), calls
    abi = _mod("abi")
    launched = [n.args[0].value for n in ast.walk(_module_tree(name))
                if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "launch" and isinstance(n.args[0], ast.Constant)]
    for symbol in launched:     # named after the symbol that is called: a declared one that returns a status and takes a stream last
        res, args = abi.SIGNATURES[symbol]
        assert res is abi.c_int and args[-1] is abi.c_void_p, symbol


def test_abi_has_the_launch_pattern_once():
    calls = [n.func for n in ast.walk(_module_tree("abi")) if isinstance(n, ast.Call)]
    assert sum(isinstance(f, ast.Name) and f.id == "current_stream" for f in calls) == 1         # in launch, nowhere else
    assert sum(isinstance(f, ast.Attribute) and f.attr == "launch" for f in calls) == 1          # the timer's, in launch
    # SIGNATURES: one ctypes type per C type — each entry is, by identity, a value of the one map (a single dict literal), or a pointer
    abi = _mod("abi")
    maps = [n.value for n in ast.walk(_module_tree("abi")) if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "C_TYPES"]
    assert len(maps) == 1 and isinstance(maps[0], ast.Dict) and [k.value for k in maps[0].keys] == list(abi.C_TYPES)
    assert all(isinstance(v, (ast.Name, ast.Constant)) for v in maps[0].values)
    allowed = list(abi.C_TYPES.values()) + [abi.c_void_p, abi.c_char_p]
    assert len(abi.SIGNATURES) > 100
    for name, (res, args) in abi.SIGNATURES.items():
        assert all(any(t is a for a in allowed) for t in [res] + args), name
        assert all(t is not None for t in args), name


def _hip_lib_aliases(tree):
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            names.update(a.asname or a.name for a in node.names if a.name == "hip_lib")
        elif isinstance(node, ast.Import):
            names.update(a.asname for a in node.names if a.name.endswith(".hip_lib") and a.asname)
        elif isinstance(node, ast.arg) and node.arg == "hip":         # the conftest fixture
            names.add("hip")
    return names


def test_nobody_assigns_on_the_namespace():
    """``hip_lib.X = ...`` would bind a copy the owner never reads: state is assigned in its owner module."""
    found = []
    for base in ("gdrnpp_bop2022_amd", "tests", "tools", "oracle"):
        for d, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if not f.endswith(".py"):
                    continue
                try:
                    tree = _tree(os.path.join(d, f))
                except SyntaxError:
                    continue
                aliases = _hip_lib_aliases(tree)
                for node in ast.walk(tree):
                    targets = node.targets if isinstance(node, ast.Assign) else [node.target] if isinstance(node, (ast.AugAssign, ast.AnnAssign)) else []
                    for t in targets:
                        for el in (t.elts if isinstance(t, (ast.Tuple, ast.List)) else [t]):
                            if isinstance(el, ast.Attribute) and isinstance(el.value, ast.Name) and el.value.id in aliases:
                                found.append(f"{os.path.join(d, f)}:{node.lineno} {el.value.id}.{el.attr}")
    assert not found, found


def test_library_path_and_loader_message():
    hip_lib = _mod()
    if "GDRNPP_HIP_LIB" not in os.environ:
        assert hip_lib.LIB_PATH == os.path.join(ROOT, "gdrnpp_bop2022_amd", "libgdrnpp_hip.so")
    env = dict(os.environ, GDRNPP_HIP_LIB="/somewhere/else/lib.so")
    out = subprocess.run([sys.executable, "-c", "from gdrnpp_bop2022_amd import hip_lib; print(hip_lib.LIB_PATH)"], cwd=ROOT, env=env,
                         capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "/somewhere/else/lib.so"
    with pytest.raises(RuntimeError) as err:
        hip_lib.load("/nonexistent")
    assert str(err.value) == ("gdrnpp_bop2022_amd: HIP extension /nonexistent is missing — run `python -c 'import __graft_entry__ as g; "
                              "g.build()'` (or `make -C gdrnpp_bop2022_amd/csrc`).  There is no CPU fallback.")
