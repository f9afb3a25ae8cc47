"""``gdrn_modeling/engine.py`` is the public namespace of five modules and nothing else.  CPU only: no device, no library call."""
import ast
import importlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "gdrnpp_bop2022_amd.gdrn_modeling"

# table order = dependency order: a module imports only from those in front of it
MODULES = ("records", "post", "range_check", "streams", "roi_stream")

# every public name engine.py defined while it still held the code, and the module that owns it now
PUBLIC = {
    "records": ("shard_range", "class_sorted_order", "PER_ROI_DETECTION_KEYS", "GLOBAL_DETECTION_KEYS", "sort_detections_by_class",
                "records_in_roi_order", "PAD_ROI_ID", "gather_records", "records_to_bop", "BOP_CSV_HEADER", "save_bop_csv"),
    "post": ("coor_planes", "GdrnHipPost", "xyz_back_projection", "render_roi_xyz_batch", "upnp_weights_from_cov", "pose_from_upnp",
             "mask_rles"),
    "range_check": ("X3_OVERFLOW_STEPS_TO_GIVE_UP", "range_reruns", "StepHandle", "launch_with_range_check", "run_with_range_check"),
    "streams": ("inference_step_async", "inference_step", "default_compute_streams", "default_graph_streams",
                "streams_overlap_ratio", "StepStreams", "GraphHandle", "GraphedInference", "GraphedStepStreams"),
    "roi_stream": ("rois_from_detections", "detections_from_yolox", "detections_from_bop_json", "packed_layout", "fill_packed",
                   "packed_views", "upload_packed", "roi_host_arrays", "batch_from_uploaded", "batch_data_test_gpu", "RoiPacker",
                   "h2d_overlap", "RoiStreamScheduler"),
}


def test_engine_exports_every_public_name_as_the_owners_object():
    engine = importlib.import_module(PKG + ".engine")
    names = [n for owner in MODULES for n in PUBLIC[owner]]
    assert len(names) == len(set(names)) == 45
    for owner in MODULES:
        mod = importlib.import_module(f"{PKG}.{owner}")
        for n in PUBLIC[owner]:
            assert getattr(engine, n) is getattr(mod, n), n
    assert sorted(engine.__all__) == sorted(names)
    # the mutable counters stay with their owner: a re-exported int would be a stale copy
    assert not hasattr(engine, "_X3_OVERFLOW_STEPS") and not hasattr(engine, "_RANGE_RERUNS")


def test_engine_module_holds_only_docstring_imports_and_all():
    path = os.path.join(ROOT, "gdrnpp_bop2022_amd", "gdrn_modeling", "engine.py")
    body = ast.parse(open(path).read()).body
    assert isinstance(body[0], ast.Expr) and isinstance(body[0].value, ast.Constant) and isinstance(body[0].value.value, str)
    for node in body[1:]:
        if isinstance(node, ast.ImportFrom):
            assert node.level == 1 and node.module in MODULES, ast.dump(node)
        else:
            assert isinstance(node, ast.Assign) and [t.id for t in node.targets] == ["__all__"], ast.dump(node)


@pytest.mark.parametrize("index", range(len(MODULES)), ids=MODULES)
def test_modules_import_in_table_order_without_cycles(index):
    """A fresh interpreter imports ONE module; of the six files only those in front of it in the table may have been loaded."""
    name = MODULES[index]
    code = (f"import importlib, sys; importlib.import_module({PKG + '.' + name!r}); "
            f"print(' '.join(m for m in {MODULES + ('engine',)!r} if {PKG + '.'!r} + m in sys.modules))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout.split()
    assert name in out and set(out) <= set(MODULES[:index + 1]), out
