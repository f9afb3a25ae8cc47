"""C-ABI surface: the shared library loads and exports every symbol include/gdrnpp_hip.h declares
(no compute calls — runs without a GPU)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


HEADER = os.path.join(ROOT, "include", "gdrnpp_hip.h")


def _declared_names():
    """Every ``name(`` of the header outside its comments, in order, repeats included."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", text)
    skip = {"defined", "void"}
    return [n for n in names if n not in skip and not n.isupper()]


def _declared_symbols():
    return sorted(set(_declared_names()))


def test_header_parses_to_expected_symbols():
    syms = _declared_symbols()
    for must in ["farthest_point_sampling", "farthest_point_sampling_init_center", "uncertainty_pnp",
                 "gdrnpp_fps", "gdrnpp_nnd_forward", "gdrnpp_generate_hypothesis", "gdrnpp_voting_for_hypothesis",
                 "gdrnpp_uncertainty_pnp_batched", "gdrnpp_depth_refine", "gdrnpp_render_depth",
                 "gdrnpp_decode_correspondences", "gdrnpp_pose_from_pred_centroid_z"]:
        assert must in syms


def test_library_exports_every_declared_symbol():
    from gdrnpp_bop2022_amd import hip_lib

    assert os.path.exists(hip_lib.LIB_PATH), "build the HIP extension first (__graft_entry__.build())"
    lib = ctypes.CDLL(hip_lib.LIB_PATH)
    for name in _declared_symbols():
        assert hasattr(lib, name), f"{name} declared in include/gdrnpp_hip.h but not exported"


def test_library_exports_nothing_but_the_header():
    """csrc/exports.map: the dynamic symbol table holds exactly the prototypes of include/gdrnpp_hip.h — no mangled
    gdrnpp:: helpers, no __hip_cuid_* markers."""
    import subprocess

    from gdrnpp_bop2022_amd import hip_lib

    out = subprocess.run(["nm", "-D", "--defined-only", hip_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert exported == _declared_symbols()


def _isa_checker():
    import importlib.util

    spec = importlib.util.spec_from_file_location("check_isa_hazards", os.path.join(ROOT, "tools", "check_isa_hazards.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_shipped_device_code_holds_no_swizzled_packed_fp32():
    """MI355X returns wrong values in lanes 48..63 for v_pk_{add,mul}_f32 with op_sel:[0,1] while another wave of the SIMD issues
    double-rate f16 / bf16 MFMAs (two streams sharing the chip: profiles/r05p_pk_hazard_probe.txt, tests/test_gpu_streams2.py).  The library is built
    with -fno-slp-vectorize (the SLP vectorizer is what emits that form); this disassembles every gfx950 code object that was
    actually linked.  The link step of csrc/Makefile runs the same check."""
    from gdrnpp_bop2022_amd import hip_lib

    chk = _isa_checker()
    if chk.tool("llvm-objdump") is None:
        pytest.skip("no llvm-objdump")
    n_obj, n_pk, bad = chk.scan(hip_lib.LIB_PATH)
    assert n_obj == len([f for f in os.listdir(os.path.join(ROOT, "gdrnpp_bop2022_amd", "csrc")) if f.endswith(".hip")])
    assert n_pk > 1000, "the depthwise / GroupNorm kernels are packed-fp32 code: the scan must see it"
    assert bad == []


def test_the_isa_check_catches_the_swizzled_form(tmp_path):
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    chk = _isa_checker()
    src = tmp_path / "k.hip"
    src.write_text("""#include <hip/hip_runtime.h>
using f2 = __attribute__((ext_vector_type(2))) float;
extern "C" __global__ void k(f2* p) {
  f2 a = p[threadIdx.x], b = p[threadIdx.x + 64], r;
  asm volatile("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(b));
  p[threadIdx.x] = r;
}
""")
    lib = tmp_path / "libk.so"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-shared", "-fPIC", str(src), "-o", str(lib)], check=True, capture_output=True)
    n_obj, n_pk, bad = chk.scan(str(lib))
    assert n_obj == 1 and n_pk == 1 and len(bad) == 1 and "op_sel:[0,1]" in bad[0]
    assert chk.main(["check", str(lib)]) == 1


def test_python_binding_covers_header():
    from gdrnpp_bop2022_amd import hip_lib

    assert sorted(hip_lib.SIGNATURES) == _declared_symbols()
    lib = hip_lib.load()
    assert lib.gdrnpp_version() >= 100


def test_binding_holds_every_prototype_the_header_declares():
    """The parser reads prototypes with a regular expression: one it failed to match must not drop out silently.  The count is taken
    against this file's own, independent search for ``name(``."""
    from gdrnpp_bop2022_amd.hip_lib import abi

    signatures, structs, defines = abi.parse_header(HEADER)
    assert len(signatures) == len(_declared_names()) == len(_declared_symbols()) > 100
    assert list(signatures) == _declared_names()                                   # in the header's order
    assert signatures == abi.SIGNATURES and defines == abi.DEFINES and list(structs) == list(abi.STRUCTS)
    assert abi.parse_header(open(HEADER).read())[0] == signatures                  # text or path
    assert signatures["gdrnpp_last_error"] == (abi.c_char_p, []) and signatures["gdrnpp_version"] == (abi.c_int, [])
    assert signatures["gdrnpp_set_option"] == (abi.c_int, [abi.c_char_p, abi.c_int])
    assert signatures["gdrnpp_get_option"] == (abi.c_int, [abi.c_char_p, abi.c_void_p])
    assert signatures["farthest_point_sampling"] == (None, [abi.c_void_p, abi.c_void_p, abi.c_int, abi.c_int])
    assert signatures["gdrnpp_layernorm_nhwc"][1][4:7] == [abi.c_long, abi.c_int, abi.c_float]
    assert signatures["gdrnpp_gt_xyz_crop"][1][7:11] == [abi.c_double, abi.c_double, abi.c_void_p, abi.c_longlong]


def _host_cc():
    import shutil

    found = [p for p in (shutil.which("clang"), "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang", shutil.which("cc"), shutil.which("gcc"))
             if p and os.path.exists(p)]
    return found[0] if found else None


def test_derived_structs_have_the_compilers_layout(tmp_path):
    """sizeof and every offsetof of the ctypes structs, asserted by the host C compiler against the header itself."""
    import subprocess

    from gdrnpp_bop2022_amd.hip_lib import abi

    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler")
    assert list(abi.STRUCTS) == ["gdrnpp_meshes", "gdrnpp_roi_table", "gdrnpp_ranger_tensor", "gdrnpp_ranger_work", "gdrnpp_ranger_long_row"]
    assert [ctypes.sizeof(s) for s in abi.STRUCTS.values()] == [48, 96, 96, 24, 16]
    lines = ["#include <stddef.h>", '#include "gdrnpp_hip.h"']
    for name, struct in abi.STRUCTS.items():
        assert issubclass(struct, ctypes.Structure) and struct.__name__ == name
        lines.append(f'_Static_assert(sizeof({name}) == {ctypes.sizeof(struct)}, "sizeof {name}");')
        for field, ctype in struct._fields_:
            at = getattr(struct, field)
            lines.append(f'_Static_assert(offsetof({name}, {field}) == {at.offset} && sizeof((({name}*)0)->{field}) == {ctypes.sizeof(ctype)}, '
                         f'"{name}.{field}");')
    assert len(lines) == 2 + 5 + 7 + 12 + 17 + 5 + 3

    def compiles(text, tag):
        src = tmp_path / f"{tag}.c"
        src.write_text(text)
        return subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)], capture_output=True, text=True)

    ok = compiles("\n".join(lines) + "\n", "layout")
    assert ok.returncode == 0, ok.stderr
    shifted = compiles("\n".join(lines).replace("offsetof(gdrnpp_ranger_work, count) == 12", "offsetof(gdrnpp_ranger_work, count) == 16") + "\n", "shifted")
    assert shifted.returncode != 0 and "gdrnpp_ranger_work.count" in shifted.stderr          # the check bites
    # what the wrappers rely on: members by position and by keyword, pointer members take None and integers, reserved[2] is an array
    m = abi.gdrnpp_meshes(None, None, None, None, 2, 5, 8)
    assert (m.verts, m.n_obj, m.max_verts, m.max_faces) == (None, 2, 5, 8)
    assert abi.gdrnpp_roi_table(roi_id=64).roi_id == 64 and len(abi.STRUCTS["gdrnpp_ranger_tensor"]().reserved) == 2
    assert all(t is abi.c_void_p for _, t in abi.gdrnpp_roi_table._fields_)


def test_python_constants_are_the_headers_defines():
    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.hip_lib import abi

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = {name: int(value.strip("()")) for name, value in re.findall(r"#define\s+(GDRNPP_\w+)[ \t]+(\(?-?\d+\)?)", text)}
    assert len(declared) == 14 and abi.DEFINES == declared
    D = abi.DEFINES
    assert (D["GDRNPP_EINVAL"], D["GDRNPP_ELIMIT"]) == (-1, -2)
    assert hip_lib.RANGER_TILE == D["GDRNPP_RANGER_TILE"] == 12288
    assert (hip_lib.RANGER_RECTIFIED, hip_lib.RANGER_LOOKAHEAD, hip_lib.RANGER_NAN_TO_NUM) == (1, 2, 4) \
        == (D["GDRNPP_RANGER_RECTIFIED"], D["GDRNPP_RANGER_LOOKAHEAD"], D["GDRNPP_RANGER_NAN_TO_NUM"])
    assert (hip_lib.A_F16X2_ROWS, hip_lib.C_F16X2_ROWS) == (1, 2) == (D["GDRNPP_A_F16X2_ROWS"], D["GDRNPP_C_F16X2_ROWS"])
    assert (hip_lib.X3_NONFINITE, hip_lib.X3_SMALL_ROWS) == (1, 2) == (D["GDRNPP_SPLIT2_NONFINITE"], D["GDRNPP_SPLIT2_SMALL_ROWS"])
    assert hip_lib.CONV_ACTS == {"none": 0, "silu": 1, "sigmoid": 2, "yolox_box": 3} \
        == {k: D["GDRNPP_ACT_" + k.upper()] for k in ("none", "silu", "sigmoid", "yolox_box")}
    assert hip_lib.RANGER_COEFS == ("beta1", "beta2", "one_minus_beta1", "one_minus_beta2", "eps", "alpha", "wd_lr", "step_lr")
    assert all(type(v) is int for v in (hip_lib.RANGER_TILE, hip_lib.RANGER_NAN_TO_NUM, hip_lib.C_F16X2_ROWS, hip_lib.X3_SMALL_ROWS))


def test_header_parser_reads_a_small_header_and_refuses_what_it_cannot_place():
    from gdrnpp_bop2022_amd.hip_lib import abi

    signatures, structs, defines = abi.parse_header("""
#ifndef SMALL_H_
#define SMALL_H_
#define GDRNPP_A 7 /* seven */
#define GDRNPP_B (-3)
/* an earlier form, kept for the record:
 *   int foo(int x);
 */
// and int baz(int x); in a line comment
typedef struct pair {
  const float* p;     /* [n] */
  float a, b;
  long long n;
  int reserved[2];
  const char* tag;
} pair;
const char* name(void);
size_t count(const pair* pairs, long long n,
             double scale, void* stream);
void  plain ( float* x , int n ) ;
#endif
""")
    assert defines == {"GDRNPP_A": 7, "GDRNPP_B": -3}
    assert signatures == {"name": (abi.c_char_p, []), "count": (abi.c_size_t, [abi.c_void_p, abi.c_longlong, abi.c_double, abi.c_void_p]),
                          "plain": (None, [abi.c_void_p, abi.c_int])}
    assert list(structs) == ["pair"] and [f[0] for f in structs["pair"]._fields_] == ["p", "a", "b", "n", "reserved", "tag"]
    assert [f[1] for f in structs["pair"]._fields_][:4] == [abi.c_void_p, abi.c_float, abi.c_float, abi.c_longlong]
    assert structs["pair"]._fields_[5][1] is abi.c_void_p and ctypes.sizeof(structs["pair"]) == 40

    def refused(text, quoting):
        with pytest.raises(ValueError, match=quoting):
            abi.parse_header(text)

    refused("int ok(int n);\nint grow(float* x, unsigned long n, void* stream);\n", r"unsigned long.*int grow\(float\* x, unsigned long n, void\* stream\)")
    refused("int f(int n);\nuint8_t g(void);\n", "uint8_t")
    refused("int f(int n, void);\n", "int f")
    refused("int f(int, float* x);\n", "int f")                                # a parameter without a name
    refused("int f(int n)\nint g(int n);\n", "int f")                          # a lost semicolon
    refused("typedef struct s {\n  int a : 3;\n  int b;\n} s;\n", "a : 3")
    refused("typedef struct s {\n  struct { int a; } in;\n  int b;\n} s;\n", "struct s")
    refused("typedef struct s {\n  unsigned flags;\n} s;\n", "unsigned flags")
    refused("typedef struct s {\n  void v;\n} s;\n", "void v")
    refused("#define GDRNPP_MASK 0x10\nint f(int n);\n", "GDRNPP_MASK 0x10")
    with pytest.raises(RuntimeError, match="/nowhere/gdrnpp_hip.h is missing"):
        abi.parse_header("/nowhere/gdrnpp_hip.h")


def test_header_path_and_its_override():
    """The header is found from the package directory, GDRNPP_HIP_HEADER names another, and a missing one stops the import by name."""
    import subprocess
    import sys

    from gdrnpp_bop2022_amd.hip_lib import abi

    if "GDRNPP_HIP_HEADER" not in os.environ:
        assert abi.HEADER_PATH == HEADER
    env = dict(os.environ, GDRNPP_HIP_HEADER="/somewhere/else/gdrnpp_hip.h")
    out = subprocess.run([sys.executable, "-c", "from gdrnpp_bop2022_amd import hip_lib"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode != 0 and "RuntimeError: gdrnpp_bop2022_amd: C header /somewhere/else/gdrnpp_hip.h is missing" in out.stderr


def test_retired_options_are_unknown():
    """The 256x256 three-product tiles and the 3x3 convolution on the pipelined six-product kernel are gone with their switches: a
    stale A/B script fails instead of measuring the default twice."""
    from gdrnpp_bop2022_amd import hip_lib

    for name in ("split2_wide", "split_gemm_pipe_conv"):
        with pytest.raises(RuntimeError, match=f"unknown option '{name}'"):
            hip_lib.set_option(name, 1)
    hip_lib.set_option("split_gemm_panel", 4)   # (its default)


def test_missing_library_fails_loudly(tmp_path):
    from gdrnpp_bop2022_amd import hip_lib

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_lib.load(str(tmp_path / "libgdrnpp_hip.so"))


def test_wrappers_reject_cpu_tensors():
    import torch

    from gdrnpp_bop2022_amd import hip_lib

    with pytest.raises(RuntimeError, match="CUDA"):
        hip_lib.dev_ptr(torch.zeros(3), torch.float32, "x")
