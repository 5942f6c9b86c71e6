"""CPU: the mirrors of include/cpuvox_gpu_model_brush.h, whose entry points form a family of their own (prefix cvxd_, beside cvxc_, cvxp_, cvxq_,
cvxv_, cvxs_, cvxm_ and the host library's cvxh_; the diagnostic cvxd_clip_census of include/cpuvox_gpu_diag.h carries the same prefix and is no
part of it) and which is therefore no row of gpu.ABI_HEADERS: this file does for it what tests/test_abi_pair_sweep.py does for its header, with
the readers of tests/abilib.py alone.  The export list gpu.MODEL_BRUSH_EXPORTS, the symbols of both libraries, the argtypes of gpu._bind, the
three structs against their ctypes classes, numpy dtypes and C# structs field by field, the DllImports of host/csharp/CpuVoxGpuModelBrush.cs,
and what the header says is not part of it."""
import ctypes as C
import os
import re

import abilib as A
from cpuvox_amd import gpu

HEADER, CS = "cpuvox_gpu_model_brush.h", "CpuVoxGpuModelBrush.cs"
PREFIX = "cvxd_"
EXPERIMENT_LIBRARY = os.path.join(A.ROOT, "cpuvox_amd", "libcpuvox_gpu_exp.so")
NAMES = ["cvxd_model_mass", "cvxd_models_brush", "cvxd_models_brush_device"]
PARAMETERS = {"cvxd_models_brush": 11, "cvxd_models_brush_device": 11, "cvxd_model_mass": 3}
STRUCTS = {"cvxd_model_result": (gpu.ModelBrushResult, gpu.MODEL_BRUSH_RESULT_DTYPE, "CvxdModelResult", 128),
           "cvxd_instance_result": (gpu.ModelBrushInstanceResult, gpu.MODEL_BRUSH_INSTANCE_RESULT_DTYPE, "CvxdInstanceResult", 16),
           "cvxd_brush_summary": (gpu.ModelBrushSummary, gpu.MODEL_BRUSH_SUMMARY_DTYPE, "CvxdBrushSummary", 32)}
OTHER_FAMILIES = ("cvx_", "cvxc_", "cvxp_", "cvxq_", "cvxv_", "cvxs_", "cvxm_", "cvxh_")
OTHER_HEADERS = ("cpuvox_gpu_contacts.h", "cpuvox_gpu_pair_contacts.h", "cpuvox_gpu_model_pick.h", "cpuvox_gpu_model_draw.h", "cpuvox_gpu_sweep.h", "cpuvox_gpu_pair_sweep.h",
                 "cpuvox_gpu_models.h", "cpuvox_gpu_lift.h", "cpuvox_gpu.h", "cpuvox_host.h")


def _cs_imports():
    """abilib.cs_imports reads cvx_ names only: the same pattern for this family."""
    out = {}
    for m in re.finditer(r"\[DllImport\(Lib\)\]\s*public static extern\s+([A-Za-z]+)\s+(" + PREFIX + r"[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", A.csharp_text(CS), flags=re.S):
        params = m.group(3).strip()
        assert m.group(2) not in out, f"{CS} imports {m.group(2)} twice"
        out[m.group(2)] = (m.group(1), [] if not params else [p.strip() for p in params.split(",")])
    return out


def _plain(name):
    return name.rstrip("_").lower()


def test_the_header_declares_nothing_with_another_prefix():
    """Why the other ABI tests still pass: with their prefixes the reader finds no entry point and no struct in this header, so no list of
    another family grows; and no other header declares a cvxd_ name but the diagnostics', which keep their one."""
    text = A.header_text(HEADER)
    for prefix in OTHER_FAMILIES:
        assert A.c_functions(HEADER, prefix=prefix) == {}, prefix
        assert not re.search(r"typedef\s+struct\s+" + prefix + r"[a-z]", text), f"a struct of the family {prefix}"
        assert not re.search(r"#\s*define\s+" + prefix.upper(), text), f"a constant of the family {prefix}"
    assert HEADER not in [row[0] for row in gpu.ABI_HEADERS]
    for _, exports, _ in gpu.ABI_HEADERS:
        assert not [n for n in exports if n.startswith(PREFIX)]
    assert len(gpu.PAIR_SWEEP_EXPORTS) == 2 and len(gpu.SWEEP_EXPORTS) == 4 and len(gpu.PAIR_CONTACTS_EXPORTS) == 4 and len(gpu.CONTACTS_EXPORTS) == 3
    assert len(gpu.MODEL_PICK_EXPORTS) == 2 and len(gpu.MODEL_DRAW_EXPORTS) == 4 and len(gpu.LIFT_EXPORTS) == 3
    others = gpu.CONTACTS_EXPORTS + gpu.PAIR_CONTACTS_EXPORTS + gpu.MODEL_PICK_EXPORTS + gpu.MODEL_DRAW_EXPORTS + gpu.SWEEP_EXPORTS + gpu.PAIR_SWEEP_EXPORTS + gpu.EXPORTS
    assert not [n for n in others if n.startswith(PREFIX)]
    for other in OTHER_HEADERS:
        assert A.c_functions(other, prefix=PREFIX) == {}, other
    assert sorted(A.c_functions("cpuvox_gpu_diag.h", prefix=PREFIX)) == ["cvxd_clip_census"]


def test_the_export_list_is_what_the_header_declares():
    declared = A.c_functions(HEADER, prefix=PREFIX)
    assert sorted(declared) == sorted(gpu.MODEL_BRUSH_EXPORTS) == NAMES and len(set(gpu.MODEL_BRUSH_EXPORTS)) == len(gpu.MODEL_BRUSH_EXPORTS) == 3


def test_both_libraries_export_the_list():
    product = gpu.lib()
    assert not [n for n in gpu.MODEL_BRUSH_EXPORTS if not hasattr(product, n)], gpu.lib_path()
    experiment = C.CDLL(EXPERIMENT_LIBRARY)
    assert not [n for n in gpu.MODEL_BRUSH_EXPORTS if not hasattr(experiment, n)], EXPERIMENT_LIBRARY


def test_argtypes_follow_the_header():
    library = gpu.lib()
    for name, (ret, params) in A.c_functions(HEADER, prefix=PREFIX).items():
        entry = getattr(library, name)
        assert A.ctypes_kind(entry.restype) == A.c_kind(ret), f"{name}: returns {ret}, restype {entry.restype}"
        assert entry.argtypes is not None and len(entry.argtypes) == len(params) == PARAMETERS[name], f"{name}: {len(params)} parameters in {HEADER}"
        for i, (a, b) in enumerate(zip(params, entry.argtypes)):
            assert A.c_kind(a) == A.ctypes_kind(b), f"{name} parameter {i}: C `{a}` vs {b.__name__}"


def test_every_entry_point_has_a_dllimport_with_matching_parameters():
    declared, imports = A.c_functions(HEADER, prefix=PREFIX), _cs_imports()
    assert sorted(declared) == sorted(imports) and len(imports) == 3
    for name, (ret, params) in declared.items():
        cs_ret, cs_params = imports[name]
        assert len(params) == len(cs_params), f"{name}: {len(params)} C parameters, {len(cs_params)} in the DllImport"
        for i, (a, b) in enumerate(zip(params, cs_params)):
            assert A.c_kind(a) == A.cs_kind(b), f"{name} parameter {i}: C `{a}` vs C# `{b}`"
        assert A.c_kind(ret) == A.cs_kind(cs_ret)
    assert A.cs_imports(CS) == {}, "the file imports nothing of the cvx_ lists"


def test_the_header_declares_three_structs_and_no_constant():
    constants, _, _ = A.abi()
    assert sorted(A.c_structs(HEADER, constants)) == sorted(STRUCTS)
    assert A.c_constants(HEADER, constants) == {} and A.cs_constants(CS) == {}, "the limits are CVX_BRUSH_MAX_STROKES and CVX_MODELS_MAX_*, their headers'"
    assert sorted(A.cs_structs(CS)) == sorted(row[2] for row in STRUCTS.values())
    assert constants["CVX_BRUSH_MAX_STROKES"] == 4096


def test_the_struct_mirrors():
    constants, known, _ = A.abi()
    structs = dict(known, **A.c_structs(HEADER, constants))
    cs_structs = A.cs_structs(CS)
    for name, (structure, dtype, cs_name, size) in STRUCTS.items():
        slots, total, _ = A.layout(structs[name].fields, structs)
        assert total == size == structs[name].stated, f"{name}: {total} bytes computed, {structs[name].stated} stated in the header"
        assert A.ctypes_layout(structure) == (slots, total), f"{name} vs {structure.__name__}"
        assert A.dtype_layout(dtype) == (slots, total), f"{name} vs its dtype"
        attrs, declared = cs_structs[cs_name]
        assert "LayoutKind.Sequential" in attrs and declared.stated == total, f"{CS}: `struct {cs_name} // {total} bytes` expected"
        theirs = ([(_plain(s.name), s.offset, s.size) for s in A.cs_layout(cs_structs, cs_name)[0]], A.cs_layout(cs_structs, cs_name)[1])
        ours = ([(_plain(s.name), s.offset, s.size) for s in A.layout(structs[name].fields, structs, leaves=True)[0]], total)
        assert theirs == ours, f"{name} vs {cs_name} in {CS}"
    assert [s.name for s in A.layout(structs["cvxd_model_result"].fields, structs)[0]] == ["voxels", "carved", "painted", "sum", "moment", "min", "max", "pad_"]
    # the nine sums sit as cvx_lifted_piece's do, one after the other: cvxd_model_mass hands them to that struct's formula
    lifted, result = gpu.LIFTED_PIECE_DTYPE, gpu.MODEL_BRUSH_RESULT_DTYPE
    assert result.fields["moment"][1] - result.fields["sum"][1] == lifted.fields["moment"][1] - lifted.fields["sum"][1] == 24


def test_the_calls_take_the_models_and_the_strokes_of_their_headers():
    """The header includes the models' header (which includes cpuvox_gpu.h, the strokes') and declares no model, instance or stroke struct of its
    own; the C# file uses CpuVoxGpuModels.cs's and CpuVoxGpu.cs's."""
    text = A.header_text(HEADER)
    assert '#include "cpuvox_gpu_models.h"' in text and len(re.findall(r"typedef\s+struct", text)) == 3
    assert "const cvx_brush_stroke *strokes" in text and "const cvx_model *models" in text and "cvxd_instance_result *instanceResults" in text
    cs = A.csharp_text(CS)
    assert "CvxModel* models" in cs and "CvxModelInstance* instances" in cs and "BrushStroke* strokes" in cs
    assert "struct BrushStroke" not in cs and "struct CvxModel" not in cs
    assert "BrushStroke" in A.cs_structs("CpuVoxGpu.cs") and "CvxModel" in A.cs_structs("CpuVoxGpuModels.cs")
    with open(os.path.join(A.ROOT, "include", HEADER)) as f:
        comments = " ".join(re.sub(r"\s*\n\s*\*\s*", " ", f.read()).split())  # (header_text leaves the comments out)
    for line in ("FILL", "splitting a body that a carve has cut in two", "cvx_world_lift_pieces", "shrinking a model to its new box", "a device-resident instance list"):
        assert line in comments.split("Not part of this:")[1], f"the header says what is not part of this: {line}"
    for line in ("The two forms are EQUAL", "EVERY instance of a model contributes", "a sibling d' with the same image is carved", "WRITTEN IN PLACE",
                 "two models whose arrays overlap in memory", "never returns CVX_ERR_NOT_READY"):
        assert line in comments, line
