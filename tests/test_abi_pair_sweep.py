"""CPU: the mirrors of include/cpuvox_gpu_pair_sweep.h, whose entry points form a family of their own (prefix cvxm_, beside cvxc_, cvxp_, cvxq_,
cvxv_, cvxs_ and the host library's cvxh_) and which is therefore no row of gpu.ABI_HEADERS: this file does for it what tests/test_abi_sweep.py
does for its header, with the readers of tests/abilib.py alone.  The export list gpu.PAIR_SWEEP_EXPORTS, the symbols of both libraries, the
argtypes of gpu._bind, the two structs -- one of them holds a whole cvxs_sweep_result -- against their ctypes classes, numpy dtypes and C#
structs field by field, the DllImports of host/csharp/CpuVoxGpuPairSweep.cs, and what the header says is not part of it."""
import ctypes as C
import os
import re

import abilib as A
from cpuvox_amd import gpu

HEADER, CS = "cpuvox_gpu_pair_sweep.h", "CpuVoxGpuPairSweep.cs"
SWEEP_HEADER, SWEEP_CS = "cpuvox_gpu_sweep.h", "CpuVoxGpuSweep.cs"
PREFIX = "cvxm_"
EXPERIMENT_LIBRARY = os.path.join(A.ROOT, "cpuvox_amd", "libcpuvox_gpu_exp.so")
NAMES = ["cvxm_pair_sweep", "cvxm_pair_sweep_device"]
PARAMETERS = {"cvxm_pair_sweep": 12, "cvxm_pair_sweep_device": 12}
STRUCTS = {"cvxm_pair_sweep_result": (gpu.PairSweepResult, gpu.PAIR_SWEEP_RESULT_DTYPE, "CvxmPairSweepResult", 56),
           "cvxm_pair_sweeps_summary": (gpu.PairSweepsSummary, gpu.PAIR_SWEEPS_SUMMARY_DTYPE, "CvxmPairSweepsSummary", 32)}
OTHER_FAMILIES = ("cvx_", "cvxc_", "cvxp_", "cvxq_", "cvxv_", "cvxs_", "cvxh_", "cvxd_")
OTHER_HEADERS = ("cpuvox_gpu_contacts.h", "cpuvox_gpu_pair_contacts.h", "cpuvox_gpu_model_pick.h", "cpuvox_gpu_model_draw.h", "cpuvox_gpu_sweep.h", "cpuvox_gpu_models.h",
                 "cpuvox_gpu.h", "cpuvox_host.h", "cpuvox_gpu_diag.h")


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
    another family grows -- cvxs_ stays at four, cvxp_ at four --; and no other header declares a cvxm_ name."""
    text = A.header_text(HEADER)
    for prefix in OTHER_FAMILIES:
        assert A.c_functions(HEADER, prefix=prefix) == {}, prefix
        assert not re.search(r"typedef\s+struct\s+" + prefix + r"[a-z]", text), f"a struct of the family {prefix}"
        assert not re.search(r"#\s*define\s+" + prefix.upper(), text), f"a constant of the family {prefix}"
    assert HEADER not in [row[0] for row in gpu.ABI_HEADERS]
    for _, exports, _ in gpu.ABI_HEADERS:
        assert not [n for n in exports if n.startswith(PREFIX)]
    assert len(gpu.SWEEP_EXPORTS) == 4 and len(gpu.PAIR_CONTACTS_EXPORTS) == 4 and len(gpu.CONTACTS_EXPORTS) == 3 and len(gpu.MODEL_PICK_EXPORTS) == 2
    assert len(gpu.MODEL_DRAW_EXPORTS) == 4
    others = gpu.CONTACTS_EXPORTS + gpu.PAIR_CONTACTS_EXPORTS + gpu.MODEL_PICK_EXPORTS + gpu.MODEL_DRAW_EXPORTS + gpu.SWEEP_EXPORTS + gpu.EXPORTS
    assert not [n for n in others if n.startswith(PREFIX)]
    for other in OTHER_HEADERS:
        assert A.c_functions(other, prefix=PREFIX) == {}, other


def test_the_export_list_is_what_the_header_declares():
    declared = A.c_functions(HEADER, prefix=PREFIX)
    assert sorted(declared) == sorted(gpu.PAIR_SWEEP_EXPORTS) == NAMES and len(set(gpu.PAIR_SWEEP_EXPORTS)) == len(gpu.PAIR_SWEEP_EXPORTS) == 2


def test_both_libraries_export_the_list():
    product = gpu.lib()
    assert not [n for n in gpu.PAIR_SWEEP_EXPORTS if not hasattr(product, n)], gpu.lib_path()
    experiment = C.CDLL(EXPERIMENT_LIBRARY)
    assert not [n for n in gpu.PAIR_SWEEP_EXPORTS if not hasattr(experiment, n)], EXPERIMENT_LIBRARY


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
    assert sorted(declared) == sorted(imports) and len(imports) == 2
    for name, (ret, params) in declared.items():
        cs_ret, cs_params = imports[name]
        assert len(params) == len(cs_params), f"{name}: {len(params)} C parameters, {len(cs_params)} in the DllImport"
        for i, (a, b) in enumerate(zip(params, cs_params)):
            assert A.c_kind(a) == A.cs_kind(b), f"{name} parameter {i}: C `{a}` vs C# `{b}`"
        assert A.c_kind(ret) == A.cs_kind(cs_ret)
    assert A.cs_imports(CS) == {}, "the file imports nothing of the cvx_ lists"


def test_the_header_declares_two_structs_and_no_constant():
    constants, _, _ = A.abi()
    assert sorted(A.c_structs(HEADER, constants)) == sorted(STRUCTS)
    assert A.c_constants(HEADER, constants) == {} and A.cs_constants(CS) == {}, "the limits are CVXS_MAX_MOTION and CVXP_MAX_PAIRS, their headers'"
    assert sorted(A.cs_structs(CS)) == sorted(row[2] for row in STRUCTS.values())
    assert gpu.SWEEP_MAX_MOTION == A.c_constants(SWEEP_HEADER, constants)["CVXS_MAX_MOTION"] == 4096


def test_the_struct_mirrors():
    """The result holds a whole cvxs_sweep_result: its layout comes from that struct's own header and C# file, and is compared leaf by leaf."""
    constants, known, _ = A.abi()
    structs = dict(known, **A.c_structs(SWEEP_HEADER, constants))
    structs.update(A.c_structs(HEADER, constants))
    cs_structs = dict(A.cs_structs(SWEEP_CS), **A.cs_structs(CS))
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
    nested = gpu.PAIR_SWEEP_RESULT_DTYPE.fields["sweep"]
    assert nested[0] == gpu.SWEEP_RESULT_DTYPE and nested[1] == 0 and gpu.PairSweepResult.sweep.size == C.sizeof(gpu.SweepResult) == 48
    assert [s.name for s in A.layout(structs["cvxm_pair_sweep_result"].fields, structs, leaves=True)[0]] == ["steps", "hit", "axis", "sign", "free", "at", "pad_", "a", "b"]


def test_the_calls_take_the_models_the_sweep_and_the_pair_structs():
    """The header includes the two headers whose records it uses and declares no model, contact or sweep struct of its own; the C# file uses
    CpuVoxGpuModels.cs's, CpuVoxGpuSweep.cs's and CpuVoxGpuPairContacts.cs's."""
    text = A.header_text(HEADER)
    assert '#include "cpuvox_gpu_sweep.h"' in text and '#include "cpuvox_gpu_pair_contacts.h"' in text
    assert len(re.findall(r"typedef\s+struct", text)) == 2
    assert "cvxs_sweep_result sweep;" in text and "cvxp_pair_result *contacts" in text and "cvxp_pair_result *contactsDevice" in text
    assert "const int32_t *pairs" in text and "const int32_t *motions" in text
    cs = A.csharp_text(CS)
    assert "CvxModel* models" in cs and "CvxModelInstance* instances" in cs and "CvxpPairResult* contacts" in cs and "public CvxsSweepResult sweep;" in cs
    assert "struct CvxsSweepResult" not in cs and "struct CvxpPairResult" not in cs
    assert "CvxsSweepResult" in A.cs_structs(SWEEP_CS) and "CvxpPairResult" in A.cs_structs("CpuVoxGpuPairContacts.cs")
    with open(os.path.join(A.ROOT, "include", HEADER)) as f:
        comments = " ".join(re.sub(r"\s*\n\s*\*\s*", " ", f.read()).split())  # (header_text leaves the comments out)
    for line in ("rotation during the motion", "sub-voxel motion", "a point list", "a swept broad phase", "a device-resident instance list"):
        assert line in comments.split("Not part of this:")[1], f"the header says what is not part of this: {line}"
    assert "No point list is part of this call" in comments and "b is the frame" in comments
    with open(os.path.join(A.ROOT, "include", SWEEP_HEADER)) as f:
        assert "sweeps of one body against another" in f.read(), "that header is as it was"
