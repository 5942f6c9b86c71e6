"""CPU: the mirrors of include/cpuvox_gpu_sweep.h, whose entry points form a family of their own (prefix cvxs_, beside cvxc_, cvxp_, cvxq_, cvxv_
and the host library's cvxh_) and which is therefore no row of gpu.ABI_HEADERS: this file does for it what tests/test_abi_model_draw.py does for
its header, with the readers of tests/abilib.py alone.  The export list gpu.SWEEP_EXPORTS, the symbols of both libraries, the argtypes of
gpu._bind, the two structs against their ctypes classes, numpy dtypes and C# structs field by field, the motion limit against its twins, and the
DllImports of host/csharp/CpuVoxGpuSweep.cs."""
import ctypes as C
import os
import re

import abilib as A
from cpuvox_amd import gpu

HEADER, CS = "cpuvox_gpu_sweep.h", "CpuVoxGpuSweep.cs"
PREFIX = "cvxs_"
EXPERIMENT_LIBRARY = os.path.join(A.ROOT, "cpuvox_amd", "libcpuvox_gpu_exp.so")
NAMES = ["cvxs_instance_moved", "cvxs_sweep_offset", "cvxs_world_sweep", "cvxs_world_sweep_device"]
PARAMETERS = {"cvxs_world_sweep": 13, "cvxs_world_sweep_device": 13, "cvxs_sweep_offset": 4, "cvxs_instance_moved": 3}
STRUCTS = {"cvxs_sweep_result": (gpu.SweepResult, gpu.SWEEP_RESULT_DTYPE, "CvxsSweepResult", 48),
           "cvxs_sweeps_summary": (gpu.SweepsSummary, gpu.SWEEPS_SUMMARY_DTYPE, "CvxsSweepsSummary", 32)}
CONSTANTS = {"CVXS_MAX_MOTION": 4096}
OTHER_FAMILIES = ("cvx_", "cvxc_", "cvxp_", "cvxq_", "cvxv_")


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


def test_the_header_declares_nothing_the_pinned_lists_count():
    """Why the other ABI tests still pass: with their prefixes the reader finds no entry point in this header, so it needs no row in
    gpu.ABI_HEADERS and no list there or of the four other families grows; and no other family lists a cvxs_ name."""
    for prefix in OTHER_FAMILIES:
        assert A.c_functions(HEADER, prefix=prefix) == {}, prefix
    assert HEADER not in [row[0] for row in gpu.ABI_HEADERS]
    for _, exports, _ in gpu.ABI_HEADERS:
        assert not [n for n in exports if n.startswith(PREFIX)]
    assert len(gpu.CONTACTS_EXPORTS) == 3 and len(gpu.PAIR_CONTACTS_EXPORTS) == 4 and len(gpu.MODEL_PICK_EXPORTS) == 2 and len(gpu.MODEL_DRAW_EXPORTS) == 4
    assert not [n for n in gpu.CONTACTS_EXPORTS + gpu.PAIR_CONTACTS_EXPORTS + gpu.MODEL_PICK_EXPORTS + gpu.MODEL_DRAW_EXPORTS + gpu.EXPORTS if n.startswith(PREFIX)]
    for other in ("cpuvox_gpu_contacts.h", "cpuvox_gpu_pair_contacts.h", "cpuvox_gpu_model_pick.h", "cpuvox_gpu_model_draw.h", "cpuvox_gpu_models.h", "cpuvox_gpu.h"):
        assert A.c_functions(other, prefix=PREFIX) == {}, other


def test_the_export_list_is_what_the_header_declares():
    declared = A.c_functions(HEADER, prefix=PREFIX)
    assert sorted(declared) == sorted(gpu.SWEEP_EXPORTS) == NAMES and len(set(gpu.SWEEP_EXPORTS)) == len(gpu.SWEEP_EXPORTS) == 4


def test_both_libraries_export_the_list():
    product = gpu.lib()
    assert not [n for n in gpu.SWEEP_EXPORTS if not hasattr(product, n)], gpu.lib_path()
    experiment = C.CDLL(EXPERIMENT_LIBRARY)
    assert not [n for n in gpu.SWEEP_EXPORTS if not hasattr(experiment, n)], EXPERIMENT_LIBRARY


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
    assert sorted(declared) == sorted(imports) and len(imports) == 4
    for name, (ret, params) in declared.items():
        cs_ret, cs_params = imports[name]
        assert len(params) == len(cs_params), f"{name}: {len(params)} C parameters, {len(cs_params)} in the DllImport"
        for i, (a, b) in enumerate(zip(params, cs_params)):
            assert A.c_kind(a) == A.cs_kind(b), f"{name} parameter {i}: C `{a}` vs C# `{b}`"
        assert A.c_kind(ret) == A.cs_kind(cs_ret)
    assert A.cs_imports(CS) == {}, "the file imports nothing of the cvx_ lists"


def test_the_header_declares_two_structs_and_one_constant_with_their_twins():
    constants, _, _ = A.abi()
    assert sorted(A.c_structs(HEADER, constants)) == sorted(STRUCTS)
    assert A.c_constants(HEADER, constants) == CONSTANTS
    assert gpu.SWEEP_MAX_MOTION == 4096 and A.cs_constants(CS) == CONSTANTS
    assert sorted(A.cs_structs(CS)) == sorted(row[2] for row in STRUCTS.values())


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


def test_the_calls_take_the_models_and_the_contacts_structs():
    """The header includes cpuvox_gpu_contacts.h and declares neither a model struct nor a contact record of its own; the C# file uses
    CpuVoxGpuModels.cs's and CpuVoxGpuContacts.cs's."""
    text = A.header_text(HEADER)
    assert '#include "cpuvox_gpu_contacts.h"' in text and "typedef struct cvx_" not in text and "typedef struct cvxc_" not in text
    assert "cvxc_contact_result *contacts" in text and "cvxc_contact_point *points" in text and "const cvx_model_instance *in" in text
    cs = A.csharp_text(CS)
    assert "CvxModel* models" in cs and "CvxModelInstance* instances" in cs and "CvxcContactResult* contacts" in cs and "CvxcContactPoint* points" in cs
    assert {"CvxModel", "CvxModelInstance"} <= set(A.cs_structs("CpuVoxGpuModels.cs")) and {"CvxcContactResult", "CvxcContactPoint"} <= set(A.cs_structs("CpuVoxGpuContacts.cs"))
    with open(os.path.join(A.ROOT, "include", HEADER)) as f:
        comments = f.read()  # (header_text leaves the comments out)
    for line in ("sweeps of one body against another", "rotation during the motion", "sub-voxel motion", "a device-resident instance list"):
        assert line in comments, f"the header says what is not part of this: {line}"
