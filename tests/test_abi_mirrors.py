"""CPU: the one check of the C ABI's mirrors.  The headers under include/ are the ABI; everything that restates them is compared with what
tests/abilib.py reads from them: the export lists of gpu.ABI_HEADERS, the symbols of the libraries, the argtypes of gpu._bind, the ctypes
structures and numpy dtypes, the constants, the DllImports, structs and constants of host/csharp/ (which cannot be compiled here, so it is kept
honest by parsing), and the test models' own copies.  A new header adds a row to gpu.ABI_HEADERS, its structs rows to abilib.MIRRORS."""
import ctypes as C
import importlib
import itertools
import os

import numpy as np
import pytest

import abilib as A
from cpuvox_amd import gpu, host

ROOT = A.ROOT
HEADERS = [pytest.param(*row, id=row[0]) for row in gpu.ABI_HEADERS]
CS_HEADERS = [pytest.param(header, cs, id=cs) for header, _, cs in gpu.ABI_HEADERS if cs]
EXPERIMENT_LIBRARY = os.path.join(ROOT, "cpuvox_amd", "libcpuvox_gpu_exp.so")
DIAG_HEADER = "cpuvox_gpu_diag.h"

# What the headers cannot say.  The list lengths: include/cpuvox_gpu.h's stays what its hosts were built against.
EXPORT_COUNTS = {"cpuvox_gpu.h": 83, "cpuvox_gpu_heights.h": 4, "cpuvox_gpu_models.h": 5, "cpuvox_gpu_spread.h": 2, "cpuvox_gpu_surface_rects.h": 3,
                 "cpuvox_gpu_snapshot.h": 6, "cpuvox_gpu_lift.h": 3, DIAG_HEADER: 9}
# The sizes of the structs whose header states none (the reference's blittable layouts and the three the first binding test pinned).
PINNED_BYTES = {"cvx_segment_data": 36, "cvx_camera_data": 108, "cvx_counters": 88, "cvx_raybuffer_layout": 24, "cvx_row_span": 24}
# The result codes have no twin in gpu: the wrappers raise on any non-zero code, and the ..._fail_cleanly tests compare with these literals.
RESULT_CODES = {"CVX_OK": 0, "CVX_ERR_INVALID_ARGUMENT": -1, "CVX_ERR_HIP": -2, "CVX_ERR_NOT_READY": -3, "CVX_ERR_CAPACITY": -4, "CVX_ERR_TIMEOUT": -5}
SPREAD_TILE = ("CVX_SPREAD_TILE_X", "CVX_SPREAD_TILE_Y", "CVX_SPREAD_TILE_Z")  # Python keeps the three as the tuple gpu.SPREAD_TILE
# Limits a host sizes its buffers by, as literals
PINNED_CONSTANTS = {"CVX_NAV_MAX_GOALS": 4096, "CVX_LIGHT_MAX_LAMPS": 4096, "CVX_LAMP_MAX_RADIUS": 64}
# The constants a C# file must declare (any other CVX_ constant it declares must be the header's too)
CS_CONSTANTS = {
    "CpuVoxGpu.cs": ("CVX_LIGHT_MAX_LAMPS", "CVX_LAMP_MAX_RADIUS", "CVX_SURFACE_OUTSIDE_DEFAULT", "CVX_SURFACE_IGNORE_COLOUR"),
    "CpuVoxGpuHeights.cs": ("CVX_HEIGHTS_WALLED",),
    "CpuVoxGpuModels.cs": ("CVX_MODELS_MAX_MODELS", "CVX_MODELS_MAX_INSTANCES"),
    "CpuVoxGpuSpread.cs": ("CVX_SPREAD_MAX_SEEDS", "CVX_SPREAD_MAX_STEPS", "CVX_SPREAD_UNREACHED", "CVX_SPREAD_BLOCKED"),
    "CpuVoxGpuSnapshot.cs": ("CVX_SNAPSHOT_IGNORE_COLOUR",),
    "CpuVoxGpuLift.cs": ("CVX_LIFT_COPY", "CVX_LIFT_REMOVE"),
}
NO_ARGTYPES = {"cvx_version": "takes no argument"}
# (model module, its attribute, the gpu attribute it equals); a ..._NAMES tuple equals the names of the gpu dtype.  The models are written
# independently of the binding on purpose, so their literals also pin the values.
MODEL_TWINS = [
    ("piecesmodel", "PIECE_DTYPE", "PIECE_DTYPE"), ("piecesmodel", "GROUND", "ANCHOR_GROUND"), ("piecesmodel", "OUTSIDE", "ANCHOR_OUTSIDE"),
    ("piecesmodel", "LARGEST", "ANCHOR_LARGEST"),
    ("liftmodel", "LIFTED_PIECE_DTYPE", "LIFTED_PIECE_DTYPE"), ("liftmodel", "COPY", "LIFT_COPY"), ("liftmodel", "REMOVE", "LIFT_REMOVE"),
    ("snapshotmodel", "CHANGE_DTYPE", "SNAPSHOT_CHANGE_DTYPE"), ("snapshotmodel", "IGNORE_COLOUR", "SNAPSHOT_IGNORE_COLOUR"),
    ("spreadmodel", "AIR", "SPREAD_AIR"), ("spreadmodel", "SOLID", "SPREAD_SOLID"), ("spreadmodel", "UNREACHED", "SPREAD_UNREACHED"),
    ("spreadmodel", "BLOCKED", "SPREAD_BLOCKED"),
    ("surfacemodel", "QUAD_DTYPE", "SURFACE_QUAD_DTYPE"), ("surfacemodel", "SUMMARY_NAMES", "SURFACE_SUMMARY_DTYPE"),
    ("surfacemodel", "OUTSIDE_DEFAULT", "SURFACE_OUTSIDE_DEFAULT"), ("surfacemodel", "IGNORE_COLOUR", "SURFACE_IGNORE_COLOUR"),
    ("surfacerectsmodel", "RECT_DTYPE", "SURFACE_RECT_DTYPE"), ("surfacerectsmodel", "SUMMARY_NAMES", "SURFACE_RECTS_SUMMARY_DTYPE"),
    ("cavitymodel", "SUMMARY_NAMES", "CAVITIES_SUMMARY_DTYPE"), ("cavitymodel", "OPEN_DEFAULT", "CAVITY_OPEN_DEFAULT"),
    ("navmodel", "STEP_DTYPE", "NAV_STEP_DTYPE"),
    ("lightmodel", "TO_RGB", "LIGHT_TO_RGB"), ("lightmodel", "TO_ALPHA", "LIGHT_TO_ALPHA"),
    ("movemodel", "UNIT", "MOVE_UNIT"), ("movemodel", "SOLID_BELOW", "MOVE_SOLID_BELOW"), ("movemodel", "SOLID_SIDES", "MOVE_SOLID_SIDES"),
    ("movemodel", "RESTING", "MOVED_RESTING"), ("movemodel", "STARTS_SOLID", "MOVED_STARTS_SOLID"), ("movemodel", "STEPPED", "MOVED_STEPPED"),
    ("movemodel", "INVALID", "MOVED_INVALID"),
]


def _differ(mirror, header):
    """(the first field of a mirror's layout that is not the header's, the header's field there), for the message of a failure."""
    pairs = itertools.zip_longest(mirror[0], header[0])
    return next(((a, b) for a, b in pairs if a != b), ("total", mirror[1], header[1]))


def _plain(name):
    """Field names compare across the languages without case or the trailing underscore of pad_ (C# has Pad, BoxMin)."""
    return name.rstrip("_").lower()


# ---- per header: the export list, the libraries, the DllImports, the argtypes ----------------------------------------------------------------

@pytest.mark.parametrize("header,exports,cs", HEADERS)
def test_the_export_list_is_what_the_header_declares(header, exports, cs):
    declared = A.c_functions(header)
    assert len(set(exports)) == len(exports), f"{header}: its list names {sorted(n for n in set(exports) if exports.count(n) > 1)} twice"
    assert sorted(exports) == sorted(declared), f"{header}: declared but not listed {sorted(set(declared) - set(exports))}, listed but not declared " \
                                                f"{sorted(set(exports) - set(declared))}"
    assert len(exports) == EXPORT_COUNTS[header], header


def test_no_entry_point_is_declared_by_two_headers():
    assert sorted(EXPORT_COUNTS) == sorted(row[0] for row in gpu.ABI_HEADERS)
    on_disk = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if A.c_functions(f))
    assert on_disk == sorted(EXPORT_COUNTS), "every header under include/ that declares cvx_ entry points has a row in gpu.ABI_HEADERS"
    for (a, a_exports, _), (b, b_exports, _) in itertools.combinations(gpu.ABI_HEADERS, 2):
        assert not set(a_exports) & set(b_exports), f"{a} and {b} both list {sorted(set(a_exports) & set(b_exports))}"
        assert not set(A.c_functions(a)) & set(A.c_functions(b)), f"{a} and {b} both declare {sorted(set(A.c_functions(a)) & set(A.c_functions(b)))}"


@pytest.mark.parametrize("header,exports,cs", HEADERS)
def test_the_libraries_export_the_list(header, exports, cs):
    """The product library exports every product header's list and none of the diagnostics; the experiment build exports all of them."""
    product = gpu.lib()
    if header == DIAG_HEADER:
        assert not [n for n in exports if hasattr(product, n)], "the product library exports diagnostics"
    else:
        assert not [n for n in exports if not hasattr(product, n)], gpu.lib_path()
        assert b"gfx950" in product.cvx_version()
    if header in ("cpuvox_gpu.h", DIAG_HEADER) and not os.path.exists(EXPERIMENT_LIBRARY):
        return  # (these two lists were only ever looked at in an experiment build that is there; the later headers require it)
    experiment = C.CDLL(EXPERIMENT_LIBRARY)
    assert not [n for n in exports if not hasattr(experiment, n)], EXPERIMENT_LIBRARY


def test_the_host_library_exports_what_its_header_declares():
    declared = A.c_functions("cpuvox_host.h", prefix="cvxh_")
    assert declared and not [n for n in declared if not hasattr(host.lib(), n)]


@pytest.mark.parametrize("header,cs", CS_HEADERS)
def test_every_entry_point_has_a_dllimport_with_matching_parameters(header, cs):
    declared, imports = A.c_functions(header), A.cs_imports(cs)
    assert sorted(declared) == sorted(imports), f"{cs}: missing {sorted(set(declared) - set(imports))}, extra {sorted(set(imports) - set(declared))}"
    for name, (ret, params) in declared.items():
        cs_ret, cs_params = imports[name]
        assert len(params) == len(cs_params), f"{name}: {len(params)} C parameters, {len(cs_params)} in the DllImport of {cs}"
        for i, (a, b) in enumerate(zip(params, cs_params)):
            assert A.c_kind(a) == A.cs_kind(b), f"{name} parameter {i}: C `{a}` vs C# `{b}` in {cs}"
        assert A.c_kind(ret) == A.cs_kind(cs_ret), f"{name}: returns {ret} in C, {cs_ret} in {cs}"


@pytest.mark.parametrize("header,exports,cs", HEADERS)
def test_argtypes_follow_the_header(header, exports, cs):
    """What gpu._bind tells ctypes about every entry point: as many argtypes as the header has parameters, of the same kinds, and a restype of the
    return type's kind (ctypes' default is int)."""
    library = gpu._bind(EXPERIMENT_LIBRARY) if header == DIAG_HEADER else gpu.lib()
    for name, (ret, params) in A.c_functions(header).items():
        entry = getattr(library, name)
        assert A.ctypes_kind(entry.restype) == A.c_kind(ret), f"{name}: returns {ret}, restype {entry.restype}"
        if entry.argtypes is None:
            assert name in NO_ARGTYPES and not params, f"{name}: gpu._bind gives it no argtypes"
            continue
        assert len(entry.argtypes) == len(params), f"{name}: {len(params)} parameters in {header}, {len(entry.argtypes)} argtypes"
        for i, (a, b) in enumerate(zip(params, entry.argtypes)):
            assert A.c_kind(a) == A.ctypes_kind(b), f"{name} parameter {i}: C `{a}` vs {b.__name__}"


# ---- per struct ----------------------------------------------------------------------------------------------------------------------------------

def test_every_struct_of_the_headers_has_a_row():
    _, structs, _ = A.abi()
    assert sorted(structs) == sorted(A.MIRRORS), f"without a row in abilib.MIRRORS: {sorted(set(structs) - set(A.MIRRORS))}, rows without a struct: " \
                                                 f"{sorted(set(A.MIRRORS) - set(structs))}"
    assert set(PINNED_BYTES) == {n for n, s in structs.items() if s.stated is None}, "a struct whose header states no size has its size pinned here"


@pytest.mark.parametrize("name", sorted(A.MIRRORS))
def test_struct_mirrors(name):
    """The layout computed from the header's own field list (natural alignment) against the size the header states, every field of the ctypes
    class and of the dtype (name, offset, size) and every field of the C# struct (name without case, offset, size, nested structs flattened)."""
    _, structs, owner = A.abi()
    structure, dtype, cs_name = A.MIRRORS[name]
    slots, total, _ = A.layout(structs[name].fields, structs)
    assert total == (PINNED_BYTES[name] if structs[name].stated is None else structs[name].stated), f"{name}: {total} bytes computed"
    if structure is not None:
        assert A.ctypes_layout(structure) == (slots, total), f"{name} vs {structure.__name__}: {_differ(A.ctypes_layout(structure), (slots, total))}"
    if dtype is not None:
        assert A.dtype_layout(dtype) == (slots, total), f"{name} vs its dtype: {_differ(A.dtype_layout(dtype), (slots, total))}"
        if structure is not None and name != "cvx_mesh_vertex":  # (MESH_VERTEX_DTYPE is the one dtype written by hand)
            assert dtype == np.dtype(structure), name
    if cs_name is not None:
        cs = next(cs for header, _, cs in gpu.ABI_HEADERS if header == owner[name])
        cs_structs = A.cs_structs(cs)
        assert cs_name in cs_structs, f"{cs} has no struct {cs_name}"
        attrs, declared = cs_structs[cs_name]
        assert "LayoutKind.Sequential" in attrs, cs_name
        if cs != "CpuVoxGpu.cs":  # the later files state each struct's size beside its name
            assert declared.stated == total, f"{cs}: `struct {cs_name} // {total} bytes` expected"
        theirs = ([(_plain(s.name), s.offset, s.size) for s in A.cs_layout(cs_structs, cs_name)[0]], A.cs_layout(cs_structs, cs_name)[1])
        ours = ([(_plain(s.name), s.offset, s.size) for s in A.layout(structs[name].fields, structs, leaves=True)[0]], total)
        assert theirs == ours, f"{name} vs {cs_name} in {cs}: {_differ(theirs, ours)}"


# ---- constants -----------------------------------------------------------------------------------------------------------------------------------

def test_constants_equal_the_headers():
    constants, _, _ = A.abi()
    assert len(constants) >= 68
    for name, value in constants.items():
        if name in RESULT_CODES:
            assert value == RESULT_CODES[name], name
        elif name in SPREAD_TILE:
            assert value == gpu.SPREAD_TILE[SPREAD_TILE.index(name)], name
        else:
            assert hasattr(gpu, name[4:]), f"{name} has no twin gpu.{name[4:]}"
            assert A.int32(value) == A.int32(getattr(gpu, name[4:])), f"{name} = {value} in its header, gpu.{name[4:]} = {getattr(gpu, name[4:])}"
    assert not (set(RESULT_CODES) | set(SPREAD_TILE) | set(PINNED_CONSTANTS)) - set(constants)
    for name, value in PINNED_CONSTANTS.items():
        assert constants[name] == value, name
    assert gpu.LOD_LEVELS == host.LOD_LEVELS
    # the spread tile: the public header's macros are also the constants of the rules and of the kernel
    rules_h = open(os.path.join(ROOT, "cpuvox_amd", "csrc", "cvx_spread.h")).read()
    assert "kSpreadTileX = CVX_SPREAD_TILE_X, kSpreadTileY = CVX_SPREAD_TILE_Y, kSpreadTileZ = CVX_SPREAD_TILE_Z" in rules_h


@pytest.mark.parametrize("header,cs", CS_HEADERS)
def test_csharp_constants_equal_the_headers(header, cs):
    constants, _, _ = A.abi()
    declared = {name: value for name, value in A.cs_constants(cs).items() if name.startswith("CVX_")}
    assert not [n for n in CS_CONSTANTS.get(cs, ()) if n not in declared], f"{cs} must declare {CS_CONSTANTS[cs]}"
    for name, value in declared.items():
        assert name in constants, f"{cs}: {name} is in no header"
        assert A.int32(value) == A.int32(constants[name]), f"{cs}: {name} = {value}, {constants[name]} in its header"


def test_the_expression_reader_takes_the_grammar_and_nothing_else():
    assert [A.evaluate(e) for e in ("0x3B", "1 << 6", "(-2)", "-(1 << 31)", "1 | 1 << 4", "(int32_t)0x7FFFFFFF", "65534u")] == [59, 64, -2, -2**31, 17, 2**31 - 1, 65534]
    assert A.evaluate("A | 2", {"A": 4}) == 6 and A.int32(A.evaluate("1 << 31")) == A.evaluate("int.MinValue")
    for bad in ("__import__('os')", "1 + 1", "sizeof(int)", "UNKNOWN", "(1", "1 2"):
        with pytest.raises(ValueError):
            A.evaluate(bad)


# ---- the models' own copies and the array builders ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("module,attribute,twin", MODEL_TWINS, ids=[f"{m}.{a}" for m, a, _ in MODEL_TWINS])
def test_model_twins(module, attribute, twin):
    theirs, ours = getattr(importlib.import_module(module), attribute), getattr(gpu, twin)
    if attribute.endswith("_NAMES"):
        assert tuple(theirs) == ours.names
    elif isinstance(ours, np.dtype):
        assert theirs == ours and A.dtype_layout(theirs) == A.dtype_layout(ours)
    else:
        assert theirs == ours


def test_array_builders_fill_the_structs_byte_for_byte():
    import lightmodel
    import movemodel

    assert gpu.LIFTED_PIECE_DTYPE["piece"] == gpu.PIECE_DTYPE
    assert len(lightmodel.words(lightmodel.params((0, 0, 0), (1, 1, 1)))) * 4 == C.sizeof(gpu.LightParams) == 64
    assert np.int32(gpu.MOVED_INVALID) == np.int32(-2**31)
    arr = gpu.bodies_array([{"pos": (1, 2, 3), "size": (4, 5, 6)}, movemodel.body((7, 8, 9), (1, 1, 1), (-1, -2, -3), 5, 3)])
    assert arr.tobytes() == np.array([1, 2, 3, 4, 5, 6, 0, 0, 0, 0, 0, 0, 7, 8, 9, 1, 1, 1, -1, -2, -3, 5, 3, 0], dtype=np.int32).tobytes()
    assert gpu.bodies_array(arr) is not None and gpu.bodies_array(arr).tobytes() == arr.tobytes()
    lamps = gpu.lamps_array([((1, -2, 3), 4, 5), dict(pos=(6, 7, 8), radius=9, level=10)])
    assert np.frombuffer(bytes(lamps), dtype=np.int32).tolist() == [1, -2, 3, 4, 5, 0, 0, 0, 6, 7, 8, 9, 10, 0, 0, 0]
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"all {len(gpu.EXPORTS)} exports" in readme and "all 64 exports" in readme and "cvx_world_light_lamps" in readme
