"""The C ABI as its sources state it, read once for tests/test_abi_mirrors.py and tests/test_abi.py: the functions, complete structs and integer
constants of a header under include/, the DllImports, structs and constants of a file under host/csharp/ (which no machine here can compile), the
layout both give a struct, and MIRRORS, the table of what mirrors each struct in Python and C#."""
import collections
import ctypes as C
import os
import re

from cpuvox_amd import dist, gpu, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Field = collections.namedtuple("Field", "name base pointer extents")   # `const uint8_t *rgba` is ("rgba", "uint8_t", True, ()); extents are ints
Struct = collections.namedtuple("Struct", "fields stated")              # stated: the header's or the C# file's `N bytes` remark, or None
Slot = collections.namedtuple("Slot", "name offset size")

C_SCALARS = {"int8_t": 1, "uint8_t": 1, "char": 1, "int16_t": 2, "uint16_t": 2, "int32_t": 4, "uint32_t": 4, "int": 4, "float": 4, "int64_t": 8,
             "uint64_t": 8, "double": 8}
CS_SCALARS = {"byte": 1, "sbyte": 1, "short": 2, "ushort": 2, "int": 4, "uint": 4, "float": 4, "long": 8, "ulong": 8, "double": 8, "IntPtr": 8}
POINTER_BYTES = 8


def header_text(header, comments=False):
    text = open(os.path.join(ROOT, "include", header)).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def csharp_text(name):
    return open(os.path.join(ROOT, "host", "csharp", name)).read()


# ---- integer constant expressions: decimal, hex, <<, |, unary minus, parentheses, integer casts and names already known ------------------------

def evaluate(expression, known=()):
    """The value of an integer constant expression of a header or a C# file; ValueError for anything outside the grammar."""
    tokens = re.findall(r"0[xX][0-9a-fA-F]+|\d+|<<|[|()\-]|[A-Za-z_][\w.]*|\S", re.sub(r"(?<=[0-9a-fA-F])[uUlL]+\b", "", expression))
    at = 0

    def peek():
        return tokens[at] if at < len(tokens) else None

    def take(want=None):
        nonlocal at
        token = peek()
        if token is None or (want is not None and token != want):
            raise ValueError(f"`{expression}`: `{want or 'a value'}` expected at token {at}")
        at += 1
        return token

    def unary():
        token = take()
        if token == "-":
            return -unary()
        if token == "(":
            if peek() in C_SCALARS or peek() in CS_SCALARS:  # a cast: the comparisons are made on 32-bit values anyway
                take(), take(")")
                return unary()
            value = either()
            take(")")
            return value
        if re.fullmatch(r"0[xX][0-9a-fA-F]+|\d+", token):
            return int(token, 0)
        if token == "int.MinValue":
            return -(1 << 31)
        if token in known:
            return known[token]
        raise ValueError(f"`{expression}`: `{token}` is no integer constant")

    def shift():
        value = unary()
        while peek() == "<<":
            take()
            value <<= unary()
        return value

    def either():
        value = shift()
        while peek() == "|":
            take()
            value |= shift()
        return value

    value = either()
    if at != len(tokens):
        raise ValueError(f"`{expression}`: `{tokens[at]}` left over")
    return value


def int32(value):
    """`1 << 31` in an enum, int.MinValue in C# and -(1 << 31) in Python are one 32-bit word."""
    return C.c_int32(value).value


# ---- the C side -----------------------------------------------------------------------------------------------------------------------------

def c_functions(header, prefix="cvx_"):
    """{name: (return type, [parameter declarations])} of every function the header declares."""
    out = {}
    for m in re.finditer(r"\b([a-z_0-9 ]+?[ \*]+)(" + prefix + r"[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header_text(header)):
        params = m.group(3).strip()
        assert m.group(2) not in out, f"{header} declares {m.group(2)} twice"
        out[m.group(2)] = (m.group(1).strip(), [] if params in ("", "void") else [p.strip() for p in params.split(",")])
    return out


def c_constants(header, known=()):
    """{name: value} of the header's enum entries and object-like #defines with a value, in order; `known` resolves names of other headers."""
    text, out = header_text(header), {}
    scope = collections.ChainMap(out, dict(known))
    found = [(m.start(), 0, m.group(1), m.group(2)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M)]
    for m in re.finditer(r"\benum\b[^{;]*\{(.*?)\}", text, flags=re.S):
        for k, entry in enumerate(filter(None, (e.strip() for e in m.group(1).split(",")))):
            name, _, expression = (part.strip() for part in entry.partition("="))
            found.append((m.start(), k, name, expression or (None if k else "0")))  # without a value: one more than the entry before it
    for _, _, name, expression in sorted(found):
        out[name] = previous = previous + 1 if expression is None else evaluate(expression, scope)
    return out


def c_structs(header, constants=()):
    """{name: Struct} of the complete `typedef struct name { ... } name;` of the header, macro extents resolved from `constants`."""
    out = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", header_text(header, comments=True), flags=re.S):
        name, body = m.group(1), m.group(2)
        assert m.group(3) == name, f"{header}: struct {name} is typedef'd {m.group(3)}"
        stated = re.match(r"\s*/\*\s*(\d+) bytes", body)
        fields = []
        for statement in filter(None, (s.strip() for s in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"))):
            decl = re.fullmatch(r"(?:const\s+)?(\w+)\s*(?:const\s+)?(.+)", statement, flags=re.S)
            assert decl, f"{header}: {name}: `{statement}`"
            for declarator in decl.group(2).split(","):
                d = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*((?:\[\w+\]\s*)*)", declarator)
                assert d, f"{header}: {name}: `{statement}`"
                extents = tuple(evaluate(e, constants) for e in re.findall(r"\[(\w+)\]", d.group(3)))
                fields.append(Field(d.group(2), decl.group(1), bool(d.group(1)), extents))
        out[name] = Struct(fields, int(stated.group(1)) if stated else None)
    return out


def layout(fields, structs, scalars=C_SCALARS, pack=8, leaves=False):
    """Natural alignment, capped at `pack`: ([Slot per field], total bytes, alignment).  leaves=True gives a nested struct's fields in its place."""
    slots, at, widest = [], 0, 1
    for f in fields:
        inner = None
        if f.pointer:
            size = align = POINTER_BYTES
        elif f.base in scalars:
            size = align = scalars[f.base]
        else:
            assert f.base in structs, f"the type `{f.base}` of `{f.name}` is unknown"
            inner, size, align = layout(structs[f.base].fields, structs, scalars, pack, leaves)
        align = min(align, pack)
        at = -(-at // align) * align
        count = 1
        for e in f.extents:
            count *= e
        if inner is not None and leaves and count == 1:
            slots += [Slot(s.name, at + s.offset, s.size) for s in inner]
        else:
            slots.append(Slot(f.name, at, size * count))
        at += size * count
        widest = max(widest, align)
    return slots, -(-at // widest) * widest, widest


def ctypes_layout(structure):
    return [Slot(name, getattr(structure, name).offset, getattr(structure, name).size) for name, *_ in structure._fields_], C.sizeof(structure)


def dtype_layout(dtype):
    return [Slot(name, dtype.fields[name][1], dtype.fields[name][0].itemsize) for name in dtype.names], dtype.itemsize


def c_kind(declaration):
    """A C parameter or return type as one of ptr, i32, i64, f32, f64, void."""
    d = declaration.replace("const ", "").strip()
    if "*" in d or "[" in d:
        return "ptr"
    base = d.split()[0]
    return {"int": "i32", "int32_t": "i32", "uint32_t": "i32", "int64_t": "i64", "uint64_t": "i64", "float": "f32", "double": "f64"}.get(base, base)


def ctypes_kind(ctype):
    """The same for an entry of argtypes or a restype; None (restype of a void function) is void."""
    if ctype is None:
        return "void"
    if ctype in (C.c_void_p, C.c_char_p) or issubclass(ctype, C._Pointer):
        return "ptr"
    return {C.c_int32: "i32", C.c_uint32: "i32", C.c_int64: "i64", C.c_float: "f32", C.c_double: "f64"}[ctype]  # (c_int is c_int32)


# ---- the C# side ----------------------------------------------------------------------------------------------------------------------------

def cs_imports(name):
    """{name: (return type, [parameter declarations])} of the file's [DllImport(Lib)] lines."""
    out = {}
    for m in re.finditer(r"\[DllImport\(Lib\)\]\s*public static extern\s+([A-Za-z]+)\s+(cvx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", csharp_text(name), flags=re.S):
        params = m.group(3).strip()
        assert m.group(2) not in out, f"{name} imports {m.group(2)} twice"
        out[m.group(2)] = (m.group(1), [] if not params else [p.strip() for p in params.split(",")])
    return out


def cs_kind(declaration):
    d = declaration.strip()
    if d.startswith("out ") or "*" in d or d.split()[0] == "IntPtr":
        return "ptr"
    return {"int": "i32", "uint": "i32", "long": "i64", "ulong": "i64", "float": "f32", "double": "f64", "void": "void"}[d.split()[0]]


def cs_structs(name):
    """{struct name: (the StructLayout arguments, Struct)} of the file; Struct.stated is the `// N bytes` remark on the struct's line."""
    out = {}
    for m in re.finditer(r"\[StructLayout\(([^\]]*)\)\]\s*public (?:unsafe )?struct (\w+)[ \t]*(?://[ \t]*(\d+) bytes)?[^{]*\{(.*?)\n\t\}", csharp_text(name), flags=re.S):
        fields = []
        for statement in filter(None, (s.strip() for s in re.sub(r"//[^\n]*", "", m.group(4)).split(";"))):
            decl = re.fullmatch(r"(?:public\s+)?(?:fixed\s+)?(\w+)(\*?)\s+(.+)", statement, flags=re.S)
            assert decl, f"{name}: {m.group(2)}: `{statement}`"
            for declarator in decl.group(3).split(","):
                d = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", declarator)
                assert d, f"{name}: {m.group(2)}: `{statement}`"
                fields.append(Field(d.group(1), decl.group(1), bool(decl.group(2)), (int(d.group(2)),) if d.group(2) else ()))
        out[m.group(2)] = (m.group(1), Struct(fields, int(m.group(3)) if m.group(3) else None))
    return out


def cs_layout(structs, name, leaves=True):
    """layout() of a struct of cs_structs() under its Pack (8 when it names none)."""
    attrs, struct = structs[name]
    pack = re.search(r"Pack\s*=\s*(\d+)", attrs)
    return layout(struct.fields, {n: s for n, (_, s) in structs.items()}, CS_SCALARS, int(pack.group(1)) if pack else 8, leaves)


def cs_constants(name):
    """{name: value} of the file's `const int` declarations."""
    out = {}
    for m in re.finditer(r"\bconst int\s+([^;]+);", csharp_text(name)):
        for entry in m.group(1).split(","):
            key, _, expression = (part.strip() for part in entry.partition("="))
            out[key] = evaluate(expression, out)
    return out


# ---- what mirrors what ------------------------------------------------------------------------------------------------------------------------

# C struct -> (ctypes class, numpy dtype, the C# struct in the header's file), None where there is none.  Every complete
# struct of a header of gpu.ABI_HEADERS has a row: tests/test_abi_mirrors.py fails for one without.
MIRRORS = {
    "cvx_segment_data": (host.SegmentData, None, "SegmentData"),          # (these two: cpuvox_amd.host owns the frame set-up that fills them;
    "cvx_camera_data": (host.CameraData, None, "CameraData"),             # passed on as ctypes arrays, never viewed through numpy)
    "cvx_counters": (gpu.Counters, None, "Counters"),                     # read field by field
    "cvx_row_span": (None, dist.SPAN_DTYPE, "RowSpan"),                   # no class: cpuvox_amd.dist fills a numpy array for the device
    "cvx_raybuffer_layout": (gpu.RaybufferLayout, None, "RaybufferLayout"),
    "cvx_brush_stroke": (gpu.BrushStroke, gpu.STROKE_DTYPE, "BrushStroke"),
    "cvx_pick_ray": (gpu.PickRay, gpu.PICK_RAY_DTYPE, "PickRay"),
    "cvx_pick_hit": (gpu.PickHit, gpu.PICK_HIT_DTYPE, "PickHit"),
    "cvx_mesh_vertex": (host.MeshVertex, gpu.MESH_VERTEX_DTYPE, "MeshVertex"),  # the class is the host library's; gpu keeps the dtype only
    "cvx_mesh_texture": (gpu._TextureStruct, None, "MeshTexture"),        # holds a pointer: no dtype
    "cvx_copy_placement": (gpu.CopyPlacement, gpu.COPY_PLACEMENT_DTYPE, "CopyPlacement"),
    "cvx_piece": (gpu.Piece, gpu.PIECE_DTYPE, "Piece"),
    "cvx_pieces_summary": (gpu.PiecesSummary, gpu.PIECES_SUMMARY_DTYPE, "PiecesSummary"),
    "cvx_settle_summary": (gpu.SettleSummary, gpu.SETTLE_SUMMARY_DTYPE, "SettleSummary"),
    "cvx_cavity_params": (gpu.CavityParams, None, "CavityParams"),        # parameters and single results need no array view: no dtype
    "cvx_cavities_summary": (gpu.CavitiesSummary, gpu.CAVITIES_SUMMARY_DTYPE, "CavitiesSummary"),
    "cvx_light_params": (gpu.LightParams, None, "LightParams"),
    "cvx_lamp": (gpu.Lamp, None, "Lamp"),                                 # gpu.lamps_array builds a ctypes array
    "cvx_move_body": (gpu.MoveBody, gpu.MOVE_BODY_DTYPE, "MoveBody"),
    "cvx_move_result": (gpu.MoveResult, gpu.MOVE_RESULT_DTYPE, "MoveResult"),
    "cvx_nav_params": (gpu.NavParams, None, "NavParams"),
    "cvx_nav_step": (gpu.NavStep, gpu.NAV_STEP_DTYPE, "NavStep"),
    "cvx_nav_summary": (gpu.NavSummary, gpu.NAV_SUMMARY_DTYPE, "NavSummary"),
    "cvx_surface_quad": (gpu.SurfaceQuad, gpu.SURFACE_QUAD_DTYPE, "SurfaceQuad"),
    "cvx_surface_summary": (gpu.SurfaceSummary, gpu.SURFACE_SUMMARY_DTYPE, "SurfaceSummary"),
    "cvx_model_map": (gpu.ModelMap, None, "CvxModelMap"),
    "cvx_model": (gpu.Model, None, "CvxModel"),                           # holds pointers
    "cvx_model_instance": (gpu.ModelInstance, None, "CvxModelInstance"),
    "cvx_spread_params": (gpu.SpreadParams, None, "CvxSpreadParams"),
    "cvx_spread_seed": (gpu.SpreadSeed, gpu.SPREAD_SEED_DTYPE, "CvxSpreadSeed"),
    "cvx_spread_summary": (gpu.SpreadSummary, gpu.SPREAD_SUMMARY_DTYPE, "CvxSpreadSummary"),
    "cvx_surface_rect": (gpu.SurfaceRect, gpu.SURFACE_RECT_DTYPE, "CvxSurfaceRect"),
    "cvx_surface_rects_summary": (gpu.SurfaceRectsSummary, gpu.SURFACE_RECTS_SUMMARY_DTYPE, "CvxSurfaceRectsSummary"),
    "cvx_snapshot_info": (gpu.SnapshotInfo, None, "CvxSnapshotInfo"),
    "cvx_snapshot_change": (gpu.SnapshotChange, gpu.SNAPSHOT_CHANGE_DTYPE, "CvxSnapshotChange"),
    "cvx_snapshot_diff_summary": (gpu.SnapshotDiffSummary, None, "CvxSnapshotDiffSummary"),
    "cvx_lifted_piece": (gpu.LiftedPiece, gpu.LIFTED_PIECE_DTYPE, "CvxLiftedPiece"),
    "cvx_lift_summary": (gpu.LiftSummary, None, "CvxLiftSummary"),
}


def abi():
    """Everything the headers of gpu.ABI_HEADERS state, read once: ({constant: value}, {struct: Struct}, {struct: its header}), later headers
    seeing the constants and structs of earlier ones, as their #include of cpuvox_gpu.h lets them."""
    if not _ABI:
        constants, structs, owner = {}, {}, {}
        for header, _, _ in gpu.ABI_HEADERS:
            constants.update(c_constants(header, constants))
            for name, struct in c_structs(header, constants).items():
                assert name not in structs, f"{header} declares struct {name} again"
                structs[name], owner[name] = struct, header
        _ABI.extend((constants, structs, owner))
    return _ABI


_ABI = []
