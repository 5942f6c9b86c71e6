"""CPU: the blittable structs of host/csharp/CpuVoxGpu.cs (the P/Invoke binding a reference maintainer adds) have the
reference's field lists, packing and sizes.  The headers cannot say this: it pins the binding to the original's sources.  What the headers
can say (DllImports, layouts, constants) is tests/test_abi_mirrors.py's; the file cannot be compiled in this image, so both read it with the
parsers of tests/abilib.py."""
import abilib as A

STRUCTS = A.cs_structs("CpuVoxGpu.cs")


def _fields(name):
    return [f.name for f in STRUCTS[name][1].fields]


def test_blittable_structs_have_the_reference_layout():
    attrs, _ = STRUCTS["SegmentData"]  # RenderManager.SegmentData, RenderManager.cs:503-510: 4 x float2 + int
    assert "LayoutKind.Sequential" in attrs and "Pack = 4" in attrs
    assert _fields("SegmentData") == ["MinScreen", "MaxScreen", "CamLocalPlaneRayMin", "CamLocalPlaneRayMax", "RayCount"]
    assert A.cs_layout(STRUCTS, "SegmentData")[1] == 36
    attrs, _ = STRUCTS["CameraData"]  # CameraData.cs:11-16
    assert "LayoutKind.Sequential" in attrs and "Pack = 4" in attrs
    assert _fields("CameraData") == ["WorldToScreenMatrix", "PositionXZ", "PositionY", "InverseElementIterationDirection", "pad", "FarClip", "LODDistances"]
    assert A.cs_layout(STRUCTS, "CameraData")[1] == 108
    for name, size in (("Counters", 88), ("RaybufferLayout", 24), ("RowSpan", 24)):
        assert "LayoutKind.Sequential" in STRUCTS[name][0] and A.cs_layout(STRUCTS, name)[1] == size, name
