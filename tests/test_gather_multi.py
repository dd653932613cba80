"""No GPU: the declarations of i2r_rows_gather_multi in include/i2r_hip.h and their ctypes mirrors in cabi agree (struct layout, segment
limit, program op, export name), and the additive change left I2R_ABI_VERSION at 17."""
import ctypes as C
import os
import re

from i2r_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()

C_TYPES = {"const void*": C.c_void_p, "void*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64}


def _struct_fields(name):
    """[(field, ctypes type)] of a one-line `typedef struct NAME { ... } NAME;` of the header"""
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, flags=re.S)
    assert m, name
    out = []
    for decl in m.group(1).split(";"):
        decl = re.sub(r"/\*.*?\*/", "", decl).strip()
        if not decl:
            continue
        t, names = re.match(r"((?:const )?\w+\*?)\s+(.*)", decl).groups()
        out += [(n.strip(), t) for n in names.split(",")]
    return out


def test_header_declares_struct_limit_and_op():
    assert re.search(r"^#define I2R_MAX_GATHER_SEGS 8$", HEADER, flags=re.M)
    assert re.search(r"\bI2R_OP_ROWS_GATHER_MULTI = 31\b", HEADER)
    assert re.search(r"^I2R_API int i2r_rows_gather_multi\(const i2r_gather_multi_args\* a, void\* stream\);", HEADER, flags=re.M)
    assert [n for n, _ in _struct_fields("i2r_gather_seg")] == ["src", "out", "map", "n_out", "n_src", "row_bytes"]
    assert re.search(r"typedef struct i2r_gather_multi_args \{ i2r_gather_seg seg\[I2R_MAX_GATHER_SEGS[^\]]*\]; int32_t n_seg; \} i2r_gather_multi_args;", HEADER)


def test_cabi_mirrors_the_header_layout():
    fields = _struct_fields("i2r_gather_seg")
    assert [n for n, _ in cabi.GatherSeg._fields_] == [n for n, _ in fields]

    class FromHeader(C.Structure):
        _fields_ = [(n, C_TYPES[t]) for n, t in fields]
    assert C.sizeof(cabi.GatherSeg) == C.sizeof(FromHeader) == 40
    for n, _ in fields:
        assert getattr(cabi.GatherSeg, n).offset == getattr(FromHeader, n).offset, n
        assert getattr(cabi.GatherSeg, n).size == getattr(FromHeader, n).size, n
    assert cabi.MAX_GATHER_SEGS == 8 and cabi.GROUPS_OP_ROWS_GATHER_MULTI == 31

    class MultiFromHeader(C.Structure):
        _fields_ = [("seg", FromHeader * 8), ("n_seg", C.c_int32)]
    assert C.sizeof(cabi.GatherMultiArgs) == C.sizeof(MultiFromHeader) == 8 * 40 + 8
    assert cabi.GatherMultiArgs.n_seg.offset == 320


def test_export_and_abi_version():
    assert "i2r_rows_gather_multi" in cabi.EXPORTS
    assert re.search(r"^#define I2R_ABI_VERSION 17$", HEADER, flags=re.M) and cabi.ABI_VERSION == 17
    L = cabi.load_library()
    assert L.i2r_abi_version() == 17
    assert L.i2r_rows_gather_multi.argtypes[0] is C.POINTER(cabi.GatherMultiArgs)
