"""No GPU: the declarations of i2r_rows_gather_multi in include/i2r_hip.h and their ctypes mirrors in cabi agree (struct layout, segment
limit, program op, export name), the additive change left I2R_ABI_VERSION at 17, and Program.rows_gather_multi fills the segment
fields from Acts and raw buffers as the kernel reads them."""
import ctypes as C
import os
import re

import pytest
import torch

from i2r_amd import cabi, engine

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


def test_program_segments_carry_windows_sizes_and_row_bytes():
    """three segments -- an fp32 Act pair, a 16-bit pair, a raw source the program does not own -- with windows into source and output"""
    P = engine.Program(torch.device("cpu"))
    tab = torch.zeros(8, dtype=torch.int32)
    a32, o32 = P.alloc(6, 4, 3, 48), P.alloc(10, 4, 3, 48)             # rows of 4 * 3 * 48 floats
    a16, o16 = P.alloc(6, 2, 2, 78, dt=1), P.alloc(8, 2, 2, 78, dt=1)  # rows of 2 * 2 * 80 bf16 (78 channels in rows of 80)
    mask = engine.Act(torch.zeros(5 * 8 * 4), 5, 8, 4, 1, 1)           # [5, 1, 8, 4] masks: rows of 32 floats
    raw = engine._RawAct(4096, mask, n=3)
    a = P.rows_gather_multi([(a32, o32, tab, 5, 3, 2, 4), (a16, o16, tab, 8, 4, 1, 0), (raw, mask, tab, 5, 3, 0, 0)])
    assert P.ops[-1] == (cabi.GROUPS_OP_ROWS_GATHER_MULTI, 0, a) and a.n_seg == 3
    rows = [4 * 3 * 48 * 4, 2 * 2 * 80 * 2, 8 * 4 * 4]
    want = [(a32.ptr + 2 * rows[0], o32.ptr + 4 * rows[0], 5, 3), (a16.ptr + rows[1], o16.ptr, 8, 4), (4096, mask.ptr, 5, 3)]
    for g, row, (src, out, n_out, n_src) in zip(a.seg, rows, want):
        assert (g.src, g.out, g.map, g.n_out, g.n_src, g.row_bytes) == (src, out, tab.data_ptr(), n_out, n_src, row)
    assert all((g.src, g.out, g.n_out, g.row_bytes) == (None, None, 0, 0) for g in a.seg[3:])
    assert any(t is tab for t in P.keep)


def test_program_refuses_odd_rows_and_windows_past_the_output():
    P = engine.Program(torch.device("cpu"))
    tab = torch.zeros(8, dtype=torch.int32)
    odd = engine.Act(torch.zeros(4 * 3), 4, 3, 1, 1, 1)  # rows of 3 floats: 12 bytes
    with pytest.raises(AssertionError):
        P.rows_gather_multi([(engine._RawAct(4096, odd), odd, tab, 4, 4, 0, 0)])
    src, out = P.alloc(6, 2, 2, 16), P.alloc(6, 2, 2, 16)
    P.rows_gather_multi([(src, out, tab, 4, 6, 0, 2)])  # crops 2..5: the last window that fits
    with pytest.raises(AssertionError):
        P.rows_gather_multi([(src, out, tab, 4, 6, 0, 3)])
    with pytest.raises(AssertionError):
        P.rows_gather_multi([(src, out, tab, 4, 6, 1, 0)])  # source window past src.n
    with pytest.raises(AssertionError):
        P.rows_gather_multi([(src, out, tab[:3], 4, 6, 0, 0)])  # table shorter than n_out
