"""-m gpu: i2r_rows_gather_multi through the raw C-ABI against torch.index_select, bit for bit: eight segments in one launch (rows of
16 B, 48 B, 4096 B and 40000 B -- 2500 chunks, three workgroups of uneven share per row), tables with -1, repeats and the last valid
index, an empty segment, canaries of 64 rows on both sides of every output; out-of-range entries against a source allocated four marker
rows larger than n_src says (so even a kernel without the check would stay inside the allocation); the rejected calls; the program op."""
import ctypes as C

import pytest
import torch

from i2r_amd import cabi

pytestmark = pytest.mark.gpu
CANARY_ROWS, CANARY, MARKER = 64, 0x5A, 0xAB
INT32_MIN = -2 ** 31


class Seg:
    """one segment: a random byte source of n_src rows (+ `slack` marker rows behind them), an output between two canary blocks"""

    def __init__(self, seed, row_bytes, n_src, table, slack=0):
        g = torch.Generator().manual_seed(seed)
        self.row_bytes, self.n_src, self.n_out = row_bytes, n_src, len(table)
        src = torch.randint(1, MARKER, (n_src + slack, row_bytes), dtype=torch.uint8, generator=g)  # (no zero and no marker byte in a real row)
        src[n_src:] = MARKER
        self.src = src.cuda()
        self.table = torch.tensor(table, dtype=torch.int32).cuda()
        self.buf = torch.full((2 * CANARY_ROWS + self.n_out, row_bytes), CANARY, dtype=torch.uint8, device="cuda")
        self.out = self.buf[CANARY_ROWS:CANARY_ROWS + self.n_out]

    def fill(self, g, n_src=None):
        g.src, g.out, g.map = self.src.data_ptr(), self.out.data_ptr(), self.table.data_ptr()
        g.n_out, g.n_src, g.row_bytes = self.n_out, self.n_src if n_src is None else n_src, self.row_bytes

    def want(self):
        t = self.table.long()
        ok = (t >= 0) & (t < self.n_src)
        rows = torch.index_select(self.src, 0, torch.where(ok, t, torch.zeros_like(t)))
        return torch.where(ok[:, None], rows, torch.zeros_like(rows))

    def canaries_intact(self):
        return bool((self.buf[:CANARY_ROWS] == CANARY).all() and (self.buf[CANARY_ROWS + self.n_out:] == CANARY).all())

    def untouched(self):
        return bool((self.buf == CANARY).all())


def _args(segs):
    a = cabi.GatherMultiArgs()
    a.n_seg = len(segs)
    for g, s in zip(a.seg, segs):
        if s is not None:
            s.fill(g)
    return a


def _call(a):
    rc = cabi.lib().i2r_rows_gather_multi(C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _main_segments():
    return [Seg(1, 16, 3, [2]),
            Seg(2, 48, 4, [-1, 3, 3, 0, 1]),
            Seg(3, 4096, 6, [5, -1, 0, 5, 2]),
            Seg(4, 40000, 3, [2, 0, -1, 2, 1]),   # 2500 chunks a row: three workgroups of 834, 834 and 832
            None,                                 # n_out == 0: skipped, its null pointers are never read
            Seg(6, 16, 5, [4, 4, -1, 0, 4]),
            Seg(7, 4096, 2, [1]),
            Seg(8, 48, 1, [0])]


def test_eight_segments_in_one_launch_bit_equal_to_torch():
    segs = _main_segments()
    assert _call(_args(segs)) == 0, cabi.lib().i2r_last_error()
    for i, s in enumerate(segs):
        if s is None:
            continue
        assert torch.equal(s.out, s.want()), "segment %d" % i
        assert s.canaries_intact(), "segment %d wrote outside its rows" % i


def test_out_of_range_entries_give_zero_rows():
    n_src = 5
    for row_bytes in (48, 40000):
        s = Seg(11, row_bytes, n_src, [n_src, 4, n_src + 3, INT32_MIN, 0, -1], slack=4)
        assert _call(_args([s])) == 0, cabi.lib().i2r_last_error()
        assert torch.equal(s.out, s.want()) and s.canaries_intact()
        assert not (s.out == MARKER).any(), "a row behind n_src was read"
        assert (s.out[[0, 2, 3, 5]] == 0).all() and (s.out[[1, 4]] != 0).all()


@pytest.mark.parametrize("case", ["row_bytes", "misaligned_out", "src_is_out", "n_seg"])
def test_rejected_calls_write_nothing(case):
    segs = [Seg(21, 48, 4, [0, 1, 2]), Seg(22, 4096, 2, [1, 0])]
    a = _args(segs)
    if case == "row_bytes":
        a.seg[1].row_bytes = 24
    elif case == "misaligned_out":
        a.seg[1].out = a.seg[1].out + 8
    elif case == "src_is_out":
        a.seg[1].src = a.seg[1].out
    else:
        a.n_seg = 9
    assert _call(a) != 0
    assert cabi.lib().i2r_last_error().decode().startswith("i2r_rows_gather_multi")
    assert all(s.untouched() for s in segs), "a rejected call must launch nothing"


def test_empty_segments_launch_nothing():
    a = cabi.GatherMultiArgs()
    for n in (0, 3, 8):
        a.n_seg = n  # (all n_out == 0, all pointers null)
        assert _call(a) == 0
    s = Seg(31, 48, 4, [0, 1])
    a = _args([s])
    a.seg[0].n_out = 0
    assert _call(a) == 0 and s.untouched()


def test_program_op_gives_the_same_bits():
    direct, via_op = _main_segments(), _main_segments()
    assert _call(_args(direct)) == 0
    a = _args(via_op)
    ops = (cabi.Op * 1)()
    ops[0].kind, ops[0].lane, ops[0].args = cabi.GROUPS_OP_ROWS_GATHER_MULTI, 0, C.cast(C.pointer(a), C.c_void_p)
    cur = torch.cuda.current_stream().cuda_stream
    streams = (C.c_void_p * 4)(cur, cur, cur, cur)
    cabi.check(cabi.lib().i2r_run_program(ops, 1, streams, None), "i2r_run_program")
    torch.cuda.synchronize()
    for d, v in zip(direct, via_op):
        if d is not None:
            assert torch.equal(d.buf, v.buf) and torch.equal(v.out, v.want())
