"""CPU: the combination of validation numbers across data-parallel ranks -- the C-ABI surface of i2r_val_combine, the numpy restatement
tests/_val_combine_ref.py on the reference's own output cut into shards (tests/golden/val_metrics_reference.npz), the gather of the rows
at world size 2 over gloo, and the bookkeeping of caller.PoseTable."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _val_combine_ref as cref
import _val_ref
from i2r_amd import cabi, caller
from i2r_amd import dist as i2r_dist
from test_val_metrics import _c_struct_fields, case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (fixture case, crops per shard): an empty rank in the middle, one crop per rank, and the two smallest cuts
SHARDED = [(2, (2, 0, 3)), (2, (1, 1, 1, 1, 1)), (3, (1, 2)), (4, (1, 1))]
_CACHE = {}


def shard_results(ci, shards, use_w=True):
    """_val_ref.val_metrics on every non-empty shard of case ci (computed once) -> list of Result | None"""
    key = (ci, shards, use_w)
    if key not in _CACHE:
        d = case(ci)
        assert sum(shards) == d.S
        out, lo = [], 0
        for n in shards:
            sl = slice(lo, lo + n)
            out.append(_val_ref.val_metrics(d.output[sl], d.target[sl], d.target_weight[sl], use_w) if n else None)
            lo += n
        _CACHE[key] = out
    return _CACHE[key]


def shard_rows(ci, shards, use_w=True):
    J = case(ci).J
    return np.stack([cref.row(n, r.sse, r.hits, r.valid) if n else cref.row(0, J=J) for n, r in zip(shards, shard_results(ci, shards, use_w))])


def test_header_binding_and_exports_agree_and_abi_stays_17():
    import __graft_entry__
    header = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert int(re.search(r"#define I2R_ABI_VERSION (\d+)", header).group(1)) == 17 == cabi.ABI_VERSION
    assert re.search(r"^I2R_API\s+int\s+i2r_val_combine\s*\(const i2r_val_combine_args\* a, void\* stream\);", header, flags=re.M)
    assert "i2r_val_combine" in cabi.EXPORTS and "i2r_val_combine" in __graft_entry__._declared_exports()
    fields = _c_struct_fields(header, "i2r_val_combine_args")
    assert fields == [(n, t) for n, t in cabi.ValCombineArgs._fields_]
    assert [n for n, _ in fields] == ["parts", "sse", "hits", "valid", "loss", "acc", "avg_acc", "cnt", "n_crops", "meter", "n_part", "joints", "h", "w"]
    assert ctypes.sizeof(cabi.ValCombineArgs) == 10 * 8 + 4 * 4
    assert "2^31 - 1" in re.search(r"/\* i2r_val_combine --.*?\*/", header, flags=re.S).group(0), "the precondition on the total crop count"
    if not os.path.exists(cabi.LIB_PATH):
        __graft_entry__.build()
    assert "i2r_val_combine" in __graft_entry__.exported_symbols(cabi.LIB_PATH)
    L = cabi.load_library()
    assert L.i2r_abi_version() == 17 and L.i2r_val_combine.argtypes[0]._type_ is cabi.ValCombineArgs


@pytest.mark.parametrize("ci,shards", SHARDED)
def test_restatement_on_shards_reproduces_the_reference(ci, shards):
    d = case(ci)
    rows = shard_rows(ci, shards)
    r = cref.combine(rows, d.h, d.w)
    whole = _val_ref.val_metrics(d.output, d.target, d.target_weight, True)
    assert r.n_crops == d.S
    assert np.array_equal(r.acc, d.acc) and r.avg_acc == float(d.avg_acc) and r.cnt == int(d.cnt)
    assert np.array_equal(r.hits, whole.hits) and np.array_equal(r.valid, whole.valid)
    rel = abs(r.loss - float(d.loss64_w1)) / float(d.loss64_w1)
    print("case %d shards %s: loss %.17g, fixture float64 %.17g, rel %.3g" % (ci, shards, r.loss, float(d.loss64_w1), rel))
    assert rel <= 2.0 ** 20 * 2.0 ** -53
    # the inputs bite: a joint that counts in one shard and not in another, a joint that counts nowhere, and a wrong plain average
    per = [s for s in shard_results(ci, shards) if s is not None]
    holes = sum(int(s.valid[j] == 0 and r.valid[j] > 0) for s in per for j in range(d.J))
    dead = int((r.valid == 0).sum())
    naive = float(np.mean([s.avg_acc for s in per]))
    print("case %d shards %s: %d (shard, joint) pairs without a counted crop, %d joints without one anywhere, mean of shard avg_acc %.6g vs %.6g"
          % (ci, shards, holes, dead, naive, r.avg_acc))
    assert holes >= 1 and dead >= 1 and naive != r.avg_acc
    # one part is the whole batch: the restatement's tail is _val_ref's
    one = cref.combine(cref.row(d.S, whole.sse, whole.hits, whole.valid)[None], d.h, d.w)
    assert one.loss == whole.loss and np.array_equal(one.acc, whole.acc) and one.avg_acc == whole.avg_acc and one.cnt == whole.cnt


def test_restatement_edges():
    J = 3
    r = cref.combine(np.zeros((4, 1 + 3 * J)), 8, 6, meter=(m := [1.0, 2.0, 3.0, 4.0]))
    assert r.n_crops == 0 and r.loss == 0 and r.acc.tolist() == [0.0] * (J + 1) and r.cnt == 0 and m == [1.0, 2.0, 3.0, 4.0]
    junk = cref.row(0, [5.0] * J, [1] * J, [1] * J)                      # n_crops == 0: the row is not read
    real = cref.row(2, [1.0, 2.0, 3.0], [1, 0, 0], [2, 1, 0])
    m = [0.0] * 4
    r = cref.combine(np.stack([junk, real, cref.row(-2, [7.0] * J, [1] * J, [1] * J)]), 8, 6, meter=m)
    assert r.sse.tolist() == [1.0, 2.0, 3.0] and r.acc.tolist() == [0.25, 0.5, 0.0, -1.0] and r.cnt == 2 and r.n_crops == 2
    assert m == [r.loss * 2, 2.0, 0.5, 2.0]


def _gloo_worker(rank, world, port, J):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ms, ns = [], [3, 0]
        for r in range(world):
            m = caller.ValMetrics()
            if ns[r]:
                m.sse = torch.arange(J, dtype=torch.float64) * 0.37 + 1.0 / 3.0
                m.hits = torch.arange(J, dtype=torch.int32) % 3
                m.valid = torch.arange(J, dtype=torch.int32) % 3 + 1
            else:   # a rank without images: val_metrics launched nothing and returned zeros
                m.sse, m.hits, m.valid = torch.zeros(J, dtype=torch.float64), torch.zeros(J, dtype=torch.int32), torch.zeros(J, dtype=torch.int32)
            ms.append(m)
        want = torch.stack([caller.val_sums_row(m, n) for m, n in zip(ms, ns)])
        assert want.dtype == torch.float64 and want.shape == (2, 1 + 3 * J) and want[0, 0] == 3 and not want[1].any() and want[0, 1:].any()
        got = i2r_dist.gather_val_sums(ms[rank], ns[rank])
        assert got.dtype == torch.float64 and torch.equal(got, want), (rank, got)
    finally:
        dist.destroy_process_group()


def test_gather_val_sums_world2_gloo():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_gloo_worker, args=(2, port, 14), nprocs=2, join=True)


def test_pose_table_bookkeeping():
    J = 3
    width = J * 3 + 2
    t = caller.PoseTable(J, "cpu", capacity=4)
    full = torch.arange(11 * width, dtype=torch.float32).reshape(11, width)
    ids = np.arange(100, 111)
    assert len(t) == 0 and t.rows().shape == (0, width) and t.image_ids().size == 0
    t.append(full[:3], ids[:3])
    first = t.buf
    t.append(full[:0], [])                                   # an empty append is a no-op
    assert len(t) == 3 and t.buf is first
    t.append(full[3:4], ids[3:4])                            # exactly full: no growth yet
    assert t.buf is first and t.buf.shape[0] == 4
    t.append(full[4:5], [int(ids[4])])                       # across the boundary: doubled, rows and ids kept
    assert t.buf.shape[0] == 8 and torch.equal(t.rows(), full[:5]) and t.image_ids().tolist() == ids[:5].tolist()
    t.append(full[5:], torch.as_tensor(ids[5:]))             # more than one doubling would give: 5 + 6 = 11 -> 16
    assert t.buf.shape[0] == 16 and len(t) == 11 and torch.equal(t.rows(), full) and t.image_ids().tolist() == ids.tolist()
    assert t.image_ids().dtype == np.int64 and t.rows().data_ptr() == t.buf.data_ptr(), "rows() is a view"
    with pytest.raises(AssertionError):
        t.append(full[:2, :-1], ids[:2])
    with pytest.raises(AssertionError):
        t.append(full[:2], ids[:3])
