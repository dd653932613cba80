"""CPU: the surface of the attention per person -- the C-ABI declaration of i2r_attn_person_maps and its op kind, the identities of the
float64 reference (tests/_attn_person_ref.py), and the ValueErrors of net.person_relations that need no engine."""
import ctypes
import os
import re

import pytest
import torch

from _attn_person_ref import as_maps, full_map, reduce_persons
from i2r_amd import cabi, config, models
from i2r_amd.engine import PersonMaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_attn_person_maps_and_op_kind():
    header = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert re.search(r"^I2R_API int i2r_attn_person_maps\(const i2r_attn_person_args\* a, void\* stream\);", header, flags=re.M)
    assert re.search(r"I2R_OP_ATTN_PERSON = 32\b", header) and cabi.CAPTURE_OP_ATTN_PERSON == 32
    assert int(re.search(r"#define I2R_ABI_VERSION (\d+)", header).group(1)) == cabi.ABI_VERSION == 17
    assert "i2r_attn_person_maps" in cabi.EXPORTS
    fields = re.search(r"typedef struct i2r_attn_person_args \{(.*?)\} i2r_attn_person_args;", header, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == [f for f, _ in cabi.AttnPersonArgs._fields_]
    n_ptr = sum(1 for _, t in cabi.AttnPersonArgs._fields_ if t is cabi._fp)
    assert n_ptr == 9 and names[:n_ptr] == [f for f, t in cabi.AttnPersonArgs._fields_ if t is cabi._fp]  # pointers first: no padding holes
    assert all(t is cabi._i32 for _, t in cabi.AttnPersonArgs._fields_[n_ptr:])
    assert ctypes.sizeof(cabi.AttnPersonArgs) == 8 * n_ptr + 4 * (len(names) - n_ptr) == 120  # the header's struct: 9 pointers, 12 int32
    api = open(os.path.join(ROOT, "intra-and-inter-human-relation-network-for-mpee_amd", "csrc", "i2r_api.hip")).read()
    assert re.search(r"case I2R_OP_ATTN_PERSON: rc = i2r_attn_person_maps\(", api)  # (one runner serves i2r_run_program and _timed)


def test_built_library_exports_attn_person_maps():
    L = cabi.load_library()
    assert L.i2r_abi_version() == 17
    assert L.i2r_attn_person_maps.argtypes[0]._type_ is cabi.AttnPersonArgs
    assert L.i2r_attn_person_maps(None, None) == -1 and b"null pointer" in L.i2r_last_error()  # (rejected on the host: no GPU needed)


@pytest.mark.parametrize("T", [1, 12, 192])
def test_reference_identities(T):
    g = torch.Generator().manual_seed(T)
    for P, heads, hp in ((1, 1, 16), (3, 2, 16), (5, 1, 32)):
        L = P * T
        qk = torch.randn(L, 2 * heads * hp + 8, generator=g, dtype=torch.float64)
        full = full_map(qk, heads, hp, heads * hp + 8)
        assert (full.sum(1) - 1).abs().max().item() < 1e-12
        D, F, R, R2 = reduce_persons(full, T)
        assert D.shape == F.shape == (P, L) and R.shape == R2.shape == (P, P)
        assert (D.sum(1) - 1).abs().max().item() < 1e-12 and (R.sum(1) - 1).abs().max().item() < 1e-12
        assert (F.sum(0) - 1).abs().max().item() < 1e-12
        assert (R - R2).abs().max().item() < 1e-12
        # against the definitions, entry by entry
        i, j = P - 1, 0
        assert abs(R[i, j].item() - full[i * T:(i + 1) * T, j * T:(j + 1) * T].sum().item() / T) < 1e-12
        assert abs(D[i, L - 1].item() - full[i * T:(i + 1) * T, L - 1].mean().item()) < 1e-12
        assert abs(F[j, L - 1].item() - full[L - 1, j * T:(j + 1) * T].sum().item()) < 1e-12
        if P == 1:
            assert abs(R.item() - 1) < 1e-12


def test_reference_maps_layout_and_interpolate():
    g = torch.Generator().manual_seed(5)
    P, h, w = 2, 3, 4
    rows = torch.rand(P, P * h * w, generator=g, dtype=torch.float64)
    m = as_maps(rows, h, w)
    assert m.shape == (P, P, h, w) and torch.equal(m[1, 0].reshape(-1), rows[1, :h * w]) and torch.equal(m[0, 1].reshape(-1), rows[0, h * w:])
    up = as_maps(rows, h, w, 2)
    assert up.shape == (P, P, 6, 8) and up.dtype == torch.float64
    assert abs(up[1, 1, 0, 0].item() - m[1, 1, 0, 0].item()) < 1e-12  # (align_corners=False: the corner sample is the corner value)
    assert abs(up[1, 1, 1, 1].item() - (0.75 * (0.75 * m[1, 1, 0, 0] + 0.25 * m[1, 1, 0, 1]) + 0.25 * (0.75 * m[1, 1, 1, 0] + 0.25 * m[1, 1, 1, 1])).item()) < 1e-12


def test_person_maps_modes():
    assert (PersonMaps().mode, PersonMaps("dependency").mode, PersonMaps("affect", 4).mode, PersonMaps("affect", 4).upsample) == (0, 1, 2, 4)
    for bad in ("rows", 3, True):
        with pytest.raises(ValueError):
            PersonMaps(bad)
    with pytest.raises(ValueError):
        PersonMaps("affect", 0)


def test_person_relations_raises_without_an_inter_human_stack():
    x, m = torch.zeros(1, 3, 256, 192), torch.zeros(1, 1, 256, 192)
    cfg = config.load_config("tph_192_p6_b4")
    with pytest.raises(ValueError, match="no inter-human stack"):
        models.transpose_h.get_pose_net(cfg, is_train=False).person_relations(x, m, [1])
    with pytest.raises(ValueError, match="no inter-human stack"):
        models.hrformer.get_pose_net(config.load_config("hrt_192_p4_b4"), is_train=False).person_relations(x, m, [1])
    win = config.load_config("tph_192_p6_b4", ["MODEL.ATTENTION_TYPE", "window", "MODEL.N_HEAD", 4])
    with pytest.raises(ValueError, match="ATTENTION_TYPE"):
        models.interformer.get_pose_net(win, is_train=False).person_relations(x, m, [1])
    net = models.interformer.get_pose_net(cfg, is_train=False)
    with pytest.raises(ValueError, match="maps"):
        net.person_relations(x, m, [1], maps="rows")
