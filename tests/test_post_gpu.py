"""-m gpu: flip-test merge and keypoint decode (the steps right after the forward in validate()) vs the CPU oracle: whole-model flip
tests, and the two kernels of csrc/i2r_post.hip directly through the C-ABI on the case table of tests/_post_cases.py."""
import numpy as np
import pytest
import torch

import _post_cases as pc
import i2r_cpu
import post_cpu
from _golden import setup
from i2r_amd import cabi, caller, config, models, synth

pytestmark = pytest.mark.gpu


def _peaky_heatmaps(S, J, h, w, seed):
    """Gaussian bumps (sigma 2, like the training targets) at random sub-pixel positions + low noise, some near borders."""
    u = synth.uniform01(seed, "bumps", S * J * 3).reshape(S, J, 3)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    hm = np.zeros((S, J, h, w), np.float32)
    for s in range(S):
        for j in range(J):
            cx, cy = u[s, j, 0] * (w - 1), u[s, j, 1] * (h - 1)
            hm[s, j] = (0.2 + 0.8 * u[s, j, 2]) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 2.0 ** 2))
    hm += 0.01 * synth.uniform01(seed, "noise", hm.size).reshape(hm.shape).astype(np.float32)
    hm[0, 0] = -1.0  # all-negative map: maxval <= 0 -> coords (0, 0), no refinement (inference.py:42-45)
    return hm


@pytest.mark.parametrize("h,w,J", [(64, 48, 14), (96, 72, 17)])
def test_decode_matches_oracle(h, w, J):
    S = 5
    hm = _peaky_heatmaps(S, J, h, w, 3)
    center = (synth.uniform01(1, "c", S * 2).reshape(S, 2) * 400 + 100).astype(np.float32)
    scale = (synth.uniform01(1, "s", S * 2).reshape(S, 2) * 1.5 + 0.5).astype(np.float32)
    ref_p, ref_m = post_cpu.get_final_preds(hm, center, scale, 11)
    got_p, got_m = caller.decode(torch.from_numpy(hm).cuda(), center, scale, 11)
    torch.cuda.synchronize()
    assert np.array_equal(got_m.cpu().numpy(), ref_m)
    err = np.abs(got_p.cpu().numpy() - ref_p).max()
    assert err < 2e-2, "decoded keypoints differ by %.4f px (input-image pixels)" % err  # float32 vs float64 log/Taylor
    # heat-map coordinates (no transform): tighter
    ref_p2, _ = post_cpu.get_final_preds(hm, None, None, 11, transform_back=False)
    got_p2, _ = caller.decode(torch.from_numpy(hm).cuda(), blur_kernel=11, transform_back=False)
    assert np.abs(got_p2.cpu().numpy() - ref_p2).max() < 5e-3


def test_flip_test_single_batched_forward_matches_two_oracle_forwards():
    cfg, sd, x, m, length, g = setup("w48_l213")
    net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    pairs = caller.FLIP_PAIRS["crowdpose"]
    got = net.forward_flip(x.cuda(), m.cuda(), length, pairs).cpu()
    ref = post_cpu.flip_test(lambda a, b, c: i2r_cpu.forward(sd, cfg, a, b, c), x, m, length, pairs)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() < 1e-3
    # and the plain forward is unaffected by the cached flip program
    plain = net(x.cuda(), m.cuda(), length).cpu()
    assert (plain - i2r_cpu.forward(sd, cfg, x, m, length)).abs().max().item() < 1e-3


@pytest.mark.parametrize("tag", ["bare_cv_l21", "w48_nh8_l21", "tph2s_up_fk3_l12", "bare_win_l213"])
def test_flip_test_of_variant_configs(tag):
    """the batched flip test on settings no shipped yaml uses: the concatenated cat_vec embedding (its kernel mirrors the mask itself),
    the multi-head general encoder (token groups doubled), UpConv + 3x3 heads"""
    cfg, sd, x, m, length, g = setup(tag)
    net = eval("models." + cfg.MODEL.NAME + ".get_pose_net")(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    pairs = caller.FLIP_PAIRS["crowdpose" if cfg.MODEL.NUM_JOINTS == 14 else "coco"]
    got = net.forward_flip(x.cuda(), m.cuda(), length, pairs).cpu()

    def multi(a, b, c):
        z = i2r_cpu.forward(sd, cfg, a, b, c)
        return z["multi"] if isinstance(z, dict) else z
    ref = post_cpu.flip_test(multi, x, m, length, pairs)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() < 1e-3 * max(1.0, ref.abs().max().item() / 8)


def test_flip_test_two_stage_dict_model():
    cfg, sd, x, m, length, g = setup("tph_l21")
    net = models.interformer.get_pose_net(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    pairs = caller.FLIP_PAIRS["crowdpose"]
    got = net.forward_flip(x.cuda(), m.cuda(), length, pairs).cpu()
    ref = post_cpu.flip_test(lambda a, b, c: i2r_cpu.forward(sd, cfg, a, b, c), x, m, length, pairs)
    assert (got - ref).abs().max().item() < 1e-3


# ------------------------------------------------------------------------------------------------------------------------------
# i2r_decode and i2r_flip_merge through the C-ABI, on the case table (tests/_post_cases.py; its conditions: tests/test_post_oracle.py)
# ------------------------------------------------------------------------------------------------------------------------------
GUARD = 64   # floats in front of and behind every output, which no launch may touch


def _guarded(n):
    """n NaN floats between two guards of 7.0 -> (whole buffer, device address of the payload)"""
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    buf[:GUARD] = 7.0
    buf[GUARD + n:] = 7.0
    return buf, buf.data_ptr() + 4 * GUARD


def _payload(buf, shape):
    a = buf.cpu().numpy()
    assert (a[:GUARD] == 7.0).all() and (a[len(a) - GUARD:] == 7.0).all(), "wrote outside the output"
    return a[GUARD:len(a) - GUARD].reshape(shape)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _decode_raw(c, transform_back):
    """i2r_decode on a case, outputs pre-filled with NaN -> (preds [S, J, 2], maxvals [S, J, 1]) numpy"""
    S, J, h, w = c.hm.shape
    hm = torch.tensor(c.hm).cuda()   # (a copy: the table's arrays are read-only)
    ce, sc = torch.tensor(c.center).cuda(), torch.tensor(c.scale).cuda()
    pb, pp = _guarded(S * J * 2)
    mb, mp = _guarded(S * J)
    cabi.check(cabi.lib().i2r_decode(hm.data_ptr(), ce.data_ptr() if transform_back else None, sc.data_ptr() if transform_back else None,
                                     pp, mp, S, J, h, w, c.ksize, int(transform_back), _stream()), "i2r_decode")
    torch.cuda.synchronize()
    return _payload(pb, (S, J, 2)), _payload(mb, (S, J, 1))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_decode_case_table(name):
    """every case of the table against the float64 oracle: maxvals and unrefined (integer) positions bit for bit, refined positions
    within the fp32-vs-float64 bound of test_decode_matches_oracle (5e-3 heat-map px), the same bound carried through the inverse crop
    transform; every output element written, none beside them"""
    c = pc.BY_NAME[name]
    ref_p, ref_m = pc.expected(name, False)
    got_p, got_m = _decode_raw(c, False)
    assert np.isfinite(got_p).all() and np.isfinite(got_m).all(), "%s: output elements left unwritten or not finite" % name
    assert np.array_equal(_bits(got_m), _bits(ref_m)), "%s: maxvals differ" % name
    integer = pc.integer_mask(name)
    assert np.array_equal(_bits(got_p[integer]), _bits(ref_p[integer])), "%s: integer peak positions differ:\n%s\n%s" % (
        name, got_p[integer], ref_p[integer])
    err = float(np.abs(got_p.astype(np.float64) - ref_p).max())
    ref_t, _ = pc.expected(name, True)
    got_t, got_mt = _decode_raw(c, True)
    assert np.isfinite(got_t).all() and np.array_equal(_bits(got_mt), _bits(ref_m)), name
    err_t, bar_t = float(np.abs(got_t.astype(np.float64) - ref_t).max()), pc.TOL * c.ratio()
    print("%s: worst |got - oracle| %.3e heat-map px (bar %.1e), %.3e image px (bar %.3e)" % (name, err, pc.TOL, err_t, bar_t))
    assert err < pc.TOL, "%s: worst error %.3e heat-map px, bar %.1e" % (name, err, pc.TOL)
    assert err_t < bar_t, "%s: worst error %.3e image px after the inverse crop transform, bar %.3e" % (name, err_t, bar_t)


def test_decode_with_the_config_default_blur_kernel():
    """TEST.BLUR_KERNEL of a config that does not set it is 3 (as in the reference's default.py): OpenCV's fixed {.25, .5, .25}, not
    the Gaussian formula"""
    k = config.default_config().TEST.BLUR_KERNEL
    c = pc.BY_NAME["skewed-64x48-k%d" % k]
    assert k == 3 and c.ksize == k
    got_p, got_m = caller.decode(torch.tensor(c.hm).cuda(), c.center.copy(), c.scale.copy(), k)
    ref_p, ref_m = pc.expected(c.name, True)
    err = float(np.abs(got_p.cpu().numpy().astype(np.float64) - ref_p).max())
    assert np.array_equal(got_m.cpu().numpy(), ref_m)
    assert err < pc.TOL * c.ratio(), "worst error %.3e image px, bar %.3e" % (err, pc.TOL * c.ratio())
    got_h, _ = caller.decode(torch.tensor(c.hm).cuda(), blur_kernel=k, transform_back=False)
    err_h = float(np.abs(got_h.cpu().numpy().astype(np.float64) - pc.expected(c.name, False)[0]).max())
    assert err_h < pc.TOL, "worst error %.3e heat-map px" % err_h


def test_decode_and_flip_merge_of_nothing_touch_nothing():
    L = cabi.lib()
    hm = torch.zeros(1, 2, 8, 6, device="cuda")
    pb, pp = _guarded(4)
    mb, mp = _guarded(2)
    assert L.i2r_decode(hm.data_ptr(), None, None, pp, mp, 0, 2, 8, 6, 11, 0, _stream()) == 0
    ob, op = _guarded(96)
    jm = torch.arange(2, dtype=torch.int32, device="cuda")
    assert L.i2r_flip_merge(hm.data_ptr(), hm.data_ptr(), jm.data_ptr(), op, 0, 2, 8, 6, _stream()) == 0
    torch.cuda.synchronize()
    assert np.isnan(_payload(pb, (4,))).all() and np.isnan(_payload(mb, (2,))).all() and np.isnan(_payload(ob, (96,))).all()


# what the host refuses before any launch (csrc/i2r_post.hip: every I2R_CHECK_ARG of the two entry points stands in front of the
# launch); the buffers are nevertheless as large as the call describes
_DECODE_OK = dict(n=1, joints=2, h=8, w=6, k=11, tb=1, center=True)
DECODE_REJECTED = {
    "even blur size": dict(k=4), "blur size 0": dict(k=0), "blur size 33": dict(k=33), "negative blur size": dict(k=-3),
    "w == 1": dict(w=1), "161 x 120": dict(h=161, w=120), "h == 0": dict(h=0), "h < 0": dict(h=-8), "joints == 0": dict(joints=0),
    "n == -1": dict(n=-1), "null center with transform_back": dict(center=False),
}


@pytest.mark.parametrize("what", sorted(DECODE_REJECTED))
def test_decode_rejects(what):
    a = dict(_DECODE_OK, **DECODE_REJECTED[what])
    size = max(1, abs(a["n"]) * max(1, a["joints"]) * max(1, abs(a["h"])) * max(1, a["w"]))
    hm = torch.zeros(size, device="cuda")
    ce = torch.full((2,), 100.0, device="cuda")
    pb, pp = _guarded(4)
    mb, mp = _guarded(2)
    L = cabi.lib()
    rc = L.i2r_decode(hm.data_ptr(), ce.data_ptr() if a["center"] else None, ce.data_ptr(), pp, mp, a["n"], a["joints"], a["h"], a["w"],
                      a["k"], a["tb"], _stream())
    assert rc < 0 and (L.i2r_last_error() or b"") != b"", what
    torch.cuda.synchronize()
    assert np.isnan(_payload(pb, (4,))).all() and np.isnan(_payload(mb, (2,))).all()


FLIP_REJECTED = {"joints == 0": dict(joints=0), "h == 0": dict(h=0), "w == 0": dict(w=0), "w < 0": dict(w=-7), "n == -1": dict(n=-1),
                 "null y": dict(null="y"), "null y_flipped": dict(null="yf"), "null joint map": dict(null="jm"), "null out": dict(null="out")}


@pytest.mark.parametrize("what", sorted(FLIP_REJECTED))
def test_flip_merge_rejects(what):
    a = dict(dict(n=1, joints=2, h=9, w=7, null=None), **FLIP_REJECTED[what])
    y = torch.zeros(2 * 9 * 7, device="cuda")
    jm = torch.arange(2, dtype=torch.int32, device="cuda")
    ob, op = _guarded(2 * 9 * 7)
    ptr = {"y": y.data_ptr(), "yf": y.data_ptr(), "jm": jm.data_ptr(), "out": op}
    if a["null"]:
        ptr[a["null"]] = None
    L = cabi.lib()
    rc = L.i2r_flip_merge(ptr["y"], ptr["yf"], ptr["jm"], ptr["out"], a["n"], a["joints"], a["h"], a["w"], _stream())
    assert rc < 0 and (L.i2r_last_error() or b"") != b"", what
    torch.cuda.synchronize()
    assert np.isnan(_payload(ob, (2 * 9 * 7,))).all()


FLIP_CASES = {  # name -> (joints, flip pairs, (n, h, w), out aliases y, y_flipped is the second half of y's allocation)
    "crowdpose-3x9x7": (14, caller.FLIP_PAIRS["crowdpose"], (3, 9, 7), False, False),        # 2646 elements: no multiple of 256
    "coco-1x64x48": (17, caller.FLIP_PAIRS["coco"], (1, 64, 48), False, False),
    "identity-2x5x1": (5, [], (2, 5, 1), False, False),
    "coco-2x5x1": (17, caller.FLIP_PAIRS["coco"], (2, 5, 1), False, False),
    "crowdpose-1x64x48-in-place": (14, caller.FLIP_PAIRS["crowdpose"], (1, 64, 48), True, False),
    "coco-3x9x7-in-place": (17, caller.FLIP_PAIRS["coco"], (3, 9, 7), True, True),
    "crowdpose-3x9x7-one-allocation": (14, caller.FLIP_PAIRS["crowdpose"], (3, 9, 7), False, True),
}


@pytest.mark.parametrize("name", sorted(FLIP_CASES))
def test_flip_merge_bit_equal(name):
    """i2r_flip_merge itself: bit-equal to (y + flip_back(y_flipped)) * 0.5 in fp32 -- one add and one exact halving per element"""
    J, pairs, (n, h, w), in_place, one_alloc = FLIP_CASES[name]
    both = ((synth.uniform01(5, "flip/" + name, 2 * n * J * h * w) * 4.0 - 2.0).astype(np.float32)).reshape(2 * n, J, h, w)
    y, yf = both[:n], both[n:]
    ref = (y + post_cpu.flip_back(yf, pairs)) * np.float32(0.5)
    assert ref.dtype == np.float32
    jm = caller.joint_map(pairs, J).cuda()
    tot = n * J * h * w
    if one_alloc:   # as the engine's batched flip forward hands them over: one tensor, the mirrored half behind the plain one
        dev = torch.from_numpy(both).cuda()
        dy, dyf = dev[:n], dev[n:]
    else:
        dy, dyf = torch.from_numpy(y.copy()).cuda(), torch.from_numpy(yf.copy()).cuda()
    ob, op = _guarded(tot)
    out_ptr = dy.data_ptr() if in_place else op   # (every element reads only its own y[i]: out may be y)
    cabi.check(cabi.lib().i2r_flip_merge(dy.data_ptr(), dyf.data_ptr(), jm.data_ptr(), out_ptr, n, J, h, w, _stream()), "i2r_flip_merge")
    torch.cuda.synchronize()
    if in_place:
        got = dy.cpu().numpy()
        assert np.isnan(_payload(ob, (tot,))).all()
        assert np.array_equal(dyf.cpu().numpy(), yf)
    else:
        got = _payload(ob, (n, J, h, w))
        assert np.array_equal(dy.cpu().numpy(), y) and np.array_equal(dyf.cpu().numpy(), yf)
    assert np.array_equal(_bits(got), _bits(ref)), "%s: %d of %d elements differ" % (name, (_bits(got) != _bits(ref)).sum(), tot)
