"""Caller-side pieces of the reference's validate() loop that sit right after the forward (SURVEY.md section 8 a-caller, 8f):
flip-test merge and heatmap -> keypoint decode, both on the device through the C-ABI (no heatmap D2H, no Python loop).

    out   = model.forward_flip(x, pos_mask, length, FLIP_PAIRS['crowdpose'])      # function.py:135-162
    preds, maxvals = decode(out, center, scale, cfg.TEST.BLUR_KERNEL)              # function.py:190 -> inference.py:90

and of what every dataset class does with the key points before it writes a result (lib/dataset/coco.py:377-412, lib/nms/nms.py:75-181):
per-person rescoring and per-image OKS-NMS / soft-OKS-NMS, one device kernel, no host synchronisation:

    nms   = rescore_nms_cfg(cfg, preds, maxvals, scale, box_score, length)         # coco.py:384-412
    rows  = results(preds, maxvals, nms, length, image_ids, center, scale)         # the one copy to the host
"""
import ctypes

import torch

from . import cabi

# left/right joint pairs (reference lib/dataset/crowdpose.py:98-99, coco.py:100-101, ochuman.py:95)
FLIP_PAIRS = {
    "crowdpose": [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11]],
    "coco": [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]],
    "ochuman": [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]],
}


def joint_map(flip_pairs, num_joints):
    """int32 [J]: source channel of the mirrored heatmap for every output joint (flip_back, utils/transforms.py:24-28)."""
    m = list(range(num_joints))
    for a, b in flip_pairs:
        m[a], m[b] = b, a
    return torch.tensor(m, dtype=torch.int32)


def decode(heatmaps, center=None, scale=None, blur_kernel=11, transform_back=True):
    """get_final_preds (lib/core/inference.py:90-112) on the device.
    heatmaps [S, J, h, w] fp32 cuda; center / scale [S, 2] (numpy or tensor) -> (preds [S, J, 2], maxvals [S, J, 1]) cuda."""
    assert heatmaps.is_cuda and heatmaps.dtype == torch.float32 and heatmaps.dim() == 4
    hm = heatmaps.contiguous()
    S, J, h, w = hm.shape
    dev = hm.device
    preds = torch.empty(S, J, 2, dtype=torch.float32, device=dev)
    maxvals = torch.empty(S, J, 1, dtype=torch.float32, device=dev)
    if S == 0:  # (a data-parallel rank without images: nothing to decode)
        return preds, maxvals
    c = s = None
    if transform_back:
        c = torch.as_tensor(center, dtype=torch.float32).to(dev).contiguous()
        s = torch.as_tensor(scale, dtype=torch.float32).to(dev).contiguous()
        assert c.shape == (S, 2) and s.shape == (S, 2)
    st = torch.cuda.current_stream(dev).cuda_stream
    cabi.check(cabi.lib().i2r_decode(hm.data_ptr(), c.data_ptr() if c is not None else None,
                                     s.data_ptr() if s is not None else None, preds.data_ptr(), maxvals.data_ptr(),
                                     S, J, h, w, int(blur_kernel), int(bool(transform_back)), st), "i2r_decode")
    return preds, maxvals


# per-joint OKS sigmas (reference lib/nms/nms.py:79-81), keyed by joint count: 17 = COCO / OCHuman, 14 = CrowdPose
SIGMAS = {
    17: tuple(v / 10.0 for v in (.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89)),
    14: tuple(v / 10.0 for v in (.79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89, .62, .79)),
}
MAX_DETS = 20             # soft_oks_nms keeps at most 20 persons per image (nms.py:161)
NMS_MAX_PERSONS = 1024    # i2r_pose_nms: persons of one image
_SIGMAS_DEV = {}


class PoseNms:
    """What i2r_pose_nms writes, device tensors of fixed size: score [S] fp32 (the rescored value), rank [S] int32 (position of the crop
    in the `keep` list of its image, -1 = suppressed or beyond max_dets), n_keep [n_img] int32."""
    __slots__ = ("score", "rank", "n_keep")

    def __init__(self, score, rank, n_keep):
        self.score, self.rank, self.n_keep = score, rank, n_keep


def rescore_nms(preds, maxvals, scale_or_area, box_score, length, in_vis_thre, oks_thre, soft=False, sigmas=None, oks_vis_thre=None,
                max_dets=MAX_DETS, max_persons=None):
    """Rescoring (coco.py:384-396) + OKS-NMS (nms.py:101-128) or, soft=True, soft-OKS-NMS (nms.py:142-181) of every image of the batch,
    on the current stream, without a host synchronisation or a device-to-host copy.
    preds [S, J, 2], maxvals [S, J, 1] as decode() returns them; scale_or_area: [S, 2] (area = prod(scale * 200), function.py:220) or
    [S]; box_score [S]; length: persons per image, a list (a host-to-device copy of its prefix sums is queued) or an int tensor (prefix
    sums on its device; then max_persons, a host-side bound of the persons of one image, defaults to min(S, 1024)).
    oks_vis_thre: the in_vis_thre ARGUMENT of oks_nms, which the dataset classes never pass (None = all joints count).  -> PoseNms."""
    assert preds.is_cuda and preds.dtype == torch.float32 and preds.dim() == 3 and preds.shape[2] == 2
    dev = preds.device
    S, J = preds.shape[0], preds.shape[1]

    def f32(t, shape):
        t = torch.as_tensor(t, dtype=torch.float32).to(dev, non_blocking=True).contiguous()
        assert tuple(t.shape) == shape, (tuple(t.shape), shape)
        return t
    preds = preds.contiguous()
    maxvals = f32(maxvals.reshape(S, J), (S, J))
    sa = torch.as_tensor(scale_or_area, dtype=torch.float32)
    sa = f32(sa, (S, 2) if sa.dim() == 2 else (S,))
    box_score = f32(box_score, (S,))
    if sigmas is None:
        if J not in SIGMAS:
            raise cabi.I2RError("rescore_nms: no sigma table for %d joints -- pass sigmas" % J)
        if (J, dev) not in _SIGMAS_DEV:   # (uploaded once per device)
            # a blocking copy: the table is there when this returns, whichever stream a later call runs on
            _SIGMAS_DEV[(J, dev)] = torch.tensor(SIGMAS[J], dtype=torch.float32).to(dev)
        sigmas = _SIGMAS_DEV[(J, dev)]
    else:
        sigmas = f32(sigmas, (J,))
    if torch.is_tensor(length):
        n_img = int(length.shape[0])
        off = torch.zeros(n_img + 1, dtype=torch.int32, device=dev)
        off[1:] = torch.cumsum(length.to(dev, non_blocking=True), 0)
        bound = min(S, NMS_MAX_PERSONS) if max_persons is None else int(max_persons)
    else:
        length = [int(v) for v in length]
        n_img = len(length)
        assert sum(length) == S, (sum(length), S)
        prefix = [0]
        for v in length:
            prefix.append(prefix[-1] + v)
        off = torch.tensor(prefix, dtype=torch.int32).to(dev, non_blocking=True)
        bound = max(length + [0]) if max_persons is None else int(max_persons)
    score = torch.empty(S, dtype=torch.float32, device=dev)
    rank = torch.empty(S, dtype=torch.int32, device=dev)
    n_keep = torch.zeros(n_img, dtype=torch.int32, device=dev)   # (a batch without any crop launches nothing: its images keep 0)
    a = cabi.PoseNmsArgs(preds=preds.data_ptr(), maxvals=maxvals.data_ptr(), scale=sa.data_ptr() if sa.dim() == 2 else None,
                         area=sa.data_ptr() if sa.dim() == 1 else None, box_score=box_score.data_ptr(), img_off=off.data_ptr(),
                         sigmas=sigmas.data_ptr(), score=score.data_ptr(), rank=rank.data_ptr(), n_keep=n_keep.data_ptr(),
                         in_vis_thre=float(in_vis_thre), oks_thre=float(oks_thre), oks_vis_thre=float(oks_vis_thre or 0.0),
                         n_crops=S, n_img=n_img, joints=J, max_persons=bound, soft=int(bool(soft)), max_dets=int(max_dets),
                         use_oks_vis=int(oks_vis_thre is not None))
    cabi.check(cabi.lib().i2r_pose_nms(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream), "i2r_pose_nms")
    return PoseNms(score, rank, n_keep)


def rescore_nms_cfg(cfg, preds, maxvals, scale_or_area, box_score, length, **kw):
    """rescore_nms with the thresholds of a config: TEST.IN_VIS_THRE, TEST.OKS_THRE, TEST.SOFT_NMS and the sigma table of MODEL.NUM_JOINTS
    (what COCODataset / CrowdPoseDataset / OCHumanDataset .evaluate() read from it)."""
    assert preds.shape[1] == cfg.MODEL.NUM_JOINTS, (tuple(preds.shape), cfg.MODEL.NUM_JOINTS)
    return rescore_nms(preds, maxvals, scale_or_area, box_score, length, cfg.TEST.IN_VIS_THRE, cfg.TEST.OKS_THRE, soft=cfg.TEST.SOFT_NMS, **kw)


def results(preds, maxvals, nms, length, image_ids, center, scale):
    """The host-visible end: ONE copy to the host (key points, score and rank packed into one tensor), then per image the kept persons
    in `keep` order as rows shaped like _coco_keypoint_results_one_category_kernel's (coco.py:452-485) without the category:
    image_id, keypoints [x, y, v] * J flattened, score, center, scale.  length / image_ids: per image; center / scale: [S, 2] per crop.
    As in evaluate(), an image whose `keep` is empty (it has no persons) contributes nothing.  Writes no file.  -> list of per-image lists."""
    S, J = preds.shape[0], preds.shape[1]
    packed = torch.cat([preds.reshape(S, J * 2), maxvals.reshape(S, J), nms.score.reshape(S, 1).to(preds.dtype),
                        nms.rank.reshape(S, 1).to(preds.dtype)], 1).cpu().numpy()   # (rank < 2^24: exact in fp32)
    center = torch.as_tensor(center).reshape(S, 2).tolist()
    scale = torch.as_tensor(scale).reshape(S, 2).tolist()
    length = [int(v) for v in length]
    assert sum(length) == S and len(image_ids) == len(length)
    out, o = [], 0
    for img, n in zip(image_ids, length):
        kept = sorted((int(packed[o + p, J * 3 + 1]), o + p) for p in range(n) if packed[o + p, J * 3 + 1] >= 0)
        rows = []
        for _, s in kept:
            kp = [float(v) for j in range(J) for v in (packed[s, 2 * j], packed[s, 2 * j + 1], packed[s, 2 * J + j])]
            rows.append(dict(image_id=img, keypoints=kp, score=float(packed[s, J * 3]), center=center[s], scale=scale[s]))
        out.append(rows)
        o += n
    return out
