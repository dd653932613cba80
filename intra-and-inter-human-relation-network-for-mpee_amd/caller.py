"""Caller-side pieces of the reference's validate() loop that sit right after the forward (SURVEY.md section 8 a-caller, 8f):
flip-test merge and heatmap -> keypoint decode, both on the device through the C-ABI (no heatmap D2H, no Python loop).

    out   = model.forward_flip(x, pos_mask, length, FLIP_PAIRS['crowdpose'])      # function.py:135-162
    preds, maxvals = decode(out, center, scale, cfg.TEST.BLUR_KERNEL)              # function.py:190 -> inference.py:90

and of what every dataset class does with the key points before it writes a result (lib/dataset/coco.py:377-412, lib/nms/nms.py:75-181):
per-person rescoring and per-image OKS-NMS / soft-OKS-NMS, one device kernel, no host synchronisation:

    nms   = rescore_nms_cfg(cfg, preds, maxvals, scale, box_score, length)         # coco.py:384-412
    rows  = results(preds, maxvals, nms, length, image_ids, center, scale)         # the one copy to the host

and of the two numbers validate() logs per batch (function.py:167-174: JointsMSELoss, lib/core/loss.py:15-41, and the PCK accuracy,
lib/core/evaluate.py:41-71), from the joint positions alone -- the target heat maps are never stored, nothing is copied to the host:

    meter = ValMeter(device)                                                       # the two AverageMeters, once per epoch
    jhm   = heatmap_joints(joints, center, scale, cfg.MODEL.HEATMAP_SIZE)          # JointsDataset.py:295-320 (host, float64)
    m     = val_metrics_cfg(cfg, out, joints_hm=jhm, joints_vis=vis, meter=meter)  # function.py:167-174; m.pred = accuracy's pred
    valid_loss, valid_acc = meter.result()                                         # end of the epoch: the one copy to the host

and of both across the ranks of a data-parallel run: the raw sums of every rank's batch combined into the numbers of the whole batch
(val_sums_row / val_combine; dist.val_metrics_all is the gather in front of them), and the rows of dist.gather_poses collected over the
steps of an epoch on the device for one oks_eval at its end (PoseTable).

and of the one training step the project serves, the re-fit of final_layer on frozen features (the criterion + backward of train(),
function.py:30, restricted to that layer): the loss and its gradient in one fused kernel, the optimizer step in torch:

    hi   = model.head_input(x, pos_mask, length)                                   # the tensor final_layer reads, copied out
    fit  = HeadFit.from_model(model)                                               # or HeadFit(hi.cin, new_joint_count, cfg=cfg)
    loss = fit.step(hi.feat, joints_hm=jhm, joints_vis=vis)                        # head_grad + optimizer.step(), no host copy

and of the closed form of that re-fit: the normal equations of the loss in the layer's weight and bias, collected in one pass per batch
and solved per joint at the end -- the exact minimiser after one epoch:

    acc  = HeadSolve(hi.cin, new_joint_count, cfg=cfg)                             # float64 state on the device
    acc.add(hi.feat, joints_hm=jhm, joints_vis=vis)                                # i2r_head_normal, once per batch, no host copy
    fit  = acc.head_fit()                                                          # a HeadFit at the solution: commit(), state(), step()
"""
import collections
import ctypes

import numpy as np
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


# LOSS.USE_DIFFERENT_JOINTS_WEIGHT tables of the dataset classes (reference lib/dataset/coco.py:106-112, crowdpose.py:104-110,
# ochuman.py:101-107), keyed like FLIP_PAIRS
JOINTS_WEIGHT = {
    "coco": (1., 1., 1., 1., 1., 1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1., 1.2, 1.2, 1.5, 1.5),
    "crowdpose": (1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1.),
    "ochuman": (1., 1., 1., 1., 1., 1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1., 1.2, 1.2, 1.5, 1.5),
}


def heatmap_joints(joints, center, scale, heatmap_size):
    """Image-space joints -> heat-map coordinates, the reference's joints_heatmap (JointsDataset.py:295-320 at rot 0): host, float64.
    joints [S, J, 2 or 3] (x, y first), center / scale [S, 2], heatmap_size (w, h) -> float64 numpy [S, J, 2].  cv2-unpinned like the
    rest of the input side: the transform is input.affine_transforms, not cv2.getAffineTransform.  The validation half only; training
    samples (rotation, rescaling, flip, half-body box) get their joints_hm from input.train_inputs_batch."""
    from . import input as i2r_input
    j = np.asarray(joints, dtype=np.float64)
    S = j.shape[0]
    t = i2r_input.affine_transforms(center, scale, heatmap_size)                    # [S, 2, 3]
    pt = np.concatenate([j[:, :, :2], np.ones((S, j.shape[1], 1))], 2)              # affine_transform: t . (x, y, 1)
    return np.matmul(t[:, None], pt[..., None])[..., 0]


def _dev(t, dtype, dev, shape):
    t = torch.as_tensor(t, dtype=dtype).to(dev, non_blocking=True).contiguous()
    assert tuple(t.shape) == shape, (tuple(t.shape), shape)
    return t


def _joint_inputs(joints_hm, joints_vis, joints_weight, dev):
    hm = torch.as_tensor(joints_hm)
    assert hm.dtype == torch.float64 and hm.dim() == 3 and hm.shape[2] == 2, "joints_hm: float64 [S, J, 2] (heatmap_joints)"
    S, J = hm.shape[0], hm.shape[1]
    hm = hm.to(dev, non_blocking=True).contiguous()
    vis = torch.as_tensor(joints_vis, dtype=torch.float32)
    if vis.dim() == 3:                     # the reference's [S, J, 3] array: column 0
        vis = vis[:, :, 0]
    vis = _dev(vis, torch.float32, dev, (S, J))
    jw = _dev(joints_weight, torch.float32, dev, (J,)) if joints_weight is not None else None
    return hm, vis, jw


def joint_targets(joints_hm, joints_vis, heatmap_size, sigma=2, joints_weight=None, want_target=True, device=None):
    """generate_target (JointsDataset.py:394-450) for every crop on the device.  joints_hm float64 [S, J, 2] (heatmap_joints), joints_vis
    [S, J] (or the reference's [S, J, 3]), heatmap_size (w, h) -> (target [S, J, h, w] fp32 | None, target_weight [S, J] fp32)."""
    dev = torch.device(device) if device is not None else (joints_hm.device if torch.is_tensor(joints_hm) and joints_hm.is_cuda
                                                          else torch.device("cuda", torch.cuda.current_device()))
    hm, vis, jw = _joint_inputs(joints_hm, joints_vis, joints_weight, dev)
    S, J = hm.shape[0], hm.shape[1]
    w, h = int(heatmap_size[0]), int(heatmap_size[1])
    tw = torch.empty(S, J, dtype=torch.float32, device=dev)
    target = torch.empty(S, J, h, w, dtype=torch.float32, device=dev) if want_target else None
    if S == 0:
        return target, tw
    a = cabi.JointTargetsArgs(joints_hm=hm.data_ptr(), joints_vis=vis.data_ptr(), joints_weight=jw.data_ptr() if jw is not None else None,
                              target_weight=tw.data_ptr(), target=target.data_ptr() if want_target else None, sigma=float(sigma),
                              n_crops=S, joints=J, h=h, w=w)
    with torch.cuda.device(dev):
        cabi.check(cabi.lib().i2r_joint_targets(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream), "i2r_joint_targets")
    return target, tw


class ValMetrics:
    """What i2r_val_metrics writes, device tensors: loss [1], acc [J + 1], avg_acc [1] float64; cnt [1] int32; pred [S, J, 2] fp32
    (accuracy's fourth return value); sse [J] float64, hits [J], valid [J] int32 (raw sums: shards can be combined exactly, see
    val_combine).  n_crops int32 [1], the total crop count, is set by val_combine alone (val_metrics' caller knows S; there it stays
    unset), and val_combine's pred is None: the arg-max coordinates stay with the rank that computed them."""
    __slots__ = ("loss", "acc", "avg_acc", "cnt", "pred", "sse", "hits", "valid", "n_crops")


class ValMeter:
    """validate()'s two AverageMeters (losses, acc; function.py:168-174) as four doubles on the device: sum of loss * S, sum of S, sum of
    avg_acc * cnt, sum of cnt.  val_metrics(..., meter=) adds to it in stream order; result() is the one copy to the host."""

    def __init__(self, device):
        self.buf = torch.zeros(4, dtype=torch.float64, device=device)

    def reset(self):
        self.buf.zero_()

    def result(self):
        """-> (losses.avg, acc.avg); a meter that saw no sample / no counted joint gives 0 for it, as AverageMeter does"""
        ls, ln, as_, an = self.buf.cpu().tolist()
        return (ls / ln if ln != 0 else 0.0), (as_ / an if an != 0 else 0.0)


def val_metrics(output, target=None, target_weight=None, *, joints_hm=None, joints_vis=None, sigma=2, joints_weight=None,
                use_target_weight=True, meter=None):
    """JointsMSELoss + accuracy of one batch (function.py:167-172) on the current stream, without a host synchronisation.
    output [S, J, h, w] fp32 cuda, plus ONE target form: the data loader's tensors (target [S, J, h, w], target_weight [S, J] or
    [S, J, 1]), or the joints themselves (joints_hm float64 [S, J, 2], joints_vis, sigma, joints_weight as joint_targets takes them): the
    target is then evaluated inside the kernel.  meter: a ValMeter to update.  -> ValMetrics."""
    assert output.is_cuda and output.dtype == torch.float32 and output.dim() == 4
    if (target is None) == (joints_hm is None):
        raise cabi.I2RError("val_metrics: give either target (+ target_weight) or joints_hm (+ joints_vis)")
    out = output.contiguous()
    S, J, h, w = out.shape
    dev = out.device
    r = ValMetrics()
    f64 = torch.zeros(J + 1 + 1 + 1 + J, dtype=torch.float64, device=dev)    # (a batch without crops launches nothing: all 0)
    i32 = torch.zeros(1 + 2 * J, dtype=torch.int32, device=dev)
    r.acc, r.avg_acc, r.loss, r.sse = f64[:J + 1], f64[J + 1:J + 2], f64[J + 2:J + 3], f64[J + 3:]
    r.cnt, r.hits, r.valid = i32[:1], i32[1:1 + J], i32[1 + J:]
    r.pred = torch.empty(S, J, 2, dtype=torch.float32, device=dev)
    ws = torch.empty(2 * S * J, dtype=torch.float64, device=dev)              # 16 bytes per map
    a = cabi.ValMetricsArgs(output=out.data_ptr(), ws=ws.data_ptr(), loss=r.loss.data_ptr(), acc=r.acc.data_ptr(), avg_acc=r.avg_acc.data_ptr(),
                            cnt=r.cnt.data_ptr(), pred=r.pred.data_ptr(), sse=r.sse.data_ptr(), hits=r.hits.data_ptr(), valid=r.valid.data_ptr(),
                            meter=meter.buf.data_ptr() if meter is not None else None, sigma=float(sigma), n_crops=S, joints=J, h=h, w=w,
                            use_target_weight=int(bool(use_target_weight)))
    if target is not None:
        assert target.is_cuda and target.dtype == torch.float32 and tuple(target.shape) == (S, J, h, w), tuple(target.shape)
        keep = [target.contiguous()]
        a.target = keep[0].data_ptr()
        if target_weight is not None:
            keep.append(_dev(torch.as_tensor(target_weight).reshape(S, J), torch.float32, dev, (S, J)))
            a.target_weight = keep[1].data_ptr()
        elif use_target_weight:
            raise cabi.I2RError("val_metrics: use_target_weight without target_weight")
    else:
        keep = _joint_inputs(joints_hm, joints_vis, joints_weight, dev)
        assert tuple(keep[0].shape) == (S, J, 2), (tuple(keep[0].shape), (S, J))
        a.joints_hm, a.joints_vis = keep[0].data_ptr(), keep[1].data_ptr()
        a.joints_weight = keep[2].data_ptr() if keep[2] is not None else None
    if meter is not None:
        assert meter.buf.device == dev
    if S == 0:  # (a data-parallel rank without images: nothing is launched, the results stay 0, the meter untouched)
        return r
    with torch.cuda.device(dev):
        cabi.check(cabi.lib().i2r_val_metrics(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream), "i2r_val_metrics")
    return r


def val_metrics_cfg(cfg, output, target=None, target_weight=None, **kw):
    """val_metrics with what the reference's criterion and dataset class read from a config: LOSS.USE_TARGET_WEIGHT,
    LOSS.USE_DIFFERENT_JOINTS_WEIGHT (the JOINTS_WEIGHT table of DATASET.DATASET), MODEL.SIGMA, MODEL.HEATMAP_SIZE.
    LOSS.USE_OHKM raises: the reference's JointsOHKMMSELoss.forward takes no `length` and cannot run under validate() either."""
    if cfg.LOSS.USE_OHKM:
        raise cabi.I2RError("val_metrics_cfg: LOSS.USE_OHKM -- the reference's OHKM loss does not run under validate(); not provided")
    w, h = int(cfg.MODEL.HEATMAP_SIZE[0]), int(cfg.MODEL.HEATMAP_SIZE[1])
    assert tuple(output.shape[1:]) == (cfg.MODEL.NUM_JOINTS, h, w), (tuple(output.shape), cfg.MODEL.NUM_JOINTS, h, w)
    if target is None and cfg.LOSS.USE_DIFFERENT_JOINTS_WEIGHT and "joints_weight" not in kw:
        if cfg.DATASET.DATASET not in JOINTS_WEIGHT:
            raise cabi.I2RError("val_metrics_cfg: no joints_weight table for dataset %r -- pass joints_weight" % cfg.DATASET.DATASET)
        kw["joints_weight"] = JOINTS_WEIGHT[cfg.DATASET.DATASET]
    return val_metrics(output, target, target_weight, sigma=cfg.MODEL.SIGMA, use_target_weight=cfg.LOSS.USE_TARGET_WEIGHT, **kw)


def val_sums_row(m, n_crops):
    """What one rank contributes to the all-gather in front of val_combine: float64 [1 + 3 J] = n_crops, sse[J], hits[J], valid[J] on
    m's device (the integers as doubles: exact below 2^53).  n_crops is the host's number (output.shape[0]); a rank without images passes
    the all-zero ValMetrics val_metrics returned and 0.  No host synchronisation."""
    n = torch.full((1,), float(int(n_crops)), dtype=torch.float64, device=m.sse.device)
    return torch.cat([n, m.sse.to(torch.float64), m.hits.to(torch.float64), m.valid.to(torch.float64)])


def val_combine(parts, h, w, meter=None):
    """The loss / accuracy of the WHOLE batch from the rows of its parts (i2r_val_combine): parts float64 [n_part, 1 + 3 J] cuda, one
    val_sums_row per part stacked in rank order; (h, w) the heat-map size.  Runs on the current stream without a host synchronisation.
    Totals are added in ascending part index, so every rank that holds the same rows gets the same bits; one part reproduces
    val_metrics' own loss, acc, avg_acc, cnt and meter update bit for bit.  meter: a ValMeter, updated with the total crop count as
    val_metrics would have been on the whole batch (left alone when there is no crop at all).
    -> ValMetrics of the whole batch: sse, hits, valid the totals, n_crops int32 [1] the total crop count, pred None."""
    assert parts.is_cuda and parts.dtype == torch.float64 and parts.dim() == 2 and parts.shape[0] >= 1, (parts.dtype, tuple(parts.shape))
    assert parts.shape[1] >= 4 and (parts.shape[1] - 1) % 3 == 0, tuple(parts.shape)
    parts = parts.contiguous()
    n_part, J = int(parts.shape[0]), (int(parts.shape[1]) - 1) // 3
    dev = parts.device
    r = ValMetrics()
    f64 = torch.empty(J + 1 + 1 + 1 + J, dtype=torch.float64, device=dev)    # (every element is written by the kernel)
    i32 = torch.empty(2 + 2 * J, dtype=torch.int32, device=dev)
    r.acc, r.avg_acc, r.loss, r.sse = f64[:J + 1], f64[J + 1:J + 2], f64[J + 2:J + 3], f64[J + 3:]
    r.cnt, r.n_crops, r.hits, r.valid = i32[:1], i32[1:2], i32[2:2 + J], i32[2 + J:]
    r.pred = None
    if meter is not None:
        assert meter.buf.device == dev
    a = cabi.ValCombineArgs(parts=parts.data_ptr(), sse=r.sse.data_ptr(), hits=r.hits.data_ptr(), valid=r.valid.data_ptr(), loss=r.loss.data_ptr(),
                            acc=r.acc.data_ptr(), avg_acc=r.avg_acc.data_ptr(), cnt=r.cnt.data_ptr(), n_crops=r.n_crops.data_ptr(),
                            meter=meter.buf.data_ptr() if meter is not None else None, n_part=n_part, joints=J, h=int(h), w=int(w))
    with torch.cuda.device(dev):
        cabi.check(cabi.lib().i2r_val_combine(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream), "i2r_val_combine")
    return r


# ---- head re-fit: final_layer trained on frozen features (the one gradient of the project; DESIGN.md 'i2r_head_grad') -----------------
HeadGrad = collections.namedtuple("HeadGrad", "loss dw db sse")   # device tensors: float64 [1], fp32 [J, cin], fp32 [J], float64 [J]


def _head_inputs(feat, weight, bias):
    """feat [S, h, w, cs] fp32 NHWC cuda (I2RModule.head_input; any NHWC tensor with cs % 4 == 0), weight [J, cin(, 1, 1)], bias [J]
    -> (feat, weight [J, cin], bias, S, h, w, cs, J, cin), contiguous on feat's device"""
    assert feat.is_cuda and feat.dtype == torch.float32 and feat.dim() == 4, "feat: fp32 NHWC [S, h, w, cs] on the device"
    feat = feat.contiguous()
    S, h, w, cs = feat.shape
    wt = weight.detach()
    J = wt.shape[0]
    wt = _dev(wt.reshape(J, -1), torch.float32, feat.device, (J, wt.numel() // J))
    b = _dev(bias.detach(), torch.float32, feat.device, (J,))
    cin = wt.shape[1]
    if cin > cs:
        raise cabi.I2RError("head: the weight has %d input channels, feat only %d" % (cin, cs))
    return feat, wt, b, S, h, w, cs, J, cin


def _pad16(wt, cin):
    """[J, cin] -> ([J, cin16] with zero columns up to the next multiple of 16, cin16): the matrix-pipe entries take whole 16-channel
    steps; feat's channels behind cin are the engine's zero padding, which a zero weight leaves out of every sum exactly"""
    c16 = -(-cin // 16) * 16
    if c16 == cin:
        return wt, cin
    return torch.cat([wt, wt.new_zeros(wt.shape[0], c16 - cin)], 1).contiguous(), c16


def head_apply(feat, weight, bias):
    """final_layer on features: feat [S, h, w, cs] NHWC, weight [J, cin(, 1, 1)], bias [J] -> heat maps [S, J, h, w] (i2r_head, the
    kernel the forward ends in).  With it a fit loop can run val_metrics on held-out crops without the model."""
    feat, wt, b, S, h, w, cs, J, cin = _head_inputs(feat, weight, bias)
    if cin % 4:
        wt, cin = _pad16(wt, cin)
        if cin > cs:
            raise cabi.I2RError("head_apply: cin padded to %d exceeds feat's %d channels" % (cin, cs))
    out = torch.empty(S, J, h, w, dtype=torch.float32, device=feat.device)
    if S == 0:
        return out
    with torch.cuda.device(feat.device):
        cabi.check(cabi.lib().i2r_head(feat.data_ptr(), wt.data_ptr(), b.data_ptr(), out.data_ptr(), S, h, w, cin, cs, J,
                                       torch.cuda.current_stream(feat.device).cuda_stream), "i2r_head")
    return out


def head_grad(feat, weight, bias, target=None, target_weight=None, *, joints_hm=None, joints_vis=None, sigma=2, joints_weight=None,
              use_target_weight=True):
    """JointsMSELoss of final_layer(feat) and its gradient with respect to final_layer, in one pass over feat (i2r_head_grad), on the
    current stream without a host synchronisation.  feat [S, h, w, cs] fp32 NHWC (I2RModule.head_input), weight [J, cin(, 1, 1)], bias
    [J], plus ONE target form as val_metrics takes it.  cin that is no multiple of 16 (DIM_MODEL 78) runs at the next one: feat must hold
    that many channels, zeros behind cin (head_input's padding is that).  -> HeadGrad(loss [1] f64, dw [J, cin], db [J], sse [J] f64)."""
    if (target is None) == (joints_hm is None):
        raise cabi.I2RError("head_grad: give either target (+ target_weight) or joints_hm (+ joints_vis)")
    feat, wt, b, S, h, w, cs, J, cin_true = _head_inputs(feat, weight, bias)
    wt, cin = _pad16(wt, cin_true)
    dev = feat.device
    f64 = torch.zeros(1 + J, dtype=torch.float64, device=dev)                 # (a batch without crops launches nothing: all 0)
    dw = torch.zeros(J, cin, dtype=torch.float32, device=dev)
    db = torch.zeros(J, dtype=torch.float32, device=dev)
    r = HeadGrad(f64[:1], dw[:, :cin_true], db, f64[1:])
    nbytes = ctypes.c_int64(0)
    cabi.check(cabi.lib().i2r_head_grad_ws_bytes(S, h, w, cin, J, ctypes.byref(nbytes)), "i2r_head_grad_ws_bytes")
    ws = torch.empty((nbytes.value + 7) // 8, dtype=torch.float64, device=dev)
    a = cabi.HeadGradArgs(feat=feat.data_ptr(), w=wt.data_ptr(), bias=b.data_ptr(), ws=ws.data_ptr(), dw=dw.data_ptr(), db=db.data_ptr(),
                          loss=r.loss.data_ptr(), sse=r.sse.data_ptr(), sigma=float(sigma), n_crops=S, h=h, w_=w, cin=cin, in_cs=cs, w_cs=cin,
                          joints=J, use_target_weight=int(bool(use_target_weight)))
    if target is not None:
        assert target.is_cuda and target.dtype == torch.float32 and tuple(target.shape) == (S, J, h, w), tuple(target.shape)
        keep = [target.contiguous()]
        a.target = keep[0].data_ptr()
        if target_weight is not None:
            keep.append(_dev(torch.as_tensor(target_weight).reshape(S, J), torch.float32, dev, (S, J)))
            a.target_weight = keep[1].data_ptr()
        elif use_target_weight:
            raise cabi.I2RError("head_grad: use_target_weight without target_weight")
    else:
        keep = _joint_inputs(joints_hm, joints_vis, joints_weight, dev)
        assert tuple(keep[0].shape) == (S, J, 2), (tuple(keep[0].shape), (S, J))
        a.joints_hm, a.joints_vis = keep[0].data_ptr(), keep[1].data_ptr()
        a.joints_weight = keep[2].data_ptr() if keep[2] is not None else None
    if S == 0:
        return r
    with torch.cuda.device(dev):
        cabi.check(cabi.lib().i2r_head_grad(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream), "i2r_head_grad")
    return r


class HeadFit:
    """final_layer re-trained on frozen features: the usual way onto another joint set or domain (a 17-joint COCO checkpoint on the 14
    CrowdPose joints).  weight [J, cin, 1, 1] and bias [J] are nn.Parameters on the device; step() fills their .grad from head_grad and
    lets the optimizer move them -- the update of ~1.6 k numbers is plumbing and stays in torch.  optimizer: a torch.optim optimizer over
    (weight, bias), or a callable params -> optimizer; default what the reference's get_optimizer builds from cfg.TRAIN (Adam at
    TRAIN.LR; TRAIN.OPTIMIZER 'sgd': SGD with TRAIN.MOMENTUM, WD, NESTEROV), Adam at 1e-4 without a cfg.

        hi  = net.head_input(x, pos_mask, length)                        # frozen features, once per batch (or cached for the run)
        fit = HeadFit.from_model(net)                                    # or HeadFit(hi.cin, 14) for a new joint set
        loss = fit.step(hi.feat, joints_hm=jhm, joints_vis=vis)          # one train() iteration; no copy to the host
        fit.commit(net)                                                  # same joint count: the model now predicts with the new head"""

    def __init__(self, cin, joints, weight=None, bias=None, optimizer=None, cfg=None, device=None):
        dev = torch.device(device) if device is not None else (weight.device if weight is not None and weight.is_cuda
                                                               else torch.device("cuda", torch.cuda.current_device()))
        self.cin, self.joints, self.cfg = int(cin), int(joints), cfg
        if weight is None:  # nn.Conv2d's own initialisation of a 1x1 layer: kaiming_uniform(a = sqrt 5) = U(-1 / sqrt(cin), 1 / sqrt(cin)) for both
            bound = 1.0 / np.sqrt(self.cin)
            weight = (torch.rand(self.joints, self.cin, 1, 1) * 2 - 1) * bound
            bias = (torch.rand(self.joints) * 2 - 1) * bound if bias is None else bias
        elif bias is None:
            bias = torch.zeros(self.joints)
        self.weight = torch.nn.Parameter(weight.detach().to(dev, torch.float32).reshape(self.joints, self.cin, 1, 1).clone())
        self.bias = torch.nn.Parameter(bias.detach().to(dev, torch.float32).reshape(self.joints).clone())
        params = [self.weight, self.bias]
        if optimizer is None:
            T = cfg.TRAIN if cfg is not None else None
            if T is not None and T.OPTIMIZER == "sgd":
                optimizer = torch.optim.SGD(params, lr=T.LR, momentum=T.MOMENTUM, weight_decay=T.WD, nesterov=T.NESTEROV)
            elif T is None or T.OPTIMIZER == "adam":
                optimizer = torch.optim.Adam(params, lr=T.LR if T is not None else 1e-4)
            else:
                raise ValueError("HeadFit: TRAIN.OPTIMIZER %r ('adam' or 'sgd'); pass optimizer=" % (T.OPTIMIZER,))
        elif not isinstance(optimizer, torch.optim.Optimizer):
            optimizer = optimizer(params)
        self.optimizer = optimizer

    @classmethod
    def from_model(cls, net, optimizer=None):
        """start from the model's own final_layer (its config gives the default optimizer)"""
        t = net._tensors()
        w, b = t["final_layer.weight"], t["final_layer.bias"]
        if w.shape[2:] != (1, 1):
            raise ValueError("HeadFit: final_layer is %d x %d; the head re-fit is for a 1x1 layer" % tuple(w.shape[2:]))
        return cls(w.shape[1], w.shape[0], w, b, optimizer=optimizer, cfg=net.cfg, device=w.device)

    def grad(self, feat, target=None, target_weight=None, **kw):
        """head_grad at the current parameters; with a cfg, sigma / use_target_weight / the dataset's joints_weight table default to what
        val_metrics_cfg reads from it"""
        cfg = self.cfg
        if cfg is not None:
            kw.setdefault("sigma", cfg.MODEL.SIGMA)
            kw.setdefault("use_target_weight", cfg.LOSS.USE_TARGET_WEIGHT)
            if target is None and cfg.LOSS.USE_DIFFERENT_JOINTS_WEIGHT and "joints_weight" not in kw and \
                    len(JOINTS_WEIGHT.get(cfg.DATASET.DATASET, ())) == self.joints:
                kw["joints_weight"] = JOINTS_WEIGHT[cfg.DATASET.DATASET]
        return head_grad(feat, self.weight, self.bias, target, target_weight, **kw)

    def step(self, feat, target=None, target_weight=None, **kw):
        """one iteration of train(): the gradient into .grad, optimizer.step() -> the loss BEFORE the update (float64 [1], device)"""
        g = self.grad(feat, target, target_weight, **kw)
        self.weight.grad = g.dw.reshape(self.weight.shape).contiguous()
        self.bias.grad = g.db
        self.optimizer.step()
        return g.loss

    def state(self):
        return {"final_layer.weight": self.weight.detach().clone(), "final_layer.bias": self.bias.detach().clone()}

    def commit(self, net):
        """write the head into the model's parameters and drop its packed engines (rebuilt at the next forward).  ValueError when the
        joint count differs from cfg.MODEL.NUM_JOINTS: build a net with the new NUM_JOINTS and load the old state dict with state() laid
        over it."""
        if self.joints != net.cfg.MODEL.NUM_JOINTS:
            raise ValueError("HeadFit.commit: %d joints, the model has NUM_JOINTS %d -- build a model with NUM_JOINTS %d and load "
                             "dict(old_state, **fit.state())" % (self.joints, net.cfg.MODEL.NUM_JOINTS, self.joints))
        t = net._tensors()
        w, b = t["final_layer.weight"], t["final_layer.bias"]
        if tuple(w.shape) != tuple(self.weight.shape):
            raise ValueError("HeadFit.commit: weight %s, the model's final_layer is %s" % (tuple(self.weight.shape), tuple(w.shape)))
        with torch.no_grad():
            w.copy_(self.weight.detach())
            b.copy_(self.bias.detach())
        net._invalidate()


# ---- head re-fit in closed form: the normal equations from one pass over the features (DESIGN.md 'i2r_head_normal') -------------------
# device tensors: A float64 [J, cin + 1, cin + 1], r float64 [J, cin + 1], c float64 [J], n int64 [1]; the bias entry is index cin
HeadNormal = collections.namedtuple("HeadNormal", "A r c n")


def head_normal_state(cin, joints, device):
    """a zero state for head_normal at that (true) channel count"""
    m = int(cin) + 1
    return HeadNormal(torch.zeros(joints, m, m, dtype=torch.float64, device=device), torch.zeros(joints, m, dtype=torch.float64, device=device),
                      torch.zeros(joints, dtype=torch.float64, device=device), torch.zeros(1, dtype=torch.int64, device=device))


def head_normal(feat, target=None, target_weight=None, *, joints_hm=None, joints_vis=None, sigma=2, joints_weight=None, use_target_weight=True,
                state=None, cin=None):
    """The normal equations of JointsMSELoss in final_layer's (W, b) on frozen features, accumulated INTO state in one pass over feat
    (i2r_head_normal), on the current stream without a host synchronisation.  feat [S, h, w, cs] fp32 NHWC (I2RModule.head_input) plus
    ONE target form as head_grad takes it.  cin: the layer's input channels (default: the state's, else cs); one that is no multiple of
    16 runs at the next one -- feat must hold that many channels, zeros behind cin (head_input's padding is that).  state: a HeadNormal
    of dense tensors for that cin (None: a fresh zero state).  -> HeadNormal(A, r, c, n), the state itself."""
    if (target is None) == (joints_hm is None):
        raise cabi.I2RError("head_normal: give either target (+ target_weight) or joints_hm (+ joints_vis)")
    assert feat.is_cuda and feat.dtype == torch.float32 and feat.dim() == 4, "feat: fp32 NHWC [S, h, w, cs] on the device"
    feat = feat.contiguous()
    S, h, w, cs = feat.shape
    dev = feat.device
    if state is not None:
        cin = state.r.shape[1] - 1 if cin is None else int(cin)
    elif cin is None:
        cin = cs
    if target is not None:
        J = target.shape[1]
    else:
        J = (joints_hm if isinstance(joints_hm, torch.Tensor) else np.asarray(joints_hm)).shape[1]
    if state is None:
        state = head_normal_state(cin, J, dev)
    m = cin + 1
    for t, shape, dt in ((state.A, (J, m, m), torch.float64), (state.r, (J, m), torch.float64), (state.c, (J,), torch.float64), (state.n, (1,), torch.int64)):
        if not (t.is_cuda and t.device == dev and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous()):
            raise cabi.I2RError("head_normal: state tensor %s %s on %s, wanted dense %s %s on %s" % (tuple(t.shape), t.dtype, t.device, shape, dt, dev))
    c16 = -(-cin // 16) * 16
    if c16 > cs:
        raise cabi.I2RError("head_normal: cin %d runs at %d channels, feat has only %d" % (cin, c16, cs))
    nbytes = ctypes.c_int64(0)
    cabi.check(cabi.lib().i2r_head_normal_ws_bytes(S, h, w, c16, J, ctypes.byref(nbytes)), "i2r_head_normal_ws_bytes")
    ws = torch.empty((nbytes.value + 7) // 8, dtype=torch.float64, device=dev)
    a = cabi.HeadNormalArgs(feat=feat.data_ptr(), ws=ws.data_ptr(), A=state.A.data_ptr(), r=state.r.data_ptr(), c=state.c.data_ptr(), n=state.n.data_ptr(),
                            sigma=float(sigma), n_crops=S, h=h, w_=w, cin=c16, in_cs=cs, cin_out=cin, ld=m, joints=J,
                            use_target_weight=int(bool(use_target_weight)))
    if target is not None:
        assert target.is_cuda and target.dtype == torch.float32 and tuple(target.shape) == (S, J, h, w), tuple(target.shape)
        keep = [target.contiguous()]
        a.target = keep[0].data_ptr()
        if target_weight is not None:
            keep.append(_dev(torch.as_tensor(target_weight).reshape(S, J), torch.float32, dev, (S, J)))
            a.target_weight = keep[1].data_ptr()
        elif use_target_weight:
            raise cabi.I2RError("head_normal: use_target_weight without target_weight")
    else:
        keep = _joint_inputs(joints_hm, joints_vis, joints_weight, dev)
        assert tuple(keep[0].shape) == (S, J, 2), (tuple(keep[0].shape), (S, J))
        a.joints_hm, a.joints_vis = keep[0].data_ptr(), keep[1].data_ptr()
        a.joints_weight = keep[2].data_ptr() if keep[2] is not None else None
    if S == 0:
        return state
    with torch.cuda.device(dev):
        cabi.check(cabi.lib().i2r_head_normal(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream), "i2r_head_normal")
    return state


def solve_normal(A, r, n, ridge=0.0, rcond=None):
    """numpy float64: per joint the minimiser of L + (ridge / 2) ||W||^2, i.e. the solution of (A_j + ridge n J diag(1 .. 1, 0)) w~ = r_j
    (the bias is not penalised), by a symmetric eigendecomposition; directions with an eigenvalue <= rcond * lmax are dropped, which
    gives the minimum-norm minimiser there (dead or padded channels; a joint that is never visible gets zeros).  rcond defaults to
    (cin + 1) 2^-52, numpy's float64 convention.  -> w~ float64 [J, cin + 1]"""
    A, r = np.asarray(A, np.float64), np.asarray(r, np.float64)
    J, m, _ = A.shape
    rcond = m * 2.0 ** -52 if rcond is None else float(rcond)
    pen = np.ones(m)
    pen[-1] = 0.0
    out = np.zeros((J, m))
    for j in range(J):
        lam, V = np.linalg.eigh(A[j] + (float(ridge) * float(n) * J) * np.diag(pen))
        keep = lam > rcond * max(float(lam[-1]), 0.0)
        Vk = V[:, keep]
        out[j] = Vk @ ((Vk.T @ r[j]) / lam[keep])
    return out


class HeadSolve:
    """final_layer re-fitted in closed form: add() every batch of frozen features once (one pass each, i2r_head_normal), solve() for
    the exact minimiser of JointsMSELoss over everything added.

        acc = HeadSolve(hi.cin, 14, cfg=cfg)
        for batch in loader:                                             # one epoch; several augmented ones add up the same way
            hi = net.head_input(x, pos_mask, length)
            acc.add(hi.feat, joints_hm=jhm, joints_vis=vis)              # no copy to the host
        fit = acc.head_fit()                                             # a HeadFit at the solution: commit(net), state(), step()"""

    def __init__(self, cin, joints, cfg=None, device=None):
        self.cin, self.joints, self.cfg = int(cin), int(joints), cfg
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.state = head_normal_state(self.cin, self.joints, self.device)

    def add(self, feat, target=None, target_weight=None, **kw):
        """accumulate a batch; with a cfg, sigma / use_target_weight / the dataset's joints_weight table default as in HeadFit.grad"""
        cfg = self.cfg
        if cfg is not None:
            kw.setdefault("sigma", cfg.MODEL.SIGMA)
            kw.setdefault("use_target_weight", cfg.LOSS.USE_TARGET_WEIGHT)
            if target is None and cfg.LOSS.USE_DIFFERENT_JOINTS_WEIGHT and "joints_weight" not in kw and \
                    len(JOINTS_WEIGHT.get(cfg.DATASET.DATASET, ())) == self.joints:
                kw["joints_weight"] = JOINTS_WEIGHT[cfg.DATASET.DATASET]
        head_normal(feat, target, target_weight, state=self.state, cin=self.cin, **kw)
        return self

    def merge(self, other):
        """add another accumulator's state (the state is additive: a data-parallel fit would all-reduce it)"""
        if (other.cin, other.joints) != (self.cin, self.joints):
            raise ValueError("HeadSolve.merge: (cin, joints) %s into %s" % ((other.cin, other.joints), (self.cin, self.joints)))
        for mine, theirs in zip(self.state, other.state):
            mine += theirs.to(self.device)
        return self

    def _host(self):
        """the one copy of the state to the host -> (A, r, c, n) numpy"""
        m = self.cin + 1
        flat = torch.cat([self.state.A.reshape(-1), self.state.r.reshape(-1), self.state.c, self.state.n.to(torch.float64)]).cpu().numpy()
        J = self.joints
        A, r = flat[:J * m * m].reshape(J, m, m), flat[J * m * m:J * m * m + J * m].reshape(J, m)
        return A, r, flat[-1 - J:-1], int(flat[-1])

    def loss(self, weight, bias):
        """L(W, b) over everything added, evaluated in float64 from the state (no feature is read) -> float"""
        A, r, c, n = self._host()
        J = self.joints
        wt = np.concatenate([torch.as_tensor(weight).detach().cpu().numpy().astype(np.float64).reshape(J, self.cin),
                             torch.as_tensor(bias).detach().cpu().numpy().astype(np.float64).reshape(J, 1)], 1)
        if n == 0:
            return 0.0
        return float((np.einsum("ja,jab,jb->j", wt, A, wt) - 2.0 * (wt * r).sum(1) + c).sum() / (2.0 * n * J))

    def solve(self, ridge=0.0, rcond=None):
        """-> (weight [J, cin, 1, 1], bias [J]) fp32 on the device: solve_normal on the host (the copy of the state is the only
        synchronisation of a fit), rounded once to fp32"""
        A, r, _, n = self._host()
        wt = solve_normal(A, r, n, ridge, rcond).astype(np.float32)
        return (torch.from_numpy(np.ascontiguousarray(wt[:, :self.cin])).reshape(self.joints, self.cin, 1, 1).to(self.device),
                torch.from_numpy(np.ascontiguousarray(wt[:, self.cin])).to(self.device))

    def head_fit(self, ridge=0.0, rcond=None, optimizer=None):
        """a HeadFit that starts at the solution"""
        w, b = self.solve(ridge, rcond)
        return HeadFit(self.cin, self.joints, w, b, optimizer=optimizer, cfg=self.cfg, device=self.device)


# ---- keypoint OKS evaluation: COCOeval(gt, dt, 'keypoints') and the per-person-count table of lib/utils/KeypointEvaluator.py, on the device
OKS_THRS = tuple(float(v) for v in np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True))      # Params.iouThrs
OKS_REC_THRS = tuple(float(v) for v in np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True))  # Params.recThrs
OKS_AREA_RNG = ((0.0, 1e5 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2))                                    # all, medium, large
OKS_STATS_NAMES = ("AP", "Ap .5", "AP .75", "AP (M)", "AP (L)", "AR", "AR .5", "AR .75", "AR (M)", "AR (L)")        # coco.py:507
OKS_MAX_DETS, OKS_MAX_GT_PER_IMG, OKS_MAX_DT_PER_IMG = 32, 256, 1024   # limits of i2r_oks_match


class GtTable:
    """The ground truth of an evaluation as i2r_oks_match reads it, built once on the host: images sorted by id, every image's person
    annotations in file order.  Device tensors: kpts f64 [n_gt, J, 3], area f64 [n_gt], bbox f64 [n_gt, 4], flags int32 [n_gt] (bit 0
    iscrowd, bit 1 ignore = iscrowd or num_keypoints == 0), off int32 [n_img + 1].  Host: image_ids int64 [n_img] (sorted), counts int64
    [n_img] (annotations per image), max_gt (the largest count)."""

    def __init__(self, image_ids, kpts, area, bbox, flags, counts, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.image_ids = image_ids
        self.counts = counts
        self.n_img, self.n_gt, self.joints = int(image_ids.numel()), int(kpts.shape[0]), int(kpts.shape[1])
        self.max_gt = int(counts.max()) if self.n_img else 0
        off = torch.zeros(self.n_img + 1, dtype=torch.int32)
        off[1:] = torch.cumsum(counts, 0)
        pin = (lambda t: t.pin_memory()) if self.device.type == "cuda" else (lambda t: t)
        up = lambda t: pin(t.contiguous()).to(self.device, non_blocking=True)
        self.kpts, self.area, self.bbox, self.flags, self.off = up(kpts), up(area), up(bbox), up(flags), up(off)

    @classmethod
    def from_arrays(cls, image_ids, gt_image_id, keypoints, area, bbox, iscrowd=None, num_keypoints=None, device="cuda"):
        """image_ids: every image of the set (one without annotations is still evaluated); per annotation: gt_image_id, keypoints
        [n, J, 3] (x, y, v), area, bbox [n, 4] (x, y, w, h), iscrowd (default 0), num_keypoints (default: the number of v > 0)."""
        ids = torch.as_tensor(np.asarray(image_ids, np.int64).reshape(-1))
        ids, _ = torch.sort(ids)
        if ids.numel() > 1 and bool((ids[1:] == ids[:-1]).any()):
            raise ValueError("GtTable: an image id occurs twice")
        kp = torch.as_tensor(np.asarray(keypoints, np.float64))
        n = kp.shape[0]
        kp = kp if kp.dim() == 3 else kp.reshape(n, -1, 3)
        gid = torch.as_tensor(np.asarray(gt_image_id, np.int64).reshape(-1))
        crowd = torch.zeros(n, dtype=torch.int64) if iscrowd is None else torch.as_tensor(np.asarray(iscrowd).astype(np.int64).reshape(-1))
        nk = (kp[:, :, 2] > 0).sum(1) if num_keypoints is None else torch.as_tensor(np.asarray(num_keypoints, np.int64).reshape(-1))
        idx = torch.searchsorted(ids, gid).clamp_(max=max(ids.numel() - 1, 0))
        if n and (ids.numel() == 0 or bool((ids[idx] != gid).any())):
            raise ValueError("GtTable: an annotation of an image that is not in the set")
        order = torch.sort(idx, stable=True)[1]   # (grouped by image, file order inside an image)
        flags = ((crowd != 0).to(torch.int32) | (((crowd != 0) | (nk == 0)).to(torch.int32) << 1))
        counts = torch.bincount(idx, minlength=ids.numel()) if n else torch.zeros(ids.numel(), dtype=torch.int64)
        area = torch.as_tensor(np.asarray(area, np.float64).reshape(-1))
        bbox = torch.as_tensor(np.asarray(bbox, np.float64).reshape(n, 4))
        return cls(ids, kp[order], area[order], bbox[order], flags[order], counts, device)

    @classmethod
    def from_coco(cls, dataset, device="cuda"):
        """dataset: a COCO key-point annotation file (path) or its dict: `images`, `annotations`, `categories`.  Persons only."""
        if not isinstance(dataset, dict):
            import json
            with open(dataset) as f:
                dataset = json.load(f)
        cats = [c["id"] for c in dataset.get("categories", []) if c.get("name") == "person"]
        anns = [a for a in dataset.get("annotations", []) if not cats or a.get("category_id") in cats]
        J = len(anns[0]["keypoints"]) // 3 if anns else 17
        return cls.from_arrays([im["id"] for im in dataset["images"]], [a["image_id"] for a in anns],
                               np.asarray([a["keypoints"] for a in anns], np.float64).reshape(len(anns), J, 3),
                               [a["area"] for a in anns], np.asarray([a["bbox"] for a in anns], np.float64).reshape(len(anns), 4),
                               [a.get("iscrowd", 0) for a in anns], [a["num_keypoints"] for a in anns], device=device)


class OksEval:
    """What oks_eval returns, device tensors: stats f64 [n_group + 1, 10] (row n_group = every image), precision f64 [n_group + 1, n_thr,
    n_rec, n_area], recall f64 [n_group + 1, n_thr, n_area], npig int32 [n_group + 1, n_area]; names: the ten names of evaluate();
    group_names: the level names of the groups + 'all'.  match: the per-detection outputs of i2r_oks_match in the grouped order
    (perm: grouped position -> input index): plain tensors that dist.gather_poses-style gathers can carry."""

    def __init__(self, stats, precision, recall, npig, group_names, match):
        self.stats, self.precision, self.recall, self.npig = stats, precision, recall, npig
        self.names, self.group_names, self.match = OKS_STATS_NAMES, tuple(group_names), match

    def name_values(self, group=None):
        """the OrderedDict evaluate() returns (coco.py:430); group: None = every image, else a group index or level name.
        This is the copy to the host."""
        from collections import OrderedDict
        g = len(self.group_names) - 1 if group is None else (self.group_names.index(group) if isinstance(group, str) else int(group))
        return OrderedDict(zip(self.names, self.stats[g].cpu().tolist()))


def person_count_groups(counts, start_points=(1, 2, 6, 10)):
    """ClusterMode.get_cluster_level (lib/utils/KeypointEvaluator.py:528-544) for every image: counts -> (int32 tensor of group indices,
    level names).  Level c{i+1} holds the counts in [start_points[i], start_points[i + 1]), the last level everything from the last start
    point on; a count below the first start point (0 persons) is in no group: -1."""
    sp = [int(v) for v in start_points]
    assert len(sp) >= 2 and all(b > a for a, b in zip(sp, sp[1:])), sp
    c = torch.as_tensor(counts).to(torch.int64)
    grp = torch.bucketize(c, torch.tensor(sp, dtype=torch.int64, device=c.device), right=True) - 1
    return grp.to(torch.int32), ["c%d" % (i + 1) for i in range(len(sp))]


_OKS_CONST = {}


def _oks_const(key, values, dev):
    """small float64 tables on the device, uploaded once per (values, device) with a blocking copy (see _SIGMAS_DEV)"""
    k = (key, tuple(values), dev)
    if k not in _OKS_CONST:
        _OKS_CONST[k] = torch.tensor(list(values), dtype=torch.float64).to(dev)
    return _OKS_CONST[k]


def oks_eval(gt, image_ids, keypoints, scores, valid=None, *, sigmas=None, groups=None, max_dets=20, thr=None, area_rng=None, rec_thr=None,
             want_oks=False):
    """COCOeval(gt, dt, 'keypoints').evaluate() / accumulate() / summarize() on the current stream: i2r_oks_match + i2r_oks_accumulate,
    the ten numbers from their arrays with torch.  Nothing is copied to the host and nothing waits for the device.
    gt: GtTable.  image_ids: host list / array / tensor, one id per detection (a device tensor is copied to the host first); an id that is
    not in the table is a ValueError (loadRes asserts the same).  keypoints [N, J, 2 or 3] and scores [N] on the device, e.g. decode()'s
    preds and PoseNms.score; valid [N] (bool / uint8 / int), e.g. PoseNms.rank >= 0.
    groups: (int tensor [n_img] of group indices in the table's image order, level names) as person_count_groups returns it.
    The limits of i2r_oks_match (1024 detections and 256 gts of one image, max_dets <= 32) apply to the rows as given: `valid` lives on
    the device, so rows it masks out still count towards the 1024 of their image; drop them before the call where that matters.
    Defaults: COCOeval's key-point parameters (thresholds .5:.05:.95, 101 recall thresholds, areas all / medium / large, maxDets 20) and
    the sigma table of J = 17 or 14; the stats rows follow summarize (AP / AR at thresholds .5 and .75 are -1 when `thr` lacks them;
    area columns 1 and 2 are 'medium' and 'large').  -> OksEval."""
    assert isinstance(gt, GtTable)
    dev = gt.device
    assert keypoints.device == dev and keypoints.dim() == 3 and keypoints.shape[2] in (2, 3), (keypoints.device, tuple(keypoints.shape))
    N, J = int(keypoints.shape[0]), int(keypoints.shape[1])
    if gt.n_gt and gt.joints != J:
        raise ValueError("oks_eval: %d joints, the ground truth has %d" % (J, gt.joints))
    if sigmas is None:
        if J not in SIGMAS:
            raise cabi.I2RError("oks_eval: no sigma table for %d joints -- pass sigmas" % J)
        sigmas = SIGMAS[J]
    sig = _oks_const("sigmas", [float(v) for v in sigmas], dev)
    assert sig.numel() == J, (sig.numel(), J)
    thr = OKS_THRS if thr is None else tuple(float(v) for v in thr)
    rec_thr = OKS_REC_THRS if rec_thr is None else tuple(float(v) for v in rec_thr)
    area_rng = OKS_AREA_RNG if area_rng is None else tuple((float(a), float(b)) for a, b in area_rng)
    nT, nR, nA = len(thr), len(rec_thr), len(area_rng)
    thr_d, rec_d = _oks_const("thr", thr, dev), _oks_const("rec", rec_thr, dev)
    rng_d = _oks_const("rng", [v for ab in area_rng for v in ab], dev)
    # host plumbing, vectorised: image index of every detection, the grouping permutation, the offsets
    ids = image_ids.cpu() if torch.is_tensor(image_ids) else torch.as_tensor(np.asarray(image_ids, np.int64))
    ids = ids.to(torch.int64).reshape(-1)
    assert ids.numel() == N, (ids.numel(), N)
    idx = torch.searchsorted(gt.image_ids, ids).clamp_(max=max(gt.n_img - 1, 0))
    if N and (gt.n_img == 0 or bool((gt.image_ids[idx] != ids).any())):
        raise ValueError("oks_eval: Results do not correspond to current coco set (an image id is not in the ground truth)")
    idx_s, perm = torch.sort(idx, stable=True)
    cnt = torch.bincount(idx, minlength=gt.n_img) if N else torch.zeros(gt.n_img, dtype=torch.int64)
    max_dt = int(cnt.max()) if gt.n_img else 0
    off = torch.zeros(gt.n_img + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(cnt, 0)
    host = torch.cat([off, idx_s, perm]).to(torch.int32)   # (one upload)
    if dev.type == "cuda":
        host = host.pin_memory()
    host = host.to(dev, non_blocking=True)
    dt_off, dt_img, perm_d = host[:gt.n_img + 1], host[gt.n_img + 1:gt.n_img + 1 + N], host[gt.n_img + 1 + N:].to(torch.int64)
    kp = keypoints[:, :, :2].to(torch.float32)[perm_d].contiguous()
    sc = torch.as_tensor(scores).to(dev, non_blocking=True).to(torch.float32).reshape(N)[perm_d].contiguous()
    va = None if valid is None else (torch.as_tensor(valid).to(dev, non_blocking=True).reshape(N) != 0).to(torch.uint8)[perm_d].contiguous()
    if groups is None:
        n_group, img_group, group_names = 0, None, []
    else:
        img_group, group_names = groups
        group_names = list(group_names)
        n_group = len(group_names)
        img_group = torch.as_tensor(img_group).to(dev, non_blocking=True).to(torch.int32).contiguous()
        assert img_group.numel() == gt.n_img, (img_group.numel(), gt.n_img)
    dt_rank = torch.empty(N, dtype=torch.int32, device=dev)
    dt_match = torch.empty(nA, N, dtype=torch.int32, device=dev)   # (uint32 bit rows held in int32 tensors)
    dt_ignore = torch.empty(nA, N, dtype=torch.int32, device=dev)
    gt_ignore = torch.empty(nA, gt.n_gt, dtype=torch.uint8, device=dev)
    oks = oks_off = None
    if want_oks:
        o = torch.zeros(gt.n_img + 1, dtype=torch.int64)
        o[1:] = torch.cumsum(cnt * gt.counts, 0)
        oks = torch.empty(int(o[-1]), dtype=torch.float64, device=dev)
        oks_off = o.to(dev, non_blocking=True)
    st = torch.cuda.current_stream(dev).cuda_stream
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    m = cabi.OksMatchArgs(dt_kpts=ptr(kp), dt_score=ptr(sc), dt_valid=ptr(va), dt_off=dt_off.data_ptr(), gt_kpts=ptr(gt.kpts),
                          gt_area=ptr(gt.area), gt_bbox=ptr(gt.bbox), gt_flags=ptr(gt.flags), gt_off=gt.off.data_ptr(),
                          sigmas=sig.data_ptr(), thr=thr_d.data_ptr(), area_rng=rng_d.data_ptr(), dt_rank=ptr(dt_rank), dt_match=ptr(dt_match),
                          dt_ignore=ptr(dt_ignore), gt_ignore=ptr(gt_ignore), oks=ptr(oks), oks_off=ptr(oks_off),
                          oks_len=oks.numel() if oks is not None else 0, n_dt=N, n_gt=gt.n_gt, n_img=gt.n_img, joints=J, n_thr=nT, n_area=nA,
                          max_dets=int(max_dets), max_dt_per_img=max_dt, max_gt_per_img=gt.max_gt)
    cabi.check(cabi.lib().i2r_oks_match(ctypes.byref(m), st), "i2r_oks_match")
    # the global score order (plumbing): a stable descending sort over the grouped detections; those that take no part go behind
    key = torch.where((dt_rank >= 0) & (sc == sc), sc, torch.full_like(sc, float("-inf")))   # (a NaN score ranks as -inf, as in the kernel)
    # (inside an image the pre-sort order has to be the rank order, which for equal scores is the input order: the grouped order)
    order = torch.sort(key, descending=True, stable=True)[1].to(torch.int32)
    precision = torch.empty(n_group + 1, nT, nR, nA, dtype=torch.float64, device=dev)
    recall = torch.empty(n_group + 1, nT, nA, dtype=torch.float64, device=dev)
    npig = torch.empty(n_group + 1, nA, dtype=torch.int32, device=dev)
    acc = cabi.OksAccumulateArgs(dt_match=ptr(dt_match), dt_ignore=ptr(dt_ignore), dt_rank=ptr(dt_rank), order=ptr(order), dt_img=ptr(dt_img),
                                 img_group=ptr(img_group), gt_ignore=ptr(gt_ignore), gt_off=gt.off.data_ptr(), rec_thr=rec_d.data_ptr(),
                                 precision=precision.data_ptr(), recall=recall.data_ptr(), npig=npig.data_ptr(), n_dt=N, n_gt=gt.n_gt,
                                 n_img=gt.n_img, n_part=N, n_group=n_group, n_thr=nT, n_area=nA, n_rec=nR)
    cabi.check(cabi.lib().i2r_oks_accumulate(ctypes.byref(acc), st), "i2r_oks_accumulate")

    # summarize (_summarizeKps): the mean over the entries > -1, -1 when there are none
    def mean_valid(x):   # x [n_group + 1, ...]
        x = x.reshape(n_group + 1, -1)
        ok = x > -1
        n = ok.sum(1)
        return torch.where(n > 0, torch.where(ok, x, torch.zeros_like(x)).sum(1) / n.clamp(min=1), torch.full_like(x[:, 0], -1.0))
    minus = torch.full((n_group + 1,), -1.0, dtype=torch.float64, device=dev)
    t_of = lambda v: thr.index(v) if v in thr else None   # (a slice below, never an index list: that would be an upload that waits)
    cols = []
    for src, is_ap in ((precision, True), (recall, False)):
        area = (lambda s, a: s[:, :, :, a]) if is_ap else (lambda s, a: s[:, :, a])
        cols.append(mean_valid(area(src, 0)))
        for v in (.5, .75):
            i = t_of(v)
            cols.append(mean_valid(area(src[:, i:i + 1], 0)) if i is not None else minus)
        for a in (1, 2):
            cols.append(mean_valid(area(src, a)) if a < nA else minus)
    stats = torch.stack(cols, 1)
    match = dict(rank=dt_rank, match=dt_match, ignore=dt_ignore, gt_ignore=gt_ignore, perm=perm_d, oks=oks, oks_off=oks_off)
    return OksEval(stats, precision, recall, npig, group_names + ["all"], match)


def oks_eval_cfg(cfg, gt, image_ids, keypoints, scores, valid=None, **kw):
    """oks_eval with the sigma table of MODEL.NUM_JOINTS (17: COCO / OCHuman, 14: the table lib/nms/nms.py uses for CrowdPose)."""
    J = cfg.MODEL.NUM_JOINTS
    assert keypoints.shape[1] == J, (tuple(keypoints.shape), J)
    if "sigmas" not in kw:
        if J not in SIGMAS:
            raise cabi.I2RError("oks_eval_cfg: no sigma table for MODEL.NUM_JOINTS = %d -- pass sigmas" % J)
        kw["sigmas"] = SIGMAS[J]
    return oks_eval(gt, image_ids, keypoints, scores, valid, **kw)


class PoseTable:
    """The detections of an evaluation, collected on the device over the steps (and ranks) of a validation pass: a growable table of the
    rows dist.gather_poses returns, [n, J * 3 + 2] (key points, rescored value, NMS rank as a float; -1 = suppressed), and one image id
    per row on the host.  append() copies on the current stream and never waits for the device; the buffer doubles when it is full (one
    device copy).  Images are never split across ranks or steps, so inside an image the rows keep their input order, which is all
    oks_eval's result depends on: evaluate() gives the bits of one oks_eval call on the same detections."""

    def __init__(self, joints, device, capacity=1024, dtype=torch.float32):
        self.joints, self.n = int(joints), 0
        self.buf = torch.empty(max(int(capacity), 1), self.joints * 3 + 2, dtype=dtype, device=device)
        self.ids = np.empty(self.buf.shape[0], np.int64)

    def __len__(self):
        return self.n

    def append(self, rows, image_ids):
        """rows [k, J * 3 + 2] on the table's device (dist.gather_poses' result, or one rank's own rows), image_ids: k host integers"""
        ids = np.asarray(image_ids, np.int64).reshape(-1)
        k = int(rows.shape[0])
        assert rows.dim() == 2 and rows.shape[1] == self.buf.shape[1] and ids.size == k, (tuple(rows.shape), tuple(self.buf.shape), ids.size)
        if k == 0:
            return
        assert rows.device == self.buf.device and rows.dtype == self.buf.dtype, (rows.device, rows.dtype)
        cap = self.buf.shape[0]
        if self.n + k > cap:
            while self.n + k > cap:
                cap *= 2
            buf = torch.empty(cap, self.buf.shape[1], dtype=self.buf.dtype, device=self.buf.device)
            buf[:self.n].copy_(self.buf[:self.n])
            self.buf = buf
            self.ids = np.concatenate([self.ids[:self.n], np.empty(cap - self.n, np.int64)])
        self.buf[self.n:self.n + k].copy_(rows)
        self.ids[self.n:self.n + k] = ids
        self.n += k

    def rows(self):
        """the live view [n, J * 3 + 2] (valid until the next append that grows the buffer)"""
        return self.buf[:self.n]

    def image_ids(self):
        return self.ids[:self.n]

    def evaluate(self, gt, **kw):
        """oks_eval(gt, image ids, key points, rescored value, valid = rank >= 0, **kw) on what has been collected -> OksEval"""
        J, rows = self.joints, self.rows()
        return oks_eval(gt, self.image_ids(), rows[:, :J * 3].reshape(self.n, J, 3), rows[:, J * 3], rows[:, J * 3 + 1] >= 0, **kw)
