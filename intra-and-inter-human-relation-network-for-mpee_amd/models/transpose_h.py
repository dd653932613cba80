"""TransPose-H intra-human stage. Mirror of reference lib/models/transpose_h.py: TransPoseH (:416), forward (:649-655) returning
(features [S, d, H/4, W/4], heatmaps [S, J, H/4, W/4]), get_pose_net(cfg, is_train, pretrained_path, is_end2end) (:691) -- the
factory InterFormer.__init__ reaches with eval('models.' + cfg.MODEL.SINGLEFORMER + '.get_pose_net') (interformer.py:139).
Inside the 2-stage module the same parameters live under the ``singleformer.`` prefix and run as part of one program
(models/interformer.py); this module is the stand-alone form (e.g. for checking a first-stage checkpoint on its own)."""
import torch

from .. import arch
from ._base import I2RModule


def param_spec(cfg, prefix=""):
    return arch.transpose_h_spec(cfg, prefix)


class TransPoseH(I2RModule):
    def __init__(self, cfg, **kwargs):
        super().__init__(cfg, arch.transpose_h_spec(cfg, ""))

    def _engine_name(self):
        return "transpose_h"

    def forward(self, x):
        """x [S, 3, H, W] -> (features, heatmaps)  (transpose_h.py:649-655)"""
        hooked = self._hooked()
        with torch.no_grad():
            if not hooked:
                return self.engine().forward_single(x)
            out, maps = self.engine().forward_single(x, capture={(st, i) for st, i, _ in hooked})
            self._serve_hooks(hooked, maps)
            return out

    def attention_at(self, x, points, mode="dependency", layers=None, upsample=True):
        """I2RModule.attention_at for the stand-alone stage: -> ((features, heatmaps), {("global_encoder", layer): [S, K, 1, h r, w r]})"""
        eng = self.engine()
        capture, queries = self._query_plan(eng, x, points, mode, layers, upsample)
        with torch.no_grad():
            out, maps = eng.forward_single(x, capture=capture, queries=queries)
        return out, self._query_result(maps, lambda st: True)


def get_pose_net(cfg, is_train, pretrained_path="", is_end2end=False, **kwargs):
    if is_train:
        raise NotImplementedError("i2r_amd implements the inference path only (is_train=False)")
    return TransPoseH(cfg, **kwargs).eval()
