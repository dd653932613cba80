"""nn.Module shell shared by the model factories: a parameter tree with the reference's state-dict keys
whose forward() runs the HIP engine.  The module owns the parameters (load_state_dict / .cuda() / DataParallel
work as for the reference, tools/test.py:87-118); packed device copies (one Engine per device, shared with DataParallel
replicas) are rebuilt lazily after any change.  After an in-place weight edit that bypasses load_state_dict / .to(),
call _invalidate()."""
import collections
import math

import torch
import torch.nn as nn

from .. import arch, synth


# Encoder stacks whose attention maps the forward hooks can capture (state-dict prefix of the stack -> the `reduce` conv that feeds it, or
# None): the reference's visualize.py:128-268,270-420 registers hooks on <stack>.layers[i].self_attn (nn.MultiheadAttention, output[1] =
# the head-averaged weights) and on reduce.  Their `layers` containers are nn.ModuleLists, so layers[i] / len(layers) work as there.
ATTN_STACKS = {"global_encoder": "reduce", "multi_global_encoder": None, "singleformer.global_encoder": "singleformer.reduce"}


def pad_attention_maps(maps):
    """per batch entry [L_b, L_b] maps -> the reference's [batch, L, L] layout, L = max L_b: block [b, :L_b, :L_b] = maps[b], zeros
    elsewhere.  Columns L_b.. are exactly what the reference's key_padding_mask gives; rows L_b.. would be the attention of the
    zero-feature padded persons, which this port never builds."""
    L = max(m.shape[0] for m in maps)
    out = maps[0].new_zeros(len(maps), L, L)
    for b, m in enumerate(maps):
        out[b, :m.shape[0], :m.shape[1]] = m
    return out


def unpad_attention_maps(weights, lens):
    """inverse of pad_attention_maps: [batch, L, L] + per-entry lengths -> list of [L_b, L_b] views"""
    return [weights[b, :n, :n] for b, n in enumerate(lens)]


def points_to_tokens(points, in_h, in_w, fh, fw):
    """points [S, K, 2] as (x, y) in the frame of each crop's [in_h, in_w] network input -> int32 [S, K] token indices row * fw + col of the
    [fh, fw] token map: (row, col) = (int(y / down_rate), int(x / down_rate)), down_rate = in_h // fh (the reference's visualize.py:194-196).
    A NaN point means "skip" (-1); a point outside the crop raises ValueError."""
    pts = torch.as_tensor(points, dtype=torch.float64).cpu()
    if pts.dim() != 3 or pts.shape[-1] != 2:
        raise ValueError("points: shape %s, expected [crops, K, 2] holding (x, y)" % (tuple(pts.shape),))
    down = in_h // fh
    skip = torch.isnan(pts).any(-1)
    x, y = pts[..., 0].masked_fill(skip, 0.0), pts[..., 1].masked_fill(skip, 0.0)
    if bool(((x < 0) | (x >= in_w) | (y < 0) | (y >= in_h)).any()):
        raise ValueError("points: a point lies outside its %d x %d (w x h) crop" % (in_w, in_h))
    row, col = (y / down).long().clamp_(max=fh - 1), (x / down).long().clamp_(max=fw - 1)
    return (row * fw + col).masked_fill(skip, -1).to(torch.int32)


def group_tokens(tok, length, hw):
    """per-crop tokens [S, K] -> the inter-human table: per image the points of all its persons as queries, token (person, y, x) =
    person * hw + token, entry person * K + k; -> (int32 [images, max(length) * K] padded with -1, entries used per image)"""
    S, K = tok.shape
    assert S == sum(length)
    out = torch.full((len(length), max(length) * K), -1, dtype=torch.int32)
    s = 0
    for b, n in enumerate(length):
        t = tok[s:s + n].to(torch.int64)
        shift = torch.arange(n).view(n, 1) * hw
        out[b, :n * K] = torch.where(t >= 0, t + shift, t).reshape(-1).to(torch.int32)
        s += n
    return out, [n * K for n in length]


class PersonRelations:
    """what I2RModule.person_relations returns: relation {(stack, layer): [per image [P, P]]}, maps {(stack, layer): [per image [P, P, h r, w r]]}"""

    def __init__(self, relation, maps):
        self.relation, self.maps = relation, maps


class TargetRelations:
    """what I2RModule.main_target_relations returns, S = persons of the batch = groups, one per person in input order:
    members int32 [S, max_patch] (batch crop indices of person i's group, target first, -1 behind group_len[i]), group_len int32 [S],
    relation {(stack, layer): [S, max_patch]}, image_relation {(stack, layer): [per image [P, P]]}, maps {(stack, layer): [S, max_patch, h r, w r]}"""

    def __init__(self, members, group_len, relation, image_relation, maps):
        self.members, self.group_len, self.relation, self.image_relation, self.maps = members, group_len, relation, image_relation, maps


HeadInput = collections.namedtuple("HeadInput", "feat heatmaps cin")  # what I2RModule.head_input returns


def _call_forward_hooks(module, output):
    """the module's forward hooks, called as a forward of it would (inputs: none -- the fused forward has no per-module call)"""
    for hid, hook in list(module._forward_hooks.items()):
        if hid in getattr(module, "_forward_hooks_with_kwargs", {}):
            hook(module, (), {}, output)
        else:
            hook(module, (), output)


def sine_position_embedding(h, w, d_model, temperature=10000.0, scale=2 * math.pi):
    """Fixed 2-D sine table [h*w, 1, d] the reference constructors store as a frozen parameter
    (interformer_pureMulti.py:516-541, transpose_h.py:502-527): cumsum coordinates normalised to (0, 2pi],
    frequencies temperature^(2*floor(i/2)/(d/2)), sin on even / cos on odd feature slots, y half then x half."""
    half = d_model // 2
    ys = torch.arange(1, h + 1, dtype=torch.float32) / (h + 1e-6) * scale
    xs = torch.arange(1, w + 1, dtype=torch.float32) / (w + 1e-6) * scale
    i = torch.arange(half, dtype=torch.float32)
    dim_t = temperature ** (2 * torch.div(i, 2, rounding_mode="floor") / half)

    def enc(v):  # [n] -> [n, half]
        a = v[:, None] / dim_t
        return torch.stack((a[:, 0::2].sin(), a[:, 1::2].cos()), dim=2).flatten(1)

    py = enc(ys)[:, None, :].expand(h, w, half)
    px = enc(xs)[None, :, :].expand(h, w, half)
    return torch.cat((py, px), dim=2).reshape(h * w, 1, d_model).contiguous()


class I2RModule(nn.Module):
    def __init__(self, cfg, spec=None):
        super().__init__()
        self.cfg = cfg
        # device -> Engine.  ONE dict object shared by every shallow copy of this module: nn.DataParallel.replicate() copies
        # __dict__ per forward, so replicas on other devices find the engine packed by an earlier forward instead of re-packing
        # all weights each time (tools/test.py:118 wraps the model in DataParallel).
        self._engines = {}
        self.precision = "fp32"  # MFMA operand type of the conv kernels: 'fp32' (reference parity), 'bf16', 'fp16'
        spec = arch.param_spec(cfg) if spec is None else spec
        for key, shape, dtype in spec:
            parts = key.split(".")
            mod = self
            for j, p in enumerate(parts[:-1]):
                if p not in mod._modules:
                    stack_layers = p == "layers" and ".".join(parts[:j]) in ATTN_STACKS
                    mod.add_module(p, nn.ModuleList() if stack_layers else nn.Module())
                mod = mod._modules[p]
            leaf = parts[-1]
            val = torch.from_numpy(synth.make_tensor(key, shape, dtype, seed=1234))
            if leaf in ("running_mean", "running_var", "num_batches_tracked") or dtype == "int64":
                mod.register_buffer(leaf, val)
            else:
                mod.register_parameter(leaf, nn.Parameter(val, requires_grad=False))
        self._init_sine_tables()
        # hook sites, listed once: the per-forward check is a look at these modules' hook dicts
        self._attn_sites, self._reduce_sites = [], []
        mods = dict(self.named_modules())
        for stack, red in ATTN_STACKS.items():
            layers = mods.get(stack + ".layers")
            if isinstance(layers, nn.ModuleList):
                self._attn_sites += [(stack, i, layers[i].self_attn) for i in range(len(layers)) if "self_attn" in layers[i]._modules]
                if red is not None and red in mods:
                    self._reduce_sites.append((stack, mods[red]))

    def _init_sine_tables(self):
        M = self.cfg["MODEL"]
        if M["POS_EMBEDDING"] != "sine":
            return
        w, h = M["IMAGE_SIZE"]
        for name, p in self.named_parameters():
            if name.endswith("pos_embedding"):
                r = M["HRNET_RES_LAYER"] if name.startswith("singleformer.") else 0
                hh, ww = h // 2 ** r // 4, w // 2 ** r // 4
                if p.shape[0] == hh * ww:
                    p.data.copy_(sine_position_embedding(hh, ww, p.shape[2]))

    # ---- engine lifecycle ----
    def set_precision(self, precision):
        """'fp32' (default: exact-fp32 MFMA, the 1e-3 parity mode), 'bf16' or 'fp16' (BASELINE configs 3-5: 16-bit MFMA
        operands, fp32 accumulation; the conv towers store their maps in 16 bit, token rows and the transformer blocks' residual
        stream stay fp32 in HBM)."""
        from ..engine import PRECISIONS
        assert precision in PRECISIONS, precision
        self.precision = precision
        self._invalidate()
        return self

    def _invalidate(self):
        self._engines.clear()

    def load_state_dict(self, state_dict, strict=True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._invalidate()
        return out

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self._invalidate()
        return out

    def _tensors(self):
        """name -> tensor of every parameter and persistent buffer (the state-dict keys).  Unlike state_dict() this also works on the
        replicas nn.DataParallel makes for devices 1.. : torch.nn.parallel.replicate() empties their `_parameters` and keeps the
        per-device copies as plain attributes, listed in `_former_parameters`."""
        out = {}
        for prefix, m in self.named_modules():
            pre = prefix + "." if prefix else ""
            src = dict(getattr(m, "_former_parameters", None) or {})
            src.update({k: v for k, v in m._parameters.items() if v is not None})
            for k, v in src.items():
                out[pre + k] = v
            for k, v in m._buffers.items():
                if v is not None and k not in m._non_persistent_buffers_set:
                    out[pre + k] = v
        return out

    def _device(self):
        """device of the first parameter (O(1) per forward; DataParallel replicas keep theirs in `_former_parameters`)"""
        for m in self.modules():
            for v in m._parameters.values():
                if v is not None:
                    return v.device
            for v in (getattr(m, "_former_parameters", None) or {}).values():
                if v is not None:
                    return v.device
        raise RuntimeError("module has no parameters")

    def engine(self):
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError(
                "i2r_amd models run on an MI355X through the HIP extension only; move the module to the GPU "
                "(model.cuda()) -- there is no CPU execution path in the product (the CPU oracle lives in oracle/).")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        eng = self._engines.get(dev)
        if eng is None:  # (cache miss only: walk the module tree for the full name -> tensor map the engine is packed from)
            from ..engine import Engine
            eng = self._engines[dev] = Engine(self.cfg, self._tensors(), dev, self.precision, name=self._engine_name())
        return eng

    def _engine_name(self):
        return None  # MODEL.NAME

    def forward_flip(self, x, pos_mask, length, flip_pairs):
        """Flip test of validate() (lib/core/function.py:142-162) in ONE batched forward: returns
        (model(x)['multi'] + flip_back(model(flip(x))['multi'], flip_pairs)) * 0.5 ."""
        from ..caller import joint_map
        if torch.is_tensor(length):
            length = length.tolist()
        eng = self.engine()
        jm = joint_map(flip_pairs, self.cfg["MODEL"]["NUM_JOINTS"]).to(eng.device)
        with torch.no_grad():
            return eng.forward(x, pos_mask, [int(n) for n in length], flip_joint_map=jm)

    def forward_main_target(self, x, pos_mask, length, boxes, max_patch=None, flip_pairs=None, share_first_stage=None, rollout=None):
        """The model side of the reference's grouped test mode (PATCH_MODE main_target: collater.get_max_patch + validate_main_target,
        lib/dataset/collater.py:35-51, lib/core/function.py:289-468): every person is the target of a group of itself and its
        min(n, max_patch) - 1 nearest neighbours in the image (input.main_target_groups, by the boxes' top-left corners), the model runs
        on the groups and only the target's heat maps are kept.  x, pos_mask, length: the ordinary collated batch; boxes: [S, >= 2]
        (x, y, ...) per crop; max_patch: default cfg.DATASET.MAX_PATCH; flip_pairs: merge with the flip test as forward_flip does.
        share_first_stage (Engine.forward_groups): None -- the HRNet-tower models share their first stage, every other model runs the
        expanded batch; True -- the TransPose-H / HRFormer first stages run once per person too (ValueError where the tail cannot take
        gathered rows); False -- always the expanded batch.
        -> [S, J, H/4, W/4], one row per person in input order, so decode / val_metrics / rescore_nms / oks_eval take it with the
        ordinary per-person centres and scales."""
        from ..input import main_target_groups
        if rollout is not None:
            raise ValueError("forward_main_target: rollout= is not served (no attention-map capture on the grouped forward)")
        if torch.is_tensor(length):
            length = length.tolist()
        length = [int(n) for n in length]
        if max_patch is None:
            max_patch = (self.cfg.get("DATASET") or {}).get("MAX_PATCH")
            if max_patch is None:
                raise ValueError("forward_main_target: max_patch is not given and the config has no DATASET.MAX_PATCH")
        eng = self.engine()
        jm = None
        if flip_pairs is not None:
            from ..caller import joint_map
            jm = joint_map(flip_pairs, self.cfg["MODEL"]["NUM_JOINTS"]).to(eng.device)
        assert x.shape[0] == sum(length), "sum(length)=%d != number of crops %d" % (sum(length), x.shape[0])
        with torch.no_grad():
            groups = main_target_groups(boxes, length, int(max_patch), eng.device)
            return eng.forward_groups(x, pos_mask, groups.members, groups.group_len, flip_joint_map=jm, share_first_stage=share_first_stage)

    def main_target_relations(self, x, pos_mask, length, boxes, max_patch=None, layers=None, maps=None, upsample=False, share_first_stage=None,
                              flip_pairs=None):
        """person_relations for the grouped test mode: forward_main_target's heat maps and, from the SAME forward, how much every person
        -- the target of its group -- attends to each member of the group, and where.  With P the head-averaged softmax(q k^T) of a layer
        of the inter-human stack over the group's members * h * w tokens, the target's tokens first:
          relation   r[j]    = mean over the target's tokens q of the sum over the tokens k of member j of P[q, k]      (sums to 1)
          dependency D_t[k]  = mean over the target's tokens q of P[q, k]: where the target looks, one map per member   (sums to 1)
          affect     F_t[j, q] = sum over the tokens k of member j of P[q, k]: the target's token q's share for member j (sum over j = 1)
        -- row 0 of what person_relations gives on the expanded batch (x[members], pos_mask[members], group_len), at 1 / m of its work.
        x, pos_mask, length, boxes, max_patch, share_first_stage: as forward_main_target; layers, maps, upsample: as person_relations.
        -> (heat maps [S, J, H/4, W/4], result): result.members int32 [S, max_patch] (row i: the batch crop indices of person i's group,
          target first, -1 behind result.group_len[i]); result.relation[(stack, layer)] [S, max_patch] (row i: r of person i's group, 0
          behind its members); result.image_relation[(stack, layer)] = a list with one [P_img, P_img] tensor per image, R[i, j] = r_i at
          j's slot where j is in i's group, 0 elsewhere (rows sum to 1; with max_patch >= P_img the grouped counterpart of
          person_relations' R); result.maps[(stack, layer)] [S, max_patch, h r, w r], slot s = the map on member s (dependency) or the
          target's own token map for member s (affect), zeros behind the group; empty without maps.  relation and maps are views of one
          buffer; nothing is read back from the device.
        ValueError: flip_pairs (the flip test is not served here), a stand-alone first stage, ATTENTION_TYPE window, a layer of another
        stack, a bad maps, and wherever forward_groups refuses.  Forward hooks are not served by this call."""
        from ..engine import TargetMaps
        from ..input import main_target_groups
        name = self._engine_name() or self.cfg["MODEL"]["NAME"]
        if flip_pairs is not None:
            raise ValueError("main_target_relations: flip_pairs is not served (no flip test on the grouped forward's relations)")
        if name in ("transpose_h", "hrformer", "hrnet"):
            raise ValueError("main_target_relations: %s has no inter-human stack" % name)
        if name == "interformer" and self.cfg["MODEL"]["ATTENTION_TYPE"] != "default":
            raise ValueError("main_target_relations: ATTENTION_TYPE %r has no encoder stack to capture" % (self.cfg["MODEL"]["ATTENTION_TYPE"],))
        if isinstance(maps, bool) or maps not in (None, "dependency", "affect"):
            raise ValueError("maps %r: None, 'dependency' or 'affect'" % (maps,))
        if torch.is_tensor(length):
            length = length.tolist()
        length = [int(n) for n in length]
        if max_patch is None:
            max_patch = (self.cfg.get("DATASET") or {}).get("MAX_PATCH")
            if max_patch is None:
                raise ValueError("main_target_relations: max_patch is not given and the config has no DATASET.MAX_PATCH")
        max_patch = int(max_patch)
        eng = self.engine()
        st = eng.inter_stack
        capture = {(st, i) for i in range(eng.capture_stacks().get(st, 0))} if layers is None else {(str(s), int(i)) for s, i in layers}
        other = sorted({s for s, _ in capture} - {st})
        if other or not capture:
            raise ValueError("main_target_relations: %s is not this model's inter-human stack %r" % (other or "an empty layer set", st))
        fh, fw = eng.capture_map_sizes(x.shape[2], x.shape[3])[st]
        scale = x.shape[2] // fh if upsample is True else max(int(upsample), 1)
        S = x.shape[0]
        assert S == sum(length), "sum(length)=%d != number of crops %d" % (sum(length), S)
        with torch.no_grad():
            groups = main_target_groups(boxes, length, max_patch, eng.device)
            out, (rel, views) = eng.forward_groups(x, pos_mask, groups.members, groups.group_len, share_first_stage=share_first_stage,
                                                   relations=TargetMaps(maps, scale, slots=max_patch), capture=capture)
            mh, mw = fh * scale, fw * scale
            relation = {k: v[0].as_strided((S, max_patch), (max_patch, 1)) for k, v in rel.items()}
            dense = {k: v[0].as_strided((S, max_patch, mh, mw), (max_patch * mh * mw, mh * mw, mw, 1)) for k, v in views.items()}
            # the tables, dense: slot s of group g at g * max_patch + s (index plumbing on the device, from host-made index tables)
            dev, glen = eng.device, groups.group_len
            slot = torch.tensor([g * max_patch + s for g, n in enumerate(glen) for s in range(n)], dtype=torch.long).to(dev)
            members = torch.full((S * max_patch,), -1, dtype=torch.int32, device=dev).index_copy_(0, slot, groups.members).view(S, max_patch)
            first = torch.tensor([o for b, n in enumerate(length) for o in [sum(length[:b])] * n], dtype=torch.long).to(dev)  # the image's first crop, per person
            col = (members.long() - first.view(S, 1)).clamp_(min=0)
            image_relation = {}
            for k, r in relation.items():  # (a slot behind the group adds its 0 to column 0: every (i, j) of a group is written once)
                big = torch.zeros(S, max(length), dtype=torch.float32, device=dev).scatter_add_(1, col, r * (members >= 0))
                image_relation[k] = [big[o:o + n, :n] for o, n in zip([sum(length[:b]) for b in range(len(length))], length)]
        return out, TargetRelations(members, torch.tensor(glen, dtype=torch.int32).to(dev), relation, image_relation, dense)

    def _hooked(self):
        """(stack, layer, self_attn module) of every layer with forward hooks on its self_attn (usually none)"""
        return [site for site in self._attn_sites if site[2]._forward_hooks]

    def _serve_hooks(self, hooked, maps, length=None):
        """call the hooks of the captured stacks' reduce modules (features [S, d, h, w]) and self_attn modules ((None, weights [batch, L, L]))"""
        stacks = {st for st, _, _ in hooked}
        for st, m in self._reduce_sites:
            if st in stacks and m._forward_hooks:
                _call_forward_hooks(m, maps[(st, "input")])
        for st, i, m in hooked:
            _call_forward_hooks(m, (None, pad_attention_maps(maps[(st, i)])))

    def _query_plan(self, eng, x, points, mode, layers, upsample, length=None):
        """-> (capture set, AttnQueries) for attention_at"""
        from ..engine import AttnQueries
        stacks = eng.capture_stacks()
        capture = {(st, i) for st, n in stacks.items() for i in range(n)} if layers is None else {(str(st), int(i)) for st, i in layers}
        H, W = x.shape[2], x.shape[3]
        sizes = eng.capture_map_sizes(H, W)
        pts = torch.as_tensor(points)
        if pts.dim() != 3 or pts.shape[0] != x.shape[0]:
            raise ValueError("points: shape %s, expected [%d crops, K, 2]" % (tuple(pts.shape), x.shape[0]))
        K = pts.shape[1]
        tokens, counts, scales = {}, {}, {}
        for st in sorted({st for st, _ in capture}):
            if st not in sizes:
                raise ValueError("attention_at: this model's encoder stacks are %s" % sorted(sizes))
            fh, fw = sizes[st]
            tok = points_to_tokens(pts, H, W, fh, fw)
            r = H // fh if upsample is True else max(int(upsample), 1)
            scales[st] = r
            if length is None or st.startswith("singleformer."):
                tokens[st], counts[st] = tok, None
            else:
                tokens[st], counts[st] = group_tokens(tok, length, fh * fw)
        return capture, AttnQueries(tokens, mode, scales, counts, capacity=K)

    @staticmethod
    def _query_result(maps, intra):
        """engine views -> per (stack, layer): [S, K, 1, h r, w r] for an intra-human stack (the per-crop blocks are consecutive in the
        capture buffer: a view), the per-image list [P K, P, h r, w r] for an inter-human one"""
        out = {}
        for key, views in maps.items():
            if key[1] == "input":
                continue
            if intra(key[0]):
                v = views[0]
                out[key] = v.as_strided((len(views),) + tuple(v.shape), (v.numel(),) + tuple(v.stride()), v.storage_offset())
            else:
                out[key] = views
        return out

    def _flip_map(self, eng, flip_pairs, flip_maps, who, default):
        """flip_pairs / flip_maps of an attention call -> (the engine's flip_joint_map or None, its flip_maps)"""
        if flip_maps not in ("plain", "merged"):
            raise ValueError("%s: flip_maps %r ('plain' or 'merged')" % (who, flip_maps))
        if flip_pairs is None:
            return None, "plain"
        if flip_maps == "plain" and default != "plain":
            raise ValueError("%s: with flip_pairs only flip_maps='merged' is served (the plain pass's maps: call without flip_pairs)" % who)
        from ..caller import joint_map
        return joint_map(flip_pairs, self.cfg["MODEL"]["NUM_JOINTS"]).to(eng.device), flip_maps

    def attention_at(self, x, pos_mask, length, points, mode="dependency", layers=None, upsample=True, flip_pairs=None, flip_maps="merged"):
        """The attention maps at query points, computed on the device without ever building an [L, L] map (the reference's
        visualize.py:186-233 / :333-388 reads exactly this of its hooks' output).
        points: [S, K, 2] holding (x, y) in the frame of each crop's network input (what visualize.py builds from preds); NaN = skip (a
          zero map), outside the crop: ValueError.  Token = (int(y / down_rate), int(x / down_rate)), down_rate = input height // feature
          height -- visualize.py:194-196; its :343 divides the width by the feature HEIGHT under a "TO CHECK" comment, which is not followed.
        mode: "dependency" (row: where the query point looks) or "affect" (column: which positions look at it).
        layers: set of (stack, layer), default every layer of every encoder stack.  upsample: True = by each stack's own down_rate (every
          stack comes back at input resolution: 4 for the intra-human and 16 for the inter-human stack of a 256 x 192 model), an int = that
          scale for every stack, False / 1 = the raw token maps.
        -> (model output, {(stack, layer): maps}): intra-human stack (the group is the crop) [S, K, 1, h r, w r]; inter-human stack (the
          group is the image, all its persons' points are queries, entry person * K + k) a list with one [P_img K, P_img, h r, w r] per image.
        flip_pairs: the flip test as forward_flip runs it -- the output is forward_flip's, and the maps are those of the flip test,
          M = (P + P~) / 2 with P~ the mirrored pass's map brought back into the plain frame (flip_maps="merged", the only choice here), in
          the same layout.  The points stay in the frame of the un-mirrored crop.
        Forward hooks keep working as before; this call serves none."""
        if torch.is_tensor(length):
            length = length.tolist()
        length = [int(n) for n in length]
        eng = self.engine()
        capture, queries = self._query_plan(eng, x, points, mode, layers, upsample, length)
        jm, flip_maps = self._flip_map(eng, flip_pairs, flip_maps, "attention_at", "merged")
        with torch.no_grad():
            out, maps = eng.forward(x, pos_mask, length, flip_joint_map=jm, capture=capture, queries=queries, flip_maps=flip_maps)
        return out, self._query_result(maps, lambda st: st.startswith("singleformer."))

    def attention_at_joints(self, x, pos_mask, length, mode="dependency", layers=None, upsample=True, flip_pairs=None, flip_maps="plain"):
        """The attention maps at the joints this very forward predicts, in ONE forward and without a trip to the host -- the flow the
        reference's visualize.py is written for (its columns are labelled keypoint_name[p_id]: the query locations are a pose).  The
        same as `out = model(x, ...)`, `joints = 4 * argmax(out)`, `attention_at(x, ..., points=joints.cpu())`, but the second forward and
        the copy are gone: i2r_joint_tokens turns the heat maps into the token tables on the device (the arg-max of i2r_decode: first
        index on a tie, the point (0, 0) for a map without a positive value -- get_max_preds, lib/core/inference.py:20-48) and the query
        launches of the captured layers run behind the head.
        mode, layers, upsample: as attention_at.  flip_pairs: the flip test as forward_flip runs it -- the joints come from the MERGED
        heat maps; the attention maps with flip_maps="plain" from the plain pass alone (the mirrored pass's maps are not computed), with
        flip_maps="merged" from both passes, M = (P + P~) / 2 as attention_at defines it, queried at the same joints.
        -> (output, joints, maxvals, maps): output exactly what forward (forward_flip with flip_pairs) returns; joints [S, J, 2] holding
          (x, y) in the frame of each crop's network input and maxvals [S, J], device tensors, of output['multi'] when it is a dict; maps
          as attention_at returns them with K = J (inter-human stack: entry person * J + joint).
        Cost: every captured layer keeps its fp32 q|k activation [tokens, 2 * heads * head size] until the program ends.
        ValueError: a model without encoder stacks, ATTENTION_TYPE window.  Not served: the stand-alone first stages, the grouped
        forward, the per-person form.  Forward hooks keep working as before; this call serves none."""
        from ..engine import JointQueries
        name = self._engine_name() or self.cfg["MODEL"]["NAME"]
        if name in ("transpose_h", "hrformer", "hrnet"):
            raise ValueError("attention_at_joints: the stand-alone stage %s is not served" % name)
        if torch.is_tensor(length):
            length = length.tolist()
        length = [int(n) for n in length]
        eng = self.engine()
        stacks = eng.capture_stacks()
        capture = {(st, i) for st, n in stacks.items() for i in range(n)} if layers is None else {(str(st), int(i)) for st, i in layers}
        H, W = x.shape[2], x.shape[3]
        sizes = eng.capture_map_sizes(H, W)
        scales = {st: (H // sizes[st][0] if upsample is True else max(int(upsample), 1)) for st in {st for st, _ in capture} if st in sizes}
        jm, flip_maps = self._flip_map(eng, flip_pairs, flip_maps, "attention_at_joints", "plain")
        with torch.no_grad():
            out, (joints, maxvals, maps) = eng.forward(x, pos_mask, length, flip_joint_map=jm, capture=capture, joints=JointQueries(mode, scales),
                                                       flip_maps=flip_maps)
        return out, joints, maxvals, self._query_result(maps, lambda st: st.startswith("singleformer."))

    def person_relations(self, x, pos_mask, length, layers=None, maps=None, upsample=False, flip_pairs=None, flip_maps="merged"):
        """The inter-human attention per person, computed on the device without ever building an [L, L] map: how much person i attends to
        person j, and where on j it looks.  With P the head-averaged softmax(q k^T) of a layer of the inter-human stack over the image's
        persons * h * w tokens (what the forward hooks get):
          relation   R[i, j] = mean over the tokens q of person i of the sum over the tokens k of person j of P[q, k]   (rows sum to 1)
          dependency D[i, k] = mean over the tokens q of person i of P[q, k]: where person i looks                     (rows sum to 1)
          affect     F[j, q] = sum over the tokens k of person j of P[q, k]: token q's share for person j              (sum over j = 1)
        layers: set of (stack, layer) of the inter-human stack (Engine.inter_stack), default all its layers; maps: None, "dependency" or
        "affect"; upsample: True = by the stack's own down_rate (input resolution), an int = that scale, False / 1 = the raw token maps.
        -> (model output, result): result.relation[(stack, layer)] = a list with one [P_img, P_img] tensor per image;
          result.maps[(stack, layer)] = a list with one [P_img, P_img, h r, w r] tensor per image -- first index i (dependency) or j
          (affect), second index the person whose token map it is; empty without maps.  All are views of one buffer.
        flip_pairs: the flip test as forward_flip runs it -- the output is forward_flip's, and with P' the mirrored pass's map and mu the
          mirror of a token: R_m = (R + R') / 2, D_m[i, k] = (D[i, k] + D'[i, mu(k)]) / 2, F_m[j, q] = (F[j, q] + F'[j, mu(q)]) / 2 (sums over
          whole persons are mirror-invariant; flip_maps="merged" is the only choice here); the identities above hold for them as well.
        ValueError: a stand-alone first stage (no inter-human stack), ATTENTION_TYPE window, a layer of another stack.
        Forward hooks keep working as before; this call serves none."""
        from ..engine import PersonMaps
        name = self._engine_name() or self.cfg["MODEL"]["NAME"]
        if name in ("transpose_h", "hrformer", "hrnet"):
            raise ValueError("person_relations: %s has no inter-human stack" % name)
        if name == "interformer" and self.cfg["MODEL"]["ATTENTION_TYPE"] != "default":
            raise ValueError("person_relations: ATTENTION_TYPE %r has no encoder stack to capture" % (self.cfg["MODEL"]["ATTENTION_TYPE"],))
        if maps not in (None, "dependency", "affect"):
            raise ValueError("maps %r: None, 'dependency' or 'affect'" % (maps,))
        if torch.is_tensor(length):
            length = length.tolist()
        length = [int(n) for n in length]
        eng = self.engine()
        st = eng.inter_stack
        capture = {(st, i) for i in range(eng.capture_stacks().get(st, 0))} if layers is None else {(str(s), int(i)) for s, i in layers}
        if upsample is True:
            upsample = x.shape[2] // eng.capture_map_sizes(x.shape[2], x.shape[3])[st][0]
        jm, flip_maps = self._flip_map(eng, flip_pairs, flip_maps, "person_relations", "merged")
        with torch.no_grad():
            out, (rel, views) = eng.forward(x, pos_mask, length, flip_joint_map=jm, capture=capture, persons=PersonMaps(maps, max(int(upsample), 1)),
                                            flip_maps=flip_maps)
        return out, PersonRelations(rel, views)

    def _rollout_served(self, who, flip_pairs):
        """the refusals of a roll-out call that need no engine"""
        if flip_pairs is not None:
            raise ValueError("%s: flip_pairs is not served (a product of merged maps is not the merge of products)" % who)
        name = self._engine_name() or self.cfg["MODEL"]["NAME"]
        if name in ("transpose_h", "hrformer", "hrnet"):
            raise ValueError("%s: the stand-alone stage %s is not served" % (who, name))
        if name == "interformer" and self.cfg["MODEL"]["ATTENTION_TYPE"] != "default":
            raise ValueError("%s: ATTENTION_TYPE %r has no encoder stack to capture" % (who, self.cfg["MODEL"]["ATTENTION_TYPE"]))

    @staticmethod
    def _rollout_capture(have, who, stacks, layers):
        """stacks / layers of a roll-out call, have = the engine's capture_stacks() -> the capture set: every layer lo .. hi of every chosen stack"""
        chosen = sorted(have) if stacks is None else [str(st) for st in ([stacks] if isinstance(stacks, str) else stacks)]
        for st in chosen:
            if st not in have:
                raise ValueError("%s: this model's encoder stacks are %s, not %r" % (who, sorted(have), st))
        if layers is None:
            layers = {st: (0, have[st] - 1) for st in chosen}
        elif not isinstance(layers, dict):
            if len(layers) == 2 and all(isinstance(i, int) for i in layers):
                layers = {st: tuple(layers) for st in chosen}
            else:  # a set of (stack, layer): it has to be a range per stack (attn_capture.RolloutForm checks)
                return {(str(st), int(i)) for st, i in layers}
        capture = set()
        for st, (lo, hi) in layers.items():
            if str(st) not in have or not 0 <= int(lo) <= int(hi) < have[str(st)]:
                raise ValueError("%s: layers (%r, %r) of %r; this model's encoder stacks are %s" % (who, lo, hi, st, have))
            capture |= {(str(st), i) for i in range(int(lo), int(hi) + 1)}
        return capture

    def rollout_at(self, x, pos_mask, length, points, mode="dependency", stacks=None, layers=None, alpha=0.5, upsample=True, flip_pairs=None):
        """The attention roll-out (Abnar & Zuidema 2020) at query points: the relations THROUGH the encoder layers lo .. hi of a stack,
        computed on the device without ever building an [L, L] map.  With P_l the head-averaged softmax(q k^T) of layer l (what the
        forward hooks get),  A_l = (1 - alpha) I + alpha P_l  and  T = A_hi A_hi-1 ... A_lo  (rows sum to 1): T[q, k] is how much output
        token q of layer hi draws on input token k of layer lo.
        points, the token rule, NaN = skip, outside the crop = ValueError, mode, upsample: exactly as attention_at -- "dependency" gives
          the row T[q, :] (where the query point's output comes from), "affect" the column T[:, q] (which outputs draw on it).
        stacks: the encoder stacks to roll out, default all; layers: None = every layer of each, (lo, hi) for all of them or
          {stack: (lo, hi)}; a set of (stack, layer) with a hole is a ValueError.  alpha in [0, 1]: the weight of the attention against the
          residual path (0.5 is the paper's).  With lo == hi and alpha = 1 the result is attention_at's of that layer.
        -> (model output, {stack: maps}), maps as attention_at returns them for ONE layer.
        ValueError: flip_pairs (a product of merged maps is not the merge of products; the definition is left open), points that are not
        given (predicted-joint queries), ATTENTION_TYPE window, the stand-alone first stages.  Forward hooks keep working; this call serves none."""
        from ..engine import Rollout
        self._rollout_served("rollout_at", flip_pairs)
        if points is None or isinstance(points, str):
            raise ValueError("rollout_at: points %r -- predicted-joint queries are not served; pass [S, K, 2] points" % (points,))
        if torch.is_tensor(length):
            length = length.tolist()
        length = [int(n) for n in length]
        eng = self.engine()
        capture = self._rollout_capture(eng.capture_stacks(), "rollout_at", stacks, layers)
        capture, q = self._query_plan(eng, x, points, mode, capture, upsample, length)
        with torch.no_grad():
            out, maps = eng.forward(x, pos_mask, length, capture=capture, rollout=Rollout(q.tokens, mode, alpha, q.upsample, q.counts, q.capacity))
        maps = self._query_result({(st, 0): v for st, v in maps.items()}, lambda st: st.startswith("singleformer."))
        return out, {st: v for (st, _), v in maps.items()}

    def person_rollout(self, x, pos_mask, length, maps=None, layers=None, alpha=0.5, upsample=False, flip_pairs=None):
        """The attention roll-out of the inter-human stack per person: person_relations' three reductions of T = A_hi ... A_lo (rollout_at)
        instead of one layer's map --
          relation   R_T[i, j] = mean over the tokens q of person i of the sum over the tokens k of person j of T[q, k]   (rows sum to 1)
          dependency D_T[i, k] = mean over the tokens q of person i of T[q, k]                                          (rows sum to 1)
          affect     F_T[j, q] = sum over the tokens k of person j of T[q, k]                                            (sum over j = 1)
        i.e. how much person i's output, after the layers lo .. hi, draws on person j's input, and where.
        maps, upsample: as person_relations; layers: None = all layers of the stack, or (lo, hi); alpha: as rollout_at.
        -> (model output, result): result.relation[stack] = a list with one [P_img, P_img] tensor per image; result.maps[stack] = a list
          with one [P_img, P_img, h r, w r] tensor per image (empty without maps).  All are views of one buffer.
        ValueError: flip_pairs, ATTENTION_TYPE window, the stand-alone first stages, a layer of another stack."""
        self._rollout_served("person_rollout", flip_pairs)
        if maps not in (None, "dependency", "affect"):
            raise ValueError("maps %r: None, 'dependency' or 'affect'" % (maps,))
        from ..engine import Rollout
        if torch.is_tensor(length):
            length = length.tolist()
        length = [int(n) for n in length]
        eng = self.engine()
        capture = self._rollout_capture(eng.capture_stacks(), "person_rollout", [eng.inter_stack], layers)
        if upsample is True:
            upsample = x.shape[2] // eng.capture_map_sizes(x.shape[2], x.shape[3])[eng.inter_stack][0]
        with torch.no_grad():
            out, (rel, views) = eng.forward(x, pos_mask, length, capture=capture, rollout=Rollout(None, maps, alpha, max(int(upsample), 1)))
        return out, PersonRelations(rel, views)

    def head_input(self, x, pos_mask, length):
        """The forward, and with it the tensor final_layer reads: what a head re-fit on frozen features trains on (caller.HeadFit,
        caller.head_grad).  -> HeadInput(feat, heatmaps, cin): feat [S, h, w, cs] fp32 NHWC, a fresh tensor (channels cin .. cs - 1 are
        the engine's zero padding), heatmaps [S, J, h, w] = forward's 'multi', cin = final_layer's true input channel count.
        Served in every precision mode (the head's input is fp32 in all of them).  ValueError: FINAL_CONV_KERNEL 3, ATTENTION_TYPE
        window, a model class without the inter-human tail.  Forward hooks are not served by this call."""
        if torch.is_tensor(length):
            length = length.tolist()
        with torch.no_grad():
            hm, feat = self.engine().forward_head_input(x, pos_mask, [int(n) for n in length])
        return HeadInput(feat, hm, int(self._tensors()["final_layer.weight"].shape[1]))

    def forward(self, x, pos_mask, length):
        """model(input, pos_mask, length) -- reference lib/core/function.py:135.  With forward hooks on <stack>.layers[i].self_attn the
        same forward also computes those layers' attention maps and serves them to the hooks (visualize.py); without, the default path."""
        if torch.is_tensor(length):
            length = length.tolist()
        length = [int(n) for n in length]
        hooked = self._hooked()
        with torch.no_grad():
            if not hooked:
                return self.engine().forward(x, pos_mask, length)
            out, maps = self.engine().forward(x, pos_mask, length, capture={(st, i) for st, i, _ in hooked})
            self._serve_hooks(hooked, maps, length)
            return out
