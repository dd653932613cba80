"""The forms of an attention-map capture (Engine.forward(..., capture=, queries=, persons=)): full [L, L] maps, their rows / columns at
query points, their reductions per person, the roll-out through all captured layers of a stack (rollout=), and the target form of the
grouped forward (Engine.forward_groups(..., capture=, relations=)).  A form knows its program key, the launch a captured layer emits, the layout of one call
(plan: integers only -- sizes, offsets and tile counts as include/i2r_hip.h specifies them), the per-call fields of a launch (patch) and
the shape of what the caller gets back, and which pair of attn_bind.py does its work behind the program's head (behind).  Nothing here
touches a device or the library: Program.bind_capture (engine.py) and attn_bind.py do, for all of them.
"""
import collections
import dataclasses
import math

import torch

from . import cabi

AW_KEYS = 128  # key block of the attention-map kernels (csrc/i2r_encoder_mh.hip kAwKeys)


class AttnQueries:
    """The query form of an attention-map capture (Engine.forward(..., capture=, queries=)).
    tokens: {stack: int32 [groups, K]} token indices inside each group of that stack (intra-human: the crop's y * w + x; inter-human: the
            image's (person * h + y) * w + x), -1 = skip (an all-zero row); counts: optionally {stack: entries used per group};
    mode: 0 / "dependency" (rows: what the query token attends to) or 1 / "affect" (columns: who attends to it);
    upsample: integer bilinear scale of the returned maps (1 = raw), or {stack: scale} when the stacks differ (each stack's down_rate);
    capacity: the K a program is keyed by (default: the widest table) -- calls that differ only in points or grouping share a program."""
    MODES = {"dependency": 0, "affect": 1, 0: 0, 1: 1}

    def __init__(self, tokens, mode="dependency", upsample=1, counts=None, capacity=None):
        if mode not in self.MODES:
            raise ValueError("mode %r: 'dependency' or 'affect'" % (mode,))
        self.tokens, self.mode, self.counts = dict(tokens), self.MODES[mode], counts
        self.upsample = {st: int(r) for st, r in upsample.items()} if isinstance(upsample, dict) else int(upsample)
        self.capacity = int(capacity) if capacity is not None else max(int(torch.as_tensor(t).shape[-1]) for t in self.tokens.values())


class PersonMaps:
    """The per-person form of an attention-map capture (Engine.forward(..., capture=, persons=)): of every captured layer of the
    inter-human stack the relation matrix R[i, j] (how much of person i's attention lands on person j) per image, and with
    mode: 0 / None nothing else, 1 / "dependency" the maps D[i] (where person i looks, averaged over its tokens), 2 / "affect" the maps
    F[j] (the share of every token's attention that lands on person j); upsample: integer bilinear scale of those maps (1 = raw)."""
    MODES = {None: 0, "dependency": 1, "affect": 2, 0: 0, 1: 1, 2: 2}

    def __init__(self, mode=None, upsample=1):
        if isinstance(mode, bool) or mode not in self.MODES:
            raise ValueError("mode %r: None, 'dependency' or 'affect'" % (mode,))
        self.mode, self.upsample = self.MODES[mode], int(upsample)
        if not 1 <= self.upsample <= 64:
            raise ValueError("upsample %r (1 .. 64)" % (upsample,))


class TargetMaps:
    """The target form of an attention-map capture (Engine.forward_groups(..., capture=, relations=)): of every captured layer of the
    inter-human stack, per person group, the relations of the group's TARGET (its first member, the one grouped inference keeps) to the
    group's members -- r[j], how much of the target's attention lands on member j -- and with
    maps: None nothing else, "dependency" the maps D_t[j] (where on member j the target looks, averaged over the target's tokens),
    "affect" the maps F_t[j] (which of the target's own tokens look at member j); scale: integer bilinear scale of those maps (1 = raw);
    slots: members per group the call's buffer is laid out for (every group's blocks are `slots` entries apart, zeros behind its own
    members: the layers' blocks are dense [groups, slots, ...] tensors); default: the largest group of the call."""
    MODES = {None: 0, "dependency": 1, "affect": 2}

    def __init__(self, maps=None, scale=1, slots=None):
        if isinstance(maps, bool) or maps not in self.MODES:
            raise ValueError("maps %r: None, 'dependency' or 'affect'" % (maps,))
        self.maps, self.mode, self.scale = maps, self.MODES[maps], int(scale)
        if not 1 <= self.scale <= 64:
            raise ValueError("scale %r (1 .. 64)" % (scale,))
        self.slots = int(slots) if slots is not None else None
        if self.slots is not None and self.slots < 1:
            raise ValueError("slots %r (>= 1)" % (slots,))


class JointQueries:
    """The joint form of an attention-map capture (Engine.forward(..., capture=, joints=)): the query form whose points are the joints
    the SAME forward predicts.  The token tables are made on the device from the call's own (flip-merged) heat maps -- arg-max of every
    map as i2r_decode takes it, x 4, (int(y / down_rate), int(x / down_rate)) -- by i2r_joint_tokens, and the i2r_attn_query_maps
    launches run behind the head instead of inside their layers: no second forward, no copy to the host.  K = the model's joints; the
    inter-human stack gets all joints of all persons of the image as queries (entry person * J + j), as AttnQueries does with points.
    mode, upsample: as AttnQueries.  Cost: every captured layer keeps its fp32 q|k activation [tokens, 2 hs] until the program ends."""

    def __init__(self, mode="dependency", upsample=1):
        if mode not in AttnQueries.MODES:
            raise ValueError("mode %r: 'dependency' or 'affect'" % (mode,))
        self.mode = AttnQueries.MODES[mode]
        self.upsample = {st: int(r) for st, r in upsample.items()} if isinstance(upsample, dict) else int(upsample)


class Rollout:
    """The roll-out form of an attention-map capture (Engine.forward(..., capture=, rollout=)): the relations THROUGH the captured layers
    lo .. hi of a stack (a contiguous range) instead of the maps of each.  With P_l the head-averaged softmax(q k^T) of layer l,
      A_l = (1 - alpha) I + alpha P_l,  T = A_hi A_hi-1 ... A_lo  (rows sum to 1; Abnar & Zuidema 2020),
    T[q, k] is how much output token q of layer hi draws on input token k of layer lo (include/i2r_hip.h: i2r_attn_rollout_step).
    tokens given ({stack: int32 [groups, K]}, counts, capacity: as AttnQueries): rows T[q, :] (mode 0 / "dependency") or columns T[:, q]
      (mode 1 / "affect") at the query tokens, up-sampled by `upsample` (an int, or {stack: scale});
    tokens None: the per-person reductions of the inter-human stack -- the relation R_T [P, P] per image, and with mode 1 / "dependency"
      the maps D_T[i, k] = mean_{q in i} T[q, k], 2 / "affect" F_T[j, q] = sum_{k in j} T[q, k] (mode 0 / None: none), as PersonMaps."""

    def __init__(self, tokens=None, mode="dependency", alpha=0.5, upsample=1, counts=None, capacity=None):
        self.points = tokens is not None
        modes = AttnQueries.MODES if self.points else PersonMaps.MODES
        if isinstance(mode, bool) or mode not in modes:
            raise ValueError("mode %r: %s" % (mode, "'dependency' or 'affect'" if self.points else "None, 'dependency' or 'affect'"))
        alpha = float(alpha)
        if not 0.0 <= alpha <= 1.0:  # (NaN too)
            raise ValueError("alpha %r (0 .. 1)" % (alpha,))
        self.tokens, self.mode, self.alpha, self.counts = dict(tokens) if self.points else None, modes[mode], alpha, counts
        self.upsample = {st: int(r) for st, r in upsample.items()} if isinstance(upsample, dict) else int(upsample)
        self.capacity = 0
        if self.points:
            self.capacity = int(capacity) if capacity is not None else max(int(torch.as_tensor(t).shape[-1]) for t in self.tokens.values())


# One set of blocks of a layer's part of the per-call buffer: group g's block starts offs[g] floats behind the set, the set `base` floats
# behind the layer; shapes: the view of every group's block, None for a set nobody reads (person maps in mode 0).
Block = collections.namedtuple("Block", "offs base shapes")


@dataclasses.dataclass
class Plan:
    """what one capture (the captured layers of one stack) needs for one call"""
    n_grp: int
    ws_stride: int     # floats per workspace row: 2 * heads * ceil(max L / 128)
    ws_floats: int
    rows_floats: int   # the raw rows before up-sampling / the per-person rows (0: the form has none)
    blocks: list       # [Block]: full and query maps one set, person maps two (relations, maps)
    layer_floats: int  # every set and every layer starts on a 16-byte boundary
    n_tiles: int = 0
    n_col_tiles: int = 0
    K: int = 1
    # host int32 tensors the launches read on the device (query maps: tokens [groups, K], counts [groups]); a shape instead of a tensor:
    # an int32 table of that shape which the device fills itself (joint form: the tokens; its third table maps crops to entries)
    tables: tuple = ()
    # a merged form (Form.merge) only: the scale-1 layout of the maps both passes write before i2r_attn_flip_merge -- group g's raw
    # [rows_g, L_g] block starts raw_offs[g] floats behind either workspace of raw_floats floats
    raw_offs: tuple = ()
    raw_floats: int = 0
    # the roll-out form only: floats behind the capture's block sets (its two working matrices), and the seed of the chain: (int64 flat
    # indices into a working matrix, the value they get; everything else is 0)
    extra_floats: int = 0
    seed: tuple = ()


@dataclasses.dataclass
class Capture:
    """one captured encoder stack of a program (Program.captures): made when the stack is emitted, bound per call by Program.bind_capture"""
    stack: str
    x: object               # the stack's input activation: its token map is x.h x x.w, of x.n crops
    off: list               # per block set of the form an int64 device table [x.n]: where every group's block starts
    ops: list = dataclasses.field(default_factory=list)  # [(layer, args)]: the launch of every captured layer
    grouping: dict = None   # the stack's grouping record (Program.set_groups)
    tables: list = None     # this call's Plan.tables on the device
    base: int = 0           # floats of this call's buffer in front of the capture's first block
    call: object = None     # what the form's work behind the head needs of this call (attn_bind: Merge, Chain)


@dataclasses.dataclass
class Merge:
    """a merged form's call on one capture (attn_bind.bind_merge)"""
    tok: tuple      # the token table of the plain and of the mirrored half (None, None: the per-person form has none)
    rel: list       # the per-person form: the relation workspace of either half, else None
    # per captured layer (the plain half's launch args, the mirrored half's, its AttnFlipMergeArgs or 0: a form without maps, its relation
    # blocks in the buffer or None)
    layers: list = dataclasses.field(default_factory=list)


@dataclasses.dataclass
class Chain:
    """the roll-out form's call on one capture (attn_bind.bind_rollout)"""
    X0: object      # the first working matrix, seeded with `value` at the flat indices `seed`
    seed: object
    value: float
    steps: list     # the AttnRolloutArgs in chain order
    rel: list       # per person: per group (the raw rows [P, P, h w], the relation block [P, P] they reduce into), else None


def _layer(*sets):
    """per block set the view shape of every group (None: a block of no floats) -> ([Block], floats per layer)"""
    blocks, base = [], 0
    for shapes in sets:
        offs = [0]
        for s in shapes:
            offs.append(offs[-1] + (math.prod(s) if s else 0))
        blocks.append(Block(offs, base, shapes if shapes[0] else None))
        base += -(-offs[-1] // 4) * 4
    return blocks, base


def _stride(heads, lens):
    return 2 * heads * -(-max(lens) // AW_KEYS)


def _tiles(rows, keys, key_tile=AW_KEYS):
    """one wave per (16-row tile, key block) of every group"""
    return sum(-(-r // 16) * -(-k // key_tile) for r, k in zip(rows, keys))


def _query_tables(call, stack, lens):
    """the validated tables of a call with query tokens (AttnQueries, Rollout) -> (tokens int32 [groups, K] on the host, K, entries per group)"""
    tok = torch.as_tensor(call.tokens[stack]).to("cpu", torch.int32).contiguous()
    if tok.dim() != 2 or tok.shape[0] != len(lens) or tok.shape[1] < 1:
        raise ValueError("query tokens of %r: shape %s, expected [%d groups, K]" % (stack, tuple(tok.shape), len(lens)))
    K = tok.shape[1]
    cnt = getattr(call, "counts", None)
    cnt = [int(c) for c in cnt[stack]] if cnt and cnt.get(stack) is not None else [K] * len(lens)
    if len(cnt) != len(lens) or not all(1 <= c <= K for c in cnt):
        raise ValueError("query counts of %r: %s for %d groups of up to %d entries" % (stack, cnt, len(lens), K))
    for g, (n, c) in enumerate(zip(lens, cnt)):
        if int(tok[g, :c].max()) >= n:
            raise ValueError("query token %d of group %d of %r is outside its %d tokens" % (int(tok[g, :c].max()), g, stack, n))
    return tok, K, cnt


class Form:
    """what the forms share; a form is made per call (resolve), and a program keeps the one it was built with"""
    N_BLOCKS = 1  # block sets per layer = device offset tables per capture
    call = None   # what bind_capture hands to plan() per call
    deferred = False  # True: a captured layer keeps its q|k and emits nothing; the engine runs the form's launches behind the program
    merged = False    # True (merge()): the maps of the flip test, M = (P + un-mirrored P') / 2 (i2r_attn_flip_merge)
    per_stack = False  # True: the captured layers of a stack share ONE set of blocks (their product), not one each
    zero_fill = False  # True: the blocks of a call are laid out with gaps the caller reads as zeros -- the per-call buffer starts zeroed
    J = None           # the joint form: the model's joints -- its token tables are made on the device behind the head (i2r_joint_tokens)
    # every form: entry, the C entry point of its launch; a form that can be merged: HALF, the fields of its launch args that differ between
    # the halves of the flip program -- (q|k rows, token table, workspace of the raw maps, their offsets, relation workspace), None: no such field

    def __init__(self, capture, suffix=()):
        self.capture, self.key = capture, ("capture", capture) + suffix  # (key: the part of the program key behind the shape)

    # the bind / run pair of attn_bind.py that does this form's work behind the program's head; None: every launch is in the program
    behind = property(lambda self: "rollout" if self.per_stack else "merge" if self.merged else "launches" if self.deferred else None)

    def begin(self, stack, x, table):  # -> the Capture of a stack a program emits; table() makes one device offset table
        return Capture(stack, x, [table() for _ in range(self.N_BLOCKS)])

    share = staticmethod(lambda plans: None)  # what the plans of all captures of a call must agree on, once they are made: nothing
    sets = staticmethod(lambda cap: len(cap.ops))  # the sets of blocks a capture has in the per-call buffer: one per captured layer

    def merge(self):
        """This form under the flip test with flip_maps="merged": the program is the flip program, whose stacks run the mirrored crops as
        a second half of doubled groups.  Every captured layer keeps its q|k; behind the program the form's launch runs at scale 1 on the
        plain half and, with the mirrored token table, on the mirrored half, both into workspaces laid out by Plan.raw_offs, and
        i2r_attn_flip_merge writes the merged, up-sampled maps into the capture buffer.  The key gains a marker."""
        self.merged = self.deferred = True
        self.key = self.key + ("flip-merged",)
        return self

    def _raw(self, p, rows, lens):
        """fills in the scale-1 layout of a merged form's plan p: rows[g] x lens[g] floats per group"""
        if self.merged:
            (blk,), p.raw_floats = _layer([(r, n) for r, n in zip(rows, lens)])
            p.raw_offs = tuple(blk.offs[:-1])
        return p

    @staticmethod
    def result(views, inputs, behind=None):
        """views: per block set {(stack, layer): per group a view}; inputs(): {(stack, "input"): features}; behind: what the run of the
        form's pair returned -> what the caller gets"""
        return {**views[0], **inputs()}


def _scales(who, up, stacks):
    """upsample of a call (an int, or {stack: scale}) -> ((stack, scale), ...) of the captured stacks"""
    try:
        return tuple((st, int(up[st] if isinstance(up, dict) else up)) for st in stacks)
    except KeyError as e:
        raise ValueError("%s.upsample has no scale for stack %s" % (who, e))


class FullForm(Form):
    """[L, L] maps (i2r_attn_weights)"""
    entry = "i2r_attn_weights"

    def launch(self, cap, qk, L, goff):
        """-> (op kind, args) of one captured layer: cap its Capture, qk its q|k activation, L its pack; patch() fills in the rest"""
        return cabi.CAPTURE_OP_ATTN_WEIGHTS, cabi.AttnWeightsArgs(qk.ptr, 0, goff.data_ptr(), cap.off[0].data_ptr(), 0, 0, L["heads"], L["hp"],
                                                                  L["hs"], qk.cs, 0, 0)

    def plan(self, stack, hw, lens, heads, call=None):
        """hw: the stack's token map (h, w); lens: tokens of every group to compute; heads: the widest head count among the launches"""
        blocks, n_layer = _layer([(n, n) for n in lens])
        stride = _stride(heads, lens)
        return Plan(len(lens), stride, stride * sum(lens), 0, blocks, n_layer, n_tiles=_tiles(lens, lens))

    @staticmethod
    def share(plans):
        """the i2r_attn_weights launches of all captures read ONE stride, the widest, and the workspace has the most rows of any at it"""
        stride, rows = max(p.ws_stride for p in plans), max(p.ws_floats // p.ws_stride for p in plans)
        for p in plans:
            p.ws_stride, p.ws_floats = stride, rows * stride

    @staticmethod
    def patch(a, p, out, ws, rows, tables, host_off):
        """the per-call fields of a launch: p its capture's plan, out its layer in the buffer, ws / rows / p.tables on the device, the host's group offsets"""
        a.out, a.ws = out, ws
        a.n_grp, a.n_tiles, a.ws_stride = p.n_grp, p.n_tiles, p.ws_stride


class QueryForm(Form):
    """rows (mode 0) / columns (mode 1) of the maps at query points, up-sampled by the stack's scale (i2r_attn_query_maps): no [L, L]
    block exists, the workspaces are O(K L)"""
    entry, HALF = "i2r_attn_query_maps", ("qk", "q_tok", "out", "out_off", None)

    def __init__(self, capture, queries):
        mode, stacks = int(queries.mode), sorted({st for st, _ in capture})
        missing = set(stacks) - set(queries.tokens)
        if missing:
            raise ValueError("queries.tokens has no table for %s" % sorted(missing))
        scales = _scales("queries", queries.upsample, stacks)
        if mode not in (0, 1) or not all(1 <= r <= 64 for _, r in scales):
            raise ValueError("queries: mode %r (0 dependency, 1 affect), upsample %r (1 .. 64)" % (queries.mode, queries.upsample))
        Form.__init__(self, capture, ("query", mode, int(queries.capacity), scales))
        self.call, self.mode, self.scales = queries, mode, dict(scales)

    def launch(self, cap, qk, L, goff):
        return cabi.CAPTURE_OP_ATTN_QUERY, cabi.AttnQueryArgs(
            qk=qk.ptr, grp_off=goff.data_ptr(), out_off=cap.off[0].data_ptr(), heads=L["heads"], hp=L["hp"], k_off=L["hs"], qk_cs=qk.cs,
            mode=self.mode, K=1, scale=1 if self.merged else self.scales[cap.stack], h=cap.x.h, w=cap.x.w)

    def plan(self, stack, hw, lens, heads, call=None):
        """call: the AttnQueries of this call -- tokens[stack] int32 [groups, K] (-1 = skip), optionally counts[stack] (entries per group)"""
        tok, K, cnt = _query_tables(call, stack, lens)
        return self._layout(self.scales[stack], hw, lens, heads, K, cnt, (tok, torch.tensor(cnt, dtype=torch.int32)))

    def _layout(self, scale, hw, lens, heads, K, cnt, tables):
        """the plan of groups of lens tokens that use cnt of the K entries of their table rows"""
        mode, (h, w) = self.mode, hw
        assert all(n % (h * w) == 0 for n in lens)
        blocks, n_layer = _layer([(c, n // (h * w), h * scale, w * scale) for n, c in zip(lens, cnt)])
        stride = _stride(heads, lens)
        tiles = (_tiles(cnt, lens), 0) if mode == 0 else (_tiles(lens, lens), _tiles(lens, cnt, 16))
        rows = K * sum(lens) if scale > 1 and not self.merged else 1  # (a merged form's launches run at scale 1: no rows workspace)
        return self._raw(Plan(len(lens), stride, stride * (len(lens) * K if mode == 0 else sum(lens)), rows, blocks, n_layer, *tiles, K=K,
                              tables=tables), cnt, lens)

    @staticmethod
    def patch(a, p, out, ws, rows, tables, host_off):
        a.out, a.ws, a.rows, (a.q_tok, a.q_cnt), a.grp_off_host = out, ws, rows, tables[:2], host_off
        a.n_grp, a.n_tiles, a.n_col_tiles, a.ws_stride, a.K = p.n_grp, p.n_tiles, p.n_col_tiles, p.ws_stride, p.K


class JointForm(QueryForm):
    """the query form at the joints the same forward predicts (JointQueries): the tables are made on the device behind the head
    (i2r_joint_tokens), so the launches of the captured layers run there too -- a captured layer keeps its q|k activation and emits
    nothing.  Key: the query form's with K = the model's joints, plus a marker."""
    deferred = True

    def __init__(self, capture, joints, n_joints):
        QueryForm.__init__(self, capture, AttnQueries({st: () for st, _ in capture}, joints.mode, joints.upsample, capacity=n_joints))
        self.key, self.call, self.J = self.key + ("joints",), joints, int(n_joints)

    def plan(self, stack, hw, lens, heads, call=None):
        """every group holds n / (h w) persons of J joints: counts and table width are known without the tokens, which are not validated
        here (the kernels clamp a device table's entries).  tables: the token table's shape (the device fills it), the counts, and
        [2, crops] = (group, slot in the group) of every crop for i2r_joint_tokens"""
        J, pers = self.J, [n // (hw[0] * hw[1]) for n in lens]
        crops = [(g, p) for g, n in enumerate(pers) for p in range(n)]
        K = max(pers) * J
        tables = ((len(lens), K), torch.tensor([n * J for n in pers], dtype=torch.int32), torch.tensor(crops, dtype=torch.int32).t().contiguous())
        return self._layout(self.scales[stack], hw, lens, heads, K, [n * J for n in pers], tables)

    @staticmethod
    def result(views, inputs, behind=None):  # behind: (joints, maxvals) of i2r_joint_tokens; no copy of the stacks' inputs: nobody asks for them
        return tuple(behind) + (views[0],)  # (joints, maxvals, maps)


class _PerPerson(Form):
    """what the two forms that reduce the maps per person share: two block sets per layer, (relation, maps); OP: (op kind, args class)"""
    N_BLOCKS = 2

    def launch(self, cap, qk, L, goff):
        rel_off, maps_off = cap.off
        return self.OP[0], self.OP[1](
            qk=qk.ptr, grp_off=goff.data_ptr(), rel_off=rel_off.data_ptr(), maps_off=maps_off.data_ptr(), heads=L["heads"], hp=L["hp"],
            k_off=L["hs"], qk_cs=qk.cs, seg=cap.x.h * cap.x.w, mode=self.mode, scale=1 if self.merged else self.scale, h=cap.x.h, w=cap.x.w)

    @staticmethod
    def patch(a, p, out, ws, rows, tables, host_off):
        a.rel, a.maps, a.ws, a.rows, a.grp_off_host = out, out + 4 * p.blocks[1].base, ws, rows, host_off
        a.n_grp, a.ws_stride = p.n_grp, p.ws_stride

    @staticmethod
    def result(views, inputs, behind=None):
        return tuple(views)  # (relation, maps)


class PersonForm(_PerPerson):
    """the maps reduced per person (i2r_attn_person_maps): every group is an image of P_g persons of h w tokens; per layer the [P, P]
    relation blocks, then (mode 1: dependency, 2: affect) the [P, P, h r, w r] map blocks.  The workspaces are O(P L)."""
    entry, HALF, OP = "i2r_attn_person_maps", ("qk", None, "maps", "maps_off", "rel"), (cabi.CAPTURE_OP_ATTN_PERSON, cabi.AttnPersonArgs)

    def __init__(self, capture, persons):
        self.mode, self.scale = int(persons.mode), int(persons.upsample)
        Form.__init__(self, capture, ("persons", self.mode, self.scale))
        self.scales = {st: self.scale for st, _ in capture}  # (as the query form's: per stack)

    def plan(self, stack, hw, lens, heads, call=None):
        mode, scale, (h, w) = self.mode, self.scale, hw
        assert all(n % (h * w) == 0 for n in lens)
        pers = [n // (h * w) for n in lens]
        blocks, n_layer = _layer([(p, p) for p in pers], [(p, p, h * scale, w * scale) if mode else None for p in pers])
        stride = _stride(heads, lens)
        twice = mode == 1 and scale > 1 and not self.merged  # (the raw D rows behind F; a merged form's launches run at scale 1)
        p = Plan(len(lens), stride, stride * sum(lens), (2 if twice else 1) * max(pers) * sum(lens), blocks, n_layer)
        return self._raw(p, pers, lens) if mode else p


class TargetForm(_PerPerson):
    """the target's rows of the maps reduced per person (i2r_attn_target_maps; TargetMaps): every group is a person group of m_g members
    of h w tokens whose first member is the target; per layer the relation blocks [m_g], then (mode 1: dependency, 2: affect) the map
    blocks [m_g, h r, w r].  Group g's blocks start g * slots entries behind the set (slots >= every m_g), so a layer's set is a dense,
    zero-padded [groups, slots (, h r, w r)] tensor.  The workspaces are O(L): `rows` holds F_t, sum L_g floats, and behind it the raw
    D_t for mode 1 at scale > 1."""
    entry, zero_fill, OP = "i2r_attn_target_maps", True, (cabi.CAPTURE_OP_ATTN_TARGET, cabi.AttnTargetArgs)

    def __init__(self, capture, targets):
        self.mode, self.scale = int(targets.mode), int(targets.scale)
        Form.__init__(self, capture, ("targets", self.mode, self.scale))
        self.call = targets

    def plan(self, stack, hw, lens, heads, call=None):
        """call: the TargetMaps of this call (its slots; None: the largest group's members)"""
        mode, scale, (h, w) = self.mode, self.scale, hw
        assert all(n % (h * w) == 0 for n in lens)
        pers = [n // (h * w) for n in lens]
        slots = getattr(call, "slots", None) or max(pers)
        if slots < max(pers):
            raise ValueError("relations: a group of %d members, the call is laid out for %d" % (max(pers), slots))
        m_floats = h * scale * w * scale
        rel = Block([g * slots for g in range(len(lens) + 1)], 0, [(p,) for p in pers])
        base = -(-rel.offs[-1] // 4) * 4
        maps = Block([g * slots * m_floats if mode else 0 for g in range(len(lens) + 1)], base, [(p, h * scale, w * scale) for p in pers] if mode else None)
        twice = mode == 1 and scale > 1  # (the raw D_t rows behind F_t)
        stride = _stride(heads, lens)
        return Plan(len(lens), stride, stride * sum(lens), (2 if twice else 1) * sum(lens), [rel, maps], base + -(-maps.offs[-1] // 4) * 4, K=slots)


class RolloutForm(Form):
    """the relations through the captured layers lo .. hi of every captured stack (Rollout; i2r_attn_rollout_step): a chain of thin
    products X' = (1 - alpha) X + alpha X P_l (side 0, layers hi -> lo) or ... X P_l^T (side 1, lo -> hi) from a seed X_0, ping-pong
    between two working matrices [K_g, L_g] per group behind the stack's blocks in the capture buffer; the last step writes (and
    up-samples) into the blocks.  Deferred: a captured layer keeps its q|k and the engine runs the chain behind the head.  Per stack ONE
    set of result blocks -- at query tokens the layout of the query form, per person that of the per-person form (relation, maps) --
    and a last, view-less set: the scale-1 layout of the working matrices.  alpha is per call: it is not in the key."""
    deferred = per_stack = True
    entry, sets = "i2r_attn_rollout_step", staticmethod(lambda cap: 1)

    def __init__(self, capture, rollout):
        self.points, self.mode = bool(rollout.points), int(rollout.mode)
        stacks = sorted({st for st, _ in capture})
        self.range = {}
        for st in stacks:
            layers = sorted(i for s, i in capture if s == st)
            if layers != list(range(layers[0], layers[-1] + 1)):
                raise ValueError("rollout: the layers %s of %r are not a contiguous range" % (layers, st))
            self.range[st] = (layers[0], layers[-1])
        scales = _scales("rollout", rollout.upsample, stacks)
        if not all(1 <= r <= 64 for _, r in scales):
            raise ValueError("rollout: upsample %r (1 .. 64)" % (rollout.upsample,))
        if self.points:
            missing = set(stacks) - set(rollout.tokens)
            if missing:
                raise ValueError("rollout.tokens has no table for %s" % sorted(missing))
            self.side = self.mode
        else:
            self.side = 1 if self.mode == 2 else 0  # (relation only: the dependency chain)
        self.N_BLOCKS = 2 if self.points else 3
        Form.__init__(self, capture, ("rollout", "points" if self.points else "persons", self.mode, int(rollout.capacity), scales))
        self.call, self.scales = rollout, dict(scales)

    def launch(self, cap, qk, L, goff):
        return None, cabi.AttnRolloutArgs(qk=qk.ptr, grp_off=goff.data_ptr(), heads=L["heads"], hp=L["hp"], k_off=L["hs"], qk_cs=qk.cs, K=1, side=self.side,
                                          seg=0 if self.points else cap.x.h * cap.x.w, scale=1, h=cap.x.h, w=cap.x.w)

    def plan(self, stack, hw, lens, heads, call=None):
        """call: the Rollout of this call (tokens, counts: as the query form; alpha)"""
        scale, (h, w) = self.scales[stack], hw
        assert all(n % (h * w) == 0 for n in lens)
        pers = [n // (h * w) for n in lens]
        if self.points:
            tok, K, cnt = _query_tables(call, stack, lens)
            tables = (torch.tensor(cnt, dtype=torch.int32),)
            sets = [[(c, p, h * scale, w * scale) for c, p in zip(cnt, pers)]]
        else:
            K, cnt, tables = max(pers), pers, ()
            sets = [[(p, p) for p in pers], [(p, p, h * scale, w * scale) if self.mode else None for p in pers]]
        blocks, n_layer = _layer(*sets)
        x_offs = [0]
        for c, n in zip(cnt, lens):
            x_offs.append(x_offs[-1] + c * n)
        x_floats = -(-x_offs[-1] // 4) * 4
        blocks.append(Block(x_offs, n_layer, None))  # (the two working matrices start behind the stack's blocks)
        idx = []
        for g, (c, n) in enumerate(zip(cnt, lens)):
            if self.points:
                k = torch.arange(c)[tok[g, :c] >= 0]
                idx.append(x_offs[g] + k * n + tok[g, :c][tok[g, :c] >= 0].long())
            else:  # row p: person p's tokens
                t = torch.arange(n)
                idx.append(x_offs[g] + (t // (h * w)) * n + t)
        value = 1.0 if self.points or self.side == 1 else 1.0 / (h * w)
        stride = _stride(heads, lens)
        return Plan(len(lens), stride, stride * sum(lens), K * sum(lens) if scale > 1 else 1, blocks, n_layer, K=K, tables=tables,
                    extra_floats=2 * x_floats, seed=(torch.cat(idx), value))

    @staticmethod
    def patch(a, p, out, ws, rows, tables, host_off):
        a.ws, a.rows, a.q_cnt, a.grp_off_host = ws, rows, tables[0] if tables else None, host_off
        a.n_grp, a.ws_stride, a.K = p.n_grp, p.ws_stride, p.K

    def result(self, views, inputs, behind=None):
        """per stack (not per layer): at query tokens {stack: per group a view}; per person ({stack: relations}, {stack: maps})"""
        strip = lambda d: {st: v for (st, _), v in d.items()}
        return strip(views[0]) if self.points else (strip(views[0]), strip(views[1]))


FLIP_MAPS = ("plain", "merged")


def resolve(capture, queries, persons, flip_joint_map, stacks, inter_stack, window, joints=None, n_joints=None, flip_maps="plain", rollout=None, *,
            targets=None):
    """What Engine.forward / forward_single were asked for -> the form of the call, None without a capture.  stacks: the engine's
    capture_stacks(); inter_stack: the prefix of its inter-human stack; window: the inter-human block is the window type; joints: a
    JointQueries of a model of n_joints joints -- with flip_maps "plain" the one form that goes with the flip test (its launches run
    behind the merge, on the plain half); flip_maps "merged": the flip test's merged maps (Form.merge) of the query, per-person or joint
    form -- never of the full [L, L] form, whose buffer it would double.  rollout: a Rollout -- the relations through the captured layers,
    a form of its own: not with the flip test (a product of merged maps is not the merge of products), nor with another form.
    targets: a TargetMaps -- the target form of the grouped forward (Engine.forward_groups(..., relations=)), a form of its own as well:
    layers of the inter-human stack only, not with the flip test, nor with another form."""
    if flip_maps not in FLIP_MAPS:
        raise ValueError("flip_maps %r: 'plain' or 'merged'" % (flip_maps,))
    if targets is not None:
        if not isinstance(targets, TargetMaps):
            raise ValueError("relations=: a TargetMaps, not %r" % (type(targets).__name__,))
        if queries is not None or persons is not None or joints is not None or rollout is not None:
            raise ValueError("relations=: not with queries=, persons=, joints= or rollout= (roll-out and predicted-joint queries are not served "
                             "on the grouped forward)")
        _no_window(window, "relations=")
        if flip_joint_map is not None or flip_maps != "plain":
            raise ValueError("relations=: not with the flip test")
        if not capture:
            raise ValueError("relations= needs capture=: the (stack, layer) set of the inter-human stack to reduce")
        return TargetForm(_capture_set(capture, stacks, inter_stack, "relations="), targets)
    if rollout is not None:
        _no_window(window, "rollout=")
        if flip_joint_map is not None or flip_maps != "plain":
            raise ValueError("rollout=: not with the flip test (a product of merged maps is not the merge of products)")
        if queries is not None or persons is not None or joints is not None:
            raise ValueError("rollout=: not with queries=, persons= or joints= (predicted-joint queries are not served)")
        if not capture:
            raise ValueError("rollout= needs capture=: the (stack, layer) range to roll out")
        capture = _capture_set(capture, stacks)
        other = sorted({st for st, _ in capture} - {inter_stack})
        if not rollout.points and other:
            raise ValueError("rollout= per person: %s is not this model's inter-human stack %r" % (other, inter_stack if inter_stack in stacks else None))
        return RolloutForm(capture, rollout)
    if flip_maps == "merged":
        if flip_joint_map is None:
            raise ValueError("flip_maps='merged' needs the flip test (flip_joint_map)")
        _no_window(window, "flip_maps='merged'")
        if sum(f is not None for f in (queries, persons, joints)) != 1:
            raise ValueError("flip_maps='merged' goes with exactly one of queries=, persons=, joints= (the full [L, L] maps are not merged)")
        return resolve(capture, queries, persons, None, stacks, inter_stack, window, joints, n_joints).merge()
    if joints is not None:
        _no_window(window, "joints=")
        if queries is not None or persons is not None:
            raise ValueError("joints=: not with queries= or persons= (the joint form makes its own tables)")
        if not stacks:
            raise ValueError("joints=: this model has no encoder stack to capture")
        if not capture:
            raise ValueError("joints= needs capture=: the (stack, layer) set whose maps to query")
        return JointForm(_capture_set(capture, stacks), joints, n_joints)
    if persons is not None:
        _no_window(window, "persons=")
        if flip_joint_map is not None or queries is not None:
            raise ValueError("persons=: not with the flip test, not with queries=")
        if not capture:
            raise ValueError("persons= needs capture=: the (stack, layer) set of the inter-human stack to reduce")
        return PersonForm(_capture_set(capture, stacks, inter_stack, "persons="), persons)
    if not capture:
        if queries is not None:
            raise ValueError("queries= needs capture=: the (stack, layer) set whose maps to query")
        return None
    capture = _capture_set(capture, stacks)
    assert flip_joint_map is None and not window, "attention maps: no flip test, no window-type block"
    return QueryForm(capture, queries) if queries is not None else FullForm(capture)


def _no_window(window, who):
    if window:
        raise ValueError("%s: ATTENTION_TYPE window has no encoder stack to capture" % who)


def _capture_set(capture, stacks, inter_stack=None, who=None):
    """-> a call's capture as a frozenset of (stack, layer) of this model's stacks; who: a form of the inter-human stack alone"""
    capture = frozenset((str(st), int(i)) for st, i in capture)
    other = sorted({st for st, _ in capture} - {inter_stack})
    if who and (other or inter_stack not in stacks):
        raise ValueError("%s: %s is not this model's inter-human stack %r (an intra-human stack has one person per group)"
                         % (who, other or "a capture", inter_stack if inter_stack in stacks else None))
    for st, i in capture:
        if st not in stacks or not 0 <= i < stacks[st]:
            raise ValueError("capture (%r, %d): this model's encoder stacks are %s" % (st, i, stacks))
    return capture
