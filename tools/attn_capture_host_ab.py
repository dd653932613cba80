"""GPU aid for changes to the HOST side of the attention-map capture (attn_capture.py, attn_bind.py, Program.bind_capture): for a fixed list of calls
it dumps what the device is handed and what comes back, so that two trees can be compared bit for bit.
    python tools/attn_capture_host_ab.py dump out.json      (uses only Engine / model API plus the program's op list: copy the tool alone
                                                             into a checkout of the other tree and run it there too)
    python tools/attn_capture_host_ab.py diff a.json b.json (-> exit 0 when identical apart from the per-call buffer's total size)
    python tools/attn_capture_host_ab.py digest a.json      (per call the counts and one sha256 over the call's record: what profiles/ keeps)
Per call: the program's op list (kind, lane), every capture launch's args after binding -- non-pointer fields by value, pointer fields
as (the buffer they point into, byte offset) --, shape and buffer offset of every returned view, a checksum of every returned tensor.
Calls: w48_pure_en6 and tph_192_p6_b4 (both stacks): full capture of every layer, attention_at in both modes with upsample on and off;
w48_pure_en6 also person_relations in all three modes at two groupings of one capacity.
The forms whose launches run behind the program's head or are not among CAPTURE_KINDS (their launches are not in the op list, and their
per-call records are the host's own business) are compared by what no tree can lay out differently -- op list, program key, whether the
call built a program, shape and buffer offset of every returned view, sha256 of every returned tensor: attention_at_joints plain,
under the flip test and flip-merged; attention_at and person_relations flip-merged; rollout_at in both modes; person_rollout with maps
None and "affect"; main_target_relations in the shared mode the model takes (else the expanded one)."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAPTURE_KINDS = (29, 30, 32)  # I2R_OP_ATTN_WEIGHTS / _QUERY / _PERSON


def _tensors(obj, path=""):
    """every tensor of what a call returned, with a stable name"""
    import torch
    if torch.is_tensor(obj):
        yield path, obj
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            yield from _tensors(obj[k], "%s[%s]" % (path, k))
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _tensors(v, "%s.%d" % (path, i))
    elif hasattr(obj, "relation"):  # models._base.PersonRelations, TargetRelations
        for field in ("relation", "maps", "members", "group_len", "image_relation"):
            if hasattr(obj, field):
                yield from _tensors(getattr(obj, field), "%s.%s" % (path, field))


def _plain(key):
    """a program key as JSON: sets in sorted order"""
    if isinstance(key, (set, frozenset)):
        return sorted(_plain(k) for k in key)
    return [_plain(k) for k in key] if isinstance(key, (tuple, list)) else key


def _describe(P, result, launches=True):
    import torch
    from i2r_amd import cabi
    spans = []  # (first byte, bytes, label) of every buffer a capture launch may point into
    views = {}
    for name, t in _tensors(result):
        st = t.untyped_storage()
        views[name] = dict(shape=list(t.shape), offset=t.storage_offset(), storage_floats=st.nbytes() // 4,
                           sha256=hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest())
        spans.append((st.data_ptr(), st.nbytes(), "result[%d floats]" % (st.nbytes() // 4)))
    held = P._capture_ws if isinstance(P._capture_ws, (list, tuple)) else [P._capture_ws]
    for group, items in (("call", held), ("program", P.keep)):
        for t in items:
            if torch.is_tensor(t):
                spans.append((t.data_ptr(), t.numel() * t.element_size(), "%s %s[%d]" % (group, str(t.dtype)[6:], t.numel())))  # (named by type and size: the same in both trees)
            elif isinstance(t, C.Array):
                spans.append((C.addressof(t), C.sizeof(t), "%s host int32[%d]" % (group, len(t))))
    per_call = {n: v["storage_floats"] for n, v in views.items() if n.startswith(".1") and "input" not in n}  # (.0: the model output)
    records = []
    for kind, lane, a in P.ops if launches else ():
        if kind not in CAPTURE_KINDS:
            continue
        rec = dict(kind=kind, lane=lane)
        for f, ty in a._fields_:
            v = getattr(a, f)
            if ty is not cabi._fp:
                rec[f] = v
                continue
            v = v or 0
            hit = [(lab, v - p0) for p0, n, lab in spans if v and p0 <= v < p0 + max(n, 1)]
            if hit and hit[0][0].startswith("result["):  # (the one buffer whose total size may differ between trees: named without it)
                hit = [("capture buffer", hit[0][1])]
            rec[f] = list(hit[0]) if hit else ("null" if not v else "unknown")
        records.append(rec)
    for v in views.values():
        del v["storage_floats"]
    return dict(ops=[[k, lane] for k, lane, _ in P.ops], launches=records, views=views, capture_buffer_floats=sorted(set(per_call.values())))


def dump(path):
    import torch
    import i2r_amd  # noqa: F401
    from i2r_amd import arch, caller, config, models, synth
    out = {}
    for name, factory in (("w48_pure_en6", models.interformer_pureMulti), ("tph_192_p6_b4", models.interformer)):
        cfg = config.load_config(name)
        net = factory.get_pose_net(cfg, is_train=False)
        net.load_state_dict(synth.make_state_dict(arch.param_spec(cfg)), strict=True)
        net = net.cuda()
        eng = net.engine()
        groupings = ([3, 1, 2], [2, 2, 2])
        data = {tuple(g): synth.make_inputs(list(g), 256, 192) for g in groupings}
        x, m, length = data[(3, 1, 2)]
        x, m = x.cuda(), m.cuda()
        pts = torch.tensor([[12.5, 20.0], [100.0, 200.0], [191.0, 255.0], [float("nan")] * 2]).repeat(x.shape[0], 1, 1)
        every = {(st, i) for st, n in eng.capture_stacks().items() for i in range(n)}
        calls = [("full", lambda: eng.forward(x, m, length, capture=every))]
        for mode in ("dependency", "affect"):
            for up in (True, False):
                calls.append(("attention_at %s upsample=%s" % (mode, up), lambda mode=mode, up=up: net.attention_at(x, m, length, pts, mode=mode, upsample=up)))
        if name == "w48_pure_en6":
            for maps in (None, "dependency", "affect"):
                for g in groupings:
                    xg, mg, lg = data[tuple(g)]
                    calls.append(("person_relations %s %s" % (maps, list(g)),
                                  lambda maps=maps, xg=xg, mg=mg, lg=lg: net.person_relations(xg.cuda(), mg.cuda(), lg, maps=maps, upsample=True)))
        calls.append(("full again", calls[0][1]))
        n_bound = len(calls)  # (the calls above: every capture launch is in the op list; the ones below: see the module docstring)
        pairs = caller.FLIP_PAIRS["crowdpose" if cfg.MODEL.NUM_JOINTS == 14 else "coco"]
        for label, kw in (("plain", {}), ("flip test", dict(flip_pairs=pairs)), ("flip merged", dict(flip_pairs=pairs, flip_maps="merged"))):
            calls.append(("attention_at_joints %s" % label, lambda kw=kw: net.attention_at_joints(x, m, length, **kw)))
        for mode in ("dependency", "affect"):
            calls.append(("attention_at %s flip merged" % mode, lambda mode=mode: net.attention_at(x, m, length, pts, mode=mode, flip_pairs=pairs, flip_maps="merged")))
            calls.append(("rollout_at %s" % mode, lambda mode=mode: net.rollout_at(x, m, length, pts, mode=mode)))
        if name == "w48_pure_en6":
            for g in groupings:
                xg, mg, lg = data[tuple(g)]
                calls.append(("person_relations dependency flip merged %s" % list(g),
                              lambda xg=xg, mg=mg, lg=lg: net.person_relations(xg.cuda(), mg.cuda(), lg, maps="dependency", upsample=True, flip_pairs=pairs, flip_maps="merged")))
                for maps in (None, "affect"):
                    calls.append(("person_rollout %s %s" % (maps, list(g)),
                                  lambda maps=maps, xg=xg, mg=mg, lg=lg: net.person_rollout(xg.cuda(), mg.cuda(), lg, maps=maps, upsample=True)))
        try:
            share = True if eng._groups_shared(256, 192, True) else None
        except ValueError:
            share = None
        boxes = (torch.rand(x.shape[0], 4, generator=torch.Generator().manual_seed(0), dtype=torch.float64) * 200).numpy()
        calls.append(("main_target_relations affect share=%s" % share,
                      lambda: net.main_target_relations(x, m, length, boxes, max_patch=2, maps="affect", upsample=True, share_first_stage=share)))
        for n, (label, fn) in enumerate(calls):
            builds = eng.n_builds
            res = fn()
            torch.cuda.synchronize()
            P = next(P for P in eng.last_programs if P.captures)
            rec = _describe(P, res, launches=n < n_bound)
            rec["program_key"] = _plain(next(k for k, v in eng.programs.items() if v[0] is P))
            rec["built"] = eng.n_builds - builds
            out["%s: %s" % (name, label)] = rec
            print(name, label, "launches", len(rec["launches"]), "views", len(rec["views"]), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


def diff(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad = sorted(set(a) ^ set(b))
    buf = []
    for call in sorted(set(a) & set(b)):
        for part in sorted(set(a[call]) | set(b[call])):
            if a[call].get(part) != b[call].get(part):
                (buf if part == "capture_buffer_floats" else bad).append("%s: %s" % (call, part))
    print(json.dumps(dict(calls=len(a), identical=not bad, differing=bad, capture_buffer_total_differs_in=buf), indent=1))
    return 1 if bad else 0


def digest(path):
    """per call: ops / capture launches / returned tensors counted, the program key, and the sha256 of the call's whole record"""
    out = {}
    for call, rec in json.load(open(path)).items():
        body = dict(rec, capture_buffer_floats=None)  # (as diff: the buffer's total is reported beside the digest, not inside it)
        out[call] = dict(ops=len(rec["ops"]), launches=len(rec["launches"]), tensors=len(rec["views"]), built=rec["built"], program_key=rec["program_key"],
                         capture_buffer_floats=rec["capture_buffer_floats"], sha256=hashlib.sha256(json.dumps(body, sort_keys=True).encode()).hexdigest())
    return out


if __name__ == "__main__":
    if sys.argv[1] == "digest":
        print(json.dumps(digest(sys.argv[2]), indent=1, sort_keys=True))
    else:
        sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else diff(sys.argv[2], sys.argv[3]))
