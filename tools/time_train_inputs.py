"""GPU measurement aid for i2r_train_inputs_cv2 (training samples on the device) beside i2r_person_inputs_cv2 (the validation kernel) on
the same persons.  Kernel time comes from a kernel trace, each trace a run of its own:

    rocprofv3 --kernel-trace --output-format csv -d T_NEW -- python tools/time_train_inputs.py run
    rocprofv3 --kernel-trace --output-format csv -d T_OLD -- python tools/time_train_inputs.py run --lib OLD/libi2r_hip.so --variants val
    python tools/time_train_inputs.py parse T_NEW T_OLD profiles/train_inputs.json

`run` launches, one variant after the other, WARMUP + REPS times each on the same tables:
  val             i2r_person_inputs_cv2: the crops at rot 0, the masks by mask_pixel_cv2
  train_r0        i2r_train_inputs_cv2, rot 0, no flip      (same maps and boxes as val: the outputs are compared bit for bit first)
  train_r30       i2r_train_inputs_cv2, rot 30, no flip     (rotated crop map; the mask through rotate_bound's 30-degree canvas)
  train_r30_flip  the same on the mirrored image
--lib: another build of the library (the parent commit's, which has `val` only), loaded with plain ctypes.
Workload: config 1's batch -- 8 images of 480 x 640, 4 persons each, 32 crops of 256 x 192; boxes of 25-60 % of the image, some over the
border.  The images stay in the caches between launches (warm): that is the state of a step whose frames were just decoded onto the
device.  bytes_out: the 32 x 4 x 256 x 192 fp32 values a launch writes; its time at the HBM peak is the floor quoted with the result.
Nothing is asserted about a time or a ratio: the numbers are written down."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_IMG, PER_IMG, IH, IW, W, H = 8, 4, 480, 640, 192, 256
VARIANTS = ("val", "train_r0", "train_r30", "train_r30_flip")
WARMUP, REPS = 3, 50
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
KERNEL = {"val": "person_inputs_cv2_k", "train": "train_inputs_cv2_k"}


def tables(inp, imgs, rot, flip):
    """-> (val rows i2r_crop_ref, train rows i2r_train_crop_ref, image rows) for the seeded persons at one augmentation"""
    rng = np.random.RandomState(3)
    S = N_IMG * PER_IMG
    bw, bh = rng.uniform(0.25, 0.6, S) * IW, rng.uniform(0.25, 0.6, S) * IH
    boxes = np.stack([rng.uniform(-0.1 * IW, IW - 0.9 * bw), rng.uniform(-0.1 * IH, IH - 0.9 * bh), bw, bh], 1)
    cs = [inp.box_to_center_scale(b, (W, H)) for b in boxes]
    cen, scl = np.stack([c for c, _ in cs]), np.stack([s for _, s in cs])
    trans = inp.affine_transforms(cen, scl, (W, H), rot=rot)
    bi = np.stack([np.trunc(boxes[:, 0]), np.trunc(boxes[:, 1]), np.trunc(boxes[:, 0] + boxes[:, 2]), np.trunc(boxes[:, 1] + boxes[:, 3])], 1).astype(np.int32)
    image = np.repeat(np.arange(N_IMG, dtype=np.int32), PER_IMG)
    val = np.zeros(S, dtype=inp._CROP_DT)
    val["inv_m"], val["box"], val["image"] = inp.cv2_inverse_batch(trans), bi, image
    M, nW, nH = inp.rotate_bound_geometry(IH, IW, rot)
    tr = np.zeros(S, dtype=inp._TRAIN_CROP_DT)
    tr["inv_m"], tr["mask_inv_m"], tr["box"], tr["image"] = val["inv_m"], inp.cv2_inverse(M).reshape(6), bi, image
    tr["nw"], tr["nh"], tr["flip"] = nW, nH, int(flip)
    irows = np.zeros(N_IMG, dtype=inp._IMG_DT)
    for i, t in enumerate(imgs):
        irows[i] = (t.data_ptr(), IH, IW, IW * 3, 0)
    return val, tr, irows


def run(args):
    import torch
    import i2r_amd  # noqa: F401
    from i2r_amd import cabi
    from i2r_amd import input as inp
    if not torch.cuda.is_available():
        raise SystemExit("time_train_inputs: no GPU -- a time is measured on the device or not at all")
    dev = torch.device("cuda", 0)
    L = C.CDLL(args.lib or cabi.LIB_PATH)
    proto = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p,
             C.c_int32, C.c_int32, C.c_void_p]
    gen = torch.Generator(dev).manual_seed(1)
    imgs = [torch.randint(0, 256, (IH, IW, 3), device=dev, dtype=torch.uint8, generator=gen) for _ in range(N_IMG)]
    S = N_IMG * PER_IMG
    x, m = torch.empty(S, 3, H, W, device=dev), torch.empty(S, 1, H, W, device=dev)
    mean_c = (C.c_float * 3)(*inp.IMAGENET_MEAN)
    istd_c = (C.c_float * 3)(*[1.0 / v for v in inp.IMAGENET_STD])
    st = torch.cuda.current_stream().cuda_stream
    kept = {}
    for v in args.variants.split(","):
        rot, flip = (30.0 if "r30" in v else 0), v.endswith("flip")
        val, tr, irows = tables(inp, imgs, rot, flip)
        rows, fn = (val, L.i2r_person_inputs_cv2) if v == "val" else (tr, L.i2r_train_inputs_cv2)
        fn.argtypes = proto
        itab = torch.from_numpy(irows.view(np.uint8).copy()).to(dev)
        ctab = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
        for _ in range(WARMUP + args.reps):
            rc = fn(itab.data_ptr(), N_IMG, ctab.data_ptr(), S, 0, mean_c, istd_c, x.data_ptr(), m.data_ptr(), H, W, st)
            assert rc == 0, rc
        torch.cuda.synchronize()
        kept[v] = (x.clone(), m.clone())
        print("%s: %d launches, mask mean %.4f, crop mean %.4f" % (v, WARMUP + args.reps, m.mean().item(), x.mean().item()), flush=True)
    if "val" in kept and "train_r0" in kept:   # a time is never quoted for a result that differs
        same = torch.equal(kept["val"][0], kept["train_r0"][0]) and torch.equal(kept["val"][1], kept["train_r0"][1])
        print("train_r0 == val bit for bit: %s" % same, flush=True)
        assert same


def durations(d, kernel):
    import csv
    import glob
    (trace,) = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]


def stat(v):
    return dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2), launches=len(v))


def parse(new_dir, old_dir, out):
    """kernel durations of the two traces -> JSON.  The train kernel's launches come in the order of VARIANTS, WARMUP + REPS each; the
    warm-up launches of every variant are dropped."""
    per = WARMUP + REPS
    tr = durations(new_dir, KERNEL["train"])
    assert len(tr) == 3 * per, len(tr)
    res = {v: stat(tr[k * per + WARMUP:(k + 1) * per]) for k, v in enumerate(VARIANTS[1:])}
    for tag, d in (("val", new_dir), ("val_parent_library", old_dir)):
        v = durations(d, KERNEL["val"])
        assert len(v) == per, len(v)
        res[tag] = stat(v[WARMUP:])
    bytes_out = N_IMG * PER_IMG * 4 * H * W * 4
    doc = dict(what="kernel duration in microseconds from rocprofv3 --kernel-trace (End - Start of every launch after %d warm-up launches), one trace "
                    "per library; warm: the same 8 images again and again" % WARMUP,
               workload=dict(images=N_IMG, image_shape=[IH, IW], crops=N_IMG * PER_IMG, output=[H, W], bytes_out=bytes_out),
               hbm_floor_us=dict(at_8_0_tb_s_spec=round(bytes_out / HBM_PEAK * 1e6, 2), at_6_29_tb_s_copy=round(bytes_out / HBM_COPY * 1e6, 2)),
               kernel_us=res)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "parse":
        parse(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        ap = argparse.ArgumentParser()
        ap.add_argument("mode", choices=["run"])
        ap.add_argument("--lib", default=None)
        ap.add_argument("--variants", default=",".join(VARIANTS))
        ap.add_argument("--reps", type=int, default=REPS)
        run(ap.parse_args())
