"""Store what two CPU tests used to read from the reference tree at run time, so that they run without it:
  tests/golden/reference_yaml.json   the reference's experiments/*.yaml as parsed by yaml.safe_load (relative path without .yaml -> mapping),
                                     read by tests/test_host.py (the loader takes them unchanged; the shipped configs carry their MODEL / TEST keys)
  tests/golden/post_reference.npz    outputs of the reference's own get_max_preds / taylor (lib/core/inference.py) and flip_back
                                     (lib/utils/transforms.py) on the seeded heat maps of tests/test_post_oracle.py, read by that test
Run where the reference exists (oracle/ref_shim.py REF_ROOT).  Usage: python oracle/make_golden_refdata.py"""
import glob
import json
import os
import sys
import types

import numpy as np
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import i2r_amd  # noqa: E402,F401
from ref_shim import REF_LIB, REF_ROOT  # noqa: E402
from i2r_amd import caller  # noqa: E402
from test_post_oracle import _hm  # noqa: E402  (the test's own input)

GOLDEN = os.path.join(ROOT, "tests", "golden")

exp = os.path.join(REF_ROOT, "experiments")
ymls = {}
for f in sorted(glob.glob(os.path.join(exp, "*", "*.yaml"))):
    with open(f) as fh:
        ymls[os.path.relpath(f, exp)[:-len(".yaml")]] = yaml.safe_load(fh)
with open(os.path.join(GOLDEN, "reference_yaml.json"), "w") as fh:
    json.dump(ymls, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("reference_yaml.json:", len(ymls), "files")

if "cv2" not in sys.modules:
    sys.modules["cv2"] = types.ModuleType("cv2")  # imported at module top only; never called by the functions used here
sys.path.insert(0, REF_LIB)
from core import inference as ref_inf  # noqa: E402
from utils import transforms as ref_tr  # noqa: E402

hm = _hm()
preds, maxvals = ref_inf.get_max_preds(hm)
lg = np.log(np.maximum(hm, 1e-10))
taylor = np.stack([np.stack([ref_inf.taylor(lg[s, j], preds[s, j].copy()) for j in range(hm.shape[1])]) for s in range(hm.shape[0])])
pairs = caller.FLIP_PAIRS["crowdpose"][:2]
flipped = ref_tr.flip_back(hm.copy(), pairs)
np.savez_compressed(os.path.join(GOLDEN, "post_reference.npz"), hm=hm, preds=preds, maxvals=maxvals, taylor=taylor,
                    flip_pairs=np.asarray(pairs), flip_back=flipped)
print("post_reference.npz:", hm.shape, taylor.shape)
