"""Generate tests/golden/cluster_levels.json by running THE REFERENCE ITSELF: ClusterMode.get_cluster_level of
lib/utils/KeypointEvaluator.py for the start points [1, 2, 6, 10] (its default) and [1, 3, 5], person counts 0 ... 40.
Run where the reference exists (oracle/ref_shim.py REF_ROOT):

    python tools/make_golden_oks_groups.py

A count the reference has no level for (0 persons: get_cluster_level returns None) is recorded as null.  Data only."""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from ref_shim import REF_LIB  # noqa: E402

START_POINTS = [[1, 2, 6, 10], [1, 3, 5]]
COUNTS = list(range(41))


def main():
    spec = importlib.util.spec_from_file_location("ref_keypoint_evaluator", os.path.join(REF_LIB, "utils", "KeypointEvaluator.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = dict(source="lib/utils/KeypointEvaluator.py ClusterMode.get_cluster_level", counts=COUNTS, cases=[])
    for sp in START_POINTS:
        mode = mod.ClusterMode(list(sp))
        out["cases"].append(dict(start_points=sp, levels=[mode.get_cluster_level(n) for n in COUNTS]))
    path = os.path.join(ROOT, "tests", "golden", "cluster_levels.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(path, ROOT))


if __name__ == "__main__":
    main()
