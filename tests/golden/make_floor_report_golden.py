"""Writes tests/golden/zind_1210_floor_02.json: ZInD building 1210, floor_02, trimmed to what the floor report reads, with the estimated
poses of the reference's tests/common/test_floor_reconstruction_report.py and what this project's emulator gives for them.

    python tests/golden/make_floor_report_golden.py PATH/TO/1210/zind_data.json

The file is DATA only: the `merger` annotation of the one floor (per panorama: image_path, label, camera_height, floor_plan_transformation
and layout_raw.vertices), the scales, the estimated poses, the numbers the reference's test expects, and the EMULATOR's results (alignment
errors and IoU counts under np.random.seed(0) and 1000 iterations).  The reference's own IoU is unpinned: cv2 is not installed where this
was written.
"""

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

FLOOR = "floor_02"
# the reference test's wSi_list: pano id -> (R row-major, t), float32 literals, s = 1.0; every other entry of the 35 is None
ESTIMATED = {
    16: ([1.0000000e00, 1.4511669e-13, -1.4511669e-13, 1.0000000e00], [3.1663807e-13, 4.0534674e-13]),
    17: ([-0.9963625, 0.08521605, -0.08521605, -0.9963625], [-0.05208764, -0.657844]),
    18: ([-0.8538526, 0.5205148, -0.5205148, -0.8538526], [0.77260476, -1.6241723]),
    20: ([0.007844, -0.99996924, 0.99996924, 0.007844], [-0.743632, 0.03829836]),
    21: ([-0.8644665, -0.50269043, 0.50269043, -0.8644665], [-1.3128754, -0.0555355]),
    22: ([-0.9977786, -0.06661703, 0.06661703, -0.9977786], [-2.2001665, -1.263223]),
    23: ([-0.9995646, -0.02950616, 0.02950616, -0.9995646], [-0.79566294, -0.76166594]),
    24: ([-0.00257046, -0.9999967, 0.9999967, -0.00257046], [-0.6911983, 0.80846286]),
    25: ([0.00632679, -0.99998, 0.99998, 0.00632679], [-1.3925239, 0.91490793]),
    26: ([-0.01266379, -0.99991983, 0.99991983, -0.01266379], [-2.4355152, 1.7160583]),
    27: ([-0.01020425, -0.9999479, 0.9999479, -0.01020425], [-2.3332891, 0.30607823]),
    28: ([-0.10058811, 0.9949282, -0.9949282, -0.10058811], [-1.3064604, 2.2962294]),
    29: ([0.02900542, 0.99957925, -0.99957925, 0.02900542], [-0.8010526, 2.38649]),
}
N_LIST = 35


def main(src: str) -> None:
    with open(src) as f:
        d = json.load(f)
    floor = {}
    for ck, complete in d["merger"][FLOOR].items():
        floor[ck] = {}
        for pk, partial in complete.items():
            floor[ck][pk] = {k: {"image_path": p["image_path"], "label": p["label"], "camera_height": p["camera_height"],
                                 "floor_plan_transformation": p["floor_plan_transformation"], "layout_raw": {"vertices": p["layout_raw"]["vertices"]}}
                             for k, p in partial.items()}
    out = {"scale_meters_per_coordinate": d["scale_meters_per_coordinate"], "merger": {FLOOR: floor},
           "estimated_wSi_list": [None if i not in ESTIMATED else {"R": ESTIMATED[i][0], "t": ESTIMATED[i][1], "s": 1.0} for i in range(N_LIST)],
           "reference_expects": {"avg_abs_rot_err": [1.37, 1e-2], "avg_abs_trans_err": [0.19, 2e-2], "percent_panos_localized": [13 / 19 * 100, 1e-2]}}
    dst = Path(__file__).resolve().parent / "zind_1210_floor_02.json"
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)

    # the parser's own result, by plain arithmetic, and the emulator's results
    import math

    parsed = {}
    for complete in floor.values():
        for partial in complete.values():
            for p in partial.values():
                tf = p["floor_plan_transformation"]
                th = math.radians(-tf["rotation"])
                parsed[int(Path(p["image_path"]).stem.split("_")[-1])] = {
                    "R": [math.cos(th), -math.sin(th), math.sin(th), math.cos(th)],
                    "t": [-tf["translation"][0] / tf["scale"], tf["translation"][1] / tf["scale"]], "s": tf["scale"], "n_vertices": len(p["layout_raw"]["vertices"])}
    out["expected_parse"] = {str(k): parsed[k] for k in sorted(parsed)}
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
    from tests import floor_report_cases as fc

    fc.emulated_1210.cache_clear()
    c, align, iou, _ = fc.emulated_1210(str(dst.parent))
    fo, io = align[4][fc.GUARD], iou[0][fc.GUARD]
    out["emulator"] = {"best": int(fo["best"]), "avg_rot_err": float(fo["avg_rot_err"]), "avg_trans_err": float(fo["avg_trans_err"]),
                       "percent_localized": float(fo["percent_localized"]), "iou_n_est": int(io["n_est"]), "iou_n_gt": int(io["n_gt"]),
                       "iou_inter": int(io["inter"]), "iou_union": int(io["uni"]), "iou": float(io["iou"]),
                       "half_integer_margin": fc.half_integer_margin(c, align[1][fc.GUARD:-fc.GUARD]),
                       "note": "the EMULATOR's values; the reference's IoU is unpinned (cv2 is not installed where this was written)"}
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
    print(dst, dst.stat().st_size, "bytes;", out["emulator"])


if __name__ == "__main__":
    main(sys.argv[1])
