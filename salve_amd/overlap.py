"""Accuracy, rotation error and translation error of the verifier against the VISUAL OVERLAP of the scored pair: the reference's
scripts/measure_acc_vs_overlap.py:45-167 without its plots.

The reference reopens the two tiles fp0 / fp1 of every prediction and takes the IoU of their occupancy masks
(salve/utils/iou_utils.py:14-37).  Prediction files of the fused path name tiles that were never written; written with
`visual_overlap=True` (evaluate.run_fused_epoch, ingest.score_floor) they carry the two pixel counts instead, in the key "overlap", counted
on the device from the very images the verifier scored (include/salve_hip.h: salve_bev_pair_overlap).  `from_tiles=True` is the host route
for prediction files of the un-fused path: the counts come from the files, read with Pillow.

    python -m salve_amd.overlap PRED_DIR [--gt-class {0,1}] [--tiles]

prints the result without its per-example records as one JSON document.  Loading ZInD's ground-truth pose graph stays outside: the pose
errors need a callable that returns the ground-truth relative pose of a pair.
"""

from __future__ import annotations

import argparse
import glob
import json
import sys
from pathlib import Path
from typing import Any, Callable, Dict, Optional, Tuple

import numpy as np

from salve_amd.common.sim2 import Sim2

LABEL_DIRS = {1: "gt_alignment_approx", 0: "incorrect_alignment"}
NUM_BINS = 10


def wrap_angle_deg(angle1: float, angle2: float) -> float:
    """The smallest difference between two angles in degrees, |((b - a + 180) % 360) - 180| (salve/utils/rotation_utils.py:45-63)."""
    return float(np.absolute((angle2 - angle1 + 180) % 360 - 180))


def counts_from_tiles(fp0: str, fp1: str) -> Tuple[int, int]:
    """(intersection, union) of the occupancy masks of two tile files, occupied = the largest channel is positive (iou_utils.py:25-26,
    35-36)."""
    from PIL import Image

    masks = []
    for fp in (fp0, fp1):
        with Image.open(fp) as im:
            f = np.asarray(im)
        masks.append((f if f.ndim == 2 else np.amax(f, axis=2)) > 0)
    return int(np.logical_and(*masks).sum()), int(np.logical_or(*masks).sum())


def parse_tile_names(fp0: str, fp1: str) -> Dict[str, Any]:
    """What scripts/measure_acc_vs_overlap.py:82-108 reads off the two tile names of a prediction, e.g.
    `.../gt_alignment_approx/0668/pair_54___door_0_0_identity_floor_rgb_floor_02_partial_room_01_pano_48.jpg`: the panorama ids (the smaller
    one first: compared as integers, pano_10 comes behind pano_9), the building (the parent directory), the floor, the pair's index within
    its label directory (a string, as there), identity | rotated, and the W/D/O pair in front of it."""
    stem = Path(fp0).stem
    i1, i2 = int(stem.split("_")[-1]), int(Path(fp1).stem.split("_")[-1])
    if i1 >= i2:
        i1, i2 = i2, i1
    configuration = "identity" if "identity" in stem else "rotated"
    tail = stem.split("___")[1]
    k = tail.find(f"_{configuration}")
    if k == -1:
        raise ValueError(f"{fp0}: the tile name carries neither 'identity' nor 'rotated' behind its W/D/O pair")
    wdo_pair_uuid = tail[:k]
    if not any(t in wdo_pair_uuid for t in ("door", "window", "opening")):
        raise ValueError(f"{fp0}: {wdo_pair_uuid!r} names no door, window or opening")
    return {"building_id": Path(fp0).parent.stem, "floor_id": stem[stem.find("floor_0"):stem.find("_partial")], "i1": i1, "i2": i2,
            "pair_idx": stem.split("_")[1], "wdo_pair_uuid": wdo_pair_uuid, "configuration": configuration}


def hypothesis_fpath(hypotheses_save_root: str, rec: Dict[str, Any]) -> str:
    """{root}/{building}/{floor}/{label}/{i1}_{i2}__{uuid}.json: the alignment hypothesis behind a prediction (the label directory by its
    ground-truth class, the uuid = W/D/O pair and configuration, as export_alignment_hypotheses.py names the files)."""
    return (f"{hypotheses_save_root}/{rec['building_id']}/{rec['floor_id']}/{LABEL_DIRS[1 if rec['y_true'] == 1 else 0]}/"
            f"{rec['i1']}_{rec['i2']}__{rec['wdo_pair_uuid']}_{rec['configuration']}.json")


def measure_acc_vs_visual_overlap(serialized_preds_json_dir: str, gt_class: int = 0, confidence_threshold: float = 0.0, from_tiles: bool = False,
                                  hypotheses_save_root: Optional[str] = None,
                                  gt_relative_pose: Optional[Callable[[str, str, int, int], Sim2]] = None) -> Dict[str, Any]:
    """How the verifier's accuracy (and, given poses, its pairs' rotation and translation error) depends on the visual overlap of the two
    texture maps: scripts/measure_acc_vs_overlap.py:45-167.  Positives and negatives are counted apart: only predictions with
    y_true == gt_class and y_hat_probs >= confidence_threshold are kept (:67-71).

    iou = intersection / (union + 1e-12) in float64 (iou_utils.py:34-37).  The two counts come from the prediction files' "overlap" key
    (written by the fused path with visual_overlap=True); from_tiles=True: from the files fp0 / fp1 name, read with Pillow -- the host
    route for prediction files of the un-fused path.

    Bins: np.digitize(iou, np.linspace(0, 1, 11)) - 1 (:146, 155-156; linspace's 0.30000000000000004 included).  An IoU of exactly 1.0
    goes to the LAST bin and is counted in `n_full_overlap`.  The reference indexes bin 10 of 10 there and raises IndexError -- and the
    quotient is exactly 1.0 in float64 for every pair of identical masks of 2^14 = 16384 pixels or more (union + 1e-12 then rounds back to
    union; below that the sum is representable and the quotient stays under 1), so its script cannot bin such a pair at all.

    Returns bin_edges [11], counts [10] (int), mean_acc [10] (percent, float32 as there; NaN for an empty bin, as its division gives),
    n_full_overlap, and examples: one record per kept prediction with iou, intersection, union, y_hat, y_true, prob and the fields of
    `parse_tile_names`.  With hypotheses_save_root and gt_relative_pose(building_id, floor_id, i1, i2) -> Sim2 (i2Ti1 of the ground truth)
    also avg_rot_err and avg_trans_err [10] (:126-143, 166-167): the hypothesis is read from `hypothesis_fpath`, the rotation error is
    wrap_angle_deg of the two angles, the translation error the norm of the difference; the records then carry rot_err and trans_err."""
    if (hypotheses_save_root is None) != (gt_relative_pose is None):
        raise ValueError("the pose errors need both hypotheses_save_root and gt_relative_pose")
    with_pose = gt_relative_pose is not None
    examples = []
    for json_fpath in sorted(glob.glob(f"{serialized_preds_json_dir}/batch*.json")):
        with open(json_fpath) as f:
            d = json.load(f)
        if not from_tiles and "overlap" not in d:
            raise KeyError(f'{json_fpath} has no "overlap" key: score with visual_overlap=True, or pass from_tiles=True (--tiles) if the tiles exist')
        for k, (y_hat, y_true, prob, fp0, fp1) in enumerate(zip(d["y_hat"], d["y_true"], d["y_hat_probs"], d["fp0"], d["fp1"])):
            if y_true != gt_class or prob < confidence_threshold:
                continue
            inter, union = counts_from_tiles(fp0, fp1) if from_tiles else (int(d["overlap"][k][0]), int(d["overlap"][k][1]))
            rec = {"iou": float(np.float64(inter) / (np.float64(union) + 1e-12)), "intersection": inter, "union": union, "y_hat": y_hat,
                   "y_true": y_true, "prob": prob, **parse_tile_names(fp0, fp1)}
            if with_pose:
                i2Ti1_gt = gt_relative_pose(rec["building_id"], rec["floor_id"], rec["i1"], rec["i2"])
                i2Ti1 = Sim2.from_json(hypothesis_fpath(hypotheses_save_root, rec))
                rec["rot_err"] = wrap_angle_deg(i2Ti1_gt.theta_deg, i2Ti1.theta_deg)
                rec["trans_err"] = float(np.linalg.norm(np.asarray(i2Ti1_gt.translation) - np.asarray(i2Ti1.translation)))
            examples.append(rec)

    bin_edges = np.linspace(0, 1, 11)
    counts, acc_bins = np.zeros(NUM_BINS), np.zeros(NUM_BINS)
    rot_bins, trans_bins = np.zeros(NUM_BINS), np.zeros(NUM_BINS)
    n_full = 0
    for rec in examples:
        b = int(np.digitize(rec["iou"], bins=bin_edges)) - 1
        if b == NUM_BINS:   # iou == 1.0
            b, n_full = NUM_BINS - 1, n_full + 1
        acc_bins[b] += rec["y_hat"] == rec["y_true"]
        counts[b] += 1
        if with_pose:
            rot_bins[b] += rec["rot_err"]
            trans_bins[b] += rec["trans_err"]
    countsf = counts.astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"bin_edges": bin_edges, "counts": counts.astype(np.int64), "mean_acc": np.divide(acc_bins.astype(np.float32), countsf) * 100,
               "n_full_overlap": n_full, "examples": examples}
        if with_pose:
            out["avg_rot_err"], out["avg_trans_err"] = np.divide(rot_bins, countsf), np.divide(trans_bins, countsf)
    return out


def as_json(result: Dict[str, Any]) -> str:
    """The result without its examples as one JSON document (an empty bin's NaN as null)."""
    clean = lambda v: [None if isinstance(x, float) and np.isnan(x) else x for x in np.asarray(v).tolist()]
    return json.dumps({k: (clean(v) if isinstance(v, np.ndarray) else v) for k, v in result.items() if k != "examples"}, indent=4)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m salve_amd.overlap", description="Verifier accuracy against the visual overlap (IoU) of the scored pairs.")
    ap.add_argument("pred_dir", metavar="PRED_DIR", help="directory of batch_*.json prediction files")
    ap.add_argument("--gt-class", type=int, choices=(0, 1), default=0, help="ground-truth class to keep: 1 positives, 0 negatives (default)")
    ap.add_argument("--tiles", action="store_true", help='take the counts from the tile files fp0 / fp1 name instead of the "overlap" key')
    args = ap.parse_args(argv)
    print(as_json(measure_acc_vs_visual_overlap(args.pred_dir, gt_class=args.gt_class, from_tiles=args.tiles)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
