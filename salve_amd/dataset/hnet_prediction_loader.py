"""MHNet predictions of a building -> one PoseGraph2d per floor holding the INFERRED W/D/Os and layout of every panorama (with the ground
truth's pose and label): the reference's salve/dataset/hnet_prediction_loader.py:26-87, 120-222.  Host only.

Deviations from the reference:
* `{predictions_data_root}/vanishing_angle/{building}.json` is optional: without it every panorama's vanishing angle is None (the reference
  opens the file unconditionally; its own test data has none, and nothing behind this loader reads the angle).
* A panorama's image path is the one its prediction file names (`{raw_dataset_dir}/{building}/panos/{stem}.jpg`), whether or not the image is on
  disk; the reference globs the panos directory for the id and fails without it.  Where the image exists both give the same path.
* A panorama id with several prediction files, other than the two known duplicates, raises ValueError (the reference reuses whatever path
  the previous panorama left in a local variable)."""

from __future__ import annotations

import glob
import json
from pathlib import Path
from typing import Any, Dict, Optional

from salve_amd.common.pano_data import PoseGraph2d, gt_pose_graph_from_json, read_zind_json
from salve_amd.dataset.mhnet_prediction import MHNetPanoStructurePrediction

IMG_H, IMG_W = 512, 1024   # hnet_prediction_loader.py:179-180
# buildings whose floors hold one panorama id twice: the prediction file the reference picks (:63-73)
KNOWN_DUPLICATES = {("1348", 5): "floor_01_partial_room_12_pano_5", ("0363", 34): "floor_02_partial_room_05_pano_34"}


def load_hnet_predictions(building_id: str, raw_dataset_dir, predictions_data_root,
                          floor_map_json: Optional[Dict[str, Any]] = None) -> Dict[str, Dict[int, MHNetPanoStructurePrediction]]:
    """floor id -> {panorama id: prediction}, for every floor of the building's `merger` annotation.  A panorama without a prediction file is
    left out (the hypothesis generator names it when it needs it)."""
    d = floor_map_json if floor_map_json is not None else read_zind_json(raw_dataset_dir, building_id)
    if "merger" not in d:
        raise ValueError(f"Building {building_id} missing `merger` data.")
    out: Dict[str, Dict[int, MHNetPanoStructurePrediction]] = {}
    for floor_id in d["merger"]:
        out[floor_id] = {}
        for i in gt_pose_graph_from_json(d, building_id, floor_id).pano_ids():
            hits = glob.glob(f"{predictions_data_root}/horizon_net/{building_id}/*_{i}.json")
            if len(hits) == 0:
                continue
            if len(hits) > 1:
                if (building_id, i) not in KNOWN_DUPLICATES:
                    raise ValueError(f"Building {building_id}: {len(hits)} MHNet prediction files for pano {i}: {sorted(hits)}")
                fpath = Path(f"{predictions_data_root}/horizon_net/{building_id}/{KNOWN_DUPLICATES[(building_id, i)]}.json")
            else:
                fpath = Path(hits[0])
            out[floor_id][i] = MHNetPanoStructurePrediction.from_json_fpath(json_fpath=fpath,
                                                                            image_fpath=Path(f"{raw_dataset_dir}/{building_id}/panos/{fpath.stem}.jpg"))
    return out


def load_vanishing_angles(predictions_data_root, building_id: str) -> Optional[Dict[int, float]]:
    """{panorama id: degrees}, or None when the building has no vanishing_angle file."""
    path = Path(predictions_data_root) / "vanishing_angle" / f"{building_id}.json"
    if not path.exists():
        return None
    with open(path) as f:
        return {int(k): v for k, v in json.load(f).items()}


def load_inferred_floor_pose_graphs(building_id: str, raw_dataset_dir, predictions_data_root) -> Optional[Dict[str, PoseGraph2d]]:
    """floor id -> PoseGraph2d of the panoramas MHNet predicted, each converted by MHNetPanoStructurePrediction.convert_to_pano_data at
    512 x 1024.  None for a building without `merger` data (the caller skips it, as the reference's exporter does)."""
    d = read_zind_json(raw_dataset_dir, building_id)
    if "merger" not in d:
        return None
    predictions = load_hnet_predictions(building_id, raw_dataset_dir, predictions_data_root, d)
    angles = load_vanishing_angles(predictions_data_root, building_id)
    graphs: Dict[str, PoseGraph2d] = {}
    for floor_id, floor_predictions in predictions.items():
        gt = gt_pose_graph_from_json(d, building_id, floor_id)
        graphs[floor_id] = PoseGraph2d(building_id, floor_id, {}, gt.scale_meters_per_coordinate)
        for i, pred in floor_predictions.items():
            graphs[floor_id].nodes[i] = pred.convert_to_pano_data(img_h=IMG_H, img_w=IMG_W, pano_id=i, gt_pose_graph=gt, img_fpath=str(pred.image_fpath),
                                                                  vanishing_angle_deg=None if angles is None else angles.get(i))
    return graphs


def load_inferred_floor_pose_graph(building_id: str, floor_id: str, raw_dataset_dir, predictions_data_root) -> PoseGraph2d:
    graphs = load_inferred_floor_pose_graphs(building_id, raw_dataset_dir, predictions_data_root)
    if graphs is None:
        raise ValueError(f"ModifiedHorizonNet (MHNet) predictions missing for all floors of ZInD Building {building_id}.")
    if floor_id not in graphs:
        raise ValueError(f"ModifiedHorizonNet (MHNet) predictions missing for {floor_id} of ZInD Building {building_id}.")
    return graphs[floor_id]


def get_floor_id_from_img_fpath(img_fpath: str) -> str:
    """`.../floor_01_partial_room_03_pano_13.jpg` -> `floor_01` (hnet_prediction_loader.py:225-235)."""
    fname = Path(img_fpath).name
    return fname[:fname.find("_partial")]
