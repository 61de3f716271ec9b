"""Modified HorizonNet (MHNet) predictions of one panorama -> its layout: the reference's salve/dataset/mhnet_prediction.py without rdp,
matplotlib or cv2.  Host only.

Deviations: the Ramer-Douglas-Peucker simplification is restated here (`rdp_iter`, the `rdp` package's default iterative algorithm as its
documentation gives it); the package is not installed where this is built, so parity with it is unpinned -- the room polygon feeds only the
layout modality, never the alignment hypotheses.  `corners_in_uv` and `floor_boundary_uncertainty` may be absent from a prediction file
(empty arrays then): neither is read by anything behind this loader."""

from __future__ import annotations

import json
from dataclasses import dataclass
from pathlib import Path
from typing import Any, List, Optional

import numpy as np

from salve_amd.common.pano_data import WDO, PanoData, PoseGraph2d
from salve_amd.utils import zind_pano_utils

RAMER_DOUGLAS_PEUCKER_EPSILON = 0.02


@dataclass
class MHNetDWO:
    """Start and end column of a door, window or opening, in [0, 1] (mhnet_prediction.py:36-55)."""

    s: float
    e: float

    @classmethod
    def from_json(cls, json_data: Any) -> "MHNetDWO":
        if len(json_data) != 2:
            raise RuntimeError("Schema error...")
        s, e = json_data
        return cls(s=s, e=e)


def merge_wdos_straddling_img_border(wdo_instances: List[MHNetDWO]) -> List[MHNetDWO]:
    """An object the panorama seam split in two becomes one (mhnet_prediction.py:286-333): with one object starting below 0.01 and one ending
    above 0.99, the FIRST of each kind are taken out and their merger (start of the right one, end of the left one) is appended."""
    if len(wdo_instances) <= 1:
        return wdo_instances
    straddles_left = [wdo.s < 0.01 for wdo in wdo_instances]
    straddles_right = [wdo.e > 0.99 for wdo in wdo_instances]
    if not (any(straddles_left) and any(straddles_right)):
        return wdo_instances
    left_idx, right_idx = int(np.argmax(np.array(straddles_left))), int(np.argmax(np.array(straddles_right)))
    merged = [wdo for i, wdo in enumerate(wdo_instances) if i not in (left_idx, right_idx)]
    merged.append(MHNetDWO(s=wdo_instances[right_idx].s, e=wdo_instances[left_idx].e))
    return merged


def _pldist(point: np.ndarray, start: np.ndarray, end: np.ndarray) -> float:
    """Distance of `point` from the line through start and end (from `start` when they coincide)."""
    if np.all(np.equal(start, end)):
        return float(np.linalg.norm(point - start))
    d, v = end - start, start - point
    return float(abs(d[0] * v[1] - d[1] * v[0]) / np.linalg.norm(d))


def rdp_iter(M: np.ndarray, epsilon: float) -> np.ndarray:
    """Ramer-Douglas-Peucker on the polyline M [n, 2], iteratively with a stack: a span keeps the point furthest from its chord (the first
    among equals) when that distance exceeds epsilon, else drops every point strictly inside it."""
    M = np.asarray(M, dtype=np.float64)
    n = len(M)
    keep = np.ones(n, dtype=bool)
    stack = [(0, n - 1)]
    while stack:
        start, last = stack.pop()
        dmax, index = 0.0, start
        for i in range(index + 1, last):
            if keep[i]:
                d = _pldist(M[i], M[start], M[last])
                if d > dmax:
                    index, dmax = i, d
        if dmax > epsilon:
            stack.append((start, index))
            stack.append((index, last))
        else:
            keep[start + 1:last] = False
    return M[keep]


@dataclass
class MHNetPanoStructurePrediction:
    """What MHNet predicted for one panorama (mhnet_prediction.py:58-132)."""

    corners_in_uv: np.ndarray
    image_height: int
    image_width: int
    floor_boundary: np.ndarray
    floor_boundary_uncertainty: np.ndarray
    doors: List[MHNetDWO]
    openings: List[MHNetDWO]
    windows: List[MHNetDWO]
    image_fpath: Path

    @classmethod
    def from_json_fpath(cls, json_fpath: Path, image_fpath: Path) -> "MHNetPanoStructurePrediction":
        for name, p in (("Image", image_fpath), ("JSON", json_fpath)):
            if not isinstance(p, Path):
                raise ValueError(f"{name} file path provided to `MHNetPanoStructurePrediction` must be a `pathlib.Path` object.")
        if not json_fpath.exists():
            raise ValueError(f"No JSON file found at {json_fpath} while loading `MHNetPanoStructurePrediction`.")
        with open(json_fpath) as f:
            d = json.load(f)["predictions"]
        wdos = {k: merge_wdos_straddling_img_border([MHNetDWO.from_json(w) for w in d["wall_features"][k]]) for k in ("door", "window", "opening")}
        raw = d["room_shape"].get("raw_predictions", {})
        return cls(corners_in_uv=np.array(d["room_shape"].get("corners_in_uv", [])).reshape(-1, 2), image_height=d["image_height"],
                   image_width=d["image_width"], floor_boundary=np.array(raw["floor_boundary"], dtype=np.float64),
                   floor_boundary_uncertainty=np.array(raw.get("floor_boundary_uncertainty", []), dtype=np.float64), doors=wdos["door"],
                   openings=wdos["opening"], windows=wdos["window"], image_fpath=image_fpath)

    def convert_to_pano_data(self, img_h: int, img_w: int, pano_id: int, gt_pose_graph: PoseGraph2d, img_fpath: str,
                             vanishing_angle_deg: Optional[float]) -> PanoData:
        """mhnet_prediction.py:191-283: the 1024 rounded boundary points through convert_points_px_to_worldmetric at a camera height of 1.0 and
        Ramer-Douglas-Peucker at epsilon 0.02; a W/D/O's end columns are clip(s * W, 0, W - 1), their rows floor_boundary[round(u)] (Python's
        round: half to even) and both through the same conversion.  Pose and label are the ground truth's."""
        camera_height_m = 1.0   # (the reference overrides the floor's camera height with 1.0)
        u, v = np.arange(1024), np.round(self.floor_boundary)
        boundary_px = np.hstack([u.reshape(-1, 1), v.reshape(-1, 1)])
        room = zind_pano_utils.convert_points_px_to_worldmetric(points_px=boundary_px, image_width=img_w, camera_height_m=camera_height_m)
        room = rdp_iter(room[:, :2], epsilon=RAMER_DOUGLAS_PEUCKER_EPSILON)
        gt = gt_pose_graph.nodes[pano_id]
        out = {"windows": [], "doors": [], "openings": []}
        for wdo_type, instances in (("windows", self.windows), ("doors", self.doors), ("openings", self.openings)):
            for wdo in instances:
                s_u = np.clip(wdo.s * img_w, a_min=0, a_max=img_w - 1)
                e_u = np.clip(wdo.e * img_w, a_min=0, a_max=img_w - 1)
                s_v, e_v = self.floor_boundary[round(float(s_u))], self.floor_boundary[round(float(e_u))]
                ends = zind_pano_utils.convert_points_px_to_worldmetric(points_px=np.array([[s_u, s_v], [e_u, e_v]]), image_width=img_w,
                                                                        camera_height_m=camera_height_m)
                out[wdo_type].append(WDO(gt.global_Sim2_local, (float(ends[0, 0]), float(ends[0, 1])), (float(ends[1, 0]), float(ends[1, 1])),
                                         -np.nan, np.nan, wdo_type))
        return PanoData(pano_id, gt.global_Sim2_local, room, img_fpath, gt.label, out["doors"], out["windows"], out["openings"], vanishing_angle_deg)
