"""A floor's panoramas as the reference holds them -- the parts of salve/common/wdo.py, salve/common/pano_data.py and
salve/common/posegraph2d.py that the layout modality and the alignment hypotheses read.  Host only.

`PoseGraph2d.nodes[i]` offers `room_vertices_local_2d`, `doors`, `windows`, `openings`; every W/D/O offers `.type` and `.vertices_local_2d`:
what layout.PanoLayouts.from_pose_graph and layout.FusedLayouts.from_pose_graph take."""

from __future__ import annotations

import json
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from salve_amd.common.sim2 import Sim2
from salve_amd.utils.rotation_utils import rotmat2d

ZIND_AVERAGE_SCALE_METERS_PER_COORDINATE = 3.5083   # posegraph2d.py:37 (floor_report.py holds the same constant)


@dataclass
class WDO:
    """One window, door or opening: the segment pt1 -> pt2 in its panorama's frame (wdo.py:12-56)."""

    global_Sim2_local: Sim2
    pt1: Tuple[float, float]
    pt2: Tuple[float, float]
    bottom_z: float
    top_z: float
    type: str           # "windows", "doors" or "openings"

    @property
    def width(self) -> float:
        return float(np.linalg.norm(np.array(self.pt1) - np.array(self.pt2)))

    @property
    def vertices_local_2d(self) -> np.ndarray:
        return np.array([self.pt1, self.pt2], dtype=np.float64)

    @property
    def vertices_global_2d(self) -> np.ndarray:
        return self.global_Sim2_local.transform_from(self.vertices_local_2d)

    def get_rotated_version(self) -> "WDO":
        return WDO(self.global_Sim2_local, self.pt2, self.pt1, self.bottom_z, self.top_z, self.type)


@dataclass
class PanoData:
    """One panorama: its pose, room and W/D/Os (pano_data.py:39-132)."""

    id: int
    global_Sim2_local: Sim2
    room_vertices_local_2d: np.ndarray
    image_path: str
    label: str
    doors: List[WDO] = field(default_factory=list)
    windows: List[WDO] = field(default_factory=list)
    openings: List[WDO] = field(default_factory=list)
    vanishing_angle_deg: Optional[float] = None

    @classmethod
    def from_json(cls, pano_data: Any) -> "PanoData":
        """The `merger` annotation of one panorama, `layout_raw` (pano_data.py:72-132): x negated in room and W/D/O vertices, the pose of
        generate_Sim2_from_floorplan_transform (:242-274).  A camera height other than 1.0 is refused, as the reference's assert does."""
        if pano_data["camera_height"] != 1.0:
            raise ValueError(f"camera_height must be 1.0, got {pano_data['camera_height']} ({pano_data.get('image_path')})")
        image_path = pano_data["image_path"]
        pano_id = int(Path(image_path).stem.split("_")[-1])
        tf = pano_data["floor_plan_transformation"]
        S = Sim2(rotmat2d(-tf["rotation"]), np.array(tf["translation"]) / tf["scale"] * np.array([-1.0, 1.0]), float(tf["scale"]))
        room = np.asarray(pano_data["layout_raw"]["vertices"], dtype=np.float64).reshape(-1, 2).copy()
        room[:, 0] *= -1
        wdos: Dict[str, List[WDO]] = {"windows": [], "doors": [], "openings": []}
        for wdo_type in ("windows", "doors", "openings"):
            data = pano_data["layout_raw"][wdo_type]
            if len(data) % 3 != 0:
                raise ValueError(f"{image_path}: {wdo_type} must hold (pt1, pt2, (bottom_z, top_z)) triplets")
            for k in range(len(data) // 3):
                pt1, pt2, (bottom_z, top_z) = list(data[3 * k]), list(data[3 * k + 1]), data[3 * k + 2]
                pt1[0] *= -1
                pt2[0] *= -1
                wdos[wdo_type].append(WDO(S, (pt1[0], pt1[1]), (pt2[0], pt2[1]), bottom_z, top_z, wdo_type))
        return cls(pano_id, S, room, image_path, pano_data["label"], wdos["doors"], wdos["windows"], wdos["openings"], None)


@dataclass
class PoseGraph2d:
    """The panoramas of one floor by id (posegraph2d.py:44-116)."""

    building_id: str
    floor_id: str
    nodes: Dict[int, PanoData]
    scale_meters_per_coordinate: float

    def pano_ids(self) -> List[int]:
        return list(self.nodes.keys())


def read_zind_json(raw_dataset_dir, building_id: str) -> Dict[str, Any]:
    with open(Path(raw_dataset_dir) / building_id / "zind_data.json") as f:
        return json.load(f)


def gt_pose_graph_from_json(floor_map_json: Dict[str, Any], building_id: str, floor_id: str) -> PoseGraph2d:
    """get_gt_pose_graph (posegraph2d.py:531-585) on a parsed zind_data.json: the `merger` annotation; a repeated panorama id keeps its first
    place and its last value ({p.id: p}, :114); a floor without a scale takes the mean of the others."""
    merger = floor_map_json["merger"]
    if floor_id not in merger:
        raise ValueError(f"Invalid floor {floor_id} specified for ZInD Building {building_id}.")
    scales = floor_map_json["scale_meters_per_coordinate"]
    scale = scales[floor_id]
    if scale is None:
        valid = [v for v in scales.values() if v is not None]
        scale = float(np.mean(valid)) if valid else ZIND_AVERAGE_SCALE_METERS_PER_COORDINATE
    nodes: Dict[int, PanoData] = {}
    for complete_room in merger[floor_id].values():
        for partial_room in complete_room.values():
            for pano in partial_room.values():
                p = PanoData.from_json(pano)
                nodes[p.id] = p
    return PoseGraph2d(building_id, floor_id, nodes, float(scale))
