"""The floor reconstruction report: how good is a floor's estimated pose graph?  The four numbers the reference is judged by -- mean rotation
error, mean translation error in metres, percent of panoramas localized, floor-plan IoU -- for every floor in two calls on the device
(include/salve_hip.h: salve_floor_align, salve_floor_iou; salve_amd/csrc/floor_report.hip).

Stands behind FloorReconstructionReport.from_est_floor_pose_graph (salve/common/floor_reconstruction_report.py:50-149, 271-338, 353-372), which
every branch of the reference's scripts/run_sfm.py:440-484 ends in: the RANSAC Sim(3) alignment of the estimate to the ground truth
(salve/utils/ransac.py, posegraph2d.py:326-383), the pose errors, and the raster IoU of the room polygons.  The random subsets are drawn HERE,
on the host (`draw_alignment_subsets`, ransac.py:41-59); everything behind the draw runs on the device.

    reports = floor_report.report(pose_graph.solve(meas, thr), [FloorTruth.from_zind_json(path, floor_id), ...])
    print(floor_report.summarize(reports))

NOT here: plots, inferred layouts, room clustering, the success-rate thresholds, drawing on the device, floors of more
than 256 panoramas.
"""

from __future__ import annotations

import ctypes
import json
import math
import os
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from salve_amd import _lib
from salve_amd.common.sim2 import Sim2
from salve_amd.utils.rotation_utils import rotmat2d

ZIND_AVERAGE_SCALE_METERS_PER_COORDINATE = 3.5083   # posegraph2d.py:37
DEFAULT_DELETE_FRAC = 0.33                                      # ransac.py:11
IOU_IMG_H = IOU_IMG_W = 501                                     # BEVParams(500, 500, 0.1), drawn into (img_h + 1) x (img_w + 1)
IOU_OFFSET_M, IOU_PX_PER_M = 25.0, 1 / 0.1


@dataclass
class FloorTruth:
    """The ground truth of one floor: what the reference's PoseGraph2d holds of get_gt_pose_graph (posegraph2d.py:531-585)."""

    building_id: str
    floor_id: str
    pano_ids: np.ndarray                   # [n] int64, ascending: compact index k is pano_ids[k]
    R: np.ndarray                          # [n, 2, 2] float32: global_Sim2_local
    t: np.ndarray                          # [n, 2] float32
    s: np.ndarray                          # [n] float64
    room_vertices: List[np.ndarray]        # per panorama [k, 2] float64: room_vertices_local_2d (x already negated)
    scale_meters_per_coordinate: float
    gt_scale: float                        # the scale of the first panorama in file order (posegraph2d.py:346-347)

    def __post_init__(self) -> None:
        n = len(self.pano_ids)
        self.pano_ids = np.asarray(self.pano_ids, dtype=np.int64).reshape(n)
        self.R, self.t = np.asarray(self.R, dtype=np.float32).reshape(n, 2, 2), np.asarray(self.t, dtype=np.float32).reshape(n, 2)
        self.s = np.asarray(self.s, dtype=np.float64).reshape(n)
        self.room_vertices = [np.asarray(v, dtype=np.float64).reshape(-1, 2) for v in self.room_vertices]
        if len(self.room_vertices) != n:
            raise ValueError("FloorTruth: one room polygon per panorama")
        if n and (np.diff(self.pano_ids) <= 0).any():
            raise ValueError("FloorTruth: pano_ids must ascend strictly")

    @classmethod
    def from_zind_json(cls, path, floor_id: str, building_id: Optional[str] = None) -> "FloorTruth":
        """Host parser of a ZInD zind_data.json: the `merger` annotation of `floor_id`, every panorama's `layout_raw` vertices with x negated
        (pano_data.py:91-94), its pose as generate_Sim2_from_floorplan_transform gives it (:242-274: the reflection, t / scale, R of -rotation),
        its id from the image name (:87), and the scale imputation of posegraph2d.py:565-579.  building_id defaults to the directory's name."""
        path = Path(path)
        with open(path) as f:
            d = json.load(f)
        if "merger" not in d or floor_id not in d["merger"]:
            raise ValueError(f"{path}: no `merger` annotation of {floor_id}")
        scales = d["scale_meters_per_coordinate"]
        scale = scales[floor_id]
        if scale is None:
            valid = [v for v in scales.values() if v is not None]
            scale = float(np.mean(valid)) if valid else ZIND_AVERAGE_SCALE_METERS_PER_COORDINATE
        nodes: Dict[int, Any] = {}   # {p.id: p}: a repeated id keeps its first place and its last value (posegraph2d.py:114)
        for complete_room in d["merger"][floor_id].values():
            for partial_room in complete_room.values():
                for pano in partial_room.values():
                    pano_id = int(Path(pano["image_path"]).stem.split("_")[-1])
                    tf = pano["floor_plan_transformation"]
                    S = Sim2(rotmat2d(-tf["rotation"]), np.array(tf["translation"]) / tf["scale"] * np.array([-1.0, 1.0]), float(tf["scale"]))
                    v = np.asarray(pano["layout_raw"]["vertices"], dtype=np.float64).reshape(-1, 2).copy()
                    v[:, 0] *= -1
                    nodes[pano_id] = (S, v)
        if not nodes:
            raise ValueError(f"{path}: {floor_id} has no panorama")
        gt_scale = next(iter(nodes.values()))[0].scale
        ids = sorted(nodes)
        return cls(building_id if building_id is not None else path.resolve().parent.name, floor_id, np.array(ids), np.stack([nodes[i][0].rotation for i in ids]),
                   np.stack([nodes[i][0].translation for i in ids]), np.array([nodes[i][0].scale for i in ids]), [nodes[i][1] for i in ids],
                   float(scale), float(gt_scale))


def keep_masks(n_valid_keep: Sequence[Sequence[int]]) -> np.ndarray:
    """uint32 [H, 8]: bit k of hypothesis h is set iff compact index k is kept."""
    bits = np.zeros((len(n_valid_keep), 32 * _lib.FLOOR_MASK_WORDS), dtype=bool)
    for h, keep in enumerate(n_valid_keep):
        bits[h, np.asarray(keep, dtype=np.int64)] = True   # (IndexError for an index beyond the 256 a floor may have)
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32)


def draw_alignment_subsets(valid: Sequence[Sequence[int]], num_iters: int = 1000, delete_frac: float = DEFAULT_DELETE_FRAC,
                           seed: int = 0) -> List[np.ndarray]:
    """Host only: per floor the KEEP masks (uint32 [H, 8]) ransac_align_poses_sim3_ignore_missing would evaluate (ransac.py:41-59) after
    np.random.seed(seed), the floors consumed in order from ONE state.  valid[f]: the compact indices present in floor f's estimate, ascending.
    nd = ceil(delete_frac * len(valid)); with len(valid) - nd < 2 there is ONE hypothesis that keeps all of `valid` and no draw is consumed;
    otherwise num_iters draws of choice(valid, nd, replace=False), each keeping `valid` minus the draw."""
    rs = np.random.RandomState(seed)
    out = []
    for v in valid:
        v = np.asarray(v, dtype=np.int64).reshape(-1)
        nd = math.ceil(delete_frac * len(v))
        if len(v) - nd < 2:
            out.append(keep_masks([v]))
            continue
        keeps = []
        for _ in range(num_iters):
            drawn = rs.choice(a=v, size=nd, replace=False)
            keeps.append(np.setdiff1d(v, drawn))
        out.append(keep_masks(keeps))
    return out


@dataclass
class FloorReport:
    building_id: str
    floor_id: str
    avg_abs_rot_err: float                  # degrees; NaN: not aligned
    avg_abs_trans_err: float                # metres
    percent_panos_localized: float
    floorplan_iou: float
    pano_ids: np.ndarray                    # the truth's, ascending
    rotation_errors: np.ndarray             # per pano id of pano_ids, NaN where the estimate has none
    translation_errors: np.ndarray          # ... in coordinate units, as the reference's array
    aligned_wSi_list: List[Optional[Sim2]]  # by pano id: the estimate in the truth's frame, scale gt_scale
    scale_meters_per_coordinate: float
    best: Optional[int] = None              # the winning subset; None: not aligned
    aSb: Optional[Dict[str, Any]] = None    # the winner's R (4), t (2), s in float64
    counts: Dict[str, int] = field(default_factory=dict)   # n_hyps, n_est, n_gt, iou_n_est, iou_n_gt, iou_inter, iou_union

    def __repr__(self) -> str:
        return (f"Abs. Rot err (deg) {self.avg_abs_rot_err:.1f}, Abs. trans err {self.avg_abs_trans_err:.2f}, "
                f"%Localized {self.percent_panos_localized:.2f},Floorplan IoU {self.floorplan_iou:.2f}")

    def summary(self) -> str:
        return f"{self.building_id} {self.floor_id}: {self!r}"

    @property
    def wSi_dict(self) -> Dict[int, Dict[str, Any]]:
        """serialize_predicted_pose_graph's `wSi_dict` (floor_reconstruction_report.py:191-217)."""
        return {i: {"R": S.rotation.tolist(), "t": S.translation.tolist(), "s": S.scale} for i, S in enumerate(self.aligned_wSi_list) if S is not None}

    def to_json(self) -> Dict[str, Any]:
        fin = lambda x: None if x is None or x != x else float(x)
        return {"building_id": self.building_id, "floor_id": self.floor_id, "scale_meters_per_coordinate": self.scale_meters_per_coordinate,
                "avg_abs_rot_err": fin(self.avg_abs_rot_err), "avg_abs_trans_err": fin(self.avg_abs_trans_err),
                "percent_panos_localized": fin(self.percent_panos_localized), "floorplan_iou": fin(self.floorplan_iou),
                "pano_ids": [int(p) for p in self.pano_ids], "rotation_errors": [fin(x) for x in self.rotation_errors],
                "translation_errors": [fin(x) for x in self.translation_errors], "best": self.best, "aSb": self.aSb,
                "counts": {k: int(v) for k, v in self.counts.items()}, "n_poses": len(self.aligned_wSi_list),
                "wSi_dict": {str(k): v for k, v in self.wSi_dict.items()}}

    @classmethod
    def from_json(cls, d: Dict[str, Any]) -> "FloorReport":
        nan = lambda x: float("nan") if x is None else float(x)
        wSi: List[Optional[Sim2]] = [None] * d["n_poses"]
        for k, r in d["wSi_dict"].items():
            wSi[int(k)] = Sim2(np.array(r["R"], dtype=np.float32).reshape(2, 2), np.array(r["t"], dtype=np.float32), float(r["s"]))
        return cls(d["building_id"], d["floor_id"], nan(d["avg_abs_rot_err"]), nan(d["avg_abs_trans_err"]), nan(d["percent_panos_localized"]),
                   nan(d["floorplan_iou"]), np.array(d["pano_ids"], dtype=np.int64), np.array([nan(x) for x in d["rotation_errors"]]),
                   np.array([nan(x) for x in d["translation_errors"]]), wSi, float(d["scale_meters_per_coordinate"]), d["best"], d["aSb"],
                   dict(d["counts"]))


METRICS = ("avg_abs_rot_err", "avg_abs_trans_err", "percent_panos_localized", "floorplan_iou")


def summarize(reports: Sequence[FloorReport]) -> Dict[str, Any]:
    """summarize_reports (floor_reconstruction_report.py:353-372): the nanmean and nanmedian of the four metrics over the floors."""
    out: Dict[str, Any] = {"n_floors": len(reports)}
    for m in METRICS:
        vals = np.array([getattr(r, m) for r in reports], dtype=np.float64)
        ok = vals[~np.isnan(vals)]
        out[m] = {"mean": float(ok.mean()) if len(ok) else float("nan"), "median": float(np.median(ok)) if len(ok) else float("nan")}
    return out


def _wSi_list(solution) -> Optional[List[Optional[Sim2]]]:
    return solution.wSi_list if hasattr(solution, "wSi_list") else (None if solution is None else list(solution))


def pack_tables(estimates: Sequence[Optional[Sequence[Optional[Sim2]]]], truths: Sequence[FloorTruth]) -> Dict[str, np.ndarray]:
    """Host only: the device tables of salve_floor_align and salve_floor_iou for these floors (without the hypotheses).  An estimated panorama
    that the truth does not hold is refused (the reference fails at gt_floor_pg.nodes[i])."""
    node_dt = _lib.GRAPH_NODE_OUT_DTYPE
    node_start = np.concatenate([[0], np.cumsum([len(tr.pano_ids) for tr in truths])]).astype(np.int32)
    N = int(node_start[-1])
    truth, est = np.zeros(N, dtype=node_dt), np.zeros(N, dtype=node_dt)
    truth["parent"] = truth["depth"] = est["parent"] = est["depth"] = -1
    valid, room, room_off = [], [], [0]
    for f, (wSi, tr) in enumerate(zip(estimates, truths)):
        n, lo = len(tr.pano_ids), int(node_start[f])
        if n > _lib.GRAPH_MAX_NODES:
            raise _lib.SalveHipError(f"floor_report: floor {tr.building_id} {tr.floor_id} has {n} panoramas, more than the {_lib.GRAPH_MAX_NODES} "
                                     "a floor may have")
        t = truth[lo:lo + n]
        t["localized"], t["R"], t["t"], t["s"] = 1, tr.R.reshape(n, 4), tr.t, tr.s
        v = []
        for p, S in enumerate(wSi or []):
            if S is None:
                continue
            k = int(np.searchsorted(tr.pano_ids, p))
            if k >= n or tr.pano_ids[k] != p:
                raise ValueError(f"floor_report: floor {tr.building_id} {tr.floor_id}: the estimate localizes panorama {p}, which the truth does not hold")
            e = est[lo + k]
            e["localized"], e["R"], e["t"], e["s"] = 1, np.asarray(S.rotation, dtype=np.float32).reshape(4), np.asarray(S.translation, dtype=np.float32), 1.0
            v.append(k)
        valid.append(np.array(v, dtype=np.int64))
        for verts in tr.room_vertices:
            room.append(verts)
            room_off.append(room_off[-1] + len(verts))
    room_xy = np.concatenate(room).reshape(-1, 2) if room else np.zeros((0, 2))
    return {"node_start": node_start, "truth": truth, "est": est, "valid": valid, "room_xy": np.ascontiguousarray(room_xy, dtype=np.float64),
            "room_off": np.array(room_off, dtype=np.int64), "gt_scale": np.array([tr.gt_scale for tr in truths], dtype=np.float64),
            "metres": np.array([tr.scale_meters_per_coordinate for tr in truths], dtype=np.float64)}


def _align16(n: int) -> int:
    return (n + 15) & ~15


def report(solutions: Sequence[Any], truths: Sequence[FloorTruth], num_iters: int = 1000, delete_frac: float = DEFAULT_DELETE_FRAC, seed: int = 0,
           device="cuda:0") -> List[FloorReport]:
    """One FloorReport per floor: solutions[f] (a pose_graph.FloorSolution, a TreeSampleSolution, or a plain wSi_list indexed by pano id; None or
    a solution without poses: nothing localized) against truths[f].  One upload, two calls (salve_floor_align, salve_floor_iou), one read of
    the device status word, one download.  A floor with no pose is reported NaN, NaN, 0, 0 as run_sfm.py:309-311 does."""
    import torch

    from salve_amd import status

    if len(solutions) != len(truths):
        raise ValueError(f"floor_report.report: {len(solutions)} solutions for {len(truths)} truths")
    for sol, tr in zip(solutions, truths):
        if hasattr(sol, "building_id") and (str(sol.building_id), str(sol.floor_id)) != (str(tr.building_id), str(tr.floor_id)):
            raise ValueError(f"floor_report.report: solution of {sol.building_id} {sol.floor_id} against the truth of {tr.building_id} {tr.floor_id}")
    F = len(truths)
    if F == 0:
        return []
    device = torch.device(device)
    lib = _lib.load()
    tb = pack_tables([_wSi_list(s) for s in solutions], truths)
    masks = draw_alignment_subsets(tb["valid"], num_iters, delete_frac, seed)
    hyp_start = np.concatenate([[0], np.cumsum([len(m) for m in masks])]).astype(np.int32)
    all_masks = np.concatenate(masks).astype(np.uint32)
    H, N, V = int(hyp_start[-1]), int(tb["node_start"][-1]), len(tb["room_xy"])

    parts = [tb["room_xy"].reshape(-1), tb["room_off"], tb["gt_scale"], tb["metres"], tb["truth"], tb["est"], tb["node_start"], hyp_start, all_masks.reshape(-1)]
    offs, blob = [], []
    for x in parts:   # (every table on a 16-byte boundary)
        offs.append(sum(len(b) for b in blob))
        raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        blob += [raw, np.zeros(_align16(len(raw)) - len(raw), dtype=np.uint8)]
    hyp_dt, fl_dt, iou_dt, node_dt = _lib.FLOOR_HYP_OUT_DTYPE, _lib.FLOOR_ALIGN_OUT_DTYPE, _lib.FLOOR_IOU_OUT_DTYPE, _lib.GRAPH_NODE_OUT_DTYPE
    sizes = [H * hyp_dt.itemsize, N * node_dt.itemsize, N * 8, N * 8, F * fl_dt.itemsize, F * iou_dt.itemsize]
    o = np.concatenate([[0], np.cumsum([_align16(x) for x in sizes])]).astype(np.int64)
    with torch.cuda.device(device):
        dev_in = torch.from_numpy(np.concatenate(blob)).to(device)
        dev_out = torch.empty(max(int(o[-1]), 16), dtype=torch.uint8, device=device)
        ws_bytes = int(lib.salve_floor_iou_workspace_bytes(V, N))
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)
        vp = ctypes.c_void_p
        pin = lambda i: vp(dev_in.data_ptr() + offs[i])
        pout = lambda i: vp(dev_out.data_ptr() + int(o[i]))
        stream = vp(torch.cuda.current_stream(device).cuda_stream)
        _lib.check(lib.salve_floor_align(pin(6), F, N, pin(4), pin(5), pin(7), pin(8), H, pin(2), pin(3), pout(0), pout(1), pout(2), pout(3), pout(4),
                                         status.ptr(device), stream), "salve_floor_align")
        _lib.check(lib.salve_floor_iou(pin(0), pin(1), V, pin(6), F, N, pout(1), pin(4), pin(3), IOU_IMG_H, IOU_IMG_W, IOU_OFFSET_M, IOU_OFFSET_M,
                                       IOU_PX_PER_M, pout(5), None, vp(ws.data_ptr()), ws_bytes, status.ptr(device), stream), "salve_floor_iou")
        status.check(device, "floor_report.report")   # (the one synchronising read)
        host = dev_out.cpu().numpy()
    nodes = host[o[1]:o[1] + sizes[1]].view(node_dt)
    rot, trans = host[o[2]:o[2] + sizes[2]].view(np.float64), host[o[3]:o[3] + sizes[3]].view(np.float64)
    floors, ious = host[o[4]:o[4] + sizes[4]].view(fl_dt), host[o[5]:o[5] + sizes[5]].view(iou_dt)

    reports = []
    for f, tr in enumerate(truths):
        lo, hi = int(tb["node_start"][f]), int(tb["node_start"][f + 1])
        fo, io = floors[f], ious[f]
        best = int(fo["best"]) if fo["best"] >= 0 else None
        wSi: List[Optional[Sim2]] = [None] * (int(tr.pano_ids[-1]) + 1 if hi > lo else 0)
        for k in np.nonzero(nodes["localized"][lo:hi])[0]:
            r = nodes[lo + k]
            wSi[int(tr.pano_ids[k])] = Sim2(np.array(r["R"], dtype=np.float32).reshape(2, 2), np.array(r["t"], dtype=np.float32), float(r["s"]))
        aSb = None if best is None else {"R": [float(x) for x in fo["R"]], "t": [float(x) for x in fo["t"]], "s": float(fo["s"])}
        counts = {"n_hyps": int(fo["n_hyps"]), "n_est": int(fo["n_est"]), "n_gt": int(fo["n_gt"]), "iou_n_est": int(io["n_est"]),
                  "iou_n_gt": int(io["n_gt"]), "iou_inter": int(io["inter"]), "iou_union": int(io["uni"])}
        reports.append(FloorReport(tr.building_id, tr.floor_id, float(fo["avg_rot_err"]), float(fo["avg_trans_err"]), float(fo["percent_localized"]),
                                   float(io["iou"]), tr.pano_ids.copy(), rot[lo:hi].copy(), trans[lo:hi].copy(), wSi, tr.scale_meters_per_coordinate,
                                   best, aSb, counts))
    return reports


def load_truths(zind_root: str, floors: Sequence[Any]) -> List[FloorTruth]:
    """FloorTruth.from_zind_json of {zind_root}/{building}/zind_data.json for every (building_id, floor_id) of `floors` (solutions, or pairs)."""
    keys = [(s.building_id, s.floor_id) if hasattr(s, "building_id") else tuple(s) for s in floors]
    return [FloorTruth.from_zind_json(f"{zind_root}/{b}/zind_data.json", fl, building_id=str(b)) for b, fl in keys]


def json_fname(rep: FloorReport) -> str:
    return f"floor_report_{rep.building_id}_{rep.floor_id}.json"


def write_json(rep: FloorReport, out_dir: str) -> str:
    os.makedirs(out_dir, exist_ok=True)
    fp = f"{out_dir}/{json_fname(rep)}"
    with open(fp, "w") as f:
        json.dump(rep.to_json(), f, indent=4)
    return fp
