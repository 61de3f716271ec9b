"""Alignment hypotheses on the device: the inferred-W/D/O path (`--wdo_source horizon_net`) of the reference's
scripts/export_alignment_hypotheses.py -- every W/D/O alignment of every panorama pair of any number of floors in ONE launch of
salve_hypotheses_generate (include/salve_hip.h states the rules, salve_amd/csrc/hypotheses.hip how they run), handed on as
ingest.FloorHypotheses without a file in between.

    floors = load_floors(raw_dataset_dir, mhnet_predictions_data_root, ["0000"])     # host: ZInD's annotation + MHNet's predictions
    hyps = generate(floors, "cuda:0")                                                # device: one launch for all floors
    ingest.score_floor(..., hypotheses=hyps[0])                                      # -> predictions, pose graph, report
    write_tree(hyps, OUT)                                                            # optional: the reference's tree of JSON files

    python -m salve_amd.hypotheses --raw-dataset-dir ZIND --mhnet-predictions-data-root DIR --hypotheses-save-root OUT --split test

Not here: `--wdo_source ground_truth` (it needs overlap_utils.determine_invalid_wall_overlap, the freespace check on shrunk room polygons),
AlignTransformType.Sim3, the debug plots.  The vanishing angles are carried (FloorInput.vanishing_angle_deg) and not read here: axis alignment
is salve_amd.pose_graph's (AxisInputs.from_floors).  There is no CPU path: a missing kernel is an error."""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from salve_amd import _lib
from salve_amd.ingest import LABEL_TYPES, FloorHypotheses, FloorPairs
from salve_amd.layout import WDO_TYPES, PanoLayouts

MIN_ALLOWED_INFERRED_WDO_WIDTH_RATIO = 0.65      # wdo_alignment.py:44
MAX_PANOS_PER_FLOOR = _lib.GRAPH_MAX_NODES      # 256, as the pose graph
MAX_WDO_PER_TYPE = _lib.HYP_MAX_WDO_PER_TYPE    # 32
ALIGNMENT_OBJECTS = ("window", "door", "opening")   # by W/D/O type code (layout.WDO_TYPES: windows, doors, openings)
CONFIGURATIONS = ("identity", "rotated")
TYPE_ORDER = (1, 0, 2)                           # align_rooms_by_wd enumerates doors, windows, openings
EXCLUDED_PANOS = {"0006": 7}                     # export_alignment_hypotheses.py:167-169: an annotation error in ZInD


@dataclass
class FloorInput:
    """What the generator reads of one floor.  Panorama k of every table is pano_ids[k]; the ids ascend."""

    building_id: str
    floor_id: str
    pano_ids: np.ndarray      # [P] int64
    layouts: PanoLayouts      # the INFERRED W/D/Os (wdo_off, wdo_xy, wdo_type; the rooms are not read)
    R: np.ndarray             # [P, 2, 2] float32: the ground truth's global_Sim2_local
    t: np.ndarray             # [P, 2] float32
    s: np.ndarray             # [P] float64
    gt_wdo_off: np.ndarray    # [P + 1] int64
    gt_wdo_xy: np.ndarray     # [*, 2, 2] float64: the ground truth's W/D/Os, LOCAL frame (any order within a panorama)
    vanishing_angle_deg: Optional[np.ndarray] = None   # [P] float64, NaN where absent: MHNet's vanishing angles (the generator does not read them;
                                                       # pose_graph.AxisInputs.from_floors does)

    def __post_init__(self) -> None:
        P = len(self.pano_ids)
        if self.vanishing_angle_deg is not None:
            self.vanishing_angle_deg = np.asarray(self.vanishing_angle_deg, dtype=np.float64).reshape(-1)
            if len(self.vanishing_angle_deg) != P:
                raise ValueError(f"building {self.building_id}, {self.floor_id}: {len(self.vanishing_angle_deg)} vanishing angles for {P} panoramas")
        self.pano_ids = np.asarray(self.pano_ids, dtype=np.int64).reshape(P)
        self.R, self.t = np.asarray(self.R, dtype=np.float32).reshape(P, 2, 2), np.asarray(self.t, dtype=np.float32).reshape(P, 2)
        self.s = np.asarray(self.s, dtype=np.float64).reshape(P)
        self.gt_wdo_off = np.asarray(self.gt_wdo_off, dtype=np.int64).reshape(-1)
        self.gt_wdo_xy = np.asarray(self.gt_wdo_xy, dtype=np.float64).reshape(-1, 2, 2)
        where = f"building {self.building_id}, {self.floor_id}"
        if P > MAX_PANOS_PER_FLOOR:
            raise ValueError(f"{where}: {P} panoramas; a floor of more than {MAX_PANOS_PER_FLOOR} is not supported")
        if P and (np.diff(self.pano_ids) <= 0).any():
            raise ValueError(f"{where}: pano_ids must ascend strictly")
        if self.layouts.P != max(P, 1):   # (PanoLayouts holds at least one panorama: a floor without any carries one empty one)
            raise ValueError(f"{where}: the layout tables hold {self.layouts.P} panoramas, pano_ids {P}")
        if len(self.gt_wdo_off) != P + 1 or int(self.gt_wdo_off[0]) != 0 or int(self.gt_wdo_off[-1]) != len(self.gt_wdo_xy) or (np.diff(self.gt_wdo_off) < 0).any():
            raise ValueError(f"{where}: gt_wdo_off must rise from 0 to {len(self.gt_wdo_xy)} over {P + 1} entries")
        if not (np.isfinite(self.gt_wdo_xy).all() and np.isfinite(self.R).all() and np.isfinite(self.t).all() and np.isfinite(self.s).all()):
            raise ValueError(f"{where}: the ground truth must be finite")
        for k in range(P):
            types = self.layouts.wdo_type[int(self.layouts.wdo_off[k]):int(self.layouts.wdo_off[k + 1])]
            counts = np.bincount(types, minlength=3)
            if int(counts.max(initial=0)) > MAX_WDO_PER_TYPE:
                T = int(np.argmax(counts))
                raise ValueError(f"{where}, panorama {int(self.pano_ids[k])}: {int(counts[T])} {WDO_TYPES[T]}; more than {MAX_WDO_PER_TYPE} W/D/Os of "
                                 "one type in a panorama are not supported")

    @classmethod
    def from_pose_graphs(cls, gt_graph, inferred_graph) -> "FloorInput":
        """gt_graph, inferred_graph: salve_amd.common.pano_data.PoseGraph2d of one floor -- the `merger` annotation and
        hnet_prediction_loader's result.  A panorama of the floor without MHNet prediction raises ValueError, as the reference's exporter does
        when it reaches the panorama's first pair (export_alignment_hypotheses.py:180-184)."""
        ids = sorted(gt_graph.nodes)
        if len(ids) > 1:
            for i in ids:
                if i not in inferred_graph.nodes and EXCLUDED_PANOS.get(gt_graph.building_id) != i:
                    raise ValueError(f"MHNet predictions for pano {i} are missing for Building {gt_graph.building_id}.")
        empty = type("EmptyNode", (), {"room_vertices_local_2d": np.zeros((0, 2)), "doors": [], "windows": [], "openings": []})()
        nodes = {i: inferred_graph.nodes.get(i, empty) for i in ids}
        layouts = PanoLayouts.from_pose_graph(type("Graph", (), {"nodes": nodes})(), ids) if ids else _no_layouts()
        gt = [[w.vertices_local_2d for w in gt_graph.nodes[i].windows + gt_graph.nodes[i].doors + gt_graph.nodes[i].openings] for i in ids]
        flat = [v for ws in gt for v in ws]
        poses = [gt_graph.nodes[i].global_Sim2_local for i in ids]
        return cls(gt_graph.building_id, gt_graph.floor_id, np.array(ids, dtype=np.int64), layouts,
                   np.array([S.rotation for S in poses], dtype=np.float32).reshape(-1, 2, 2), np.array([S.translation for S in poses], dtype=np.float32).reshape(-1, 2),
                   np.array([S.scale for S in poses], dtype=np.float64), np.concatenate([[0], np.cumsum([len(ws) for ws in gt])]).astype(np.int64),
                   np.stack(flat) if flat else np.zeros((0, 2, 2)),
                   np.array([np.nan if getattr(nodes[i], "vanishing_angle_deg", None) is None else nodes[i].vanishing_angle_deg for i in ids], dtype=np.float64))


def _no_layouts() -> PanoLayouts:
    """PanoLayouts holds at least one panorama; a floor without any carries one empty panorama that no pair names."""
    return PanoLayouts(np.zeros(2, np.int64), np.zeros((0, 2)), np.zeros(2, np.int64), np.zeros((0, 2, 2)), np.zeros(0, np.uint8))


def load_floors(raw_dataset_dir, mhnet_predictions_data_root, building_ids: Sequence[str]) -> List[FloorInput]:
    """Every floor of the buildings, in the reference's order (buildings sorted, floors in the annotation's order).  A building without
    `merger` data is skipped, as export_single_building_wdo_alignment_hypotheses does (:131-133)."""
    from salve_amd.common.pano_data import gt_pose_graph_from_json, read_zind_json
    from salve_amd.dataset import hnet_prediction_loader

    floors = []
    for building_id in sorted(building_ids):
        d = read_zind_json(raw_dataset_dir, building_id)
        if "merger" not in d:
            print(f"Building {building_id} does not have `merger` data, skipping...", file=sys.stderr)
            continue
        graphs = hnet_prediction_loader.load_inferred_floor_pose_graphs(building_id, raw_dataset_dir, mhnet_predictions_data_root)
        for floor_id in d["merger"]:
            floors.append(FloorInput.from_pose_graphs(gt_pose_graph_from_json(d, building_id, floor_id), graphs[floor_id]))
    return floors


@dataclass
class PackedFloors:
    """The host tables of one call (include/salve_hip.h: salve_hypotheses_generate), all floors behind one another."""

    floors: List[FloorInput]
    wdo_xy: np.ndarray        # float64 [n_wdo, 2, 2]
    wdo_type: np.ndarray      # uint8 [n_wdo]
    wdo_off: np.ndarray       # int64 [n_panos + 1]
    gt_xy: np.ndarray         # float64 [n_gt, 2, 2]: GLOBAL frame
    gt_off: np.ndarray        # int64 [n_panos + 1]
    poses: np.ndarray         # GRAPH_NODE_OUT_DTYPE [n_panos]
    pairs: np.ndarray         # HYP_PAIR_DTYPE [n_pairs]
    pair_floor: np.ndarray    # int64 [n_pairs]: the floor of a pair
    pair_ids: np.ndarray      # int64 [n_pairs, 2]: its two panorama ids
    n_rows: int
    max_capacity: int


def gt_global(xy: np.ndarray, R: np.ndarray, t: np.ndarray, s: float) -> np.ndarray:
    """WDO.vertices_global_2d = Sim2.transform_from: ((p @ R.T) + t) * s in float64 with R and t widened -- spelled out per entry, each
    product and sum on its own, so that the result does not depend on a BLAS."""
    R, t = R.astype(np.float64), t.astype(np.float64)
    x, y = xy[..., 0], xy[..., 1]
    return np.stack([((x * R[0, 0] + y * R[0, 1]) + t[0]) * s, ((x * R[1, 0] + y * R[1, 1]) + t[1]) * s], axis=-1)


def pack(floors: Sequence[FloorInput]) -> PackedFloors:
    """Host: concatenates the floors' tables, moves the ground truth's W/D/Os into the global frame, and names the pairs: per floor i1 < i2 over
    the ascending panorama ids, without the pairs of EXCLUDED_PANOS; a pair's capacity is its candidate count 2 d1 d2 + w1 w2 + 2 o1 o2 and its
    row offset the exclusive scan of the capacities."""
    floors = list(floors)
    n_panos = sum(len(f.pano_ids) for f in floors)
    wdo_xy, wdo_type, gt_xy, pairs, pair_floor, pair_ids = [], [], [], [], [], []
    wdo_off, gt_off = np.zeros(n_panos + 1, np.int64), np.zeros(n_panos + 1, np.int64)
    poses = np.zeros(n_panos, dtype=_lib.GRAPH_NODE_OUT_DTYPE)
    base = 0
    for fi, f in enumerate(floors):
        P = len(f.pano_ids)
        if P == 0:
            continue
        counts = np.diff(f.layouts.wdo_off)[:P]
        wdo_off[base + 1:base + P + 1] = wdo_off[base] + np.cumsum(counts)
        gt_off[base + 1:base + P + 1] = gt_off[base] + f.gt_wdo_off[1:]
        wdo_xy.append(f.layouts.wdo_xy)
        wdo_type.append(f.layouts.wdo_type)
        for k in range(P):
            gt_xy.append(gt_global(f.gt_wdo_xy[int(f.gt_wdo_off[k]):int(f.gt_wdo_off[k + 1])], f.R[k], f.t[k], float(f.s[k])))
        poses["R"][base:base + P], poses["t"][base:base + P], poses["s"][base:base + P] = f.R.reshape(P, 4), f.t, f.s
        per_type = np.zeros((P, 3), np.int64)
        for k in range(P):
            per_type[k] = np.bincount(f.layouts.wdo_type[int(f.layouts.wdo_off[k]):int(f.layouts.wdo_off[k + 1])], minlength=3)
        a, b = np.triu_indices(P, 1)
        skip = EXCLUDED_PANOS.get(f.building_id)
        if skip is not None:
            keep = (f.pano_ids[a] != skip) & (f.pano_ids[b] != skip)
            a, b = a[keep], b[keep]
        rec = np.zeros(len(a), dtype=_lib.HYP_PAIR_DTYPE)
        rec["pano1"], rec["pano2"] = base + a, base + b
        rec["capacity"] = 2 * per_type[a, 1] * per_type[b, 1] + per_type[a, 0] * per_type[b, 0] + 2 * per_type[a, 2] * per_type[b, 2]
        pairs.append(rec)
        pair_floor.append(np.full(len(a), fi, np.int64))
        pair_ids.append(np.stack([f.pano_ids[a], f.pano_ids[b]], axis=1))
        base += P
    pairs_np = np.concatenate(pairs) if pairs else np.zeros(0, dtype=_lib.HYP_PAIR_DTYPE)
    cap = pairs_np["capacity"].astype(np.int64)
    pairs_np["row_offset"] = np.cumsum(cap) - cap
    cat = lambda parts, empty: np.ascontiguousarray(np.concatenate(parts)) if parts else empty
    return PackedFloors(floors, cat(wdo_xy, np.zeros((0, 2, 2))), cat(wdo_type, np.zeros(0, np.uint8)), wdo_off, cat(gt_xy, np.zeros((0, 2, 2))), gt_off, poses,
                        pairs_np, cat(pair_floor, np.zeros(0, np.int64)), cat(pair_ids, np.zeros((0, 2), np.int64)), int(cap.sum()),
                        int(cap.max(initial=0)))


def launch(packed: PackedFloors, device, min_width_ratio: float = MIN_ALLOWED_INFERRED_WDO_WIDTH_RATIO, out_rows=None, out_pairs=None):
    """Uploads the tables and launches salve_hypotheses_generate once -> (out_rows, out_pairs): uint8 device tensors over salve_hyp_row_t
    [n_rows] and salve_hyp_pair_out_t [n_pairs].  Given buffers (at least that large) are written in place; the rows behind a pair's n_kept are
    not written."""
    import torch

    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.SalveHipError("alignment hypotheses need a HIP device ('cuda:N'); there is no CPU path")
    lib = _lib.load()
    n_pairs = len(packed.pairs)
    row_bytes, pair_bytes = _lib.HYP_ROW_DTYPE.itemsize, _lib.HYP_PAIR_OUT_DTYPE.itemsize
    if out_rows is None:
        out_rows = torch.empty(max(packed.n_rows, 1) * row_bytes, dtype=torch.uint8, device=device)
    if out_pairs is None:
        out_pairs = torch.empty(max(n_pairs, 1) * pair_bytes, dtype=torch.uint8, device=device)
    if out_rows.numel() < packed.n_rows * row_bytes or out_pairs.numel() < n_pairs * pair_bytes:
        raise ValueError("out_rows / out_pairs are smaller than the call's rows / pairs")
    if n_pairs == 0:
        return out_rows, out_pairs
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(device)
    tables = [up(a) for a in (packed.wdo_xy, packed.wdo_type, packed.wdo_off, packed.gt_xy, packed.gt_off, packed.poses, packed.pairs)]
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    with torch.cuda.device(device):
        st = lib.salve_hypotheses_generate(p(tables[0]), p(tables[1]), p(tables[2]), len(packed.wdo_type), p(tables[3]), p(tables[4]), len(packed.gt_xy), p(tables[5]),
                                           len(packed.poses), p(tables[6]), n_pairs, packed.max_capacity, float(min_width_ratio), p(out_rows), packed.n_rows,
                                           p(out_pairs), ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
        _lib.check(st, "salve_hypotheses_generate")
        torch.cuda.current_stream(device).synchronize()   # the uploaded tables go out of scope here
    return out_rows, out_pairs


def hypothesis_name(i1: int, i2: int, type_code: int, i: int, j: int, configuration: int) -> str:
    """The file name of export_alignment_hypotheses.py:234-236."""
    return f"{i1}_{i2}__{ALIGNMENT_OBJECTS[type_code]}_{i}_{j}_{CONFIGURATIONS[configuration]}.json"


def assemble(packed: PackedFloors, rows: np.ndarray, pair_out: np.ndarray, hypotheses_save_root: str = "") -> List[FloorHypotheses]:
    """rows: HYP_ROW_DTYPE [n_rows] as the device wrote them (gaps behind n_kept included), pair_out: HYP_PAIR_OUT_DTYPE [n_pairs] -> one
    FloorHypotheses per floor, its rows in the order ingest.load_floor_hypotheses gives after the reference wrote its files: the label
    directories in LABEL_TYPES order, within a label by the STRING sort of the file path, pair_idx restarting per label."""
    if len(pair_out) and int(pair_out["n_kept"].min()) < 0:
        k = int(np.argmin(pair_out["n_kept"]))
        f = packed.floors[int(packed.pair_floor[k])]
        raise _lib.SalveHipError(f"salve_hypotheses_generate: the tables of pair ({int(packed.pair_ids[k, 0])}, {int(packed.pair_ids[k, 1])}) of building "
                                 f"{f.building_id}, {f.floor_id} are malformed; the pair was not evaluated")
    out = []
    for fi, f in enumerate(packed.floors):
        sel = np.flatnonzero(packed.pair_floor == fi)
        recs = []   # (label directory, name, row)
        for k in sel:
            off, i1, i2 = int(packed.pairs["row_offset"][k]), int(packed.pair_ids[k, 0]), int(packed.pair_ids[k, 1])
            for r in range(off, off + int(pair_out["n_kept"][k])):
                row = rows[r]
                recs.append((0 if row["label"] else 1, hypothesis_name(i1, i2, int(row["type"]), int(row["i"]), int(row["j"]), int(row["configuration"])), r, i1, i2))
        recs.sort(key=lambda x: (x[0], x[1]))
        n = len(recs)
        idx = np.array([r[2] for r in recs], dtype=np.int64)
        label = np.array([1 - r[0] for r in recs], dtype=np.int64)
        pair_idx = np.concatenate([np.arange(int((label == 1).sum())), np.arange(int((label == 0).sum()))]).astype(np.int64)
        po = pair_out[sel]
        pairs = FloorPairs(i1=packed.pair_ids[sel, 0].copy(), i2=packed.pair_ids[sel, 1].copy(), n_kept=po["n_kept"].astype(np.int64),
                           n_valid=po["n_valid"].astype(np.int64), n_rejected=po["n_rejected"].astype(np.int64),
                           visibly_adjacent=po["visibly_adjacent"].astype(bool), gt_R=po["R"].reshape(-1, 2, 2).copy(), gt_t=po["t"].copy(), gt_s=po["s"].copy())
        out.append(FloorHypotheses(f.building_id, f.floor_id, np.array([r[3] for r in recs], dtype=np.int64), np.array([r[4] for r in recs], dtype=np.int64),
                                   rows["R"][idx].reshape(n, 2, 2).astype(np.float32), rows["t"][idx].reshape(n, 2).astype(np.float32), np.ones(n, dtype=np.float64),
                                   label, pair_idx, [r[1][:-len(".json")].split("__")[-1] for r in recs],
                                   [f"{hypotheses_save_root}/{f.building_id}/{f.floor_id}/{LABEL_TYPES[r[0]]}/{r[1]}" for r in recs], pairs))
    return out


def generate(floors: Sequence[FloorInput], device, min_width_ratio: float = MIN_ALLOWED_INFERRED_WDO_WIDTH_RATIO,
             hypotheses_save_root: str = "") -> List[FloorHypotheses]:
    """The alignment hypotheses of all `floors` from ONE device call -> one ingest.FloorHypotheses per floor, rows, pair_idx, pair_uuid and
    fpaths exactly as ingest.load_floor_hypotheses(hypotheses_save_root, ...) would give them after the reference's exporter (or write_tree)
    wrote its files, and `.pairs` (ingest.FloorPairs): per panorama pair the valid / rejected counts, visibly_adjacent and i2Ti1_gt."""
    packed = pack(floors)
    rows_t, pairs_t = launch(packed, device, min_width_ratio)
    rows = rows_t.cpu().numpy().view(_lib.HYP_ROW_DTYPE)[:packed.n_rows]
    pair_out = pairs_t.cpu().numpy().view(_lib.HYP_PAIR_OUT_DTYPE)[:len(packed.pairs)]
    return assemble(packed, rows, pair_out, hypotheses_save_root)


def _save_sim2(path: str, R: np.ndarray, t: np.ndarray, s: float) -> None:
    """save_Sim2 (export_alignment_hypotheses.py:75-90; io_utils.save_json_file: json.dump(..., indent=4))."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"R": np.asarray(R, dtype=np.float32).flatten().tolist(), "t": np.asarray(t, dtype=np.float32).flatten().tolist(), "s": float(s)}, f, indent=4)


def write_tree(hyps: Sequence[FloorHypotheses], hypotheses_save_root) -> int:
    """Writes the reference's tree under hypotheses_save_root: {building}/{floor}/gt_alignment_approx/ and incorrect_alignment/ with one
    {i1}_{i2}__{object}_{i}_{j}_{configuration}.json per hypothesis, and gt_alignment_exact/{i1}_{i2}.json (i2Ti1_gt) for the visibly adjacent
    pairs -> the number of hypothesis files.  For users of the reference's other scripts; score_floor(hypotheses=) needs no file."""
    n = 0
    for h in hyps:
        floor_dir = f"{hypotheses_save_root}/{h.building_id}/{h.floor_id}"
        for k in range(len(h)):
            _save_sim2(f"{floor_dir}/{LABEL_TYPES[0] if h.label[k] else LABEL_TYPES[1]}/{os.path.basename(h.fpaths[k])}", h.R[k], h.t[k], float(h.s[k]))
            n += 1
        if h.pairs is not None:
            for k in np.flatnonzero(h.pairs.visibly_adjacent):
                _save_sim2(f"{floor_dir}/gt_alignment_exact/{int(h.pairs.i1[k])}_{int(h.pairs.i2[k])}.json", h.pairs.gt_R[k], h.pairs.gt_t[k], float(h.pairs.gt_s[k]))
    return n


def floor_summary(h: FloorHypotheses) -> Tuple[int, int, float, int]:
    """(valid configurations, invalid configurations, GT-valid fraction, pairs) of a floor, as the reference logs and prints them
    (:201-202, :250-273): a pair is GT-valid when it is visibly adjacent and has an aligned hypothesis, or is neither."""
    p = h.pairs
    aligned = {(int(a), int(b)) for a, b, l in zip(h.i1, h.i2, h.label) if l}
    valid = [bool(adj) == ((int(a), int(b)) in aligned) for a, b, adj in zip(p.i1, p.i2, p.visibly_adjacent)]
    return int(p.n_valid.sum()), int(p.n_rejected.sum()), float(np.mean(valid)) if valid else float("nan"), len(valid)


def main(argv: Optional[Sequence[str]] = None) -> int:
    from salve_amd.dataset.zind_partition import DATASET_SPLITS

    ap = argparse.ArgumentParser(prog="python -m salve_amd.hypotheses", description="Alignment hypotheses of ZInD floors from MHNet's W/D/Os, generated on the device.")
    ap.add_argument("--raw-dataset-dir", required=True, help="the ZInD dataset ({building}/zind_data.json)")
    ap.add_argument("--mhnet-predictions-data-root", required=True, help="MHNet's predictions (horizon_net/{building}/*.json)")
    ap.add_argument("--hypotheses-save-root", required=True, help="where the reference's tree of JSON files is written")
    which = ap.add_mutually_exclusive_group(required=True)
    which.add_argument("--split", choices=("train", "val", "test"))
    which.add_argument("--buildings", nargs="+", metavar="ID")
    ap.add_argument("--wdo-source", default="horizon_net", choices=("horizon_net", "ground_truth"))
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.wdo_source == "ground_truth":
        print("--wdo-source ground_truth is not supported: it needs the freespace check of overlap_utils.determine_invalid_wall_overlap (shapely's negative "
              "buffer of the room polygons), which is not implemented", file=sys.stderr)
        return 2
    buildings = sorted(DATASET_SPLITS[args.split]) if args.split else sorted(args.buildings)
    floors = load_floors(args.raw_dataset_dir, args.mhnet_predictions_data_root, buildings)
    hyps = generate(floors, args.device, hypotheses_save_root=args.hypotheses_save_root)   # all floors of the chosen buildings in one device call
    written = write_tree(hyps, args.hypotheses_save_root)
    for h in hyps:
        n_valid, n_invalid, frac, n_pairs = floor_summary(h)
        print(f"Building {h.building_id}, {h.floor_id}: floor_n_valid_configurations: {n_valid}, floor_n_invalid_configurations: {n_invalid}, "
              f"{frac:.2f} GT is-valid frac. over {n_pairs} alignment pairs, {len(h)} hypotheses ({int(h.label.sum())} {LABEL_TYPES[0]})")
    print(f"wrote {written} hypothesis files under {args.hypotheses_save_root}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
