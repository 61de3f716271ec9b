"""From a floor's scored alignment hypotheses to one global Sim(2) pose per panorama: the `spanning_tree` method of the reference's
scripts/run_sfm.py:112-152 and :440-446, with and without its cycle filter, for every floor of a prediction directory in ONE launch
(include/salve_hip.h: salve_pose_graph_solve; salve_amd/csrc/pose_graph.hip).

    python -m salve_amd.pose_graph PRED_DIR --hypotheses ROOT --confidence-threshold X [--no-cycle-filter] [--rot-deg D] [--trans T] [--out DIR]
        [--method {spanning_tree,random_spanning_trees,pgo}] [--filter-by-random-spanning-trees] [--num-hypotheses H] [--sampling-fraction F] [--seed S]
        [--pgo-max-iterations K] [--pgo-no-robust] [--zind-root DIR] [--report-seed S] [--report-iters K]
        [--axis-alignment --mhnet-predictions-data-root DIR]

reads the `batch_*.json` prediction files of PRED_DIR (evaluate.run_test_epoch, evaluate.run_fused_epoch, ingest.score_floor), looks every
prediction's alignment hypothesis up under ROOT, and writes one `pose_graph_{building}_{floor}.json` per floor.

The steps, and the reference functions they stand behind:
  1. a prediction counts iff y_hat == 1 and its probability reaches the threshold   (edge_classification.py:213-251)
  2. per panorama pair the most confident one stays                                  (edge_classification.py:254-311)
  3. pairs in no consistent 3-cycle are dropped (cycle_filter)                       (cycle_consistency.py:26-91, 172-303)
  4. the relative poses are chained along a spanning tree of the largest component   (spanning_tree.py:73-141)
Where the reference leaves a choice to an unspecified iteration order, this module fixes it: among equally probable
predictions of a pair the first in row order, among equally large components the one with the lowest panorama, among several shortest paths
the one through the lowest-index neighbour of the previous BFS level.

The second method, `random_spanning_trees` (spanning_tree.py:179-384): `draw_hypotheses` draws the reference's random
subsets of the thresholded predictions on the host, `sample_trees` builds every subset's spanning tree, scores it against ALL thresholded
predictions and picks the reference's winner, all floors and hypotheses in one call (salve_pose_graph_sample_trees;
salve_amd/csrc/pose_graph_sample.hip).  The winner's subset is also the reference's edge filter in front of the first method:
`solve(meas, thr, keep_rows=combined_inlier_mask(sample_trees(meas, thr)))`.

The third method, `pgo` (run_sfm.py:448-451; pose2_slam.py:57-286): `optimise` builds the spanning tree and refines it
by pose-graph optimisation -- a robust Levenberg-Marquardt over ALL thresholded predictions between localized panoramas, every second
hypothesis of a pair and every loop closure included -- in two device calls on the same buffers (salve_pose_graph_solve, then
salve_pose_graph_optimise; salve_amd/csrc/pose_graph_pgo.hip).  The objective is exactly the reference's factor graph and the result minimises
it; gtsam is not installed where this was built, so parity with gtsam's iterates and stopping point is unpinned.

Axis alignment by vanishing angle (run_sfm.py:421-426, pose2_slam.py:217-231, axis_alignment_utils.py:175-323) is on
by default in the reference and off by default here: `axis=AxisInputs` on solve / optimise / run, `--axis-alignment` on the command line.
Every row is then turned about the W/D/O it was aligned on until the two panoramas' vanishing angles agree, by at most 15 degrees, in one
more launch in front of the others (salve_pose_graph_axis_align; salve_amd/csrc/pose_graph_axis.hip); `align_rows` is that step alone.
`--no-cycle-filter --method pgo --axis-alignment` is the reference's default pipeline; without the last flag it is that pipeline with
--use_axis_alignment off.

The evaluation against ground truth is salve_amd.floor_report: `run(..., truth=)` and `--zind-root DIR` end in one
floor_report_{building}_{floor}.json per floor.  Landmark SLAM (the reference's `pose2_slam` method) and filter_edges_by_global_local_consistency are NOT here.  A floor may have at most 256 panoramas.
"""

from __future__ import annotations

import argparse
import ctypes
import glob
import json
import math
import os
import re
import sys
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from salve_amd import _lib
from salve_amd.common.sim2 import Sim2
from salve_amd.overlap import hypothesis_fpath, parse_tile_names

ALLOWED_WDO_TYPES = ("door", "window", "opening")
ROT_THRESHOLD_DEG, TRANS_THRESHOLD = 0.5, 0.01   # filter_to_SE2_cycle_consistent_edges' own defaults (cycle_consistency.py:228-229)


def _batch_number(fpath: str) -> int:
    m = re.search(r"batch_?(\d+)", os.path.basename(fpath))
    return int(m.group(1)) if m else -1


@dataclass
class EdgeMeasurements:
    """One row per scored alignment hypothesis, of any number of floors, in the order that breaks ties among equal probabilities."""

    building_id: List[str]
    floor_id: List[str]
    i1: np.ndarray                # [N] int64 pano ids, i1 < i2
    i2: np.ndarray
    prob: np.ndarray              # [N] float32: the probability of the PREDICTED class (y_hat_probs)
    y_hat: np.ndarray             # [N] int32
    y_true: np.ndarray            # [N] int32
    R: np.ndarray                 # [N, 2, 2] float32: i2Si1
    t: np.ndarray                 # [N, 2] float32
    s: np.ndarray                 # [N] float64
    wdo_pair_uuid: List[str]      # e.g. door_3_0
    configuration: List[str]      # identity | rotated

    def __post_init__(self) -> None:
        n = len(self.building_id)
        self.i1, self.i2 = np.asarray(self.i1, dtype=np.int64).reshape(n), np.asarray(self.i2, dtype=np.int64).reshape(n)
        self.prob = np.asarray(self.prob, dtype=np.float32).reshape(n)
        self.y_hat, self.y_true = np.asarray(self.y_hat, dtype=np.int32).reshape(n), np.asarray(self.y_true, dtype=np.int32).reshape(n)
        self.R, self.t = np.asarray(self.R, dtype=np.float32).reshape(n, 2, 2), np.asarray(self.t, dtype=np.float32).reshape(n, 2)
        self.s = np.asarray(self.s, dtype=np.float64).reshape(n)
        if not (len(self.floor_id) == len(self.wdo_pair_uuid) == len(self.configuration) == n):
            raise ValueError("EdgeMeasurements: the per-row lists differ in length")
        if n and (self.i1 >= self.i2).any():
            raise ValueError("EdgeMeasurements: every row needs i1 < i2 (the hypothesis is i2Si1 of the smaller pano id)")

    def __len__(self) -> int:
        return len(self.building_id)

    @classmethod
    def from_prediction_files(cls, pred_dir: str, hypotheses_save_root: str,
                              allowed_wdo_types: Sequence[str] = ALLOWED_WDO_TYPES) -> "EdgeMeasurements":
        """Every prediction of `pred_dir`/batch_*.json with its alignment hypothesis: get_edge_classifications_from_serialized_preds
        (edge_classification.py:103-210) for all floors at once.  The pano ids are the min / max of the two tile names' (:145-151), the
        hypothesis is {root}/{building}/{floor}/{label}/{i1}_{i2}__{uuid}_{configuration}.json (:185-193), predictions of another W/D/O type
        are skipped (:175-177).  Rows keep the files' order, batch_2 before batch_10 (the reference's glob order is unspecified)."""
        cols: Dict[str, list] = {k: [] for k in ("building_id", "floor_id", "i1", "i2", "prob", "y_hat", "y_true", "R", "t", "s", "wdo_pair_uuid",
                                                 "configuration")}
        for json_fpath in sorted(glob.glob(f"{pred_dir}/batch*.json"), key=lambda fp: (_batch_number(fp), fp)):
            with open(json_fpath) as f:
                d = json.load(f)
            for y_hat, y_true, prob, fp0, fp1 in zip(d["y_hat"], d["y_true"], d["y_hat_probs"], d["fp0"], d["fp1"]):
                rec = parse_tile_names(fp0, fp1)
                if rec["wdo_pair_uuid"].split("_")[0] not in allowed_wdo_types:
                    continue
                rec["y_true"] = y_true
                fp = hypothesis_fpath(hypotheses_save_root, rec)
                if not os.path.exists(fp):
                    raise ValueError(f"{json_fpath}: no alignment hypothesis {fp} for the prediction on {fp0}")
                S = Sim2.from_json(fp)
                for k in ("building_id", "floor_id", "i1", "i2", "wdo_pair_uuid", "configuration"):
                    cols[k].append(rec[k])
                cols["prob"].append(prob); cols["y_hat"].append(y_hat); cols["y_true"].append(y_true)
                cols["R"].append(S.rotation); cols["t"].append(S.translation); cols["s"].append(S.scale)
        return cls(**cols)

    @classmethod
    def from_floor(cls, hyps, rows: Sequence[int], y_hat: Sequence[int], prob: Sequence[float]) -> "EdgeMeasurements":
        """In-memory: `hyps` is an ingest.FloorHypotheses, `rows` the indices of its scored hypotheses in the order of the prediction files
        (evaluate.run_fused_epoch(return_rows=True)), y_hat / prob their predicted class and its probability.  A hypothesis file named
        {i1}_{i2} with i1 >= i2 (the reference's exporter writes none) raises ValueError: no prediction file could name it."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        uuid = [hyps.pair_uuid[int(r)] for r in rows]
        return cls(building_id=[hyps.building_id] * len(rows), floor_id=[hyps.floor_id] * len(rows), i1=hyps.i1[rows], i2=hyps.i2[rows], prob=prob,
                   y_hat=y_hat, y_true=hyps.label[rows], R=hyps.R[rows], t=hyps.t[rows], s=hyps.s[rows],
                   wdo_pair_uuid=[u.rsplit("_", 1)[0] for u in uuid], configuration=[u.rsplit("_", 1)[1] for u in uuid])

    def floors(self) -> List[Tuple[str, str]]:
        return sorted(set(zip(self.building_id, self.floor_id)))

    def compact(self) -> List[Dict[str, Any]]:
        """Per floor (in `floors()` order): its pano ids, ascending -- compact index k is pano_ids[k], and back -- and its rows as indices
        into this table, stably sorted by the compact (i1, i2)."""
        key = np.array([f"{b}\0{f}" for b, f in zip(self.building_id, self.floor_id)], dtype=object)
        out = []
        for b, f in self.floors():
            idx = np.nonzero(key == f"{b}\0{f}")[0]
            pano_ids = np.unique(np.concatenate([self.i1[idx], self.i2[idx]]))
            c1, c2 = np.searchsorted(pano_ids, self.i1[idx]), np.searchsorted(pano_ids, self.i2[idx])
            order = np.lexsort((c2, c1))   # (stable)
            out.append({"building_id": b, "floor_id": f, "pano_ids": pano_ids, "rows": idx[order], "c1": c1[order], "c2": c2[order]})
        return out


@dataclass
class FloorSolution:
    building_id: str
    floor_id: str
    pano_ids: np.ndarray                                  # the floor's panoramas that occur in a row, ascending
    options: Dict[str, Any]                               # confidence_threshold, cycle_filter, rot_threshold_deg, trans_threshold
    i2Si1: Dict[Tuple[int, int], Sim2]                    # the chosen relative pose per pair, keyed by pano ids
    i2Si1_consistent: Dict[Tuple[int, int], Sim2]         # ... of the pairs in a consistent 3-cycle
    wSi_list: Optional[List[Optional[Sim2]]]              # by pano id, None where not localized; None when the graph has no edge
    edges: Dict[Tuple[int, int], Dict[str, Any]]          # per chosen pair: row, prob, y_true, wdo_pair_uuid, configuration and the statistics
    parent: Dict[int, int] = field(default_factory=dict)  # the spanning tree, by pano id (the origin: -1)
    depth: Dict[int, int] = field(default_factory=dict)
    counts: Dict[str, int] = field(default_factory=dict)  # n_nodes, n_rows, n_chosen, n_triplets, n_consistent_triplets, n_consistent_edges, n_localized
    origin: Optional[int] = None                          # pano id

    def summary(self) -> str:
        c = self.counts
        return (f"{self.building_id} {self.floor_id}: chosen {c['n_chosen']} consistent {c['n_consistent_edges']} edges, "
                f"localized {c['n_localized']} / {c['n_nodes']} panoramas")

    def to_json(self) -> Dict[str, Any]:
        fin = lambda x: float(x) if np.isfinite(x) else None   # (+inf: the edge lies in no 3-cycle, or the threshold is off)
        sim = lambda S: {"R": S.rotation.flatten().tolist(), "t": S.translation.flatten().tolist(), "s": S.scale}
        opts = dict(self.options)
        opts["trans_threshold"] = fin(opts["trans_threshold"])
        return {"building_id": self.building_id, "floor_id": self.floor_id, "options": opts, "pano_ids": [int(p) for p in self.pano_ids],
                "counts": {k: int(v) for k, v in self.counts.items()}, "origin": self.origin,
                "edges": [{"i1": a, "i2": b, **{k: (fin(v) if k.startswith("min_") else v) for k, v in e.items()}, "i2Si1": sim(self.i2Si1[(a, b)])}
                          for (a, b), e in self.edges.items()],
                "poses": {str(p): {**sim(S), "parent": self.parent[p], "depth": self.depth[p]}
                          for p, S in enumerate(self.wSi_list or []) if S is not None}}

    @classmethod
    def from_json(cls, d: Dict[str, Any]) -> "FloorSolution":
        inf = lambda x: float("inf") if x is None else x
        sim = lambda r: Sim2(np.array(r["R"], dtype=np.float32).reshape(2, 2), np.array(r["t"], dtype=np.float32), float(r["s"]))
        opts = dict(d["options"])
        opts["trans_threshold"] = inf(opts["trans_threshold"])
        edges = {(e["i1"], e["i2"]): {k: (inf(v) if k.startswith("min_") else v) for k, v in e.items() if k not in ("i1", "i2", "i2Si1")} for e in d["edges"]}
        rel = {(e["i1"], e["i2"]): sim(e["i2Si1"]) for e in d["edges"]}
        graph = [k for k, e in edges.items() if e["consistent"] or not opts["cycle_filter"]]
        wSi = None
        if d["origin"] is not None:
            wSi = [None] * (max(b for _, b in graph) + 1)
            for p, r in d["poses"].items():
                wSi[int(p)] = sim(r)
        return cls(d["building_id"], d["floor_id"], np.array(d["pano_ids"], dtype=np.int64), opts, rel,
                   {k: S for k, S in rel.items() if edges[k]["consistent"]}, wSi, edges, {int(p): r["parent"] for p, r in d["poses"].items()},
                   {int(p): r["depth"] for p, r in d["poses"].items()}, dict(d["counts"]), d["origin"])


def _align8(n: int) -> int:
    return (n + 7) & ~7


def _device_table(meas: EdgeMeasurements, floors: List[Dict[str, Any]], what: str):
    """(rows as GRAPH_ROW_DTYPE records in the floors' sorted order, floor_start, n_nodes, max_nodes) of `floors` (EdgeMeasurements.compact)."""
    order = np.concatenate([fl["rows"] for fl in floors]).astype(np.int64)
    N = len(order)
    table = np.zeros(N, dtype=_lib.GRAPH_ROW_DTYPE)
    table["i1"], table["i2"] = np.concatenate([fl["c1"] for fl in floors]), np.concatenate([fl["c2"] for fl in floors])
    table["prob"], table["y_hat"] = meas.prob[order], meas.y_hat[order]
    table["R"], table["t"], table["s"] = meas.R[order].reshape(N, 4), meas.t[order], meas.s[order]
    floor_start = np.concatenate([[0], np.cumsum([len(fl["rows"]) for fl in floors])]).astype(np.int32)
    n_nodes = np.array([len(fl["pano_ids"]) for fl in floors], dtype=np.int32)
    M = int(n_nodes.max())
    if M > _lib.GRAPH_MAX_NODES:   # (the library refuses it as well: SALVE_ERR_BAD_ARG)
        worst = floors[int(n_nodes.argmax())]
        raise _lib.SalveHipError(f"{what}: floor {worst['building_id']} {worst['floor_id']} has {M} panoramas, more than the "
                                 f"{_lib.GRAPH_MAX_NODES} a floor may have")
    return table, floor_start, n_nodes, M


AXIS_TYPE_CODES = {"window": 0, "door": 1, "opening": 2}   # EdgeWDOPair.alignment_object -> layout.WDO_TYPES' code (windows, doors, openings)


class AxisInputs:
    """What axis alignment by vanishing angle reads of every floor: per (building_id, floor_id) the panorama ids
    (ascending), their layout.PanoLayouts -- the INFERRED rooms and W/D/Os, panorama k of the tables being pano_ids[k] -- and one vanishing
    angle in degrees per panorama, NaN where MHNet gave none.  AxisInputs.from_floors(hypotheses.load_floors(...)), or add() floor by floor
    from arrays."""

    def __init__(self) -> None:
        self.floors: Dict[Tuple[str, str], Tuple[np.ndarray, Any, np.ndarray]] = {}

    def add(self, building_id: str, floor_id: str, pano_ids, layouts, vanishing_angle_deg) -> "AxisInputs":
        where = f"building {building_id}, {floor_id}"
        ids = np.asarray(pano_ids, dtype=np.int64).reshape(-1)
        if vanishing_angle_deg is None:
            raise ValueError(f"AxisInputs: {where}: no vanishing angles (FloorInput.vanishing_angle_deg is None)")
        angles = np.asarray(vanishing_angle_deg, dtype=np.float64).reshape(-1)
        if len(ids) and (np.diff(ids) <= 0).any():
            raise ValueError(f"AxisInputs: {where}: pano_ids must ascend strictly")
        if len(angles) != len(ids) or layouts.P != max(len(ids), 1):
            raise ValueError(f"AxisInputs: {where}: {len(ids)} pano ids, {len(angles)} vanishing angles and layouts of {layouts.P} panoramas")
        self.floors[(building_id, floor_id)] = (ids, layouts, angles)
        return self

    @classmethod
    def from_floors(cls, floor_inputs) -> "AxisInputs":
        """floor_inputs: salve_amd.hypotheses.FloorInput objects (load_floors' or from_pose_graphs')."""
        axis = cls()
        for f in floor_inputs:
            axis.add(f.building_id, f.floor_id, f.pano_ids, f.layouts, f.vanishing_angle_deg)
        return axis

    @staticmethod
    def parse_wdo_pair_uuid(wdo_pair_uuid: str) -> Tuple[int, int]:
        """door_3_0 -> (type code of "door", 3): EdgeWDOPair.from_wdo_pair_uuid's split; the index counts within the type."""
        parts = wdo_pair_uuid.split("_")
        if len(parts) != 3 or parts[0] not in AXIS_TYPE_CODES:
            raise ValueError(f"wdo_pair_uuid {wdo_pair_uuid!r} is not {{door,window,opening}}_{{i1 index}}_{{i2 index}}")
        return AXIS_TYPE_CODES[parts[0]], int(parts[1])

    def tables(self, meas: "EdgeMeasurements", floors: List[Dict[str, Any]]) -> Dict[str, np.ndarray]:
        """Host: the tables of salve_pose_graph_axis_align for `floors` (EdgeMeasurements.compact, possibly thinned by keep_rows): the
        per-panorama tables gathered in the floors' compact numbering, one W/D/O record per row in the floors' sorted order.  ValueError for a
        floor or panorama these inputs do not hold and for a row whose W/D/O its panorama's layout does not hold -- before anything is uploaded."""
        room_cnt, wdo_cnt, room_xy, wdo_xy, wdo_type, angles, pano_base, row_wdo = [], [], [], [], [], [], [], []
        base = 0
        for fl in floors:
            where = f"building {fl['building_id']}, {fl['floor_id']}"
            if (fl["building_id"], fl["floor_id"]) not in self.floors:
                raise ValueError(f"AxisInputs: {where} is not among the floors given")
            ids, lay, ang = self.floors[(fl["building_id"], fl["floor_id"])]
            want = np.asarray(fl["pano_ids"], dtype=np.int64)
            pos = np.minimum(np.searchsorted(ids, want), max(len(ids) - 1, 0))
            if len(want) and (len(ids) == 0 or (ids[pos] != want).any()):
                missing = [int(p) for p in want if p not in set(ids.tolist())]
                raise ValueError(f"AxisInputs: {where}: no layout for panoramas {missing}")
            per_type = np.zeros((len(want), 3), np.int64)
            for k, p in enumerate(pos):
                r0, r1, w0, w1 = int(lay.room_off[p]), int(lay.room_off[p + 1]), int(lay.wdo_off[p]), int(lay.wdo_off[p + 1])
                room_cnt.append(r1 - r0); wdo_cnt.append(w1 - w0)
                room_xy.append(lay.room_xy[r0:r1]); wdo_xy.append(lay.wdo_xy[w0:w1]); wdo_type.append(lay.wdo_type[w0:w1])
                per_type[k] = np.bincount(lay.wdo_type[w0:w1], minlength=3)[:3]
            angles.append(ang[pos] if len(want) else np.zeros(0))
            rec = np.zeros(len(fl["rows"]), dtype=_lib.AXIS_WDO_DTYPE)
            for k, (r, c1) in enumerate(zip(fl["rows"], fl["c1"])):
                uuid = meas.wdo_pair_uuid[int(r)]
                pair = f"pair ({int(meas.i1[r])}, {int(meas.i2[r])})"
                try:
                    code, index = self.parse_wdo_pair_uuid(uuid)
                except ValueError as e:
                    raise ValueError(f"AxisInputs: {where}, {pair}: {e}") from None
                if not 0 <= index < per_type[c1, code]:
                    raise ValueError(f"AxisInputs: {where}, {pair}: {uuid} names {ALLOWED_WDO_TYPES[(1, 0, 2)[code]]} {index} of panorama {int(meas.i1[r])}, "
                                     f"whose layout holds {int(per_type[c1, code])}")
                rec[k] = (code, index)
            row_wdo.append(rec)
            pano_base.append(base)
            base += len(want)
        cat = lambda parts, empty: np.ascontiguousarray(np.concatenate(parts)) if parts else empty
        off = lambda cnt: np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        return {"row_wdo": cat(row_wdo, np.zeros(0, dtype=_lib.AXIS_WDO_DTYPE)), "pano_base": np.asarray(pano_base, dtype=np.int32),
                "room_off": off(room_cnt), "room_xy": cat(room_xy, np.zeros((0, 2))).astype(np.float64), "wdo_off": off(wdo_cnt),
                "wdo_xy": cat(wdo_xy, np.zeros((0, 2, 2))).astype(np.float64), "wdo_type": cat(wdo_type, np.zeros(0, np.uint8)).astype(np.uint8),
                "vanishing_deg": cat(angles, np.zeros(0)).astype(np.float64)}


def _blob(parts: Sequence[Tuple[str, np.ndarray]]) -> Tuple[np.ndarray, Dict[str, int]]:
    """One upload of named tables, each at an 8-byte aligned offset."""
    chunks, offs, at = [], {}, 0
    for name, a in parts:
        b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        offs[name] = at
        chunks += [b, np.zeros(_align8(len(b)) - len(b), np.uint8)]
        at += _align8(len(b))
    return np.concatenate(chunks), offs


class _AxisCall:
    """salve_pose_graph_axis_align in front of the other entries of one call: its tables ride in the call's one upload, its three outputs
    (aligned rows | row records | floor records) in the call's one output buffer, and the next entries read the aligned rows on the device."""

    NAMES = ("row_wdo", "pano_base", "room_off", "room_xy", "wdo_off", "wdo_xy", "wdo_type", "vanishing_deg")

    def __init__(self, meas: EdgeMeasurements, floors: List[Dict[str, Any]], axis: AxisInputs, N: int) -> None:
        self.tabs = axis.tables(meas, floors)
        self.N, self.F = N, len(floors)
        self.off_axis = N * _lib.GRAPH_ROW_DTYPE.itemsize
        self.off_floors = self.off_axis + N * _lib.AXIS_ROW_OUT_DTYPE.itemsize
        self.out_bytes = self.off_floors + self.F * _lib.AXIS_FLOOR_OUT_DTYPE.itemsize

    def parts(self) -> List[Tuple[str, np.ndarray]]:
        return [(k, self.tabs[k]) for k in self.NAMES]

    def launch(self, lib, p_in: int, offs: Dict[str, int], p_out: int, status_ptr, stream) -> ctypes.c_void_p:
        """p_out: the 8-byte aligned device address of this call's outputs -> the address of the aligned row table."""
        vp, t = ctypes.c_void_p, self.tabs
        at = lambda k: vp(p_in + offs[k]) if t[k].size else None
        _lib.check(lib.salve_pose_graph_axis_align(vp(p_in + offs["rows"]) if self.N else None, self.N, vp(p_in + offs["floor_start"]), vp(p_in + offs["n_nodes"]),
                                                   self.F, at("row_wdo"), vp(p_in + offs["pano_base"]), vp(p_in + offs["room_off"]), at("room_xy"), len(t["room_xy"]),
                                                   vp(p_in + offs["wdo_off"]), at("wdo_xy"), at("wdo_type"), len(t["wdo_type"]), at("vanishing_deg"),
                                                   len(t["vanishing_deg"]), vp(p_out), vp(p_out + self.off_axis), vp(p_out + self.off_floors), status_ptr, stream),
                   "salve_pose_graph_axis_align")
        return vp(p_out)

    def decode(self, meas: EdgeMeasurements, floors: List[Dict[str, Any]], host: np.ndarray) -> Tuple[EdgeMeasurements, Dict[str, Any]]:
        """host: this call's downloaded outputs -> (the measurements with the aligned R, t, s, the per-row records in `meas`' row order)."""
        from dataclasses import replace

        rows = host[:self.off_axis].view(_lib.GRAPH_ROW_DTYPE)
        rec = host[self.off_axis:self.off_floors].view(_lib.AXIS_ROW_OUT_DTYPE)
        fo = host[self.off_floors:self.out_bytes].view(_lib.AXIS_FLOOR_OUT_DTYPE)
        order = np.concatenate([fl["rows"] for fl in floors]).astype(np.int64) if floors else np.zeros(0, np.int64)
        n = len(meas)
        R, t, s = meas.R.copy(), meas.t.copy(), meas.s.copy()
        R[order], t[order], s[order] = rows["R"].reshape(-1, 2, 2), rows["t"], rows["s"]
        info = {"status": np.full(n, -1, np.int32), "correction_deg": np.full(n, np.nan), "theta_deg": np.full(n, np.nan), "t": np.full((n, 2), np.nan)}
        for k in ("status", "correction_deg", "theta_deg", "t"):
            info[k][order] = rec[k]
        info["counts"] = [{name: int(fo[f"n_{name}"][f]) for name in _lib.AXIS_STATUS_NAMES} for f in range(self.F)]
        return replace(meas, R=R, t=t, s=s), info


def align_rows(meas: EdgeMeasurements, axis: AxisInputs, device="cuda:0", keep_rows: Optional[np.ndarray] = None) -> Tuple[EdgeMeasurements, Dict[str, Any]]:
    """Axis alignment by vanishing angle of every row of `meas` on its own (salve_pose_graph_axis_align; the reference's
    align_pair_measurement_by_vanishing_angle, axis_alignment_utils.py:175-263): one upload, one launch for all floors, one read of the device
    status word, one download -> (the measurements with R, t, s replaced where the correction applies and bit for bit the given ones where not,
    the per-row records in `meas`' row order: "status" int32 (_lib.AXIS_*; -1: the row lies outside keep_rows and was not uploaded),
    "correction_deg", "theta_deg", "t" float64 (the new pose before it is rounded; NaN where it does not apply), and "counts": per floor, in
    `meas.floors()` order, the number of rows of each status by _lib.AXIS_STATUS_NAMES).  solve / optimise / run(axis=) do this in front of
    their own entries without the download in between."""
    import torch

    from salve_amd import status

    device = torch.device(device)
    lib = _lib.load()
    floors = meas.compact()
    if not floors:
        return meas, {"status": np.zeros(0, np.int32), "correction_deg": np.zeros(0), "theta_deg": np.zeros(0), "t": np.zeros((0, 2)), "counts": []}
    floors = _keep(meas, floors, keep_rows, "pose_graph.align_rows")
    table, floor_start, n_nodes, _ = _device_table(meas, floors, "pose_graph.align_rows")
    call = _AxisCall(meas, floors, axis, len(table))
    blob, offs = _blob([("rows", table), ("floor_start", floor_start), ("n_nodes", n_nodes)] + call.parts())
    with torch.cuda.device(device):
        dev_in = torch.from_numpy(blob).to(device)
        dev_out = torch.empty(call.out_bytes, dtype=torch.uint8, device=device)
        call.launch(lib, dev_in.data_ptr(), offs, dev_out.data_ptr(), status.ptr(device), ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
        status.check(device, "pose_graph.align_rows")   # (the one synchronising read)
        host = dev_out.cpu().numpy()
    return call.decode(meas, floors, host)


def _keep(meas: EdgeMeasurements, floors: List[Dict[str, Any]], keep_rows, what: str) -> List[Dict[str, Any]]:
    if keep_rows is not None:
        keep_rows = np.asarray(keep_rows, dtype=bool).reshape(-1)
        if len(keep_rows) != len(meas):
            raise ValueError(f"{what}: keep_rows has {len(keep_rows)} entries for {len(meas)} rows")
        for fl in floors:
            k = keep_rows[fl["rows"]]
            fl["rows"], fl["c1"], fl["c2"] = fl["rows"][k], fl["c1"][k], fl["c2"][k]
    return floors


def solve(meas: EdgeMeasurements, confidence_threshold: float, cycle_filter: bool = True, rot_threshold_deg: float = ROT_THRESHOLD_DEG,
          trans_threshold: float = TRANS_THRESHOLD, device="cuda:0", keep_rows: Optional[np.ndarray] = None,
          axis: Optional[AxisInputs] = None) -> List[FloorSolution]:
    """One FloorSolution per floor of `meas` (in `meas.floors()` order): one upload, one launch for all floors, one read of the device status
    word, one download.  confidence_threshold has no default: the reference's run_sfm.py takes it from the command line.  rot_threshold_deg
    and trans_threshold are filter_to_SE2_cycle_consistent_edges' own; trans_threshold=inf gives the rotation-only filter.  cycle_filter=False
    chains the chosen edges as they are (run_sfm.py:440-446).  A floor of more than 256 panoramas is refused before anything is launched.
    keep_rows: None, or a boolean mask over `meas`; a row outside it is never a candidate (it is not uploaded; the floors keep the panorama
    numbering of the whole table, and n_rows counts the kept rows).  With a sample_trees inlier mask this is the reference's
    --filter_edges_by_random_spanning_trees.
    axis: None, or the AxisInputs of the floors: every uploaded row is first aligned by vanishing angle (salve_pose_graph_axis_align, on the same
    stream; the reference's --use_axis_alignment, run_sfm.py:421-426) and salve_pose_graph_solve reads the aligned table on the device -- still one
    upload, one read of the status word, one download.  i2Si1 then holds the aligned poses, every edge gains axis_status (a name of
    _lib.AXIS_STATUS_NAMES) and axis_correction_deg (None where there is none), and the options axis_alignment: True.  keep_rows composes: the
    kept rows are the aligned ones.  None: the launches, values and JSON are as they were."""
    import torch

    from salve_amd import status

    device = torch.device(device)
    lib = _lib.load()
    floors = meas.compact()
    F = len(floors)
    if F == 0:
        return []
    floors = _keep(meas, floors, keep_rows, "pose_graph.solve")
    table, floor_start, n_nodes, M = _device_table(meas, floors, "pose_graph.solve")
    N = len(table)
    call = _AxisCall(meas, floors, axis, N) if axis is not None else None

    # one upload: rows | floor_start | n_nodes; one output buffer: out_rows | out_nodes | out_floors (with axis: the axis tables; | its outputs)
    if call is None:
        blob = np.concatenate([table.view(np.uint8), floor_start.view(np.uint8), n_nodes.view(np.uint8)])
        offs = {"rows": 0, "floor_start": table.nbytes, "n_nodes": table.nbytes + floor_start.nbytes}
    else:
        blob, offs = _blob([("rows", table), ("floor_start", floor_start), ("n_nodes", n_nodes)] + call.parts())
    off_nodes = _align8(N * _lib.GRAPH_ROW_OUT_DTYPE.itemsize)
    off_floors = off_nodes + F * M * _lib.GRAPH_NODE_OUT_DTYPE.itemsize
    out_bytes = off_floors + F * _lib.GRAPH_FLOOR_OUT_DTYPE.itemsize
    off_axis = _align8(out_bytes)
    with torch.cuda.device(device):
        dev_in = torch.from_numpy(blob).to(device)
        dev_out = torch.empty(out_bytes if call is None else off_axis + call.out_bytes, dtype=torch.uint8, device=device)
        p_in, p_out = dev_in.data_ptr(), dev_out.data_ptr()
        vp = ctypes.c_void_p
        stream = vp(torch.cuda.current_stream(device).cuda_stream)
        ws_bytes = int(lib.salve_pose_graph_workspace_bytes(F, M))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device) if ws_bytes else None
        p_rows = vp(p_in + offs["rows"]) if call is None else call.launch(lib, p_in, offs, p_out + off_axis, status.ptr(device), stream)
        _lib.check(lib.salve_pose_graph_solve(p_rows, N, vp(p_in + offs["floor_start"]), vp(p_in + offs["n_nodes"]), F, M,
                                              float(confidence_threshold), float(rot_threshold_deg), float(trans_threshold), int(bool(cycle_filter)),
                                              vp(p_out), vp(p_out + off_nodes), vp(p_out + off_floors), vp(ws.data_ptr()) if ws is not None else None,
                                              ws_bytes, status.ptr(device), stream),
                   "salve_pose_graph_solve")
        status.check(device, "pose_graph.solve")   # (the one synchronising read)
        host = dev_out.cpu().numpy()
    out_rows = host[:N * _lib.GRAPH_ROW_OUT_DTYPE.itemsize].view(_lib.GRAPH_ROW_OUT_DTYPE)
    out_nodes = host[off_nodes:off_floors].view(_lib.GRAPH_NODE_OUT_DTYPE).reshape(F, M)
    out_floors = host[off_floors:out_bytes].view(_lib.GRAPH_FLOOR_OUT_DTYPE)
    axis_info = None
    if call is not None:
        meas, axis_info = call.decode(meas, floors, host[off_axis:])

    return _floor_solutions(meas, floors, floor_start, out_rows, out_nodes, out_floors, confidence_threshold, cycle_filter, rot_threshold_deg,
                            trans_threshold, axis_info)


def _floor_solutions(meas, floors, floor_start, out_rows, out_nodes, out_floors, confidence_threshold, cycle_filter, rot_threshold_deg,
                     trans_threshold, axis_info=None) -> List[FloorSolution]:
    """salve_pose_graph_solve's three output tables as one FloorSolution per floor.  axis_info: None, or _AxisCall.decode's records; `meas` then
    holds the aligned poses."""
    options = {"confidence_threshold": float(confidence_threshold), "cycle_filter": bool(cycle_filter), "rot_threshold_deg": float(rot_threshold_deg),
               "trans_threshold": float(trans_threshold)}
    if axis_info is not None:
        options["axis_alignment"] = True
    sim = lambda R, t, s: Sim2(np.array(R, dtype=np.float32).reshape(2, 2), np.array(t, dtype=np.float32), float(s))
    solutions = []
    for f, fl in enumerate(floors):
        lo, hi = int(floor_start[f]), int(floor_start[f + 1])
        ids = fl["pano_ids"]
        rel, rel_consistent, edges = {}, {}, {}
        for k in np.nonzero(out_rows["chosen"][lo:hi])[0]:
            r, o = int(fl["rows"][k]), out_rows[lo + k]
            pair = (int(meas.i1[r]), int(meas.i2[r]))
            rel[pair] = sim(meas.R[r], meas.t[r], meas.s[r])
            if o["consistent"]:
                rel_consistent[pair] = rel[pair]
            edges[pair] = {"row": r, "prob": float(meas.prob[r]), "y_true": int(meas.y_true[r]), "wdo_pair_uuid": meas.wdo_pair_uuid[r],
                           "configuration": meas.configuration[r], "consistent": bool(o["consistent"]), "n_triplets": int(o["n_triplets"]),
                           "n_consistent": int(o["n_consistent"]), "min_rot_err": float(o["min_rot_err"]), "min_trans_err": float(o["min_trans_err"])}
            if axis_info is not None:
                corr = float(axis_info["correction_deg"][r])
                edges[pair]["axis_status"] = _lib.AXIS_STATUS_NAMES[int(axis_info["status"][r])]
                edges[pair]["axis_correction_deg"] = corr if np.isfinite(corr) else None
        fo, nodes = out_floors[f], out_nodes[f, :len(ids)]
        wSi, parent, depth, origin = None, {}, {}, None
        if fo["origin"] >= 0:
            origin = int(ids[fo["origin"]])
            graph = rel_consistent if cycle_filter else rel
            wSi = [None] * (max(b for _, b in graph) + 1)   # greedily_construct_st_Sim2's length (spanning_tree.py:104, 110)
            for v in np.nonzero(nodes["localized"])[0]:
                p = int(ids[v])
                wSi[p] = sim(nodes["R"][v], nodes["t"][v], nodes["s"][v])
                parent[p], depth[p] = (int(ids[nodes["parent"][v]]) if nodes["parent"][v] >= 0 else -1), int(nodes["depth"][v])
        counts = {"n_nodes": len(ids), "n_rows": hi - lo, **{k: int(fo[k]) for k in ("n_chosen", "n_triplets", "n_consistent_triplets",
                                                                                    "n_consistent_edges", "n_localized")}}
        solutions.append(FloorSolution(fl["building_id"], fl["floor_id"], ids, dict(options), rel, rel_consistent, wSi, edges, parent, depth, counts,
                                       origin))
    return solutions


PGO_OPTIONS = ("robust", "max_iterations", "relative_error_tol", "absolute_error_tol", "huber_k", "odometry_sigmas", "prior_sigmas")   # optimise's own
HUBER_K, ODOMETRY_SIGMAS, PRIOR_SIGMAS = 1.345, (0.2, 0.2, 0.1), (0.3, 0.3, 0.1)   # planar_slam's own (pose2_slam.py:87-93)


@dataclass
class PgoSolution:
    """A floor's spanning tree refined by pose-graph optimisation (salve_pose_graph_optimise)."""

    building_id: str
    floor_id: str
    pano_ids: np.ndarray
    options: Dict[str, Any]                               # method, the tree's options and the optimiser's
    tree: FloorSolution                                   # the initial estimate, as `solve` returns it
    wSi_list: Optional[List[Optional[Sim2]]]              # by pano id, in the tree's shape and length: float32 Sim2 of scale 1
    pose: Dict[int, Tuple[float, float, float]]           # by pano id: x, y, theta in float64 (theta continuous from the tree's, not wrapped)
    record: Dict[str, Any]                                # the floor record: counts, stop_reason (a name of _lib.PGO_STOP_NAMES), lambda, costs

    @property
    def counts(self) -> Dict[str, int]:
        return self.tree.counts

    @property
    def origin(self) -> Optional[int]:
        return self.tree.origin

    def summary(self) -> str:
        r, fin = self.record, lambda x: "nan" if x is None else f"{x:.6g}"
        return (f"{self.building_id} {self.floor_id}: pgo over {r['n_factors']} factors, {r['n_unknown_nodes']} / {self.tree.counts['n_nodes']} panoramas, "
                f"cost {fin(r['cost_initial'])} -> {fin(r['cost_final'])} in {r['n_iterations']} iterations ({r['n_rejected']} rejected, "
                f"{r['n_downweighted']} down-weighted), stopped by {r['stop_reason']}")

    def to_json(self) -> Dict[str, Any]:
        sim = lambda S: {"R": S.rotation.flatten().tolist(), "t": S.translation.flatten().tolist(), "s": S.scale}
        opts = dict(self.options)
        opts["trans_threshold"] = opts["trans_threshold"] if np.isfinite(opts["trans_threshold"]) else None   # (as the tree's)
        return {"building_id": self.building_id, "floor_id": self.floor_id, "options": opts, "pano_ids": [int(p) for p in self.pano_ids],
                "pgo": dict(self.record), "n_poses": None if self.wSi_list is None else len(self.wSi_list),
                "poses": {str(p): {**sim(S), "pose": list(self.pose[p])} for p, S in enumerate(self.wSi_list or []) if S is not None},
                "tree": self.tree.to_json()}

    @classmethod
    def from_json(cls, d: Dict[str, Any]) -> "PgoSolution":
        sim = lambda r: Sim2(np.array(r["R"], dtype=np.float32).reshape(2, 2), np.array(r["t"], dtype=np.float32), float(r["s"]))
        wSi = None
        if d["n_poses"] is not None:
            wSi = [None] * d["n_poses"]
            for p, r in d["poses"].items():
                wSi[int(p)] = sim(r)
        opts = dict(d["options"])
        opts["trans_threshold"] = float("inf") if opts["trans_threshold"] is None else opts["trans_threshold"]
        return cls(d["building_id"], d["floor_id"], np.array(d["pano_ids"], dtype=np.int64), opts, FloorSolution.from_json(d["tree"]), wSi,
                   {int(p): tuple(r["pose"]) for p, r in d["poses"].items()}, dict(d["pgo"]))


def optimise(meas: EdgeMeasurements, confidence_threshold: float, robust: bool = True, max_iterations: int = 100, relative_error_tol: float = 1e-5,
             absolute_error_tol: float = 1e-5, keep_rows: Optional[np.ndarray] = None, device="cuda:0", huber_k: float = HUBER_K,
             odometry_sigmas: Sequence[float] = ODOMETRY_SIGMAS, prior_sigmas: Sequence[float] = PRIOR_SIGMAS, axis: Optional[AxisInputs] = None,
             **solve_options) -> List[PgoSolution]:
    """One PgoSolution per floor of `meas` (in `meas.floors()` order): the reference's `--method pgo` (run_sfm.py:448-451; pose2_slam.py:57-286
    with optimize_poses_only, without axis alignment).  One upload; salve_pose_graph_solve builds every floor's spanning tree and
    salve_pose_graph_optimise refines it over ALL thresholded predictions whose two panoramas the tree localizes, on the same device buffers
    with no download between them; one read of the device status word; one download.  solve_options: solve's cycle_filter, rot_threshold_deg,
    trans_threshold -- they shape the initial tree only (cycle_filter=False is the reference's pipeline).  keep_rows: solve's; the factors are
    then the kept rows only.  The defaults of robust, huber_k, the sigmas, max_iterations and the tolerances are the reference's and gtsam's;
    parity with gtsam's iterates is unpinned: the objective is the reference's, and the result minimises it.
    axis: solve's -- salve_pose_graph_axis_align runs first on the same stream and both later entries read its table, so the tree AND the
    factors are the aligned measurements (run_sfm.py:421-426 and pose2_slam.py:217-231: the step is a pure per-row map, so aligning every row
    once gives both); the floor record gains axis_counts.  This is the reference's default `--method pgo` run."""
    import torch

    from salve_amd import status

    unknown = set(solve_options) - {"cycle_filter", "rot_threshold_deg", "trans_threshold"}
    if unknown:
        raise TypeError(f"pose_graph.optimise: unknown options {sorted(unknown)}")
    cycle_filter = bool(solve_options.get("cycle_filter", True))
    rot_threshold_deg, trans_threshold = solve_options.get("rot_threshold_deg", ROT_THRESHOLD_DEG), solve_options.get("trans_threshold", TRANS_THRESHOLD)
    if int(max_iterations) < 0:
        raise ValueError("pose_graph.optimise: max_iterations is negative")
    for name, v in (("relative_error_tol", relative_error_tol), ("absolute_error_tol", absolute_error_tol), ("huber_k", huber_k),
                    *((f"odometry_sigmas[{i}]", x) for i, x in enumerate(odometry_sigmas)), *((f"prior_sigmas[{i}]", x) for i, x in enumerate(prior_sigmas))):
        if not float(v) > 0.0:
            raise ValueError(f"pose_graph.optimise: {name} must be positive, not {v}")
    if len(odometry_sigmas) != 3 or len(prior_sigmas) != 3:
        raise ValueError("pose_graph.optimise: three sigmas each (x, y, theta)")
    device = torch.device(device)
    lib = _lib.load()
    floors = meas.compact()
    F = len(floors)
    if F == 0:
        return []
    floors = _keep(meas, floors, keep_rows, "pose_graph.optimise")
    table, floor_start, n_nodes, M = _device_table(meas, floors, "pose_graph.optimise")
    N = len(table)
    call = _AxisCall(meas, floors, axis, N) if axis is not None else None

    # one upload: rows | floor_start | n_nodes; one output buffer: out_rows | tree nodes | tree floors | pgo nodes | pgo floors | poses
    # (with axis: the axis tables behind the upload, its outputs behind the output buffer)
    node_dt, pgo_dt = _lib.GRAPH_NODE_OUT_DTYPE, _lib.GRAPH_PGO_FLOOR_OUT_DTYPE
    if call is None:
        blob = np.concatenate([table.view(np.uint8), floor_start.view(np.uint8), n_nodes.view(np.uint8)])
        offs = {"rows": 0, "floor_start": table.nbytes, "n_nodes": table.nbytes + floor_start.nbytes}
    else:
        blob, offs = _blob([("rows", table), ("floor_start", floor_start), ("n_nodes", n_nodes)] + call.parts())
    off_nodes = _align8(N * _lib.GRAPH_ROW_OUT_DTYPE.itemsize)
    off_floors = off_nodes + F * M * node_dt.itemsize
    off_pgo_nodes = _align8(off_floors + F * _lib.GRAPH_FLOOR_OUT_DTYPE.itemsize)
    off_pgo_floors = off_pgo_nodes + F * M * node_dt.itemsize
    off_pose = off_pgo_floors + F * pgo_dt.itemsize
    out_bytes = off_pose + F * M * 24
    off_axis = _align8(out_bytes)
    sig_o, sig_p = (ctypes.c_double * 3)(*map(float, odometry_sigmas)), (ctypes.c_double * 3)(*map(float, prior_sigmas))
    with torch.cuda.device(device):
        dev_in = torch.from_numpy(blob).to(device)
        dev_out = torch.empty(out_bytes if call is None else off_axis + call.out_bytes, dtype=torch.uint8, device=device)
        p_in, p_out = dev_in.data_ptr(), dev_out.data_ptr()
        vp = ctypes.c_void_p
        stream = vp(torch.cuda.current_stream(device).cuda_stream)
        ws_bytes = max(int(lib.salve_pose_graph_workspace_bytes(F, M)), int(lib.salve_pose_graph_optimise_workspace_bytes(F, M)))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device) if ws_bytes else None
        p_ws = vp(ws.data_ptr()) if ws is not None else None
        p_rows, p_start, p_n = vp(p_in + offs["rows"]), vp(p_in + offs["floor_start"]), vp(p_in + offs["n_nodes"])
        if call is not None:
            p_rows = call.launch(lib, p_in, offs, p_out + off_axis, status.ptr(device), stream)
        _lib.check(lib.salve_pose_graph_solve(p_rows, N, p_start, p_n, F, M, float(confidence_threshold), float(rot_threshold_deg), float(trans_threshold),
                                              int(cycle_filter), vp(p_out), vp(p_out + off_nodes), vp(p_out + off_floors), p_ws, ws_bytes,
                                              status.ptr(device), stream), "salve_pose_graph_solve")
        _lib.check(lib.salve_pose_graph_optimise(p_rows, N, p_start, p_n, F, M, float(confidence_threshold), vp(p_out + off_nodes), int(bool(robust)),
                                                 float(huber_k), sig_o, sig_p, int(max_iterations), float(relative_error_tol), float(absolute_error_tol),
                                                 vp(p_out + off_pgo_nodes), vp(p_out + off_pose), vp(p_out + off_pgo_floors), p_ws, ws_bytes,
                                                 status.ptr(device), stream), "salve_pose_graph_optimise")
        status.check(device, "pose_graph.optimise")   # (the one synchronising read)
        host = dev_out.cpu().numpy()
    axis_info = None
    if call is not None:
        meas, axis_info = call.decode(meas, floors, host[off_axis:])
    trees = _floor_solutions(meas, floors, floor_start, host[:N * _lib.GRAPH_ROW_OUT_DTYPE.itemsize].view(_lib.GRAPH_ROW_OUT_DTYPE),
                             host[off_nodes:off_floors].view(node_dt).reshape(F, M),
                             host[off_floors:off_floors + F * _lib.GRAPH_FLOOR_OUT_DTYPE.itemsize].view(_lib.GRAPH_FLOOR_OUT_DTYPE), confidence_threshold,
                             cycle_filter, rot_threshold_deg, trans_threshold, axis_info)
    pgo_nodes = host[off_pgo_nodes:off_pgo_floors].view(node_dt).reshape(F, M)
    pgo_floors = host[off_pgo_floors:off_pose].view(pgo_dt)
    poses = host[off_pose:out_bytes].view(np.float64).reshape(F, M, 3)

    options = {"method": "pgo", "robust": bool(robust), "huber_k": float(huber_k), "odometry_sigmas": [float(x) for x in odometry_sigmas],
               "prior_sigmas": [float(x) for x in prior_sigmas], "max_iterations": int(max_iterations), "relative_error_tol": float(relative_error_tol),
               "absolute_error_tol": float(absolute_error_tol)}
    fin = lambda x: float(x) if np.isfinite(x) else None
    solutions = []
    for f, (fl, tree) in enumerate(zip(floors, trees)):
        ids, fo = fl["pano_ids"], pgo_floors[f]
        wSi, pose = None, {}
        if tree.wSi_list is not None:
            wSi = [None] * len(tree.wSi_list)
            for v in np.nonzero(pgo_nodes[f, :len(ids)]["localized"])[0]:
                o, p = pgo_nodes[f, v], int(ids[v])
                wSi[p] = Sim2(np.array(o["R"], dtype=np.float32).reshape(2, 2), np.array(o["t"], dtype=np.float32), float(o["s"]))
                pose[p] = tuple(float(x) for x in poses[f, v])
        record = {**{k: int(fo[k]) for k in ("n_unknown_nodes", "n_factors", "n_iterations", "n_rejected", "n_downweighted")},
                  "stop_reason": _lib.PGO_STOP_NAMES[int(fo["stop_reason"])], "lambda": float(fo["lambda"]), "cost_initial": fin(fo["cost_initial"]),
                  "cost_final": fin(fo["cost_final"])}
        if axis_info is not None:
            record["axis_counts"] = dict(axis_info["counts"][f])
        solutions.append(PgoSolution(fl["building_id"], fl["floor_id"], ids, {**tree.options, **options}, tree, wSi, pose, record))
    return solutions


@dataclass
class HypothesisDraw:
    """The random subsets of one floor, as ransac_spanning_trees draws them (spanning_tree.py:213-244)."""

    building_id: str
    floor_id: str
    candidates: np.ndarray        # [K] indices into the measurement table, in measurement order: the reference's `measurements`
    subsets: List[np.ndarray]     # per hypothesis: the drawn indices INTO `candidates`, in the order numpy drew them
    masks: np.ndarray             # [H, words] uint32: bit k = the floor's k-th row in sorted order (EdgeMeasurements.compact)


def _subset_masks(fl: Dict[str, Any], subsets_rows: Sequence[np.ndarray], words: Optional[int] = None) -> np.ndarray:
    """uint32 [H, words]: bit k of hypothesis h is set iff the floor's k-th sorted row is one of subsets_rows[h] (indices into the table)."""
    n = len(fl["rows"])
    words = (n + 31) // 32 if words is None else words
    position = {int(r): k for k, r in enumerate(fl["rows"])}
    masks = np.zeros((len(subsets_rows), words), dtype=np.uint32)
    for h, rows in enumerate(subsets_rows):
        for r in rows:
            k = position[int(r)]
            masks[h, k >> 5] |= np.uint32(1 << (k & 31))
    return masks


def draw_hypotheses(meas: EdgeMeasurements, confidence_threshold: float, num_hypotheses: int = 100, sampling_fraction: float = 0.5,
                    min_num_edges: Optional[int] = None, seed: int = 0) -> List[HypothesisDraw]:
    """Host only: per floor (in `meas.floors()` order) the subsets ransac_spanning_trees would draw from the floor's thresholded
    measurements after np.random.seed(seed) -- K candidates in measurement order, m = ceil(sampling_fraction * K) of them per subset unless
    min_num_edges is given, min(int(binom(K, m)), num_hypotheses) subsets (1000 where the binomial overflows, as the reference's `except`),
    drawn without replacement with p proportional to 1 / |i2 - i1| on the pano ids.  One RandomState(seed) per floor; a floor without a
    candidate has no hypothesis (the reference raises ValueError for it)."""
    try:
        from scipy.special import binom   # (the reference's; a float, inf where it overflows)
    except ImportError:                   # without scipy: the exact binomial, overflowing where a float does
        binom = lambda K, m: float(math.comb(K, m))

    thr = np.float32(confidence_threshold)
    candidate = (meas.y_hat == 1) & (meas.prob >= thr)
    draws = []
    for fl in meas.compact():
        cand = np.sort(fl["rows"][candidate[fl["rows"]]])   # (measurement order)
        K = len(cand)
        subsets: List[np.ndarray] = []
        if K > 0:
            m = int(math.ceil(sampling_fraction * K)) if min_num_edges is None else int(min_num_edges)
            try:
                max_unique = int(binom(K, m))
            except (OverflowError, ValueError):
                max_unique = 1000
            p = 1 / np.absolute(meas.i2[cand] - meas.i1[cand])
            p = p / np.sum(p)
            rs = np.random.RandomState(seed)
            subsets = [rs.choice(a=K, size=m, replace=False, p=p) for _ in range(min(max_unique, num_hypotheses))]
        draws.append(HypothesisDraw(fl["building_id"], fl["floor_id"], cand, subsets, _subset_masks(fl, [cand[h] for h in subsets])))
    return draws


@dataclass
class TreeSampleSolution:
    building_id: str
    floor_id: str
    pano_ids: np.ndarray
    options: Dict[str, Any]                               # method, confidence_threshold and what the hypotheses were drawn with
    best: Optional[int]                                   # the winning hypothesis of the floor; None: no hypothesis, or every one scored NaN
    wSi_list: Optional[List[Optional[Sim2]]]              # the winner's, by pano id, in greedily_construct_st_Sim2's shape and length
    inlier_rows: np.ndarray                               # the reference's best_hypothesis: indices into the measurement table, ascending
    hypotheses: List[Dict[str, Any]]                      # per hypothesis: avg_rot_err, avg_trans_err, n_localized, n_measured, n_edges, origin
    n_measurements: int                                   # the length of the measurement table (of all floors): inlier_mask's
    parent: Dict[int, int] = field(default_factory=dict)
    depth: Dict[int, int] = field(default_factory=dict)
    counts: Dict[str, int] = field(default_factory=dict)  # n_nodes, n_rows, n_candidates, n_hyps, n_improvements, n_localized, n_inliers
    origin: Optional[int] = None
    avg_rot_err: Optional[float] = None                   # the winner's
    avg_trans_err: Optional[float] = None

    @property
    def inlier_mask(self) -> np.ndarray:
        """bool over the measurement table: this floor's inlier rows (OR the floors' masks: combined_inlier_mask)."""
        mask = np.zeros(self.n_measurements, dtype=bool)
        mask[self.inlier_rows] = True
        return mask

    def summary(self) -> str:
        c = self.counts
        return (f"{self.building_id} {self.floor_id}: hypothesis {self.best} of {c['n_hyps']} keeps {c['n_inliers']} / {c['n_candidates']} measurements, "
                f"localized {c['n_localized']} / {c['n_nodes']} panoramas")

    def to_json(self) -> Dict[str, Any]:
        fin = lambda x: None if x is None or x != x else float(x)
        sim = lambda S: {"R": S.rotation.flatten().tolist(), "t": S.translation.flatten().tolist(), "s": S.scale}
        return {"building_id": self.building_id, "floor_id": self.floor_id, "options": dict(self.options), "pano_ids": [int(p) for p in self.pano_ids],
                "counts": {k: int(v) for k, v in self.counts.items()}, "origin": self.origin, "best": self.best,
                "avg_rot_err": fin(self.avg_rot_err), "avg_trans_err": fin(self.avg_trans_err), "n_measurements": int(self.n_measurements),
                "n_poses": None if self.wSi_list is None else len(self.wSi_list), "inlier_rows": [int(r) for r in self.inlier_rows],
                "hypotheses": [{k: (fin(v) if k.startswith("avg_") else v) for k, v in h.items()} for h in self.hypotheses],
                "poses": {str(p): {**sim(S), "parent": self.parent[p], "depth": self.depth[p]}
                          for p, S in enumerate(self.wSi_list or []) if S is not None}}

    @classmethod
    def from_json(cls, d: Dict[str, Any]) -> "TreeSampleSolution":
        nan = lambda x: float("nan") if x is None else x
        sim = lambda r: Sim2(np.array(r["R"], dtype=np.float32).reshape(2, 2), np.array(r["t"], dtype=np.float32), float(r["s"]))
        wSi = None
        if d["n_poses"] is not None:
            wSi = [None] * d["n_poses"]
            for p, r in d["poses"].items():
                wSi[int(p)] = sim(r)
        hyps = [{k: (nan(v) if k.startswith("avg_") else v) for k, v in h.items()} for h in d["hypotheses"]]
        return cls(d["building_id"], d["floor_id"], np.array(d["pano_ids"], dtype=np.int64), dict(d["options"]), d["best"], wSi,
                   np.array(d["inlier_rows"], dtype=np.int64), hyps, d["n_measurements"], {int(p): r["parent"] for p, r in d["poses"].items()},
                   {int(p): r["depth"] for p, r in d["poses"].items()}, dict(d["counts"]), d["origin"],
                   None if d["best"] is None else nan(d["avg_rot_err"]), None if d["best"] is None else nan(d["avg_trans_err"]))


def combined_inlier_mask(solutions: Sequence[TreeSampleSolution]) -> Optional[np.ndarray]:
    """The floors' inlier masks ORed: solve's keep_rows.  None for no floor."""
    mask = None
    for sol in solutions:
        mask = sol.inlier_mask if mask is None else (mask | sol.inlier_mask)
    return mask


def sample_trees(meas: EdgeMeasurements, confidence_threshold: float, hypotheses: Optional[Sequence[HypothesisDraw]] = None,
                 num_hypotheses: int = 100, sampling_fraction: float = 0.5, min_num_edges: Optional[int] = None, seed: int = 0,
                 device="cuda:0") -> List[TreeSampleSolution]:
    """One TreeSampleSolution per floor of `meas` (in `meas.floors()` order): the reference's ransac_spanning_trees for every floor in one
    upload, one call (two launches), one read of the device status word and one download.  hypotheses: None -- draw_hypotheses(meas,
    confidence_threshold, num_hypotheses, sampling_fraction, min_num_edges, seed) -- or its result, or subsets of the caller's own in that
    form (only `masks` is uploaded).  A floor without a hypothesis, or whose every hypothesis has a NaN error, has best None, no pose and no
    inlier, where the reference would crash."""
    import torch

    from salve_amd import status

    device = torch.device(device)
    lib = _lib.load()
    floors = meas.compact()
    F = len(floors)
    if F == 0:
        return []
    if hypotheses is None:
        hypotheses = draw_hypotheses(meas, confidence_threshold, num_hypotheses, sampling_fraction, min_num_edges, seed)
    if [(h.building_id, h.floor_id) for h in hypotheses] != [(fl["building_id"], fl["floor_id"]) for fl in floors]:
        raise ValueError("pose_graph.sample_trees: `hypotheses` must name the floors of the measurements, in their order")
    table, floor_start, n_nodes, M = _device_table(meas, floors, "pose_graph.sample_trees")
    N = len(table)
    hyp_start = np.concatenate([[0], np.cumsum([len(h.masks) for h in hypotheses])]).astype(np.int32)
    H = int(hyp_start[-1])
    words = max([1] + [(len(fl["rows"]) + 31) // 32 for fl in floors])
    masks = np.zeros((H, words), dtype=np.uint32)
    for f, h in enumerate(hypotheses):
        if h.masks.shape[1] > words or (len(h.masks) and h.masks.shape[1] != (len(floors[f]["rows"]) + 31) // 32):
            raise ValueError(f"pose_graph.sample_trees: floor {h.building_id} {h.floor_id}: the masks do not have one bit per row of the floor")
        masks[hyp_start[f]:hyp_start[f + 1], :h.masks.shape[1]] = h.masks

    tree_dt, floor_dt, node_dt = _lib.GRAPH_TREE_OUT_DTYPE, _lib.GRAPH_SAMPLE_FLOOR_OUT_DTYPE, _lib.GRAPH_NODE_OUT_DTYPE
    out_trees = np.zeros(H, dtype=tree_dt)
    out_inlier = np.zeros(N, dtype=np.int32)
    out_nodes = np.zeros((F, M), dtype=node_dt)
    out_floors = np.zeros(F, dtype=floor_dt)
    out_floors["best"] = -1
    if H > 0:
        # one upload: rows | masks | floor_start | n_nodes | hyp_start; one output buffer: out_trees | out_nodes | out_floors | out_inlier
        parts = [table.view(np.uint8), masks.reshape(-1).view(np.uint8), floor_start.view(np.uint8), n_nodes.view(np.uint8), hyp_start.view(np.uint8)]
        offs = np.concatenate([[0], np.cumsum([len(x) for x in parts])])   # (48 N, then 4-byte tables: every offset is 4-byte aligned)
        off_nodes = H * tree_dt.itemsize
        off_floors = off_nodes + F * M * node_dt.itemsize
        off_inlier = off_floors + F * floor_dt.itemsize
        out_bytes = off_inlier + 4 * N
        with torch.cuda.device(device):
            dev_in = torch.from_numpy(np.concatenate(parts)).to(device)
            dev_out = torch.empty(out_bytes, dtype=torch.uint8, device=device)
            ws_bytes = int(lib.salve_pose_graph_sample_workspace_bytes(H, M))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
            p_in, p_out = dev_in.data_ptr(), dev_out.data_ptr()
            vp = ctypes.c_void_p
            _lib.check(lib.salve_pose_graph_sample_trees(vp(p_in), N, vp(p_in + int(offs[2])), vp(p_in + int(offs[3])), F, M, float(confidence_threshold),
                                                         vp(p_in + int(offs[4])), vp(p_in + int(offs[1])), H, words, vp(p_out), vp(p_out + off_inlier),
                                                         vp(p_out + off_nodes), vp(p_out + off_floors), vp(ws.data_ptr()), ws_bytes,
                                                         status.ptr(device), vp(torch.cuda.current_stream(device).cuda_stream)),
                       "salve_pose_graph_sample_trees")
            status.check(device, "pose_graph.sample_trees")   # (the one synchronising read)
            host = dev_out.cpu().numpy()
        out_trees = host[:off_nodes].view(tree_dt)
        out_nodes = host[off_nodes:off_floors].view(node_dt).reshape(F, M)
        out_floors = host[off_floors:off_inlier].view(floor_dt)
        out_inlier = host[off_inlier:].view(np.int32)
    else:   # nothing to launch: the candidates are counted here
        thr = np.float32(confidence_threshold)
        for f in range(F):
            r = table[floor_start[f]:floor_start[f + 1]]
            out_floors["n_candidates"][f] = int(((r["y_hat"] == 1) & (r["prob"] >= thr)).sum())

    options = {"method": "random_spanning_trees", "confidence_threshold": float(confidence_threshold), "num_hypotheses": int(num_hypotheses),
               "sampling_fraction": float(sampling_fraction), "min_num_edges": min_num_edges, "seed": int(seed)}
    sim = lambda R, t, s: Sim2(np.array(R, dtype=np.float32).reshape(2, 2), np.array(t, dtype=np.float32), float(s))
    solutions = []
    for f, fl in enumerate(floors):
        lo, hi = int(floor_start[f]), int(floor_start[f + 1])
        ids, fo, nodes = fl["pano_ids"], out_floors[f], out_nodes[f, :len(fl["pano_ids"])]
        best = int(fo["best"]) if fo["best"] >= 0 else None
        inliers = np.sort(fl["rows"][np.nonzero(out_inlier[lo:hi])[0]]).astype(np.int64)
        stats = [{"avg_rot_err": float(t["avg_rot_err"]), "avg_trans_err": float(t["avg_trans_err"]), "n_localized": int(t["n_localized"]),
                  "n_measured": int(t["n_measured"]), "n_edges": int(t["n_edges"]), "origin": int(ids[t["origin"]]) if t["origin"] >= 0 else None}
                 for t in out_trees[hyp_start[f]:hyp_start[f + 1]]]
        wSi, parent, depth, origin = None, {}, {}, None
        if best is not None and stats[best]["origin"] is not None:
            origin = stats[best]["origin"]
            wSi = [None] * (int(meas.i2[inliers].max()) + 1)   # greedily_construct_st_Sim2's length (spanning_tree.py:104, 110)
            for v in np.nonzero(nodes["localized"])[0]:
                p = int(ids[v])
                wSi[p] = sim(nodes["R"][v], nodes["t"][v], nodes["s"][v])
                parent[p], depth[p] = (int(ids[nodes["parent"][v]]) if nodes["parent"][v] >= 0 else -1), int(nodes["depth"][v])
        counts = {"n_nodes": len(ids), "n_rows": hi - lo, "n_candidates": int(fo["n_candidates"]), "n_hyps": int(hyp_start[f + 1] - hyp_start[f]),
                  "n_improvements": int(fo["n_improvements"]), "n_localized": len(parent), "n_inliers": len(inliers)}
        solutions.append(TreeSampleSolution(fl["building_id"], fl["floor_id"], ids, dict(options), best, wSi, inliers, stats, len(meas), parent, depth,
                                            counts, origin, float(fo["avg_rot_err"]) if best is not None else None,
                                            float(fo["avg_trans_err"]) if best is not None else None))
    return solutions


def run(meas: EdgeMeasurements, confidence_threshold: float, method: str = "spanning_tree", filter_by_random_spanning_trees: bool = False,
        num_hypotheses: int = 100, sampling_fraction: float = 0.5, seed: int = 0, device="cuda:0", truth=None, report_options=None,
        axis: Optional[AxisInputs] = None, **solve_options):
    """What the command line and ingest.score_floor(pose_graph=...) do with their options.  method "spanning_tree": solve(meas,
    confidence_threshold, **solve_options), behind the random-spanning-trees edge filter if filter_by_random_spanning_trees; method
    "random_spanning_trees": sample_trees; method "pgo": optimise(meas, confidence_threshold, **solve_options) -- the spanning tree refined by
    pose-graph optimisation, behind the same edge filter if asked; robust, max_iterations, relative_error_tol, absolute_error_tol (and huber_k, the
    sigmas) among the options are optimise's own and belong to this method alone.  With the defaults this IS solve: the same launches and values.
    truth: None, or the floors' ground truth -- salve_amd.floor_report.FloorTruth objects, as a list in `meas.floors()` order or a dict keyed by
    (building_id, floor_id).  Then the result is (solutions, reports): floor_report.report(solutions, truths, **report_options) follows the
    solve.
    axis: None, or the floors' AxisInputs: solve's and optimise's axis alignment by vanishing angle (the reference's
    --use_axis_alignment, on by default there).  The random-spanning-trees edge filter samples the RAW rows and the alignment follows it, as in
    run_sfm.py:354-426.  Method random_spanning_trees refuses it: the reference does not align there."""
    if truth is not None:
        from salve_amd import floor_report

        solutions = run(meas, confidence_threshold, method=method, filter_by_random_spanning_trees=filter_by_random_spanning_trees,
                        num_hypotheses=num_hypotheses, sampling_fraction=sampling_fraction, seed=seed, device=device, axis=axis, **solve_options)
        truths = [truth[(s.building_id, s.floor_id)] for s in solutions] if isinstance(truth, dict) else list(truth)
        return solutions, floor_report.report(solutions, truths, device=device, **(report_options or {}))
    if method not in ("spanning_tree", "random_spanning_trees", "pgo"):
        raise ValueError(f"pose_graph.run: unknown method {method!r}")
    sampling = {"num_hypotheses": num_hypotheses, "sampling_fraction": sampling_fraction, "seed": seed}
    pgo_options = {k: solve_options.pop(k) for k in PGO_OPTIONS if k in solve_options}
    if pgo_options and method != "pgo":
        raise ValueError(f"pose_graph.run: {sorted(pgo_options)} belong to method pgo")
    if axis is not None and method == "random_spanning_trees":
        raise ValueError("pose_graph.run: method random_spanning_trees takes no axis alignment (the reference samples the raw measurements)")
    axis_option = {} if axis is None else {"axis": axis}   # (None: solve and optimise are called exactly as before)
    if method == "pgo":
        keep = None
        if filter_by_random_spanning_trees:   # the factors are then the kept rows only (run_sfm.py passes high_conf_inlier_measurements on)
            keep = combined_inlier_mask(sample_trees(meas, confidence_threshold, device=device, **sampling))
        solutions = optimise(meas, confidence_threshold, keep_rows=keep, device=device, **axis_option, **pgo_options, **solve_options)
        for sol in solutions:
            if filter_by_random_spanning_trees:
                sol.options["filter_by_random_spanning_trees"] = dict(sampling)
        return solutions
    if method == "random_spanning_trees":
        if solve_options or filter_by_random_spanning_trees:
            raise ValueError("pose_graph.run: method random_spanning_trees takes neither the cycle filter's options nor the edge filter")
        return sample_trees(meas, confidence_threshold, device=device, **sampling)
    if not filter_by_random_spanning_trees:
        return solve(meas, confidence_threshold, device=device, **axis_option, **solve_options)
    samples = sample_trees(meas, confidence_threshold, device=device, **sampling)
    solutions = solve(meas, confidence_threshold, device=device, keep_rows=combined_inlier_mask(samples), **axis_option, **solve_options)
    for sol in solutions:
        sol.options["filter_by_random_spanning_trees"] = dict(sampling)
    return solutions


def json_fname(sol) -> str:
    return f"pose_graph_{sol.building_id}_{sol.floor_id}.json"


def write_json(sol, out_dir: str) -> str:
    os.makedirs(out_dir, exist_ok=True)
    fp = f"{out_dir}/{json_fname(sol)}"
    with open(fp, "w") as f:
        json.dump(sol.to_json(), f, indent=4)
    return fp


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m salve_amd.pose_graph",
                                 description="Global panorama poses per floor from prediction files: best pair, cycle filter, spanning tree; or "
                                             "the best of many random spanning trees.")
    ap.add_argument("pred_dir", metavar="PRED_DIR", help="directory of batch_*.json prediction files")
    ap.add_argument("--hypotheses", required=True, metavar="ROOT", help="directory of the alignment hypotheses (export_alignment_hypotheses.py)")
    ap.add_argument("--confidence-threshold", type=float, required=True, help="least probability of a positive prediction that counts")
    ap.add_argument("--no-cycle-filter", action="store_true", help="chain the most confident edges as they are")
    ap.add_argument("--rot-deg", type=float, default=ROT_THRESHOLD_DEG, help="3-cycle rotation threshold in degrees (default %(default)s)")
    ap.add_argument("--trans", type=float, default=TRANS_THRESHOLD, help="3-cycle translation threshold (default %(default)s; inf: rotation only)")
    ap.add_argument("--out", metavar="DIR", default=None, help="where the pose_graph_*.json files go (default: PRED_DIR)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--method", choices=("spanning_tree", "random_spanning_trees", "pgo"), default="spanning_tree",
                    help="random_spanning_trees: the best of --num-hypotheses random subsets' trees (the cycle filter's options do not apply); "
                         "pgo: the spanning tree refined by pose-graph optimisation over all thresholded predictions -- the cycle filter's options "
                         "still shape the initial tree, and --no-cycle-filter gives the reference's pgo pipeline (run_sfm.py:448-451)")
    ap.add_argument("--pgo-max-iterations", type=int, default=None, help="method pgo: most linearisations per floor (default 100)")
    ap.add_argument("--pgo-no-robust", action="store_true", help="method pgo: plain least squares instead of the Huber loss")
    ap.add_argument("--filter-by-random-spanning-trees", action="store_true",
                    help="methods spanning_tree and pgo: keep only the predictions of the best random subset before anything else")
    ap.add_argument("--num-hypotheses", type=int, default=100, help="random subsets per floor (default %(default)s)")
    ap.add_argument("--sampling-fraction", type=float, default=0.5, help="share of a floor's thresholded predictions per subset (default %(default)s)")
    ap.add_argument("--seed", type=int, default=0, help="seed of every floor's draws (default %(default)s)")
    ap.add_argument("--zind-root", metavar="DIR", default=None,
                    help="the ZInD data set ({DIR}/{building}/zind_data.json): also write floor_report_{building}_{floor}.json per floor -- rotation and "
                         "translation error against the ground truth, percent localized, floor-plan IoU -- and print the summary")
    ap.add_argument("--axis-alignment", action="store_true",
                    help="methods spanning_tree and pgo: align every relative pose by the two panoramas' vanishing angles first (the reference's "
                         "--use_axis_alignment, which is ON by default there; here the default is off).  Needs --mhnet-predictions-data-root and --zind-root")
    ap.add_argument("--mhnet-predictions-data-root", metavar="DIR", default=None,
                    help="MHNet's predictions (horizon_net/{building}/*.json, vanishing_angle/{building}.json): the rooms, W/D/Os and angles of --axis-alignment")
    ap.add_argument("--report-seed", type=int, default=0, help="seed of the report's alignment RANSAC (default %(default)s)")
    ap.add_argument("--report-iters", type=int, default=1000, help="alignment subsets per floor (default %(default)s)")
    args = ap.parse_args(argv)
    if args.axis_alignment:
        if args.mhnet_predictions_data_root is None or args.zind_root is None:
            ap.error("--axis-alignment needs --mhnet-predictions-data-root and --zind-root")
        if args.method == "random_spanning_trees":
            ap.error("--axis-alignment belongs to --method spanning_tree or pgo")
    elif args.mhnet_predictions_data_root is not None:
        ap.error("--mhnet-predictions-data-root belongs to --axis-alignment")
    meas = EdgeMeasurements.from_prediction_files(args.pred_dir, args.hypotheses)
    if args.axis_alignment:
        from salve_amd import hypotheses

        options_axis = {"axis": AxisInputs.from_floors(hypotheses.load_floors(args.zind_root, args.mhnet_predictions_data_root,
                                                                               sorted(set(meas.building_id))))}
    else:
        options_axis = {}
    if args.method == "random_spanning_trees":
        if args.filter_by_random_spanning_trees:
            ap.error("--filter-by-random-spanning-trees belongs to --method spanning_tree or pgo")
        options = {}
    else:
        options = {"cycle_filter": not args.no_cycle_filter, "rot_threshold_deg": args.rot_deg, "trans_threshold": args.trans}
    if args.method == "pgo":
        if args.pgo_max_iterations is not None:
            if args.pgo_max_iterations < 0:
                ap.error("--pgo-max-iterations must not be negative")
            options["max_iterations"] = args.pgo_max_iterations
        if args.pgo_no_robust:
            options["robust"] = False
    elif args.pgo_max_iterations is not None or args.pgo_no_robust:
        ap.error("--pgo-max-iterations and --pgo-no-robust belong to --method pgo")
    solutions = run(meas, args.confidence_threshold, method=args.method, filter_by_random_spanning_trees=args.filter_by_random_spanning_trees,
                    num_hypotheses=args.num_hypotheses, sampling_fraction=args.sampling_fraction, seed=args.seed, device=args.device, **options_axis, **options)
    for sol in solutions:
        write_json(sol, args.out or args.pred_dir)
        print(sol.summary())
    if args.zind_root is not None:
        from salve_amd import floor_report

        reports = floor_report.report(solutions, floor_report.load_truths(args.zind_root, solutions), num_iters=args.report_iters, seed=args.report_seed,
                                      device=args.device)
        for rep in reports:
            floor_report.write_json(rep, args.out or args.pred_dir)
            print(rep.summary())
        print(json.dumps(floor_report.summarize(reports)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
