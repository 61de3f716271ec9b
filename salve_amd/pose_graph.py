"""From a floor's scored alignment hypotheses to one global Sim(2) pose per panorama: the `spanning_tree` method of the reference's
scripts/run_sfm.py:112-152 and :440-446, with and without its cycle filter, for every floor of a prediction directory in ONE launch
(include/salve_hip.h: salve_pose_graph_solve; salve_amd/csrc/pose_graph.hip).

    python -m salve_amd.pose_graph PRED_DIR --hypotheses ROOT --confidence-threshold X [--no-cycle-filter] [--rot-deg D] [--trans T] [--out DIR]

reads the `batch_*.json` prediction files of PRED_DIR (evaluate.run_test_epoch, evaluate.run_fused_epoch, ingest.score_floor), looks every
prediction's alignment hypothesis up under ROOT, and writes one `pose_graph_{building}_{floor}.json` per floor.

The steps, and the reference functions they stand behind:
  1. a prediction counts iff y_hat == 1 and its probability reaches the threshold   (edge_classification.py:213-251)
  2. per panorama pair the most confident one stays                                  (edge_classification.py:254-311)
  3. pairs in no consistent 3-cycle are dropped (cycle_filter)                       (cycle_consistency.py:26-91, 172-303)
  4. the relative poses are chained along a spanning tree of the largest component   (spanning_tree.py:73-141)
Where the reference leaves a choice to an unspecified iteration order, this module fixes it: among equally probable
predictions of a pair the first in row order, among equally large components the one with the lowest panorama, among several shortest paths
the one through the lowest-index neighbour of the previous BFS level.  Pose-graph optimisation, RANSAC over spanning trees, axis alignment
and the evaluation against ground truth are NOT here.  A floor may have at most 256 panoramas.
"""

from __future__ import annotations

import argparse
import ctypes
import glob
import json
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


def solve(meas: EdgeMeasurements, confidence_threshold: float, cycle_filter: bool = True, rot_threshold_deg: float = ROT_THRESHOLD_DEG,
          trans_threshold: float = TRANS_THRESHOLD, device="cuda:0") -> List[FloorSolution]:
    """One FloorSolution per floor of `meas` (in `meas.floors()` order): one upload, one launch for all floors, one read of the device status
    word, one download.  confidence_threshold has no default: the reference's run_sfm.py takes it from the command line.  rot_threshold_deg
    and trans_threshold are filter_to_SE2_cycle_consistent_edges' own; trans_threshold=inf gives the rotation-only filter.  cycle_filter=False
    chains the chosen edges as they are (run_sfm.py:440-446).  A floor of more than 256 panoramas is refused before anything is launched."""
    import torch

    from salve_amd import status

    device = torch.device(device)
    lib = _lib.load()
    floors = meas.compact()
    F = len(floors)
    if F == 0:
        return []
    N = len(meas)
    order = np.concatenate([fl["rows"] for fl in floors])
    table = np.zeros(N, dtype=_lib.GRAPH_ROW_DTYPE)
    table["i1"], table["i2"] = np.concatenate([fl["c1"] for fl in floors]), np.concatenate([fl["c2"] for fl in floors])
    table["prob"], table["y_hat"] = meas.prob[order], meas.y_hat[order]
    table["R"], table["t"], table["s"] = meas.R[order].reshape(N, 4), meas.t[order], meas.s[order]
    floor_start = np.concatenate([[0], np.cumsum([len(fl["rows"]) for fl in floors])]).astype(np.int32)
    n_nodes = np.array([len(fl["pano_ids"]) for fl in floors], dtype=np.int32)
    M = int(n_nodes.max())
    if M > _lib.GRAPH_MAX_NODES:   # (the library refuses it as well: SALVE_ERR_BAD_ARG)
        worst = floors[int(n_nodes.argmax())]
        raise _lib.SalveHipError(f"pose_graph.solve: floor {worst['building_id']} {worst['floor_id']} has {M} panoramas, more than the "
                                 f"{_lib.GRAPH_MAX_NODES} a floor may have")

    # one upload: rows | floor_start | n_nodes; one output buffer: out_rows | out_nodes | out_floors
    blob = np.concatenate([table.view(np.uint8), floor_start.view(np.uint8), n_nodes.view(np.uint8)])
    off_nodes = _align8(N * _lib.GRAPH_ROW_OUT_DTYPE.itemsize)
    off_floors = off_nodes + F * M * _lib.GRAPH_NODE_OUT_DTYPE.itemsize
    out_bytes = off_floors + F * _lib.GRAPH_FLOOR_OUT_DTYPE.itemsize
    with torch.cuda.device(device):
        dev_in = torch.from_numpy(blob).to(device)
        dev_out = torch.empty(out_bytes, dtype=torch.uint8, device=device)
        p_in, p_out = dev_in.data_ptr(), dev_out.data_ptr()
        vp = ctypes.c_void_p
        ws_bytes = int(lib.salve_pose_graph_workspace_bytes(F, M))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device) if ws_bytes else None
        _lib.check(lib.salve_pose_graph_solve(vp(p_in), N, vp(p_in + table.nbytes), vp(p_in + table.nbytes + floor_start.nbytes), F, M,
                                              float(confidence_threshold), float(rot_threshold_deg), float(trans_threshold), int(bool(cycle_filter)),
                                              vp(p_out), vp(p_out + off_nodes), vp(p_out + off_floors), vp(ws.data_ptr()) if ws is not None else None,
                                              ws_bytes, status.ptr(device), vp(torch.cuda.current_stream(device).cuda_stream)),
                   "salve_pose_graph_solve")
        status.check(device, "pose_graph.solve")   # (the one synchronising read)
        host = dev_out.cpu().numpy()
    out_rows = host[:N * _lib.GRAPH_ROW_OUT_DTYPE.itemsize].view(_lib.GRAPH_ROW_OUT_DTYPE)
    out_nodes = host[off_nodes:off_floors].view(_lib.GRAPH_NODE_OUT_DTYPE).reshape(F, M)
    out_floors = host[off_floors:].view(_lib.GRAPH_FLOOR_OUT_DTYPE)

    options = {"confidence_threshold": float(confidence_threshold), "cycle_filter": bool(cycle_filter), "rot_threshold_deg": float(rot_threshold_deg),
               "trans_threshold": float(trans_threshold)}
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


def json_fname(sol: FloorSolution) -> str:
    return f"pose_graph_{sol.building_id}_{sol.floor_id}.json"


def write_json(sol: FloorSolution, out_dir: str) -> str:
    os.makedirs(out_dir, exist_ok=True)
    fp = f"{out_dir}/{json_fname(sol)}"
    with open(fp, "w") as f:
        json.dump(sol.to_json(), f, indent=4)
    return fp


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m salve_amd.pose_graph",
                                 description="Global panorama poses per floor from prediction files: best pair, cycle filter, spanning tree.")
    ap.add_argument("pred_dir", metavar="PRED_DIR", help="directory of batch_*.json prediction files")
    ap.add_argument("--hypotheses", required=True, metavar="ROOT", help="directory of the alignment hypotheses (export_alignment_hypotheses.py)")
    ap.add_argument("--confidence-threshold", type=float, required=True, help="least probability of a positive prediction that counts")
    ap.add_argument("--no-cycle-filter", action="store_true", help="chain the most confident edges as they are")
    ap.add_argument("--rot-deg", type=float, default=ROT_THRESHOLD_DEG, help="3-cycle rotation threshold in degrees (default %(default)s)")
    ap.add_argument("--trans", type=float, default=TRANS_THRESHOLD, help="3-cycle translation threshold (default %(default)s; inf: rotation only)")
    ap.add_argument("--out", metavar="DIR", default=None, help="where the pose_graph_*.json files go (default: PRED_DIR)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    meas = EdgeMeasurements.from_prediction_files(args.pred_dir, args.hypotheses)
    for sol in solve(meas, args.confidence_threshold, cycle_filter=not args.no_cycle_filter, rot_threshold_deg=args.rot_deg,
                     trans_threshold=args.trans, device=args.device):
        write_json(sol, args.out or args.pred_dir)
        print(sol.summary())
    return 0


if __name__ == "__main__":
    sys.exit(main())
