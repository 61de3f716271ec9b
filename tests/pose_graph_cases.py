"""salve_pose_graph_solve (include/salve_hip.h): a numpy emulator of the entry, the case list the host and the GPU tests share, and emulated
WRONG kernels that the case list must catch.

The emulator follows the four phases the header states -- A best row per pair, B 3-cycles, C component, D BFS tree and poses -- and shares
no code with salve_amd/pose_graph.py.  Its Sim(2) arithmetic is vectorised ELEMENTWISE numpy: float32 elementwise operations never fuse a
product into a sum, so every value but one is bit-comparable with the kernel; the one is the rotation error, which carries an arctan2.

A case is a dict: name, rows (ROW records of all floors), floor_start, n_nodes, max_nodes, the four scalars, `refused` (the host refuses
it: no launch) and `reference` (the host test also compares its tree with the reference-shaped restatement).  `run_case(case, fn)` hands `fn`
three output buffers filled with SENTINEL bytes, GUARD records on both sides, and returns them with the status bit `fn` reports.

Conditions on the case list, asserted by `check_conditions` (tests/test_pose_graph_cases_host.py runs it on the CPU):
  - no 3-cycle of any case has an emulator error within a relative 1e-4 of a finite threshold, so a few-ulp difference of the device's
    atan2f cannot flip a decision (an error compared with an INFINITE threshold is decided by being finite or not: exact);
  - every `reference` case has unique shortest paths from its origin, one largest component and no tie among a pair's candidates."""

from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64
ROW = np.dtype([("i1", "<i4"), ("i2", "<i4"), ("prob", "<f4"), ("y_hat", "<i4"), ("R", "<f4", (4,)), ("t", "<f4", (2,)), ("s", "<f8")])
ROW_OUT = np.dtype([("chosen", "<i4"), ("consistent", "<i4"), ("n_triplets", "<i4"), ("n_consistent", "<i4"), ("min_rot_err", "<f4"),
                    ("min_trans_err", "<f4")])
NODE_OUT = np.dtype([("localized", "<i4"), ("parent", "<i4"), ("depth", "<i4"), ("reserved", "<i4"), ("R", "<f4", (4,)), ("t", "<f4", (2,)),
                     ("s", "<f8")])
FLOOR_OUT = np.dtype([("n_chosen", "<i4"), ("n_triplets", "<i4"), ("n_consistent_triplets", "<i4"), ("n_consistent_edges", "<i4"),
                      ("n_localized", "<i4"), ("origin", "<i4")])
SENTINEL = 0xA5   # every byte of a fresh output buffer
GUARD = 2         # records in front of and behind each output array
MAX_NODES = 256
STATUS_BAD_GRAPH_ROW = 128   # include/salve_hip.h: SALVE_STATUS_BAD_GRAPH_ROW
RAD2DEG = F32(180.0 / np.pi)
INF = F32(np.inf)
MARGIN = 1e-4

WRONG_KERNELS = ("tie_takes_last", "y_hat_ignored", "confidence_gt", "error_le", "inverse_missing_on_ac", "compose_order_swapped", "c_above_a",
                 "compose_scale_dropped", "inverse_scale_dropped", "highest_parent", "uninverted_for_p_below_v", "wrong_component_on_tie",
                 "origin_not_lowest")


# ---- Sim(2) on tuples of arrays (R00, R01, R10, R11, tx, ty, s): R, t float32, s float64; elementwise, so nothing fuses

def sim2_of_rows(rows):
    R, t = rows["R"], rows["t"]
    return (R[..., 0].astype(F32), R[..., 1].astype(F32), R[..., 2].astype(F32), R[..., 3].astype(F32), t[..., 0].astype(F32), t[..., 1].astype(F32),
            rows["s"].astype(F64))


def sim2_inverse(A, wrong=None):
    R00, R01, R10, R11, tx, ty, s = A
    sf = np.ones_like(tx) if wrong == "inverse_scale_dropped" else s.astype(F32)
    ux, uy = sf * tx, sf * ty
    n00, n01, n10, n11 = R00, R10, R01, R11
    return (n00, n01, n10, n11, (-n00) * ux + (-n01) * uy, (-n10) * ux + (-n11) * uy, 1.0 / s)


def sim2_compose(A, B, wrong=None):
    if wrong == "compose_order_swapped":
        A, B = B, A
    a00, a01, a10, a11, atx, aty, a_s = A
    b00, b01, b10, b11, btx, bty, b_s = B
    inv = np.ones_like(atx) if wrong == "compose_scale_dropped" else (1.0 / b_s).astype(F32)
    return (a00 * b00 + a01 * b10, a00 * b01 + a01 * b11, a10 * b00 + a11 * b10, a10 * b01 + a11 * b11,
            (a00 * btx + a01 * bty) + inv * atx, (a10 * btx + a11 * bty) + inv * aty, a_s * b_s)


def cycle_errors(rows, r01, r12, r02, wrong=None):
    """(rot_err_deg, trans_err), float32 arrays: the cycles whose edges (i0, i1), (i1, i2), (i0, i2) are rows r01, r12, r02."""
    with np.errstate(all="ignore"):
        S02 = sim2_of_rows(rows[r02])
        X = S02 if wrong == "inverse_missing_on_ac" else sim2_inverse(S02, wrong)
        Z = sim2_compose(sim2_compose(X, sim2_of_rows(rows[r12]), wrong), sim2_of_rows(rows[r01]), wrong)
        rot = np.abs(np.arctan2(Z[2], Z[0])).astype(F32) * RAD2DEG
        trans = np.sqrt(Z[4] * Z[4] + Z[5] * Z[5]).astype(F32)
    return rot.astype(F32), trans


def _bits(x):
    return np.asarray(x, dtype=F32).view(np.uint32)


# ---- one floor

def emulate_floor(rows, n, conf, rot_thr, trans_thr, cycle_filter, wrong=None):
    """The outputs of one well-formed floor: (row_out [len(rows)], node_out [n], floor_out [1], details).  details: the cycles with their
    errors and the graph of phases C and D, for the conditions and the host tests."""
    conf, rot_thr, trans_thr = F32(conf), F32(rot_thr), F32(trans_thr)
    row_out = np.zeros(len(rows), dtype=ROW_OUT)
    row_out["min_rot_err"], row_out["min_trans_err"] = INF, INF
    node_out = np.zeros(n, dtype=NODE_OUT)
    node_out["parent"], node_out["depth"] = -1, -1
    floor_out = np.zeros(1, dtype=FLOOR_OUT)
    floor_out["origin"] = -1

    # A: the first candidate of largest prob per pair
    chosen, tie = {}, False
    for r in range(len(rows)):
        p = rows["prob"][r]
        is_class = wrong == "y_hat_ignored" or rows["y_hat"][r] == 1
        above = (p > conf) if wrong == "confidence_gt" else (p >= conf)   # False for NaN
        if not (is_class and above):
            continue
        key = (int(rows["i1"][r]), int(rows["i2"][r]))
        if key not in chosen:
            chosen[key] = r
        else:
            best = rows["prob"][chosen[key]]
            tie = tie or p == best
            if p > best or (wrong == "tie_takes_last" and p == best):
                chosen[key] = r
    for r in chosen.values():
        row_out["chosen"][r] = 1
    adj = {v: set() for v in range(n)}
    for a, b in chosen:
        adj[a].add(b)
        adj[b].add(a)

    # B: every 3-cycle a < b < c once, from its edge (a, b)
    trip = []
    for (a, b) in sorted(chosen):
        for c in sorted(adj[a] & adj[b]):
            if c > b:
                trip.append((a, b, c))
            elif wrong == "c_above_a" and c > a:
                trip.append((a, c, b))   # the same cycle, visited a second time
    trip = np.array(trip, dtype=np.int64).reshape(-1, 3)
    r01 = np.array([chosen[(a, b)] for a, b, c in trip], dtype=np.int64)
    r12 = np.array([chosen[(b, c)] for a, b, c in trip], dtype=np.int64)
    r02 = np.array([chosen[(a, c)] for a, b, c in trip], dtype=np.int64)
    if len(trip):
        rot, trans = cycle_errors(rows, r01, r12, r02, wrong)
        if wrong == "error_le":
            ok = (rot <= rot_thr) & (trans <= trans_thr)
        else:
            ok = (rot < rot_thr) & (trans < trans_thr)    # False for a NaN error
        min_rot, min_trans = _bits(row_out["min_rot_err"]).copy(), _bits(row_out["min_trans_err"]).copy()
        for edge_rows in (r01, r12, r02):
            np.add.at(row_out["n_triplets"], edge_rows, 1)
            np.add.at(row_out["n_consistent"], edge_rows, ok.astype(np.int32))
            np.minimum.at(min_rot, edge_rows, _bits(rot))       # on the bit patterns: a NaN lies above +inf
            np.minimum.at(min_trans, edge_rows, _bits(trans))
        row_out["min_rot_err"], row_out["min_trans_err"] = min_rot.view(F32), min_trans.view(F32)
    else:
        rot = trans = np.zeros(0, dtype=F32)
        ok = np.zeros(0, dtype=bool)
    row_out["consistent"] = row_out["n_consistent"] > 0
    floor_out["n_chosen"] = len(chosen)
    floor_out["n_triplets"] = len(trip)
    floor_out["n_consistent_triplets"] = int(ok.sum())
    floor_out["n_consistent_edges"] = int(row_out["consistent"].sum())

    # C: the largest component of the graph, the one with the lowest node among equals
    graph = {k: r for k, r in chosen.items() if not cycle_filter or row_out["consistent"][r]}
    nbrs = {v: set() for v in range(n)}
    for a, b in graph:
        nbrs[a].add(b)
        nbrs[b].add(a)
    seen, comps = set(), []
    for v in range(n):
        if v in seen or not nbrs[v]:
            continue
        comp, stack = {v}, [v]
        while stack:
            for u in nbrs[stack.pop()]:
                if u not in comp:
                    comp.add(u)
                    stack.append(u)
        seen |= comp
        comps.append(sorted(comp))      # in the order of their lowest nodes
    details = {"triplets": trip, "rot": rot, "trans": trans, "ok": ok, "chosen": chosen, "graph": graph, "components": comps, "tie": tie,
               "paths": {}}
    if not comps:
        return row_out, node_out, floor_out, details
    largest = max(len(c) for c in comps)
    tied = [c for c in comps if len(c) == largest]
    comp = tied[-1] if wrong == "wrong_component_on_tie" else tied[0]
    origin = comp[-1] if wrong == "origin_not_lowest" else comp[0]

    # D: BFS by levels; the parent is the lowest-index neighbour in the previous level
    pose = {origin: tuple(np.array([x], dtype=F32) for x in (1, 0, 0, 1, 0, 0)) + (np.array([1.0], dtype=F64),)}
    depth, parent, n_paths = {origin: 0}, {origin: -1}, {origin: 1}
    level = [origin]
    while level:
        nxt = []
        for v in comp:
            if v in depth:
                continue
            cand = sorted(u for u in nbrs[v] if depth.get(u, -1) == depth[level[0]])
            if cand:
                nxt.append((v, cand[-1] if wrong == "highest_parent" else cand[0], sum(n_paths[u] for u in cand)))
        with np.errstate(all="ignore"):
            for v, p, k in nxt:
                E = sim2_of_rows(rows[[graph[(min(p, v), max(p, v))]]])
                if (p < v) != (wrong == "uninverted_for_p_below_v"):
                    E = sim2_inverse(E, wrong)
                pose[v] = sim2_compose(pose[p], E, wrong)
        for v, p, k in nxt:
            depth[v], parent[v], n_paths[v] = depth[p] + 1, p, k
        level = [v for v, _, _ in nxt]
    for v in depth:
        S = pose[v]
        node_out[v] = (1, parent[v], depth[v], 0, [S[0][0], S[1][0], S[2][0], S[3][0]], [S[4][0], S[5][0]], S[6][0])
    floor_out["n_localized"], floor_out["origin"] = len(depth), origin
    details["paths"] = n_paths
    details["tied_components"] = len(tied)
    return row_out, node_out, floor_out, details


def floor_is_well_formed(rows, n, max_nodes):
    if n < 0 or n > max_nodes:
        return False
    i1, i2 = rows["i1"].astype(np.int64), rows["i2"].astype(np.int64)
    if ((i1 < 0) | (i1 >= i2) | (i2 >= n)).any():
        return False
    key = i1 * (1 << 32) + i2
    return bool((key[1:] >= key[:-1]).all())


def emulate(case, out_rows, out_nodes, out_floors, wrong=None, details=None):
    """Write what salve_pose_graph_solve writes into the three arrays (views WITHOUT their guards); returns whether the status bit is raised.
    Node record f * max_nodes + v is written for v < n_nodes[f] only."""
    raised = False
    M = case["max_nodes"]
    for f in range(len(case["n_nodes"])):
        lo, hi, n = int(case["floor_start"][f]), int(case["floor_start"][f + 1]), int(case["n_nodes"][f])
        rows = case["rows"][lo:hi]
        if not floor_is_well_formed(rows, n, M):
            raised = True
            n = n if 0 <= n <= M else 0
            ro, no, fo, det = emulate_floor(rows[:0], n, 0, 0, 0, 1)
            ro = np.zeros(hi - lo, dtype=ROW_OUT)
            ro["min_rot_err"], ro["min_trans_err"] = INF, INF
        else:
            ro, no, fo, det = emulate_floor(rows, n, case["confidence_threshold"], case["rot_threshold_deg"], case["trans_threshold"],
                                            case["cycle_filter"], wrong)
        out_rows[lo:hi] = ro
        out_nodes[f * M:f * M + n] = no
        out_floors[f] = fo[0]
        if details is not None:
            details.append(det)
    return raised


def fresh_buffers(case):
    n_rows, F, M = len(case["rows"]), len(case["n_nodes"]), case["max_nodes"]
    mk = lambda count, dt: np.frombuffer(bytes([SENTINEL]) * ((count + 2 * GUARD) * dt.itemsize), dtype=dt).copy()
    return mk(n_rows, ROW_OUT), mk(F * M, NODE_OUT), mk(F, FLOOR_OUT)


def run_case(case, fn):
    """((out_rows, out_nodes, out_floors) WITH their guards as `fn(case, rows_view, nodes_view, floors_view)` left them, the status bit)."""
    bufs = fresh_buffers(case)
    raised = fn(case, *[b[GUARD:len(b) - GUARD] for b in bufs])
    return bufs, bool(raised)


def emulated(wrong=None):
    return lambda case, ro, no, fo: emulate(case, ro, no, fo, wrong)


# ---- building cases: relative poses from global ones, in float64, stored as the reference stores them

def _compose64(A, B):
    return (A[0] @ B[0], A[0] @ B[1] + A[1] / B[2], A[2] * B[2])


def _inverse64(A):
    return (A[0].T, -A[0].T @ (A[2] * A[1]), 1.0 / A[2])


def _rot(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s], [s, c]])


def global_poses(rng, n, scales=False):
    return [(_rot(rng.uniform(-180, 180)), rng.uniform(-5, 5, size=2), float(rng.uniform(0.5, 2.0)) if scales else 1.0) for _ in range(n)]


class FloorBuilder:
    def __init__(self, n, poses=None, rng=None):
        self.n, self.rows, self.rng = n, [], rng
        self.poses = poses

    def edge(self, i1, i2, prob=None, y_hat=1, rot_deg=0.0, shift=(0.0, 0.0), t=None, s=None):
        """One row for pair (i1, i2): the relative pose of the global poses, corrupted by a rotation and a translation."""
        S = _compose64(_inverse64(self.poses[i2]), self.poses[i1])
        S = (_rot(rot_deg) @ S[0], S[1] + np.asarray(shift, dtype=np.float64), S[2] if s is None else s)
        if prob is None:
            prob = 0.55 + 0.4 * self.rng.random()
        self.rows.append((i1, i2, F32(prob), y_hat, S[0].astype(F32).reshape(4), (S[1] if t is None else np.asarray(t)).astype(F32), float(S[2])))
        return self

    def build(self, sort=True):
        rows = np.array(self.rows, dtype=ROW) if self.rows else np.zeros(0, dtype=ROW)
        if sort:
            rows = rows[np.lexsort((rows["i2"], rows["i1"]))]   # (stable)
        return rows, self.n


def make_case(name, floors, confidence_threshold=0.5, rot_threshold_deg=0.5, trans_threshold=0.01, cycle_filter=1, max_nodes=None,
              reference=False, refused=False):
    rows = np.concatenate([r for r, _ in floors]) if floors else np.zeros(0, dtype=ROW)
    n_nodes = np.array([n for _, n in floors], dtype=np.int32)
    floor_start = np.concatenate([[0], np.cumsum([len(r) for r, _ in floors])]).astype(np.int32)
    if max_nodes is None:
        max_nodes = max(1, int(n_nodes.max())) if len(floors) else 1
    return {"name": name, "rows": rows, "floor_start": floor_start, "n_nodes": n_nodes, "max_nodes": int(max_nodes),
            "confidence_threshold": F32(confidence_threshold), "rot_threshold_deg": F32(rot_threshold_deg), "trans_threshold": F32(trans_threshold),
            "cycle_filter": int(cycle_filter), "reference": reference, "refused": refused}


def _triangle(rng, scales=False, **corrupt):
    """Nodes 0, 1, 2 with their three edges; corrupt: keyword arguments of the edge (0, 2)."""
    fb = FloorBuilder(3, global_poses(rng, 3, scales), rng)
    return fb.edge(0, 1).edge(1, 2).edge(0, 2, **corrupt)


def _banded(rng, n, band, n_chords, n_corrupt, scales=False):
    """Edges (i, i + k) for k <= band, the closing edges (0, n - 2) and (0, n - 1), random chords; a few edges corrupted.  Node n - 1 lies in
    the cycles (n - 3, n - 2, n - 1) and (0, n - 2, n - 1): the last bit of the last bitmask word is in use."""
    fb = FloorBuilder(n, global_poses(rng, n, scales), rng)
    pairs = {(i, i + k) for k in range(1, band + 1) for i in range(n - k)} | ({(0, n - 2), (0, n - 1)} if n >= 4 else set())
    while len(pairs) < (band * n + n_chords) and len(pairs) < n * (n - 1) // 2:
        a, b = sorted(rng.choice(n, size=2, replace=False).tolist())
        pairs.add((a, b))
    pairs = sorted(pairs)
    corrupt = set(rng.choice(len(pairs), size=n_corrupt, replace=False).tolist()) if n_corrupt else set()
    for k, (a, b) in enumerate(pairs):
        if k in corrupt:
            fb.edge(a, b, rot_deg=float(rng.choice([-7.0, 3.0, 40.0])) if k % 2 else 0.0, shift=(0.0, 0.0) if k % 2 else (0.4, -0.3))
        else:
            fb.edge(a, b)
    return fb


def make_cases():
    cases = []
    add = lambda *a, **k: cases.append(make_case(*a, **k))
    rng = np.random.default_rng(1900)

    add("zero-rows", [FloorBuilder(3).build()], reference=True)
    add("one-row", [FloorBuilder(2, global_poses(rng, 2), rng).edge(0, 1).build()], cycle_filter=0, reference=True)
    add("one-row-filtered", [FloorBuilder(2, global_poses(rng, 2), rng).edge(0, 1).build()], reference=True)
    add("triangle", [_triangle(rng).build()], reference=True)
    add("triangle-scales", [_triangle(rng, scales=True).build()], reference=True)
    add("triangle-broken-in-rotation", [_triangle(rng, rot_deg=2.0).build()], reference=True)
    add("triangle-broken-in-translation", [_triangle(rng, shift=(0.2, 0.1)).build()], reference=True)
    add("triangle-broken-in-translation-rotation-only-filter", [_triangle(rng, shift=(0.2, 0.1)).build()], trans_threshold=np.inf, reference=True)
    add("triangle-broken-no-filter", [_triangle(rng, rot_deg=2.0, shift=(0.2, 0.1)).build()], cycle_filter=0, reference=True)
    # a translation whose square overflows float32: its error is +inf, which is not BELOW an infinite threshold
    add("triangle-translation-overflow-rotation-only-filter", [_triangle(rng, t=(3e20, 1e20)).build()], trans_threshold=np.inf, reference=True)

    # one pair with five rows of prob exactly 1.0: the FIRST is the consistent one, the others break the triangle
    fb = FloorBuilder(3, global_poses(rng, 3), rng).edge(0, 1, prob=1.0)
    for k in range(4):
        fb.edge(0, 1, prob=1.0, rot_deg=10.0 * (k + 1))
    add("five-tied-rows", [fb.edge(1, 2, prob=1.0).edge(0, 2, prob=1.0).build()])
    # the largest prob comes LAST among a pair's rows, and behind it a lower one
    fb = FloorBuilder(3, global_poses(rng, 3), rng).edge(0, 1, prob=0.7, rot_deg=20.0).edge(0, 1, prob=0.8, rot_deg=-20.0).edge(0, 1, prob=0.95)
    add("largest-prob-last", [fb.edge(0, 1, prob=0.9, shift=(1, 1)).edge(1, 2).edge(0, 2).build()], reference=True)
    # rows of class 0 above the threshold (and above every candidate), with broken poses
    fb = FloorBuilder(3, global_poses(rng, 3), rng).edge(0, 1, prob=0.99, y_hat=0, rot_deg=30.0).edge(0, 1, prob=0.8)
    add("class-0-above-threshold", [fb.edge(1, 2, prob=0.999, y_hat=0, shift=(1, 0)).edge(1, 2, prob=0.7).edge(0, 2).edge(0, 2, prob=1.0, y_hat=2).build()],
        reference=True)
    # prob exactly at the threshold is a candidate; one ulp below is not
    thr = F32(0.9)
    fb = FloorBuilder(4, global_poses(rng, 4), rng).edge(0, 1, prob=thr).edge(1, 2, prob=0.95).edge(0, 2, prob=0.97)
    add("prob-at-threshold", [fb.edge(0, 3, prob=np.nextafter(thr, F32(0))).edge(1, 3, prob=0.99).build()], confidence_threshold=thr, reference=True)
    # NaN prob: never a candidate, in front of a valid row, and alone on a pair
    fb = FloorBuilder(4, global_poses(rng, 4), rng).edge(0, 1, prob=np.nan, rot_deg=50.0).edge(0, 1, prob=0.8).edge(1, 2).edge(0, 2)
    add("nan-prob", [fb.edge(0, 3, prob=np.nan).edge(1, 3).build()], reference=True)
    # non-finite translations: their cycles have NaN errors and are never consistent; the filter keeps them out of the tree
    fb = FloorBuilder(5, global_poses(rng, 5), rng).edge(0, 1).edge(1, 2).edge(0, 2).edge(0, 3, t=(np.inf, 0.0)).edge(1, 3)
    add("non-finite-translation", [fb.edge(0, 4).edge(1, 4, t=(np.nan, 1.0)).build()], reference=True)

    for n in (31, 32, 33, 63, 64, 65):   # the bitmask word edges
        add(f"{n}-nodes", [_banded(np.random.default_rng(n), n, 2, n, 3).build()])
        add(f"{n}-nodes-no-filter", [_banded(np.random.default_rng(1000 + n), n, 2, n // 2, 2).build()], cycle_filter=0)
    add("256-nodes-sparse", [_banded(np.random.default_rng(256), 256, 5, 300, 12).build()])
    add("257-nodes", [_banded(np.random.default_rng(257), 257, 1, 0, 0).build()], max_nodes=257, refused=True)
    # K_48 from random global poses with scales, a handful of corrupted edges
    rk = np.random.default_rng(48)
    fb = FloorBuilder(48, global_poses(rk, 48, scales=True), rk)
    bad = {(0, 5), (0, 17), (3, 40), (12, 13), (30, 47), (46, 47)}
    for a in range(48):
        for b in range(a + 1, 48):
            fb.edge(a, b, rot_deg=4.0 if (a, b) in bad and a % 2 == 0 else 0.0, shift=(0.3, 0.3) if (a, b) in bad and a % 2 else (0.0, 0.0))
    add("k48-dense", [fb.build()])
    # a path of 256 nodes: 255 BFS levels, no cycle
    rp = np.random.default_rng(255)
    fb = FloorBuilder(256, global_poses(rp, 256, scales=True), rp)
    for a in range(255):
        fb.edge(a, a + 1)
    add("path-256", [fb.build()], cycle_filter=0, reference=True)
    # two components of equal size: the one with node 0 wins; of different sizes: the larger one, which does not hold node 0
    fb = FloorBuilder(6, global_poses(rng, 6), rng).edge(0, 2).edge(2, 4).edge(0, 4).edge(1, 3).edge(3, 5).edge(1, 5)
    add("two-equal-components", [fb.build()])
    fb = FloorBuilder(6, global_poses(rng, 6), rng).edge(0, 1).edge(2, 3).edge(3, 4).edge(2, 4).edge(4, 5)
    add("larger-component-without-node-0", [fb.build()], cycle_filter=0, reference=True)
    # one component that the cycle filter splits at a bridge: {0, 1, 2} and {3, 4, 5, 6}
    fb = FloorBuilder(7, global_poses(rng, 7, scales=True), rng).edge(0, 1).edge(1, 2).edge(0, 2).edge(2, 3).edge(3, 4).edge(3, 5).edge(4, 5)
    add("filter-splits-the-component", [fb.edge(3, 6).edge(5, 6).build()], reference=True)
    add("filter-splits-the-component-no-filter", [fb.build()], cycle_filter=0)
    # several shortest paths: the square 0-1-3-2 with inconsistent poses, so that the parent shows in the pose
    fb = FloorBuilder(5, global_poses(rng, 5), rng).edge(0, 1).edge(0, 2).edge(1, 3, rot_deg=5.0).edge(2, 3, shift=(1, 0)).edge(3, 4)
    add("square-two-shortest-paths", [fb.build()], cycle_filter=0)

    # 300 floors in one launch, empty ones in between
    rf = np.random.default_rng(300)
    floors = []
    for f in range(300):
        kind = f % 5
        if kind == 1:
            floors.append(FloorBuilder(int(rf.integers(0, 4))).build())   # no rows; 0 .. 3 nodes
        else:
            n = int(rf.integers(2, 13))
            floors.append(_banded(rf, n, min(2, n - 1), n, 1 if n > 4 else 0, scales=kind == 3).build())
    add("300-floors", floors, max_nodes=12)
    add("300-floors-no-filter", floors, max_nodes=16, cycle_filter=0)

    # malformed floors between sound ones: each is written empty and raises the status bit
    good = lambda: _banded(rf, 6, 2, 3, 0).build()
    unsorted = _banded(rf, 6, 2, 3, 0).build()
    unsorted = (unsorted[0][::-1].copy(), 6)
    swapped = _banded(rf, 6, 2, 3, 0).build()
    swapped[0]["i1"][2], swapped[0]["i2"][2] = swapped[0]["i2"][2], swapped[0]["i1"][2]
    beyond = _banded(rf, 6, 2, 3, 0).build()
    beyond = (beyond[0], 5)                                   # i2 == n_nodes
    equal = _banded(rf, 6, 2, 3, 0).build()
    equal[0]["i2"][0] = equal[0]["i1"][0]
    negative = _banded(rf, 6, 2, 3, 0).build()
    negative[0]["i1"][0] = -1
    huge = _banded(rf, 6, 2, 3, 0).build()
    huge[0]["i2"][-1] = 2 ** 31 - 1
    too_many = (good()[0], 9)                                  # n_nodes above max_nodes
    negative_nodes = (np.zeros(0, dtype=ROW), -3)
    add("malformed-floors", [good(), unsorted, good(), swapped, beyond, equal, good(), negative, huge, too_many, negative_nodes, good()], max_nodes=8)
    return cases


_CASES = None


def cases():
    """The case list, built once and shared (nothing may write to its arrays)."""
    global _CASES
    if _CASES is None:
        _CASES = make_cases()
        for c in _CASES:
            for k in ("rows", "floor_start", "n_nodes"):
                c[k].setflags(write=False)
    return _CASES


def case(name):
    return next(c for c in cases() if c["name"] == name)


_EXPECTED = {}


def expected(c):
    """((out_rows, out_nodes, out_floors) with guards, status bit, per-floor details) of the emulator for a case, computed once."""
    if c["name"] not in _EXPECTED:
        details = []
        bufs, raised = run_case(c, lambda cs, ro, no, fo: emulate(cs, ro, no, fo, None, details))
        for b in bufs:
            b.setflags(write=False)
        _EXPECTED[c["name"]] = (bufs, raised, details)
    return _EXPECTED[c["name"]]


def check_conditions():
    """The two conditions of the module's docstring, for every case that is launched."""
    for c in cases():
        if c["refused"]:
            continue
        _, _, details = expected(c)
        for det in details:
            for err, thr in ((det["rot"], c["rot_threshold_deg"]), (det["trans"], c["trans_threshold"])):
                if np.isfinite(thr) and len(err):
                    close = np.abs(err.astype(F64) - F64(thr)) <= MARGIN * F64(thr)
                    assert not close.any(), (c["name"], err[close], thr)
            if c["reference"]:
                assert not det["tie"], c["name"]
                assert det.get("tied_components", 1) == 1, c["name"]
                assert all(k == 1 for k in det["paths"].values()), c["name"]
