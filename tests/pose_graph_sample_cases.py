"""salve_pose_graph_sample_trees (include/salve_hip.h): a numpy emulator of its two launches, the case list the host and the GPU tests share,
and emulated WRONG kernels that the case list must catch.

The emulator shares no code with salve_amd/pose_graph.py.  From tests/pose_graph_cases.py it takes the elementwise Sim(2) helpers, the case
builders and -- for phases C and D, which the two entries share -- `emulate_floor`, handed exactly the rows a hypothesis chose.  Phase E is
elementwise numpy in the entry's stated order: the errors of a floor's rows are laid out 256 to a line, the lines are added top to bottom
(thread t's rows lo + t, lo + t + 256, ... ascending from 0.0; a row that is not measured adds 0.0, which changes no sum of non-negative
terms), and the 256 partial sums are folded by halving.  Everything is bit-comparable with the kernel but avg_rot_err, which carries two
arctan2 per measured row.

A case is a dict: name, rows, floor_start, n_nodes, max_nodes, confidence_threshold, hyp_start, masks (uint32 [n_hyps, mask_words]), `refused`
(the library refuses it: no launch) and `reference` (the host test also compares it with a restatement of the reference's own loop).

Conditions on the case list, asserted by `check_conditions`:
  - no objective of any scan step lies within OBJ_MARGIN = 1e-3 of 0: the rotation term can move by at most 2 x ROT_ERR_ATOL / 5 = 7.8e-5
    between the device's atan2f and numpy's, more than ten times below the margin, so no decision of the scan can flip;
  - in every `reference` case no hypothesis has a tie under the three tie rules: one largest component, unique shortest paths (the graphs are
    odd cycles joined at single nodes, which keeps shortest paths unique in every subgraph), and -- by the last-masked rule -- no choice by prob.
The builders draw more hypotheses than a case keeps and drop those that would break a condition (`_prune`); what is kept is asserted."""

from __future__ import annotations

import numpy as np

from tests import pose_graph_cases as pc

F32, F64 = np.float32, np.float64
ROW, NODE_OUT = pc.ROW, pc.NODE_OUT
TREE_OUT = np.dtype([("avg_rot_err", "<f8"), ("avg_trans_err", "<f8"), ("n_localized", "<i4"), ("n_measured", "<i4"), ("n_edges", "<i4"),
                     ("origin", "<i4"), ("floor", "<i4"), ("reserved", "<i4")])
FLOOR_OUT = np.dtype([("best", "<i4"), ("n_candidates", "<i4"), ("n_hyps", "<i4"), ("n_improvements", "<i4"), ("avg_rot_err", "<f8"),
                      ("avg_trans_err", "<f8")])
SENTINEL, GUARD, THREADS = pc.SENTINEL, pc.GUARD, 256
STATUS_BAD_GRAPH_ROW = pc.STATUS_BAD_GRAPH_ROW
RAD2DEG_QUOT = F32(180.0) / F32(np.pi)       # 57.295776: numpy's float32 rad2deg multiplies by this
QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(F64)[0]
OBJ_MARGIN = 1e-3
# avg_rot_err against numpy: two angles of at most 180 degrees, each within tests/test_gpu_pose_graph.py's MIN_ROT_ERR_RTOL = 4 x 1.362e-7
ROT_ERR_ATOL = 2 * 180 * 4 * 1.362e-7        # 1.96e-4 degrees

WRONG_KERNELS = ("largest_prob", "first_masked", "score_masked_only", "no_wrap", "no_completeness", "f32_sums", "sequential_sum", "mask_word_off",
                 "non_candidate_bits", "nan_replaces", "inverse_order", "measured_needs_one_end")


def canonical(x):
    return QNAN if x != x else F64(x)


def mask_bit(mask, k, wrong=None):
    w = k >> 5
    if wrong == "mask_word_off":
        w = (w + 1) % max(len(mask), 1)
    return w < len(mask) and bool((int(mask[w]) >> (k & 31)) & 1)


def is_candidate(rows, conf):
    with np.errstate(invalid="ignore"):
        return (rows["y_hat"] == 1) & (rows["prob"] >= F32(conf))


def fold(partials, wrong=None):
    p = partials.copy()
    if wrong == "sequential_sum":
        total = p.dtype.type(0)
        for x in p:
            total = total + x
        return total
    s = THREADS // 2
    while s:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return p[0]


def stated_sum(err, wrong=None):
    """err: float64 [n_rows], 0.0 where the row is not measured.  The entry's order of additions."""
    dt = F32 if wrong == "f32_sums" else F64
    lines = -(-len(err) // THREADS)
    mat = np.zeros(lines * THREADS, dtype=dt)
    mat[:len(err)] = err.astype(dt)
    acc = np.zeros(THREADS, dtype=dt)
    for line in mat.reshape(lines, THREADS):
        acc = acc + line
    return F64(fold(acc, wrong))


def emulate_hypothesis(rows, n, conf, mask, wrong=None):
    """(tree record fields, node_out [n], details) of one hypothesis on one well-formed floor."""
    cand = is_candidate(rows, conf)
    usable = np.ones(len(rows), dtype=bool) if wrong == "non_candidate_bits" else cand
    masked = np.array([mask_bit(mask, k, wrong) for k in range(len(rows))], dtype=bool) & usable
    chosen = {}
    for r in np.nonzero(masked)[0]:
        key = (int(rows["i1"][r]), int(rows["i2"][r]))
        if key not in chosen or wrong is None or wrong not in ("largest_prob", "first_masked"):
            chosen[key] = int(r)                       # the LAST masked candidate of the pair
        elif wrong == "largest_prob" and rows["prob"][r] > rows["prob"][chosen[key]]:
            chosen[key] = int(r)
    sub = rows[sorted(chosen.values())].copy()
    sub["y_hat"], sub["prob"] = 1, F32(1.0)            # (a candidate whatever `wrong` let through)
    _, node_out, floor_out, det = pc.emulate_floor(sub, n, 0.5, 0, 0, 0)
    loc = node_out["localized"] == 1
    a, b = rows["i1"], rows["i2"]
    if wrong == "measured_needs_one_end":
        measured = cand & (loc[a] | loc[b])
    else:
        measured = cand & loc[a] & loc[b]
    if wrong == "score_masked_only":
        measured &= masked
    rot = np.zeros(len(rows), dtype=F64)
    trans = np.zeros(len(rows), dtype=F64)
    if measured.any():
        m = np.nonzero(measured)[0]
        pose = lambda v: (node_out["R"][v, 0], node_out["R"][v, 1], node_out["R"][v, 2], node_out["R"][v, 3], node_out["t"][v, 0], node_out["t"][v, 1],
                          node_out["s"][v])
        with np.errstate(all="ignore"):
            W1, W2 = pose(a[m]), pose(b[m])
            Z = pc.sim2_compose(pc.sim2_inverse(W1), W2) if wrong == "inverse_order" else pc.sim2_compose(pc.sim2_inverse(W2), W1)
            th_sim = (np.arctan2(Z[2], Z[0]).astype(F32) * RAD2DEG_QUOT).astype(F64)
            th_m = (np.arctan2(rows["R"][m, 2], rows["R"][m, 0]).astype(F32) * RAD2DEG_QUOT).astype(F64)
            if wrong == "no_wrap":
                rot[m] = np.abs(th_m - th_sim)
            else:
                d = np.fmod(th_m - th_sim + 180.0, 360.0)
                d = np.where(d < 0, d + 360.0, d)
                rot[m] = np.abs(d - 180.0)
            dx, dy = Z[4] - rows["t"][m, 0], Z[5] - rows["t"][m, 1]
            trans[m] = np.sqrt(dx * dx + dy * dy).astype(F32).astype(F64)
    n_measured = int(measured.sum())
    with np.errstate(all="ignore"):
        avg_rot = canonical(stated_sum(rot, wrong) / F64(n_measured))
        avg_trans = canonical(stated_sum(trans, wrong) / F64(n_measured))
    rec = {"avg_rot_err": avg_rot, "avg_trans_err": avg_trans, "n_localized": int(floor_out["n_localized"][0]), "n_measured": n_measured,
           "n_edges": len(chosen), "origin": int(floor_out["origin"][0])}
    det = {"tied_components": det.get("tied_components", 1), "paths": det["paths"], "masked": masked, "chosen": chosen}
    return rec, node_out, det


def scan(recs, wrong=None):
    """(best, n_improvements, best_rot, best_trans, the objectives) of the reference's scan over a floor's hypothesis records, in float64."""
    best_rot = best_trans = float("inf")
    best_n, best, n_imp, objs = 0, -1, 0, []
    for k, r in enumerate(recs):
        rot, trans, nl = float(r["avg_rot_err"]), float(r["avg_trans_err"]), int(r["n_localized"])
        rot_win = (best_rot - rot) / 5
        trans_win = (best_trans - trans) / 1
        loc_win = -(best_n - nl) / (best_n + 1e-10)
        obj = rot_win + trans_win + (0.0 if wrong == "no_completeness" else 1.33 * loc_win)
        objs.append(obj)
        if (not obj <= 0) if wrong == "nan_replaces" else (obj > 0):
            best_rot, best_trans, best_n, best, n_imp = rot, trans, nl, k, n_imp + 1
    return best, n_imp, best_rot, best_trans, objs


def _extent(table, f, limit):
    lo, hi = int(table[f]), int(table[f + 1])
    return (lo, hi) if 0 <= lo <= hi <= limit else None


def emulate(case, out_trees, out_inlier, out_nodes, out_floors, wrong=None, details=None):
    """Write what the entry writes into the four arrays (views WITHOUT their guards); returns whether the status bit is raised."""
    M, conf, F, H = case["max_nodes"], case["confidence_threshold"], len(case["n_nodes"]), len(case["masks"])
    raised = False
    row_ext = [_extent(case["floor_start"], f, len(case["rows"])) for f in range(F)]
    hyp_ext = [_extent(case["hyp_start"], f, H) for f in range(F)]
    owner = [next((f for f in range(F) if hyp_ext[f] and hyp_ext[f][0] <= h < hyp_ext[f][1]), -1) for h in range(H)]
    tables_ok = []
    for f in range(F):
        n = int(case["n_nodes"][f])
        tables_ok.append(row_ext[f] is not None and pc.floor_is_well_formed(case["rows"][row_ext[f][0]:row_ext[f][1]], n, M))
    empty_tree = lambda f: (QNAN, QNAN, 0, 0, 0, -1, f, 0)
    recs, nodes_of, dets = {}, {}, {}
    for h in range(H):
        f = owner[h]
        if f < 0 or not tables_ok[f]:
            out_trees[h] = empty_tree(f)
            continue
        lo, hi = row_ext[f]
        rec, node_out, det = emulate_hypothesis(case["rows"][lo:hi], int(case["n_nodes"][f]), conf, case["masks"][h], wrong)
        out_trees[h] = (rec["avg_rot_err"], rec["avg_trans_err"], rec["n_localized"], rec["n_measured"], rec["n_edges"], rec["origin"], f, 0)
        recs[h], nodes_of[h], dets[h] = rec, node_out, det
    for f in range(F):
        n = int(case["n_nodes"][f])
        lo, hi = row_ext[f] if row_ext[f] else (0, 0)
        n = n if 0 <= n <= M else 0
        hs, he = hyp_ext[f] if hyp_ext[f] else (0, 0)
        ok = tables_ok[f] and hyp_ext[f] is not None and all(owner[h] == f for h in range(hs, he))
        empty_nodes = np.zeros(n, dtype=NODE_OUT)
        empty_nodes["parent"], empty_nodes["depth"] = -1, -1
        det = {"objs": [], "hyps": [], "best": -1}
        if not ok:
            raised = True
            out_inlier[lo:hi] = 0
            out_nodes[f * M:f * M + n] = empty_nodes
            out_floors[f] = (-1, 0, 0, 0, QNAN, QNAN)
        else:
            rows = case["rows"][lo:hi]
            best, n_imp, best_rot, best_trans, objs = scan([recs[h] for h in range(hs, he)], wrong)
            out_floors[f] = (best, int(is_candidate(rows, conf).sum()), he - hs, n_imp, F64(best_rot) if best >= 0 else QNAN,
                             F64(best_trans) if best >= 0 else QNAN)
            out_nodes[f * M:f * M + n] = nodes_of[hs + best] if best >= 0 else empty_nodes
            out_inlier[lo:hi] = dets[hs + best]["masked"] if best >= 0 else 0
            det = {"objs": objs, "hyps": [dets[h] for h in range(hs, he)], "best": best, "recs": [recs[h] for h in range(hs, he)]}
        if details is not None:
            details.append(det)
    return raised


def fresh_buffers(case):
    n_rows, F, M, H = len(case["rows"]), len(case["n_nodes"]), case["max_nodes"], len(case["masks"])
    mk = lambda count, dt: np.frombuffer(bytes([SENTINEL]) * ((count + 2 * GUARD) * np.dtype(dt).itemsize), dtype=dt).copy()
    return mk(H, TREE_OUT), mk(n_rows, np.int32), mk(F * M, NODE_OUT), mk(F, FLOOR_OUT)


def run_case(case, fn):
    """((out_trees, out_inlier, out_nodes, out_floors) WITH their guards as `fn(case, *views)` left them, the status bit)."""
    bufs = fresh_buffers(case)
    raised = fn(case, *[b[GUARD:len(b) - GUARD] for b in bufs])
    return bufs, bool(raised)


def emulated(wrong=None):
    return lambda case, *views: emulate(case, *views, wrong)


def differences(got, want, rot_atol=ROT_ERR_ATOL):
    """What the GPU test compares, as a list of the fields that differ: everything bit for bit (guards and sentinels included) but avg_rot_err,
    which must be NaN where expected and within rot_atol elsewhere."""
    out = []
    (gt, gi, gn, gf), (wt, wi, wn, wf) = got, want
    if gi.tobytes() != wi.tobytes():
        out.append("inlier")
    if gn.tobytes() != wn.tobytes():
        out.append("nodes")
    for name, g, w in (("trees", gt, wt), ("floors", gf, wf)):
        for k in g.dtype.names:
            if k == "avg_rot_err":
                gi_, wi_ = g[k][GUARD:-GUARD], w[k][GUARD:-GUARD]
                nan = np.isnan(wi_)
                if not np.array_equal(np.isnan(gi_), nan) or gi_[nan].tobytes() != wi_[nan].tobytes():
                    out.append(f"{name}.{k} (NaN)")
                elif (~nan).any() and float(np.abs(gi_[~nan] - wi_[~nan]).max()) > rot_atol:
                    out.append(f"{name}.{k}")
                if g[k][:GUARD].tobytes() != w[k][:GUARD].tobytes() or g[k][-GUARD:].tobytes() != w[k][-GUARD:].tobytes():
                    out.append(f"{name}.{k} (guard)")
            elif g[k].tobytes() != w[k].tobytes():
                out.append(f"{name}.{k}")
    return out


# ---- building cases

def masks_of(subsets, n_rows, words=None):
    """uint32 [len(subsets), words]: bit k of word k // 32 is set iff k is in the subset (bits at or beyond n_rows are allowed)."""
    words = max(1, -(-n_rows // 32)) if words is None else words
    bits = np.zeros((len(subsets), words * 32), dtype=bool)
    for h, rows in enumerate(subsets):
        bits[h, np.asarray(rows, dtype=np.int64)] = True
    return np.packbits(bits.reshape(len(subsets), words, 32), axis=-1, bitorder="little").view("<u4").reshape(len(subsets), words)


def random_subsets(rng, n_rows, count, fraction=0.5):
    size = max(1, int(np.ceil(fraction * n_rows)))
    return [np.sort(rng.choice(n_rows, size=size, replace=False)) for _ in range(count)]


def make_case(name, floors, subsets, confidence_threshold=0.5, max_nodes=None, mask_words=None, reference=False, refused=False, hyp_start=None,
              floor_start=None):
    """floors: (rows, n) per floor; subsets: per floor a list of hypotheses, each the bit numbers (rows of the floor in sorted order) it sets."""
    base = pc.make_case(name, floors, confidence_threshold=confidence_threshold, max_nodes=max_nodes)
    words = max([1] + [-(-len(r) // 32) for r, _ in floors]) if mask_words is None else mask_words
    masks = [masks_of(s, len(r), words) for s, (r, _) in zip(subsets, floors)]
    case = {"name": name, "rows": base["rows"], "floor_start": base["floor_start"] if floor_start is None else np.asarray(floor_start, dtype=np.int32),
            "n_nodes": base["n_nodes"], "max_nodes": base["max_nodes"], "confidence_threshold": base["confidence_threshold"],
            "hyp_start": (np.concatenate([[0], np.cumsum([len(s) for s in subsets])]) if hyp_start is None else np.asarray(hyp_start)).astype(np.int32),
            "masks": np.concatenate(masks) if masks else np.zeros((0, words), dtype=np.uint32), "mask_words": words, "reference": reference,
            "refused": refused}
    return case


def _prune(floors, subsets, conf=0.5, reference=False, keep=None, mask_words=None, margin=10 * OBJ_MARGIN):
    """Drop the hypotheses whose scan step would lie within `margin` of 0 (and, for a reference case, those with a tie); keep at most `keep`."""
    out = []
    for (rows, n), subs in zip(floors, subsets):
        words = max(1, -(-len(rows) // 32)) if mask_words is None else mask_words
        kept, recs = [], []
        for s in subs:
            if keep is not None and len(kept) == keep:
                break
            rec, _, det = emulate_hypothesis(rows, n, conf, masks_of([s], len(rows), words)[0])
            if reference and (det["tied_components"] != 1 or any(k != 1 for k in det["paths"].values())):
                continue
            objs = scan(recs + [rec])[4]
            if abs(objs[-1]) < margin:   # (a NaN objective is not near 0: it never wins on any device)
                continue
            kept.append(s)
            recs.append(rec)
        out.append(kept)
    return out


def _noisy(fb, rng, pairs, rot=0.4, shift=0.03, rows_per_pair=1):
    for a, b in pairs:
        for _ in range(rows_per_pair):
            fb.edge(a, b, rot_deg=float(rng.normal(0, rot)), shift=tuple(rng.normal(0, shift, size=2)))
    return fb


def _cactus(rng, n_triangles, scales=False, rows_per_pair=1, tail=0):
    """Triangles (2 k, 2 k + 1, 2 k + 2) joined at their even nodes, then `tail` pentagons: odd cycles joined at single nodes."""
    n = 2 * n_triangles + 1 + 4 * tail
    fb = pc.FloorBuilder(n, pc.global_poses(rng, n, scales), rng)
    pairs = []
    for k in range(n_triangles):
        pairs += [(2 * k, 2 * k + 1), (2 * k + 1, 2 * k + 2), (2 * k, 2 * k + 2)]
    v = 2 * n_triangles
    for _ in range(tail):
        pairs += [(v, v + 1), (v + 1, v + 2), (v + 2, v + 3), (v + 3, v + 4), (v, v + 4)]
        v += 4
    return _noisy(fb, rng, pairs, rows_per_pair=rows_per_pair)


def _k_rows(rng, K, n=12, wide=False):
    """A floor of exactly K candidate rows on n nodes: a ring with chords, many rows per pair, every row noisy.  wide: the translation noise
    spans eleven decades, so a float64 sum of the (float32) translation errors rounds and its ORDER shows in the last bits."""
    fb = pc.FloorBuilder(n, pc.global_poses(rng, n, True), rng)
    pairs = [(i, i + 1) for i in range(n - 1)] + [(0, n - 1)] + [(i, i + 3) for i in range(n - 3)]
    for k in range(K):
        a, b = pairs[k % len(pairs)]
        scale = 10.0 ** rng.uniform(-6, 5) if wide else 0.05
        fb.edge(a, b, rot_deg=float(rng.normal(0, 0.6)), shift=tuple(rng.normal(0, scale, size=2)))
    return fb.build()


def make_cases():
    cases = []
    rng = np.random.default_rng(2900)

    def add(name, floors, subsets, prune=True, keep=None, **kw):
        if prune:
            subsets = _prune(floors, subsets, kw.get("confidence_threshold", 0.5), kw.get("reference", False), keep, kw.get("mask_words"))
        cases.append(make_case(name, floors, subsets, **kw))

    # K = 1: one row, one hypothesis
    one = pc.FloorBuilder(2, pc.global_poses(rng, 2), rng).edge(0, 1).build()
    add("k-1", [one], [[[0]]], reference=True)
    add("one-hypothesis", [_cactus(rng, 3).build()], [[list(range(9))]], reference=True)

    # a triangle plus one outlier edge to a fourth node and an outlier row on a triangle pair: hypotheses with and without them rank differently
    fb = pc.FloorBuilder(4, pc.global_poses(rng, 4), rng).edge(0, 1).edge(1, 2).edge(0, 2).edge(0, 2, rot_deg=25.0, shift=(0.8, -0.5))
    tri = fb.edge(2, 3, rot_deg=0.2).build()
    add("triangle-plus-outlier", [tri], [[[0, 1, 3, 4], [0, 1, 2, 3, 4], [0, 3, 4], [0, 2, 4]]], reference=True)

    # a pair with three candidate rows: the last masked one is neither the first nor the most probable
    fb = pc.FloorBuilder(3, pc.global_poses(rng, 3), rng).edge(0, 1, prob=0.9, rot_deg=8.0).edge(0, 1, prob=0.99, rot_deg=-6.0)
    three = fb.edge(0, 1, prob=0.7, rot_deg=0.3).edge(0, 1, prob=0.95, shift=(0.5, 0.5)).edge(1, 2, prob=0.8).edge(0, 2, prob=0.8, rot_deg=0.1).build()
    add("last-masked-of-three", [three], [[[0, 1, 2, 4, 5], [0, 1, 4, 5], [1, 2, 3, 4, 5], [0, 2, 4]]], reference=True)

    # hypotheses whose graph splits into 2 + 3 nodes against one that spans all five with a worse fit: the completeness term decides
    fb = pc.FloorBuilder(5, pc.global_poses(rng, 5), rng).edge(0, 1).edge(1, 2, rot_deg=6.0, shift=(0.3, 0.2)).edge(2, 3).edge(3, 4).edge(2, 4)
    add("split-2-plus-3", [fb.build()], [[[0, 2, 3, 4], [0, 1, 2, 4], [2, 3, 4]]], reference=True)

    # mask bits on rows that are not candidates (class 0, below the threshold, NaN prob) and beyond the floor's row count
    fb = pc.FloorBuilder(4, pc.global_poses(rng, 4), rng).edge(0, 1).edge(0, 1, prob=0.99, y_hat=0, rot_deg=30.0).edge(1, 2)
    fb = fb.edge(1, 2, prob=0.3, shift=(1.0, 0.0)).edge(0, 2, rot_deg=0.2).edge(2, 3).edge(2, 3, prob=np.nan, rot_deg=50.0)
    stray = fb.build()
    add("bits-on-non-candidates-and-beyond", [stray], [[[0, 1, 2, 3, 5, 6, 9, 20, 63], [0, 1, 3, 4, 5, 6, 7, 31, 40], [1, 2, 3, 4, 6, 8, 33]]], mask_words=2,
        reference=True)

    # K = 255 / 256 / 257 / 513: the thread stride, a partial last mask word, more than one word
    for K in (255, 256, 257, 513):
        fl = _k_rows(np.random.default_rng(K), K)
        add(f"k-{K}", [fl], [random_subsets(np.random.default_rng(7000 + K), K, 8)], keep=5)

    # float32 errors of one magnitude add up exactly in float64; errors across eleven decades do not: the stated ORDER of the sums is visible
    add("k-600-wide-range", [_k_rows(np.random.default_rng(600), 600, wide=True)], [random_subsets(np.random.default_rng(7600), 600, 8)], keep=4)

    # 33 and 65 nodes (a second and a third bitmask word); a path of 256 nodes
    for n_tri in (16, 32):
        rn = np.random.default_rng(n_tri)
        fl = _cactus(rn, n_tri, scales=True).build()
        add(f"{2 * n_tri + 1}-nodes", [fl], [random_subsets(rn, len(fl[0]), 10, 0.8)], keep=6, reference=True)
    rp = np.random.default_rng(255)
    fb = pc.FloorBuilder(256, pc.global_poses(rp, 256, scales=True), rp)
    path = _noisy(fb, rp, [(a, a + 1) for a in range(255)], rot=0.2, shift=0.01).build()
    add("path-256", [path], [[list(range(255)), list(range(100, 255)), list(range(0, 180))]], reference=True)

    # simulated and measured angles at +179.9 and -179.9 degrees: the error is 0.2, not 359.8
    poses = [(pc._rot(0.0), np.zeros(2), 1.0), (pc._rot(-179.9), np.array([1.0, 0.5]), 1.0), (pc._rot(10.0), np.array([-1.0, 2.0]), 1.0)]
    fb = pc.FloorBuilder(3, poses, rng).edge(0, 1).edge(0, 1, rot_deg=0.2).edge(1, 2).edge(0, 2, rot_deg=0.05)
    add("angles-at-the-wrap", [fb.build()], [[[0, 2, 3], [1, 2]]], reference=True)

    # a NaN translation in one measured row: a hypothesis that measures it is never chosen
    fb = pc.FloorBuilder(4, pc.global_poses(rng, 4), rng).edge(0, 1).edge(1, 2).edge(0, 2, rot_deg=0.3).edge(2, 3, rot_deg=0.2).edge(1, 3, t=(np.nan, 1.0))
    nan_floor = fb.build()
    add("nan-translation", [nan_floor], [[[0, 2, 4], [0, 1, 2], [0, 1, 3], [0, 2]]], reference=True)
    add("every-hypothesis-nan", [nan_floor], [[[0, 2, 4], [1, 3, 4], [0, 3]]])

    # 100 hypotheses on one floor
    rh = np.random.default_rng(100)
    fl = _cactus(rh, 6, scales=True, rows_per_pair=3, tail=1).build()
    add("100-hypotheses", [fl], [random_subsets(rh, len(fl[0]), 400, 0.5)], keep=100, reference=True)
    assert cases[-1]["hyp_start"][-1] == 100

    # floors with 0 hypotheses among others (one of them without a row)
    fa, fb_, fc = _cactus(rng, 2).build(), _cactus(rng, 3).build(), pc.FloorBuilder(3).build()
    add("floors-without-hypotheses", [fa, fb_, fc, _cactus(rng, 2).build()],
        [random_subsets(rng, 6, 4, 0.7), [], [], random_subsets(rng, 6, 4, 0.7)], max_nodes=9)

    # 300 floors of differing K and H in one call
    rf = np.random.default_rng(300)
    floors, subsets = [], []
    for f in range(300):
        if f % 7 == 3:
            floors.append(pc.FloorBuilder(int(rf.integers(0, 4))).build())
            subsets.append([])
        else:
            fl = _cactus(rf, int(rf.integers(1, 6)), scales=f % 3 == 0, rows_per_pair=1 + f % 2).build()
            floors.append(fl)
            subsets.append(random_subsets(rf, len(fl[0]), int(rf.integers(0, 7)), 0.6))
    add("300-floors", floors, subsets, max_nodes=12)

    # malformed tables between sound floors: each kind is written empty and raises the status bit, the others are solved
    def good():   # a sound floor of 6 rows with three hypotheses that keep the conditions
        fl = _cactus(rf, 2).build()
        subs = _prune([fl], [[np.sort(rf.choice(6, size=int(rf.integers(3, 6)), replace=False)) for _ in range(40)]], keep=3)[0]
        assert len(subs) == 3
        return fl, subs

    def build(name, mangled, **kw):
        made = [good() for _ in mangled]
        floors = [m(fl) if m else fl for m, (fl, _) in zip(mangled, made)]
        add(name, floors, [[] if len(fl[0]) == 0 else subs for fl, (_, subs) in zip(floors, made)], max_nodes=8, prune=False, **kw)

    def swapped(fl):
        fl[0]["i1"][2], fl[0]["i2"][2] = fl[0]["i2"][2], fl[0]["i1"][2]
        return fl

    def negative(fl):
        fl[0]["i1"][0] = -1
        return fl

    build("malformed-rows-and-nodes", [None, lambda fl: (fl[0][::-1].copy(), 5), None, swapped, lambda fl: (fl[0], 4), None, negative,
                                       lambda fl: (fl[0], 9), lambda fl: (np.zeros(0, dtype=ROW), -3), None])
    # 18 hypotheses; extents: 0-3 | 3 > 2 | 2-40 (beyond 18) | 40 > 12 | 12-15 | 15-18; hypotheses 3 .. 11 belong to no floor
    build("malformed-hyp-start", [None] * 6, hyp_start=[0, 3, 2, 40, 12, 15, 18])
    # floor 1's extent 3 > 1 is malformed; floor 2's 1-9 is well formed but holds floor 0's hypotheses 1 and 2
    build("overlapping-hyp-extents", [None] * 4, hyp_start=[0, 3, 1, 9, 12])
    build("malformed-floor-start", [None] * 4, floor_start=[0, 6, 30, 18, 24])
    build("negative-starts", [None] * 4, floor_start=[0, 6, -2, 18, 24], hyp_start=[0, 3, 6, -1, 12])

    add("257-nodes", [pc._banded(np.random.default_rng(257), 257, 1, 0, 0).build()], [[[0, 1, 2]]], max_nodes=257, refused=True, prune=False)
    return cases


LAUNCH_CHECKED = ("malformed-rows-and-nodes", "malformed-hyp-start", "overlapping-hyp-extents", "malformed-floor-start", "negative-starts")
_CASES = None


def cases():
    """The case list, built once and shared (nothing may write to its arrays)."""
    global _CASES
    if _CASES is None:
        _CASES = make_cases()
        for c in _CASES:
            for k in ("rows", "floor_start", "n_nodes", "hyp_start", "masks"):
                c[k].setflags(write=False)
    return _CASES


def case(name):
    return next(c for c in cases() if c["name"] == name)


_EXPECTED = {}


def expected(c):
    """((out_trees, out_inlier, out_nodes, out_floors) with guards, status bit, per-floor details) of the emulator for a case, computed once."""
    if c["name"] not in _EXPECTED:
        details = []
        bufs, raised = run_case(c, lambda cs, *views: emulate(cs, *views, None, details))
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
            for obj in det["objs"]:
                assert obj != obj or abs(obj) >= OBJ_MARGIN, (c["name"], obj)
            if c["reference"]:
                for h in det["hyps"]:
                    assert h["tied_components"] == 1 and all(k == 1 for k in h["paths"].values()), c["name"]
