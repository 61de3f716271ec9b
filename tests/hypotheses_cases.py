"""Cases and a numpy / plain-Python emulator for salve_hypotheses_generate (include/salve_hip.h) and salve_amd.hypotheses: the reference's
alignment-hypothesis export for inferred W/D/Os (scripts/export_alignment_hypotheses.py:93-273) restated from the rules of the header, sharing
no code with the library.  Python floats are IEEE float64 and nothing here is fused, so the emulator's fit, acceptance and pruning equal the
device's bit for bit; the label's atan2 is the C library's, so every label decision reports its MARGIN to its threshold and a case whose margin
is below 1e-9 is an error of the case file (`check_margins`), never a skip.

A floor is a plain dict: building_id, floor_id, pano_ids (ascending), wdos (per panorama a list of (type name, [[x1, y1], [x2, y2]]) in
PanoLayouts' order: doors, windows, openings), poses (per panorama (R [2, 2] float32, t [2] float32, s float)), gt_wdos (per panorama a list
of LOCAL segments).  A case is {name, reason, floors, min_width_ratio}.

VARIANTS names emulated WRONG kernels (and one wrong host order); tests/test_hypotheses_host.py shows that each of them fails the cases."""

import math

import numpy as np

F32 = np.float32
SENTINEL = 0xA5
GUARD = 3   # sentinel records behind each buffer
ROW = np.dtype([("R", "<f4", (4,)), ("t", "<f4", (2,)), ("type", "<i4"), ("i", "<i4"), ("j", "<i4"), ("configuration", "<i4"), ("label", "<i4"), ("reserved", "<i4")])
PAIR_OUT = np.dtype([("n_kept", "<i4"), ("n_valid", "<i4"), ("n_rejected", "<i4"), ("visibly_adjacent", "<i4"), ("R", "<f4", (4,)), ("t", "<f4", (2,)), ("s", "<f8")])
TYPE_CODE = {"windows": 0, "doors": 1, "openings": 2}
OBJECT = {0: "window", 1: "door", 2: "opening"}
CONFIGURATION = ("identity", "rotated")
LABEL_DIRS = ("gt_alignment_approx", "incorrect_alignment")
MIN_MARGIN = 1e-9
VARIANTS = ("two-point-polygons", "doors-without-rotated", "windows-with-rotated", "ratio-strictly-greater", "prune-against-all-candidates",
            "rtol-on-the-candidate", "types-in-table-order", "i-and-j-swapped", "gt-composed-the-other-way", "seven-degrees-for-openings",
            "number-sorted-order")


# ------------------------------------------------------------------------------------------------ the rules
def align(a, b, libm=False):
    """gtsam's Pose2::Align over the point pairs (a[k], b[k]) in float64 -> (R [4] float32, t [2] float32, R [4] float64, t [2] float64): aTb.
    The libm-free form of the rules: h = sqrt(c c + s s), cos = c / h, sin = s / h (identity when h == 0).  libm: the reference's form, cos and
    sin of atan2(s, c) -- the deviation tests/test_hypotheses_host.py measures."""
    n = float(len(a))

    def mean(pts):
        sx, sy = pts[0]
        for x, y in pts[1:]:
            sx, sy = sx + x, sy + y
        return sx / n, sy / n

    (cax, cay), (cbx, cby) = mean(a), mean(b)
    c = s = 0.0
    for (ax, ay), (bx, by) in zip(a, b):
        dax, day, dbx, dby = ax - cax, ay - cay, bx - cbx, by - cby
        c = c + (dbx * dax + dby * day)
        s = s + ((-dby) * dax + dbx * day)
    if libm:
        th = math.atan2(s, c)
        rc, rs = math.cos(th), math.sin(th)
    else:
        h = math.sqrt(c * c + s * s)
        rc, rs = (c / h, s / h) if h != 0.0 else (1.0, 0.0)
    tx = cax - (rc * cbx + (-rs) * cby)
    ty = cay - (rs * cbx + rc * cby)
    R64, t64 = [rc, -rs, rs, rc], [tx, ty]
    return np.array(R64, dtype=F32), np.array(t64, dtype=F32), R64, t64


def fit(a1, a2, b1, b2, two_point=False, libm=False):
    """The fit of one candidate: the five-point polygons [p1, p1, p2, p2, p1] of pano2's object (a) and pano1's (b).  p1 counts three times and
    p2 twice: the rotation is the two-point fit's, the translation is not when the widths differ (two_point: the wrong kernel that forgets it)."""
    order = (0, 1) if two_point else (0, 0, 1, 1, 0)
    return align([(a1, a2)[k] for k in order], [(b1, b2)[k] for k in order], libm=libm)


def width(p1, p2):
    dx, dy = p1[0] - p2[0], p1[1] - p2[1]
    return math.sqrt(dx * dx + dy * dy)


def width_ratio(w1, w2):
    lo, hi = (w2, w1) if w2 < w1 else (w1, w2)   # Python's min(w1, w2), max(w1, w2)
    if hi == 0.0:
        return float("nan")
    return lo / hi


def allclose_any(x, K, candidate_side=False):
    """Whether np.allclose(x, k) holds for some row k of K [n, 6]: |x - k| <= 1e-8 + 1e-5 |k| in all six entries, the KEPT one on the rtol side
    (candidate_side: the wrong side); float32 values in float64."""
    x = np.asarray(x, dtype=np.float64)
    return bool(np.any(np.all(np.abs(x - K) <= 1e-8 + 1e-5 * np.abs(x if candidate_side else K), axis=1)))


def sim2_inverse(S):
    R, t, s = S
    sf = F32(s)
    ux, uy = sf * t[0], sf * t[1]
    Rt = np.array([[R[0, 0], R[1, 0]], [R[0, 1], R[1, 1]]], dtype=F32)
    return Rt, np.array([(-Rt[0, 0]) * ux + (-Rt[0, 1]) * uy, (-Rt[1, 0]) * ux + (-Rt[1, 1]) * uy], dtype=F32), 1.0 / s


def sim2_compose(A, B):
    (RA, tA, sA), (RB, tB, sB) = A, B
    inv = F32(1.0 / sB)
    R = np.array([[RA[0, 0] * RB[0, 0] + RA[0, 1] * RB[1, 0], RA[0, 0] * RB[0, 1] + RA[0, 1] * RB[1, 1]],
                  [RA[1, 0] * RB[0, 0] + RA[1, 1] * RB[1, 0], RA[1, 0] * RB[0, 1] + RA[1, 1] * RB[1, 1]]], dtype=F32)
    t = np.array([(RA[0, 0] * tB[0] + RA[0, 1] * tB[1]) + inv * tA[0], (RA[1, 0] * tB[0] + RA[1, 1] * tB[1]) + inv * tA[1]], dtype=F32)
    return R, t, sA * sB


def as_pose(p):
    return np.asarray(p[0], dtype=F32).reshape(2, 2), np.asarray(p[1], dtype=F32).reshape(2), float(p[2])


def theta_deg(R10, R00):
    return float(np.rad2deg(np.arctan2(float(R10), float(R00))))


def obj_almost_equal(R, t, G, type_code, opening_tolerance=9.0):
    """-> (label, margin): the smallest distance of one of its comparisons to its threshold (metres, scale units or degrees)."""
    RG, tG, sG = G
    margins, ok = [], True
    for k in range(2):
        lhs, rhs = abs(float(t[k]) - float(tG[k])), 0.35 + 1e-5 * abs(float(tG[k]))
        margins.append(abs(lhs - rhs))
        ok = ok and lhs <= rhs
    lhs, rhs = abs(1.0 - sG), 0.35 + 1e-5 * abs(sG)
    margins.append(abs(lhs - rhs))
    ok = ok and lhs <= rhs
    th, th_g = theta_deg(R[2], R[0]), theta_deg(RG[1, 0], RG[0, 0])
    diff = (th_g - th + 180) % 360 - 180
    if diff < -180:
        diff = diff + 360
    tol = opening_tolerance if type_code == 2 else 7.0
    margins.append(abs(abs(diff) - tol))
    ok = ok and abs(diff) <= tol
    return int(ok), min(margins)


def point_segment_distance(p, a, b):
    dist = lambda u, v: math.sqrt((u[0] - v[0]) * (u[0] - v[0]) + (u[1] - v[1]) * (u[1] - v[1]))
    if a[0] == b[0] and a[1] == b[1]:
        return dist(p, a)
    len2 = (b[0] - a[0]) * (b[0] - a[0]) + (b[1] - a[1]) * (b[1] - a[1])
    r = ((p[0] - a[0]) * (b[0] - a[0]) + (p[1] - a[1]) * (b[1] - a[1])) / len2
    if r <= 0.0:
        return dist(p, a)
    if r >= 1.0:
        return dist(p, b)
    s = ((a[1] - p[1]) * (b[0] - a[0]) - (a[0] - p[0]) * (b[1] - a[1])) / len2
    return abs(s) * math.sqrt(len2)


def hausdorff(A, B):
    return max(max(point_segment_distance(A[0], B[0], B[1]), point_segment_distance(A[1], B[0], B[1])),
               max(point_segment_distance(B[0], A[0], A[1]), point_segment_distance(B[1], A[0], A[1])))


def to_global(seg, pose):
    R, t, s = as_pose(pose)
    R, t = R.astype(np.float64), t.astype(np.float64)
    return [(float(((x * R[0, 0] + y * R[0, 1]) + t[0]) * s), float(((x * R[1, 0] + y * R[1, 1]) + t[1]) * s)) for x, y in seg]


# ------------------------------------------------------------------------------------------------ the emulator
def emulate_pair(floor, k1, k2, min_width_ratio, variant=None):
    """One panorama pair (positions k1 < k2 in pano_ids) -> {rows, margins, n_valid, n_rejected, adjacent, gt}; rows in candidate order."""
    by_type = lambda k, T: [np.asarray(v, dtype=np.float64).tolist() for name, v in floor["wdos"][k] if TYPE_CODE[name] == T]
    kept, kept_x, margins, n_valid, n_rejected, seen = [], [], [], 0, 0, []
    P1, P2 = as_pose(floor["poses"][k1]), as_pose(floor["poses"][k2])
    G = sim2_compose(sim2_inverse(P1), P2) if variant == "gt-composed-the-other-way" else sim2_compose(sim2_inverse(P2), P1)
    for T in ((0, 1, 2) if variant == "types-in-table-order" else (1, 0, 2)):
        configurations = (0, 1) if T != 0 else (0,)
        if variant == "doors-without-rotated" and T == 1:
            configurations = (0,)
        if variant == "windows-with-rotated" and T == 0:
            configurations = (0, 1)
        for i, b in enumerate(by_type(k1, T)):
            for j, a in enumerate(by_type(k2, T)):
                for conf in configurations:
                    a1, a2 = (a[1], a[0]) if conf else (a[0], a[1])
                    R, t, _, _ = fit(a1, a2, b[0], b[1], two_point=variant == "two-point-polygons")
                    ratio = width_ratio(width(b[0], b[1]), width(a1, a2))
                    valid = ratio > min_width_ratio if variant == "ratio-strictly-greater" else ratio >= min_width_ratio
                    x = [float(v) for v in R] + [float(v) for v in t]
                    if not valid:
                        n_rejected += 1
                        continue
                    n_valid += 1
                    against = seen if variant == "prune-against-all-candidates" else kept_x
                    dup = bool(against) and allclose_any(x, np.array(against, dtype=np.float64), candidate_side=variant == "rtol-on-the-candidate")
                    seen.append(x)
                    if dup:
                        continue
                    kept_x.append(x)
                    label, margin = obj_almost_equal(R, t, G, T, opening_tolerance=7.0 if variant == "seven-degrees-for-openings" else 9.0)
                    kept.append((R, t, T, j, i, conf, label) if variant == "i-and-j-swapped" else (R, t, T, i, j, conf, label))
                    margins.append(margin)
    adjacent = any(hausdorff(to_global(A, floor["poses"][k1]), to_global(B, floor["poses"][k2])) < 0.1
                   for A in floor["gt_wdos"][k1] for B in floor["gt_wdos"][k2])
    return {"rows": kept, "margins": margins, "n_valid": n_valid, "n_rejected": n_rejected, "adjacent": adjacent, "gt": G}


def floor_pairs(floor):
    ids = list(floor["pano_ids"])
    return [(a, b) for a in range(len(ids)) for b in range(a + 1, len(ids)) if not (floor["building_id"] == "0006" and 7 in (ids[a], ids[b]))]


_CACHE = {}


def emulate_floor(floor, min_width_ratio=0.65, variant=None):
    """Every pair of the floor, in the generator's order (cached by the floor's content: the cases are fixed)."""
    key = (repr(floor), min_width_ratio, variant)
    if key not in _CACHE:
        _CACHE[key] = _emulate_floor(floor, min_width_ratio, variant)
    return _CACHE[key]


def _emulate_floor(floor, min_width_ratio, variant):
    return [dict(emulate_pair(floor, a, b, min_width_ratio, variant), i1=int(floor["pano_ids"][a]), i2=int(floor["pano_ids"][b])) for a, b in floor_pairs(floor)]


def file_name(pair, row):
    return f"{pair['i1']}_{pair['i2']}__{OBJECT[row[2]]}_{row[3]}_{row[4]}_{CONFIGURATION[row[5]]}.json"


def expected_hypotheses(pairs, variant=None):
    """The rows in ingest.load_floor_hypotheses' order -> list of (label, pair_idx, i1, i2, R, t, uuid, name): the label directories in order,
    the file names sorted as STRINGS within each."""
    out = []
    for label in (1, 0):
        rows = [(file_name(p, r), p, r) for p in pairs for r in p["rows"] if r[6] == label]
        if variant == "number-sorted-order":
            rows.sort(key=lambda x: (x[1]["i1"], x[1]["i2"], x[0]))
        else:
            rows.sort(key=lambda x: x[0])
        out += [(label, k, p["i1"], p["i2"], r[0], r[1], name[:-5].split("__")[-1], name) for k, (name, p, r) in enumerate(rows)]
    return out


def expected_buffers(case, variant=None):
    """The device buffers of one call over the case's floors, sentinel bytes where the kernel writes nothing -> (rows ROW [n_rows + GUARD],
    pair_out PAIR_OUT [n_pairs + GUARD], capacities)."""
    pairs = [p for f in case["floors"] for p in emulate_floor(f, case["min_width_ratio"], variant)]
    caps = []
    for f in case["floors"]:
        cnt = [[sum(TYPE_CODE[name] == T for name, _ in w) for T in range(3)] for w in f["wdos"]]
        caps += [2 * cnt[a][1] * cnt[b][1] + cnt[a][0] * cnt[b][0] + 2 * cnt[a][2] * cnt[b][2] for a, b in floor_pairs(f)]
    rows = np.frombuffer(bytes([SENTINEL]) * (ROW.itemsize * (sum(caps) + GUARD)), dtype=ROW).copy()
    out = np.frombuffer(bytes([SENTINEL]) * (PAIR_OUT.itemsize * (len(pairs) + GUARD)), dtype=PAIR_OUT).copy()
    off = 0
    for k, (p, cap) in enumerate(zip(pairs, caps)):
        for r, row in enumerate(p["rows"][:cap]):   # (a wrong kernel may keep more rows than the pair's capacity: n_kept tells)
            rows[off + r] = (row[0], row[1], row[2], row[3], row[4], row[5], row[6], 0)
        R, t, s = p["gt"]
        out[k] = (len(p["rows"]), p["n_valid"], p["n_rejected"], int(p["adjacent"]), R.reshape(4), t, s)
        off += cap
    return rows, out, caps


def check_margins(case):
    """The smallest label margin of the case (inf without a kept row); below MIN_MARGIN the case file is wrong."""
    m = min([x for f in case["floors"] for p in emulate_floor(f, case["min_width_ratio"]) for x in p["margins"]], default=float("inf"))
    if not m >= MIN_MARGIN:
        raise AssertionError(f"case {case['name']}: a label decision lies {m:.3e} from its threshold; the case must stay {MIN_MARGIN:.0e} clear")
    return m


# ------------------------------------------------------------------------------------------------ building floors
def rot(deg):
    th = math.radians(deg)
    return np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]], dtype=F32)


def seen_from(pose, seg):
    """A global segment in the panorama's frame: p = R^T (g / s - t)."""
    R, t, s = as_pose(pose)
    R, t = R.astype(np.float64), t.astype(np.float64)
    return [[float(R[0, 0] * (x / s - t[0]) + R[1, 0] * (y / s - t[1])), float(R[0, 1] * (x / s - t[0]) + R[1, 1] * (y / s - t[1]))] for x, y in seg]


def make_floor(building_id, floor_id, pano_ids, wdos, poses=None, gt_wdos=None):
    order = {"doors": 0, "windows": 1, "openings": 2}
    n = len(pano_ids)
    poses = poses if poses is not None else [(rot(17.0 * k), [0.5 * k, -0.25 * k], 1.0) for k in range(n)]
    return {"building_id": building_id, "floor_id": floor_id, "pano_ids": [int(i) for i in pano_ids],
            "wdos": [sorted(w, key=lambda x: order[x[0]]) for w in wdos], "poses": [as_pose(p) for p in poses],
            "gt_wdos": gt_wdos if gt_wdos is not None else [[] for _ in range(n)]}


def random_wdos(rng, n_doors, n_windows, n_openings):
    out = []
    for name, n in (("doors", n_doors), ("windows", n_windows), ("openings", n_openings)):
        for _ in range(n):
            c, th, w = rng.uniform(-3, 3, size=2), rng.uniform(0, 2 * math.pi), rng.uniform(0.7, 1.0)
            d = 0.5 * w * np.array([math.cos(th), math.sin(th)])
            out.append((name, [list(map(float, c - d)), list(map(float, c + d))]))
    return out


def house(seed, n_panos, building_id="0101", floor_id="floor_01", first_id=0, step=1):
    """A floor whose panoramas see shared doors, windows and openings from their own poses: aligned and misaligned labels, adjacent pairs."""
    rng = np.random.default_rng(seed)
    poses = [(rot(float(rng.uniform(-180, 180))), rng.uniform(-4, 4, size=2).astype(F32), float(rng.uniform(0.8, 1.25))) for _ in range(n_panos)]
    poses = [as_pose(p) for p in poses]
    shared = random_wdos(rng, 2, 1, 1)
    wdos, gt = [], []
    for k in range(n_panos):
        mine = []
        for name, seg in shared:
            if rng.uniform() < 0.75:
                local = seen_from(poses[k], seg)
                if rng.uniform() < 0.5:
                    local = local[::-1]
                # MHNet's noise: a few centimetres
                mine.append((name, [[x + float(rng.normal(0, 0.03)), y + float(rng.normal(0, 0.03))] for x, y in local]))
        mine += random_wdos(rng, int(rng.integers(0, 2)), int(rng.integers(0, 2)), 0)
        wdos.append(mine)
        gt.append([seen_from(poses[k], seg) for name, seg in shared if rng.uniform() < 0.7])
    return make_floor(building_id, floor_id, [first_id + step * k for k in range(n_panos)], wdos, poses, gt)


def _seg(x1, y1, x2, y2):
    return [[float(x1), float(y1)], [float(x2), float(y2)]]


def _windows(n, seed):
    return [w for w in random_wdos(np.random.default_rng(seed), 0, n, 0)]


def _prune_chain(order):
    """Three doors of panorama 2 whose fits against panorama 1's door differ only in tx: A = 100, B = 100.0008, C = 100.0016 -- A ~ B, B ~ C,
    A !~ C at 1e-8 + 1e-5 * 100.  Greedy pruning keeps {first, last} for the orders ABC and CBA and {B} alone for BAC."""
    tx = {"A": 100.0, "B": 100.0008, "C": 100.0016}
    return make_floor("0102", "floor_01", [0, 1], [[("windows", _seg(0, 0, 1, 0))], [("windows", _seg(tx[k], 0, tx[k] + 1, 0)) for k in order]])


# float32 neighbours found by search: |x - k| lies between 1e-8 + 1e-5 |k| and 1e-8 + 1e-5 |x|, so `x ~ k` depends on which of the two is kept
ONE_SIDED_K, ONE_SIDED_X = 1000.965576171875, 1000.9755859375


def cases():
    out = []

    def add(name, reason, floors, min_width_ratio=0.65):
        out.append({"name": name, "reason": reason, "floors": floors, "min_width_ratio": min_width_ratio})

    rng = np.random.default_rng(7)
    add("no-floor", "a call without floors launches nothing", [])
    add("empty-floor", "a floor of 0 panoramas has no pair", [make_floor("0100", "floor_01", [], [])])
    add("one-panorama", "a floor of 1 panorama has no pair", [make_floor("0100", "floor_01", [4], [random_wdos(rng, 1, 1, 1)])])
    add("two-panoramas", "the smallest floor with a pair", [house(1, 2)])
    add("panorama-without-wdos", "pairs of capacity 0 between pairs with rows", [make_floor("0100", "floor_02", [1, 2, 3], [random_wdos(rng, 1, 1, 1), [], random_wdos(rng, 2, 0, 1)])])
    add("doors-only", "one type only", [make_floor("0100", "floor_01", [0, 1], [random_wdos(rng, 2, 0, 0), random_wdos(rng, 3, 0, 0)])])
    add("windows-only", "windows have no rotated configuration", [make_floor("0100", "floor_01", [0, 1], [random_wdos(rng, 0, 2, 0), random_wdos(rng, 0, 3, 0)])])
    add("33-candidates", "33 = 3 x 11 windows: one candidate beyond 32 lanes, a partly filled wavefront", [make_floor("0100", "floor_01", [0, 1], [_windows(3, 1), _windows(11, 2)])])
    add("65-candidates", "65 = 5 x 13 windows: one candidate in the second chunk of 64", [make_floor("0100", "floor_01", [0, 1], [_windows(5, 3), _windows(13, 4)])])
    add("257-candidates", "257 = 2 x 8 x 16 doors + 1 window: five chunks, the kept list re-read from LDS",
        [make_floor("0100", "floor_01", [0, 1], [random_wdos(rng, 8, 1, 0), random_wdos(rng, 16, 1, 0)])])
    add("per-type-limit", "32 doors, 32 windows and 32 openings in both panoramas: the capacity limit of 5120 exactly",
        [make_floor("0100", "floor_01", [0, 1], [random_wdos(rng, 32, 32, 32), random_wdos(rng, 32, 32, 32)])])
    add("two-floors", "floors of 3 and 5 panoramas in one call: 3 + 10 pairs, offsets across floors", [house(2, 3, "0103"), house(3, 5, "0104", "floor_02", first_id=20)])
    add("equal-widths", "a ratio of exactly 1", [make_floor("0100", "floor_01", [0, 1], [[("doors", _seg(0, 0, 1, 0))], [("doors", _seg(3, 1, 3, 2))]])])
    add("zero-widths", "two zero widths give a NaN ratio, one gives 0: both reject",
        [make_floor("0100", "floor_01", [0, 1], [[("doors", _seg(1, 1, 1, 1)), ("doors", _seg(0, 0, 1, 0))], [("doors", _seg(2, 2, 2, 2))]])])
    add("ratio-at-threshold", "widths 0.65 and 1: the ratio equals 0.65 exactly and is accepted (>=)",
        [make_floor("0100", "floor_01", [0, 1], [[("openings", _seg(0, 0, 0.65, 0))], [("openings", _seg(2, 1, 2, 2))]])])
    add("half-turn", "an exact half turn: c < 0, s == 0, R = -I exactly", [make_floor("0100", "floor_01", [0, 1], [[("windows", _seg(1, 2, 3, 2))], [("windows", _seg(-1, -2, -3, -2))]])])
    add("quarter-turn", "an exact quarter turn: c == 0", [make_floor("0100", "floor_01", [0, 1], [[("windows", _seg(1, 2, 3, 2))], [("windows", _seg(-2, 1, -2, 3))]])])
    add("h-zero", "a zero-width object accepted at min_width_ratio 0: c = s = h = 0, R = I",
        [make_floor("0100", "floor_01", [0, 1], [[("windows", _seg(1, 1, 1, 1))], [("windows", _seg(2, 3, 4, 3))]])], min_width_ratio=0.0)
    for order in ("ABC", "CBA", "BAC"):
        add(f"prune-chain-{order}", "A ~ B, B ~ C, A !~ C: greedy pruning depends on the order and compares with the KEPT rows only", [_prune_chain(order)])
    for first, second in ((ONE_SIDED_K, ONE_SIDED_X), (ONE_SIDED_X, ONE_SIDED_K)):
        add(f"one-sided-rtol-{first}", "two fits whose difference lies between the tolerances of the two: rtol is on the kept one's side",
            [make_floor("0102", "floor_01", [0, 1], [[("windows", _seg(0, 0, 1, 0))], [("windows", _seg(first, 0, first + 1, 0)), ("windows", _seg(second, 0, second + 1, 0))]])])
    add("duplicate-across-types", "a door and an opening at the same place: the opening's fit is pruned against the door's",
        [make_floor("0100", "floor_01", [0, 1], [[("doors", _seg(0, 0, 1, 0)), ("openings", _seg(0, 0, 1, 0))], [("doors", _seg(2, 1, 2, 2)), ("openings", _seg(2, 1, 2, 2))]])])
    add("ids-2-10-100", "panorama ids that sort differently as strings and as numbers", [dict(house(4, 3, "0105"), pano_ids=[2, 10, 100])])
    add("building-0006", "building 0006: the pairs of panorama 7 are left out", [dict(house(5, 4, "0006"), pano_ids=[6, 7, 8, 9])])
    # an opening 8 degrees off the truth, near panorama 1's origin so that the translation stays in tolerance: aligned at 9 degrees, not at 7
    P1, P2 = as_pose((rot(0.0), [0.0, 0.0], 1.0)), as_pose((rot(30.0), [1.0, 0.5], 1.0))
    opening = _seg(0.2, -0.5, 0.2, 0.5)
    l1, l2 = seen_from(P1, opening), seen_from(P2, opening)
    mid = [(l2[0][0] + l2[1][0]) / 2, (l2[0][1] + l2[1][1]) / 2]
    c8, s8 = math.cos(math.radians(8.0)), math.sin(math.radians(8.0))
    l2r = [[mid[0] + c8 * (x - mid[0]) - s8 * (y - mid[1]), mid[1] + s8 * (x - mid[0]) + c8 * (y - mid[1])] for x, y in l2]
    add("opening-8-degrees", "openings tolerate 9 degrees, doors and windows 7: an opening whose fit is 8 degrees off the truth is aligned",
        [make_floor("0100", "floor_01", [0, 1], [[("openings", l1)], [("openings", l2r)]], [P1, P2], [[l1], [l2]])])
    add("door-8-degrees", "the same segments as doors: not aligned",
        [make_floor("0100", "floor_01", [0, 1], [[("doors", l1)], [("doors", l2r)]], [P1, P2], [[l1], [l2]])])
    return out


def case(name):
    return next(c for c in cases() if c["name"] == name)


def refusal_floor():
    """33 doors in one panorama: one more than the limit."""
    rng = np.random.default_rng(11)
    return make_floor("0107", "floor_03", [5, 9], [random_wdos(rng, 33, 0, 0), random_wdos(rng, 1, 0, 0)])


# ------------------------------------------------------------------------------------------------ plumbing between the cases and the library
def floor_input(floor):
    """A case's floor as the library takes it (salve_amd.hypotheses.FloorInput).  Plumbing only: no rule of the emulator passes through here."""
    from salve_amd.hypotheses import FloorInput
    from salve_amd.layout import PanoLayouts

    n = len(floor["pano_ids"])
    specs = [(np.zeros((0, 2)), [(name, np.asarray(v, dtype=np.float64)) for name, v in w]) for w in floor["wdos"]] or [(np.zeros((0, 2)), [])]
    gt = [np.asarray(s, dtype=np.float64).reshape(2, 2) for w in floor["gt_wdos"] for s in w]
    return FloorInput(floor["building_id"], floor["floor_id"], np.array(floor["pano_ids"], dtype=np.int64), PanoLayouts.from_specs(specs),
                      np.array([p[0] for p in floor["poses"]], dtype=F32).reshape(n, 2, 2), np.array([p[1] for p in floor["poses"]], dtype=F32).reshape(n, 2),
                      np.array([p[2] for p in floor["poses"]], dtype=np.float64), np.concatenate([[0], np.cumsum([len(w) for w in floor["gt_wdos"]])]).astype(np.int64),
                      np.stack(gt) if gt else np.zeros((0, 2, 2)))


def floor_dict(fi):
    """The other way round: a library FloorInput (the fixture floor, loaded by the library's host loaders) as the emulator's plain dict."""
    L = fi.layouts
    names = ("windows", "doors", "openings")
    wdos = [[(names[int(L.wdo_type[k])], L.wdo_xy[k].tolist()) for k in range(int(L.wdo_off[p]), int(L.wdo_off[p + 1]))] for p in range(len(fi.pano_ids))]
    gt = [[fi.gt_wdo_xy[k].tolist() for k in range(int(fi.gt_wdo_off[p]), int(fi.gt_wdo_off[p + 1]))] for p in range(len(fi.pano_ids))]
    return {"building_id": fi.building_id, "floor_id": fi.floor_id, "pano_ids": [int(i) for i in fi.pano_ids], "wdos": wdos,
            "poses": [as_pose((fi.R[p], fi.t[p], float(fi.s[p]))) for p in range(len(fi.pano_ids))], "gt_wdos": gt}


GOLDEN_ZIND, GOLDEN_MHNET, GOLDEN_RESULT = "zind_0000_floor_01_wdo.json", "mhnet_0000_floor_01.npz", "hypotheses_0000_floor_01.json"
MICRO = 1e6   # MHNet writes its boundaries with six decimals: the fixture holds them as integers of 1e-6 pixels, v == int / 1e6 exactly


def expand_fixture(golden_dir, tmp_dir):
    """tests/golden's two fixture files as the trees the loaders read -> (raw_dataset_dir, mhnet_predictions_data_root):
    {raw}/0000/zind_data.json and {root}/horizon_net/0000/{stem}.json, one per panorama.  The .npz holds `meta` (a JSON string: per panorama the
    stem, the image size, wall_features, and corners_in_uv where recorded), `floor_boundary` (int32 [32, 1024], the column-to-column differences
    of the boundary in 1e-6 pixels) and `uncertainty` (the same for the one panorama whose first values the reference's test records)."""
    import json
    from pathlib import Path

    golden_dir, tmp_dir = Path(golden_dir), Path(tmp_dir)
    raw, root = tmp_dir / "zind", tmp_dir / "mhnet"
    (raw / "0000").mkdir(parents=True, exist_ok=True)
    (root / "horizon_net" / "0000").mkdir(parents=True, exist_ok=True)
    (raw / "0000" / "zind_data.json").write_text((golden_dir / GOLDEN_ZIND).read_text())
    with np.load(golden_dir / GOLDEN_MHNET, allow_pickle=False) as z:
        meta = json.loads(str(z["meta"]))
        boundary = (np.cumsum(z["floor_boundary"].astype(np.int64), axis=1) / MICRO).tolist()
        uncertainty = (np.cumsum(z["uncertainty"].astype(np.int64)) / MICRO).tolist()
    for k, p in enumerate(meta["panoramas"]):
        room = {"raw_predictions": {"floor_boundary": boundary[k]}}
        if "corners_in_uv" in p:
            room["corners_in_uv"] = p["corners_in_uv"]
            room["raw_predictions"]["floor_boundary_uncertainty"] = uncertainty
        doc = {"predictions": {"image_width": p["image_width"], "image_height": p["image_height"], "room_shape": room, "wall_features": p["wall_features"]}}
        (root / "horizon_net" / "0000" / f"{p['stem']}.json").write_text(json.dumps(doc))
    return str(raw), str(root)


_OBJ, _CONF = {"d": "door", "w": "window", "o": "opening"}, {"i": "identity", "r": "rotated"}


def pack_names(hyps):
    """expected_hypotheses' rows as the golden file records them: per label directory, in order, [["{i1}_{i2}", "d0.1r w2.0i ..."], ...] -- a token
    is the object's first letter, i.j, and the configuration's first letter.  (The names of a pair are contiguous in the string sort.)"""
    out = {d: [] for d in LABEL_DIRS}
    for h in hyps:
        pair, rest = h[7][:-len(".json")].split("__")
        obj, i, j, conf = rest.split("_")
        groups = out[LABEL_DIRS[1 - h[0]]]
        if not groups or groups[-1][0] != pair:
            groups.append([pair, ""])
        groups[-1][1] = (groups[-1][1] + " " + f"{obj[0]}{i}.{j}{conf[0]}").strip()
    return out


def recorded_names(rec):
    """The golden file's names, unpacked -> [[label directory, file name], ...] in ingest.load_floor_hypotheses' order."""
    out = []
    for d in LABEL_DIRS:
        for pair, tokens in rec["names"][d]:
            for tok in tokens.split(" "):
                i, j = tok[1:-1].split(".")
                out.append([d, f"{pair}__{_OBJ[tok[0]]}_{i}_{j}_{_CONF[tok[-1]]}.json"])
    return out


def digest(hyps):
    """sha256 over the float32 R and t of expected_hypotheses' rows, in order."""
    import hashlib

    h = hashlib.sha256()
    for row in hyps:
        h.update(np.asarray(row[4], dtype="<f4").tobytes())
        h.update(np.asarray(row[5], dtype="<f4").tobytes())
    return h.hexdigest()
