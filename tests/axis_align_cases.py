"""salve_pose_graph_axis_align (include/salve_hip.h): a numpy emulator of the entry, the case list the host and the GPU tests share, the
tolerances, and emulated WRONG kernels that the case list must catch.

The emulator follows the rules the header states -- row angle in float32, everything else float64 spelled out per entry, sums in ascending
vertex order from 0.0 -- and shares no code with salve_amd/.  Scalars are numpy float64 / float32 scalars: elementwise operations never fuse a
product into a sum.

A case is a dict: name, rows (ROW records of all floors), floor_start, n_nodes, row_wdo (WDO records; the emulated wrong kernel
`i2_wdo_idx_used` reads the parallel `row_wdo_i2`), pano_base, the five layout tables, vanishing_deg, and `malformed` (the status bit is
expected).  `expected(case)` gives the three output buffers filled with SENTINEL bytes, GUARD records on both sides, as a sound kernel
leaves them.

Tolerances (derived, not measured).  The only float32 transcendental is the row angle; the device's atan2f and numpy's arctan2 are allowed a
joint 8 float32 ulps at 180 degrees, E_DEG = 8 * 2^-16 degrees = E_RAD = 2.13e-6 rad.  Everything behind it is float64, whose error is
negligible next to that.  So |dR'| <= E_RAD + 2^-23 (one float32 rounding of an entry <= 1), |dt'| <= E_RAD * s * |w| + one float32 ulp of
|t'| with w the W/D/O centre in i1's frame (the lever arm of the turn about the moved centre), correction_deg and theta_deg within E_DEG,
the unrounded translation within E_RAD * s * |w| + 1e-12.  Statuses, counts, copied rows and copied fields are compared exactly.

Conditions on the case list, asserted by `check_conditions` (tests/test_axis_align_cases_host.py runs it on the CPU):
  - no row's unfolded correction lies within MARGIN_DEG = 1e-3 degrees of a multiple of 90 or of the 45-degree fold (45 + 90 k), and no
    |correction| within 1e-3 degrees of 15: 1e-3 is about eight times E_DEG, so a few-ulp difference of the device's atan2f cannot flip a status;
  - every emulated wrong kernel flips a status, or moves an output by more than 100 times its tolerance, in at least one case -- but for
    the one the rules make invisible (INVISIBLE_KERNELS below says why), which is shown to change nothing."""

from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64
ROW = np.dtype([("i1", "<i4"), ("i2", "<i4"), ("prob", "<f4"), ("y_hat", "<i4"), ("R", "<f4", (4,)), ("t", "<f4", (2,)), ("s", "<f8")])
WDO = np.dtype([("type", "<i4"), ("index", "<i4")])
ROW_OUT = np.dtype([("status", "<i4"), ("reserved", "<i4"), ("correction_deg", "<f8"), ("theta_deg", "<f8"), ("t", "<f8", (2,))])
FLOOR_OUT = np.dtype([("n_applied", "<i4"), ("n_too_large", "<i4"), ("n_no_angle", "<i4"), ("n_no_room", "<i4"), ("n_malformed", "<i4"),
                      ("bad_extent", "<i4")])
APPLIED, TOO_LARGE, NO_ANGLE, NO_ROOM, MALFORMED = 0, 1, 2, 3, 4   # include/salve_hip.h: SALVE_AXIS_*
COUNT_FIELDS = ("n_applied", "n_too_large", "n_no_angle", "n_no_room", "n_malformed")
STATUS_BAD_AXIS_ROW = 512   # SALVE_STATUS_BAD_AXIS_ROW
SENTINEL = 0xA5             # every byte of a fresh output buffer
GUARD = 2                   # records in front of and behind each output array
MAX_ALLOWED_CORRECTION_DEG = 15.0
E_DEG = 8.0 * 2.0 ** -16
E_RAD = float(np.deg2rad(E_DEG))
MARGIN_DEG = 1e-3
WINDOW, DOOR, OPENING = 0, 1, 2   # layout.WDO_TYPES' codes; a panorama stores doors, windows, openings

WRONG_KERNELS = ("rotation_about_origin", "rotation_about_i1_centre", "correction_sign_flipped", "vp_swapped", "no_fold_at_45",
                 "threshold_on_unfolded", "too_large_corrected_anyway", "angle_from_R01", "translation_not_updated", "i2_wdo_idx_used",
                 "index_among_all_wdos", "translation_not_divided_by_scale", "degrees_into_sin_cos", "output_scale_copied")
# "scale dropped in the move" cannot be caught by any case: under the stated rule T = (ca - s' (R cb)) / s' (gtsam's s (R p + T)) the scale of
# the move cancels analytically -- T = (Rc (s t - c) + c) / s = t + R w - Rc R w, free of s -- and the written scale is 1.  check_conditions
# asserts that instead: the emulated kernel's outputs agree with the sound one's to 1e-9 on every case.  What a scale CAN spoil is the last
# division (T left as ca - s' (R cb)); that wrong kernel stands in the list above and the s != 1 cases catch it.
INVISIBLE_KERNELS = ("scale_dropped_in_move",)


# ---- the emulator

def row_angle_deg(R):
    """rotmat2theta_deg on Sim2's float32 entries: numpy evaluates arctan2 and rad2deg in float32; then widened."""
    return F64(np.rad2deg(np.arctan2(F32(R[2]), F32(R[0]))))


def fold(corr):
    """compute_vp_correction's tail: Python's % 90 (the divisor's sign), then - 90 above 45."""
    corr = F64(float(corr) % 90)
    return corr - 90 if corr > 45 else corr


def move(x, y, R, t, s, wrong=None):
    """Sim2.transform_from, ((p @ R.T) + t) * s, per entry."""
    R00, R01, R10, R11 = (F64(v) for v in R)
    tx, ty = F64(t[0]), F64(t[1])
    s = F64(1.0) if wrong == "scale_dropped_in_move" else F64(s)
    return ((x * R00 + y * R01) + tx) * s, ((x * R10 + y * R11) + ty) * s


def align_point_pairs(a, b):
    """Similarity3.Align over the pairs (a_k, b_k) restated in the plane, a = s' (R b + T), then compute_i2Ti1's degree round trip ->
    (theta_deg, T, s')."""
    n = len(a)
    sax = say = sbx = sby = F64(0.0)
    for (ax, ay), (bx, by) in zip(a, b):
        sax, say, sbx, sby = sax + ax, say + ay, sbx + bx, sby + by
    cax, cay, cbx, cby = sax / F64(n), say / F64(n), sbx / F64(n), sby / F64(n)
    H00 = H01 = H10 = H11 = F64(0.0)
    for (ax, ay), (bx, by) in zip(a, b):
        dax, day, dbx, dby = ax - cax, ay - cay, bx - cbx, by - cby
        H00, H01, H10, H11 = H00 + dax * dbx, H01 + dax * dby, H10 + day * dbx, H11 + day * dby
    phi = np.arctan2(H10 - H01, H00 + H11)
    c, s = np.cos(phi), np.sin(phi)
    x = y = F64(0.0)
    for (ax, ay), (bx, by) in zip(a, b):
        dax, day, dbx, dby = ax - cax, ay - cay, bx - cbx, by - cby
        px, py = c * dbx + (-s) * dby, s * dbx + c * dby
        x = x + (dax * px + day * py)
        y = y + (px * px + py * py)
    scale = x / y
    T = ((cax - scale * (c * cbx + (-s) * cby)) / scale, (cay - scale * (s * cbx + c * cby)) / scale)
    return F64(np.rad2deg(np.arctan2(s, c))), T, scale


def wdo_centre(seg):
    """WDO.centroid: the mean of the two endpoints."""
    return (F64(seg[0, 0]) + F64(seg[1, 0])) / F64(2.0), (F64(seg[0, 1]) + F64(seg[1, 1])) / F64(2.0)


def turn_and_align(R, t, s, seg, verts, corr, wrong=None):
    """The geometry of an applied row: i1's open room `verts` moved by (R, t, s), turned by corr degrees about the moved centre of the
    W/D/O `seg`, and i2Si1 re-estimated from the room and its turned copy -> (theta_deg, T) before they are rounded.  R: 4 entries,
    row-major, of any float type (the kernel's are the row's float32 entries, widened)."""
    rad = corr if wrong == "degrees_into_sin_cos" else np.deg2rad(corr)
    cs, sn = np.cos(rad), np.sin(rad)
    wx, wy = wdo_centre(seg)
    cx, cy = move(wx, wy, R, t, s, wrong)
    if wrong == "rotation_about_origin":
        cx, cy = F64(0.0), F64(0.0)
    elif wrong == "rotation_about_i1_centre":
        cx, cy = wx, wy
    a, b = [], []
    for vx, vy in verts:
        vx, vy = F64(vx), F64(vy)
        qx, qy = move(vx, vy, R, t, s, wrong)
        dx, dy = qx - cx, qy - cy
        a.append(((dx * cs + dy * (-sn)) + cx, (dx * sn + dy * cs) + cy))
        b.append((vx, vy))
    theta_deg, T, scale = align_point_pairs(a, b)
    if wrong == "translation_not_divided_by_scale":
        T = (T[0] * scale, T[1] * scale)
    return theta_deg, T


def emulate_row(case, f, r, wrong=None):
    """(the written row, its ROW_OUT record, details) of row r of floor f; details: the unfolded correction and the lever arm, for the
    conditions and the tolerances (None where the row did not get that far)."""
    row, w = case["rows"][r], case["row_wdo"][r]
    out, rec = row.copy(), np.zeros((), dtype=ROW_OUT)
    rec["status"], rec["correction_deg"], rec["theta_deg"], rec["t"] = MALFORMED, np.nan, np.nan, np.nan
    det = {"unfolded": None, "lever": None}
    n, base, n_panos = int(case["n_nodes"][f]), int(case["pano_base"][f]), len(case["vanishing_deg"])
    i1, i2 = int(row["i1"]), int(row["i2"])
    if n < 0 or base < 0 or base + n > n_panos or not (0 <= i1 < n and 0 <= i2 < n):
        return out, rec, det
    wtype, windex = int(w["type"]), int(case["row_wdo_i2"][r] if wrong == "i2_wdo_idx_used" else w["index"])
    if not 0 <= wtype <= 2 or windex < 0:
        return out, rec, det
    p1, p2 = base + i1, base + i2
    wlo, whi, rlo, rhi = (int(case[k][p]) for k, p in (("wdo_off", p1), ("wdo_off", p1 + 1), ("room_off", p1), ("room_off", p1 + 1)))
    if wlo < 0 or whi < wlo or whi > len(case["wdo_type"]) or rlo < 0 or rhi < rlo or rhi > len(case["room_xy"]):
        return out, rec, det
    if wrong == "index_among_all_wdos":
        held = list(range(wlo, whi))
    else:
        held = [k for k in range(wlo, whi) if int(case["wdo_type"][k]) == wtype]
    if windex >= len(held):
        return out, rec, det
    seg = case["wdo_xy"][held[windex]]
    vp1, vp2 = F64(case["vanishing_deg"][p1]), F64(case["vanishing_deg"][p2])
    if not (np.isfinite(vp1) and np.isfinite(vp2)):
        rec["status"] = NO_ANGLE
        return out, rec, det
    nv = rhi - rlo - 1   # the open polygon
    if nv < 3:
        rec["status"] = NO_ROOM
        return out, rec, det
    verts = case["room_xy"][rlo:rlo + nv]

    R = row["R"]
    theta = row_angle_deg((R[0], R[2], R[1], R[3]) if wrong == "angle_from_R01" else R)
    if wrong == "vp_swapped":
        vp1, vp2 = vp2, vp1
    unfolded = -((vp2 - vp1) + theta)
    if wrong == "correction_sign_flipped":
        unfolded = -unfolded
    det["unfolded"] = float(unfolded)
    corr = F64(float(unfolded) % 90) if wrong == "no_fold_at_45" else fold(unfolded)
    rec["correction_deg"] = corr
    too_large = abs(unfolded if wrong == "threshold_on_unfolded" else corr) > MAX_ALLOWED_CORRECTION_DEG
    if too_large and wrong != "too_large_corrected_anyway":
        rec["status"] = TOO_LARGE
        return out, rec, det

    det["lever"] = float(np.hypot(*wdo_centre(seg)))
    theta_deg, T = turn_and_align(R, row["t"], row["s"], seg, verts, corr, wrong)
    th = np.deg2rad(theta_deg)
    c2, s2 = np.cos(th), np.sin(th)
    rec["status"], rec["theta_deg"], rec["t"] = APPLIED, theta_deg, T
    out["R"] = (F32(c2), F32(-s2), F32(s2), F32(c2))
    if wrong != "translation_not_updated":
        out["t"] = (F32(T[0]), F32(T[1]))
    if wrong != "output_scale_copied":
        out["s"] = 1.0
    return out, rec, det


def emulate(case, wrong=None):
    """(out_rows [n_rows], out_axis [n_rows], out_floors [F], written [n_rows] bool, raised, details per row) without guards."""
    N, F = len(case["rows"]), len(case["n_nodes"])
    out_rows, out_axis, out_floors = np.zeros(N, dtype=ROW), np.zeros(N, dtype=ROW_OUT), np.zeros(F, dtype=FLOOR_OUT)
    written, details, raised = np.zeros(N, dtype=bool), [None] * N, False
    for f in range(F):
        lo, hi = int(case["floor_start"][f]), int(case["floor_start"][f + 1])
        if lo < 0 or hi < lo or hi > N:   # no row of such a floor can be named
            out_floors["bad_extent"][f] = 1
            raised = True
            continue
        for r in range(lo, hi):
            out_rows[r], out_axis[r], details[r] = emulate_row(case, f, r, wrong)
            written[r] = True
            out_floors[COUNT_FIELDS[int(out_axis["status"][r])]][f] += 1
        raised = raised or out_floors["n_malformed"][f] > 0
    return out_rows, out_axis, out_floors, written, bool(raised), details


def applied_row_inputs(case, r):
    """(R [2, 2] float64 as the row holds it, t, s, the W/D/O's segment, the open room) of row r of a case with sound tables."""
    row, w = case["rows"][r], case["row_wdo"][r]
    f = int(np.searchsorted(case["floor_start"], r, side="right") - 1)
    p1 = int(case["pano_base"][f]) + int(row["i1"])
    held = [k for k in range(int(case["wdo_off"][p1]), int(case["wdo_off"][p1 + 1])) if int(case["wdo_type"][k]) == int(w["type"])]
    verts = case["room_xy"][int(case["room_off"][p1]):int(case["room_off"][p1 + 1]) - 1]
    return row["R"].astype(F64).reshape(2, 2), row["t"].astype(F64), float(row["s"]), case["wdo_xy"][held[int(w["index"])]], verts


def closed_form(R, t, s, seg, corr_deg):
    """The analytic result for a ROTATION R, independent of the polygon: R' = Rc R, T = (Rc (s t - c) + c) / s, c the moved W/D/O centre
    (gtsam's convention a = s' (R' b + T), s' = s) -> (R' [2, 2], T)."""
    c = s * (R @ seg.mean(axis=0) + t)
    a = np.deg2rad(corr_deg)
    Rc = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return Rc @ R, (Rc @ (s * t - c) + c) / s


# ---- buffers, tolerances, comparison

def fresh_buffers(case):
    N, F = len(case["rows"]), len(case["n_nodes"])
    return tuple(np.frombuffer(bytes([SENTINEL]) * ((n + 2 * GUARD) * dt.itemsize), dtype=dt).copy() for n, dt in ((N, ROW), (N, ROW_OUT), (F, FLOOR_OUT)))


_EXPECTED = {}


def expected(case, wrong=None):
    """((out_rows, out_axis, out_floors) with guards as a sound kernel leaves them, raised, details).  Computed once per case and shared:
    do not write into it."""
    key = (case["name"], wrong)
    if key not in _EXPECTED:
        out_rows, out_axis, out_floors, written, raised, details = emulate(case, wrong)
        bufs = fresh_buffers(case)
        bufs[0][GUARD:-GUARD][written], bufs[1][GUARD:-GUARD][written] = out_rows[written], out_axis[written]
        bufs[2][GUARD:-GUARD] = out_floors
        _EXPECTED[key] = (bufs, raised, details)
    return _EXPECTED[key]


def tolerances(row, lever, T):
    """(R, t float32, correction / theta in degrees, unrounded t) for an applied row with W/D/O centre |w| = lever and emulator translation T."""
    lev = E_RAD * float(row["s"]) * lever
    return E_RAD + 2.0 ** -23, lev + float(np.spacing(F32(np.abs(T).max()))), E_DEG, lev + 1e-12


def compare(case, got, want, details, scale=1.0):
    """Largest tolerance-relative differences of `got` against `want` (both with guards): asserts the exact parts (statuses, reserved, counts,
    copied rows and fields, sentinels and guards) and returns {"R", "t", "correction_deg", "theta_deg", "t64"}: each the largest |difference|
    / tolerance over the case (0.0 without an applied row).  scale: the tolerances' multiplier (the wrong-kernel condition asks 100)."""
    (g_rows, g_axis, g_floors), (w_rows, w_axis, w_floors) = got, want
    name = case["name"]
    assert g_floors.tobytes() == w_floors.tobytes(), (name, g_floors[GUARD:-GUARD], w_floors[GUARD:-GUARD])
    for k in ("status", "reserved"):
        assert g_axis[k].tobytes() == w_axis[k].tobytes(), (name, k)
    for k in ("i1", "i2", "prob", "y_hat", "s"):
        assert g_rows[k].tobytes() == w_rows[k].tobytes(), (name, k)
    worst = {"R": 0.0, "t": 0.0, "correction_deg": 0.0, "theta_deg": 0.0, "t64": 0.0}
    inner = slice(GUARD, len(g_rows) - GUARD)
    applied = np.zeros(len(g_rows), dtype=bool)
    applied[inner] = (w_axis["status"][inner] == APPLIED) & (w_axis["reserved"][inner] == 0)
    has_corr = np.zeros(len(g_rows), dtype=bool)
    has_corr[inner] = applied[inner] | ((w_axis["status"][inner] == TOO_LARGE) & (w_axis["reserved"][inner] == 0))
    # everything that is not an applied row (guards, unwritten rows, copied rows): bit for bit
    assert g_rows[~applied].tobytes() == w_rows[~applied].tobytes(), name
    for k in ("theta_deg", "t"):
        assert g_axis[k][~applied].tobytes() == w_axis[k][~applied].tobytes(), (name, k)
    assert g_axis["correction_deg"][~has_corr].tobytes() == w_axis["correction_deg"][~has_corr].tobytes(), name
    for j in np.nonzero(has_corr)[0]:
        worst["correction_deg"] = max(worst["correction_deg"], abs(g_axis["correction_deg"][j] - w_axis["correction_deg"][j]) / (E_DEG * scale))
    for j in np.nonzero(applied)[0]:
        tol_R, tol_t, tol_deg, tol_t64 = tolerances(case["rows"][j - GUARD], details[j - GUARD]["lever"], w_axis["t"][j])
        d = lambda a, b: float(np.abs(np.asarray(a, dtype=F64) - np.asarray(b, dtype=F64)).max())
        dth = abs(float(g_axis["theta_deg"][j]) - float(w_axis["theta_deg"][j]))
        dth = min(dth, abs(dth - 360.0))   # (an angle at +-180 may come out on either side)
        for k, v in (("R", d(g_rows["R"][j], w_rows["R"][j]) / tol_R), ("t", d(g_rows["t"][j], w_rows["t"][j]) / tol_t), ("theta_deg", dth / tol_deg),
                     ("t64", d(g_axis["t"][j], w_axis["t"][j]) / tol_t64)):
            worst[k] = max(worst[k], v / scale)
    return worst


# ---- the cases

def rot(deg):
    a = np.deg2rad(deg)
    return np.array([np.cos(a), -np.sin(a), np.sin(a), np.cos(a)])


def room(n, seed=0, centre=(0.3, -0.2)):
    """An open star-shaped polygon of n vertices (n >= 3 is not degenerate: the radii vary)."""
    k = np.arange(n)
    rad = 2.0 + 0.35 * np.sin(1.7 * k + seed) + 0.2 * np.cos(0.9 * k * (1 + seed % 3))
    ang = 2 * np.pi * k / max(n, 1) + 0.1 * seed
    return np.stack([centre[0] + rad * np.cos(ang), centre[1] + rad * np.sin(ang)], axis=1).reshape(n, 2)


def seg(cx, cy, half=0.45, along=0.0):
    d = np.array([np.cos(along), np.sin(along)]) * half
    return np.array([[cx - d[0], cy - d[1]], [cx + d[0], cy + d[1]]])


def standard_wdos(seed=0):
    """2 doors, 3 windows, 2 openings in the stored order doors, windows, openings; the centres differ by metres, so a wrong index shows."""
    c = [(2.1, 0.4), (-1.9, 1.0), (0.5, 2.2), (-0.8, -2.0), (1.6, -1.5), (10.0, 0.7), (0.0, 0.0)]
    types = [DOOR, DOOR, WINDOW, WINDOW, WINDOW, OPENING, OPENING]
    return [(t, seg(x + 0.01 * seed, y, along=0.3 * k + seed)) for k, (t, (x, y)) in enumerate(zip(types, c))]


class Builder:
    """Panoramas (an open room, W/D/Os, an angle) and floors of rows -> a case."""

    def __init__(self, name):
        self.name, self.panos, self.floors, self.malformed = name, [], [], False

    def pano(self, verts, wdos, angle):
        self.panos.append((np.asarray(verts, dtype=F64).reshape(-1, 2), list(wdos), float(angle)))
        return len(self.panos) - 1

    def floor(self, first_pano, n_panos, rows):
        """rows: dicts i1, i2 (compact), R (4), t, s, type, index, index2."""
        self.floors.append((first_pano, n_panos, list(rows)))

    def build(self):
        rows = [r for _, _, rs in self.floors for r in rs]
        N = len(rows)
        tab = np.zeros(N, dtype=ROW)
        wdo, wdo2 = np.zeros(N, dtype=WDO), np.zeros(N, dtype=np.int32)
        for k, r in enumerate(rows):
            tab[k] = (r["i1"], r["i2"], r.get("prob", 0.5 + 0.4 * ((k * 7) % 10) / 10), r.get("y_hat", k % 5 != 0), tuple(F32(v) for v in r["R"]),
                      tuple(F32(v) for v in r["t"]), r.get("s", 1.0))
            wdo[k], wdo2[k] = (r["type"], r["index"]), r.get("index2", 0)
        closed = [np.concatenate([v, v[:1]]) if len(v) else v for v, _, _ in self.panos]
        flat = [w for _, ws, _ in self.panos for w in ws]
        off = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return {"name": self.name, "rows": tab, "row_wdo": wdo, "row_wdo_i2": wdo2, "malformed": self.malformed,
                "floor_start": off([len(rs) for _, _, rs in self.floors]).astype(np.int32),
                "n_nodes": np.array([n for _, n, _ in self.floors], dtype=np.int32), "pano_base": np.array([b for b, _, _ in self.floors], dtype=np.int32),
                "room_off": off([len(c) for c in closed]), "room_xy": (np.concatenate(closed) if closed else np.zeros((0, 2))).astype(F64).reshape(-1, 2),
                "wdo_off": off([len(ws) for _, ws, _ in self.panos]),
                "wdo_xy": (np.stack([s for _, s in flat]) if flat else np.zeros((0, 2, 2))).astype(F64),
                "wdo_type": np.array([t for t, _ in flat], dtype=np.uint8), "vanishing_deg": np.array([a for _, _, a in self.panos], dtype=F64)}


def theta_for(vp1, vp2, unfolded):
    """The row rotation (degrees, wrapped into (-180, 180]) whose correction comes out as `unfolded` (up to the float32 rounding of R)."""
    th = -(vp2 - vp1) - unfolded
    return (th + 180.0) % 360.0 - 180.0 if (th + 180.0) % 360.0 != 0 else 180.0


def own_pair(b, unfolded, theta=None, n_room=5, wdos=None, wdo=(DOOR, 0), t=(0.7, -1.1), s=1.0, seed=0, nan_on=None, index2=0):
    """A row on a panorama pair of its own: i1 with the room and the W/D/Os, i2 bare.  Given theta, vp2 follows; else theta follows the
    angles.  -> the row (compact indices relative to the pair's first panorama, to be offset by the caller)."""
    vp1 = -31.0 + 7.3 * (seed % 9)
    if theta is None:
        vp2 = 12.0 - 3.1 * (seed % 7)
        theta = theta_for(vp1, vp2, unfolded)
    else:
        theta32 = float(row_angle_deg([F32(v) for v in rot(theta)]))
        vp2 = vp1 - unfolded - theta32
    p1 = b.pano(room(n_room, seed), standard_wdos(seed) if wdos is None else wdos, np.nan if nan_on == "i1" else vp1)
    b.pano(room(4, seed + 1), [], np.nan if nan_on == "i2" else vp2)
    return {"p1": p1, "R": rot(theta), "t": t, "s": s, "type": wdo[0], "index": wdo[1], "index2": index2}


def pairs_floor(b, specs):
    """One floor of rows on pairs of their own, sorted by (i1, i2)."""
    first = len(b.panos)
    rows = []
    for k, spec in enumerate(specs):
        r = own_pair(b, seed=spec.pop("seed", k), **spec)
        r["i1"], r["i2"] = r["p1"] - first, r["p1"] - first + 1
        rows.append(r)
    b.floor(first, len(b.panos) - first, rows)


def bulk_floor(b, n_panos, n_rows, seed, rooms=(4, 5, 6, 8, 30), scales=(1.0,)):
    """One floor of n_rows rows over the pairs of n_panos shared panoramas, sorted by (i1, i2): several rows per pair that name different
    W/D/Os, row rotations over the whole circle, corrections on both sides of 15 degrees."""
    rng = np.random.RandomState(seed)
    first = len(b.panos)
    vps = rng.uniform(-44.0, 44.0, n_panos)
    for k in range(n_panos):
        b.pano(room(rooms[k % len(rooms)], seed + k), standard_wdos(seed + k), vps[k])
    pairs = [(a, c) for a in range(n_panos) for c in range(a + 1, n_panos)]
    which = np.sort(rng.randint(0, len(pairs), n_rows))
    kinds = [(DOOR, 0), (DOOR, 1), (WINDOW, 0), (WINDOW, 2), (OPENING, 0), (OPENING, 1)]
    rows = []
    for k, q in enumerate(which):
        i1, i2 = pairs[q]
        u = rng.uniform(-24.0, 24.0) + 90.0 * rng.randint(-2, 3)
        wt, wi = kinds[rng.randint(len(kinds))]
        rows.append({"i1": i1, "i2": i2, "R": rot(theta_for(vps[i1], vps[i2], u)), "t": rng.uniform(-3, 3, 2), "s": scales[k % len(scales)], "type": wt,
                     "index": wi, "index2": int(rng.randint(0, 2))})
    b.floor(first, n_panos, rows)


def _cases():
    out = []

    b = Builder("one-row")
    pairs_floor(b, [dict(unfolded=7.0)])
    out.append(b.build())

    for n in (63, 64, 65, 257):   # a wavefront's and a workgroup's edge: one thread per row, 256 threads per floor
        b = Builder(f"{n}-rows")
        bulk_floor(b, 6, n, seed=n)
        out.append(b.build())

    b = Builder("room-sizes")   # exactly 3, 4, 63, 64, 65 vertices; 2 and none: NO_ROOM
    pairs_floor(b, [dict(unfolded=6.0 + k, n_room=n) for k, n in enumerate((3, 4, 63, 64, 65, 2, 0, 1))])
    out.append(b.build())

    b = Builder("wdo-types")   # every type, index 0 and last of the type; the centres at 10 m and at the origin
    pairs_floor(b, [dict(unfolded=-9.0 + 2 * k, wdo=w, index2=i2) for k, (w, i2) in enumerate((((DOOR, 0), 1), ((DOOR, 1), 0), ((WINDOW, 0), 2), ((WINDOW, 2), 0),
                                                                                               ((OPENING, 0), 1), ((OPENING, 1), 0)))])
    out.append(b.build())

    b = Builder("quadrants")   # row rotations in all four quadrants, at and near +-180 degrees, identity
    pairs_floor(b, [dict(unfolded=(-1) ** k * (5.0 + k), theta=th) for k, th in enumerate((0.0, 30.0, 120.0, -60.0, -150.0, 179.99, -179.99, 180.0, 90.0, -90.0))])
    out.append(b.build())

    b = Builder("folds")   # both sides of the 45-degree fold, of the modulo's wrap and of 15 degrees, before and after whole turns of 90
    us = (44.9, 45.1, -44.9, -45.1, -0.5, 0.5, 89.5, 90.5, -89.5, -90.5, 14.9, 15.1, -14.9, -15.1, 104.9, 105.1, 75.1, 74.9, 190.0, -265.0, 134.9, 135.1)
    pairs_floor(b, [dict(unfolded=u, wdo=(WINDOW, 1)) for u in us])
    out.append(b.build())

    b = Builder("nan-angles")
    pairs_floor(b, [dict(unfolded=5.0, nan_on="i1"), dict(unfolded=5.0, nan_on="i2"), dict(unfolded=5.0), dict(unfolded=30.0, nan_on="i2", n_room=2)])
    out.append(b.build())

    b = Builder("scales")   # s != 1: a dropped scale shows in the moved centre; s >= 1 keeps the stated translation bound an upper bound
    pairs_floor(b, [dict(unfolded=8.0, s=1.25, wdo=(OPENING, 0)), dict(unfolded=-11.0, s=2.0, wdo=(DOOR, 1), t=(2.0, 1.5)), dict(unfolded=3.0, s=1.5, wdo=(OPENING, 1))])
    out.append(b.build())

    b = Builder("two-floors-and-an-empty-one")   # different panorama counts; the empty floor has neither rows nor panoramas
    bulk_floor(b, 5, 20, seed=11)
    b.floor(len(b.panos), 0, [])
    bulk_floor(b, 9, 30, seed=12, scales=(1.0, 1.25))
    out.append(b.build())

    b = Builder("no-floor-rows")   # a floor with panoramas and no row
    bulk_floor(b, 3, 0, seed=13)
    out.append(b.build())

    # ---- malformed tables: the row is copied unchanged with MALFORMED, the bit is raised, the other rows are aligned
    b = Builder("malformed-rows")
    bulk_floor(b, 4, 12, seed=21)
    rows = b.floors[0][2]
    rows[1]["i1"] = 4; rows[2]["i2"] = -1; rows[3]["type"] = 3; rows[4]["type"] = -1; rows[5]["index"] = -1
    rows[6]["type"], rows[6]["index"] = DOOR, 2; rows[7]["type"], rows[7]["index"] = WINDOW, 3; rows[8]["index"] = 2 ** 31 - 1; rows[9]["i1"] = 2 ** 31 - 1
    b.malformed = True
    out.append(b.build())

    b = Builder("malformed-tables")   # panorama 1's W/D/O extent leaves its table, panorama 2's room extent steps back
    bulk_floor(b, 4, 16, seed=22)
    c = b.build()
    c["wdo_off"] = c["wdo_off"].copy(); c["room_off"] = c["room_off"].copy()
    c["wdo_off"][2] = len(c["wdo_type"]) + 5
    c["room_off"][3] = c["room_off"][2] - 1
    c["malformed"] = True
    out.append(c)

    b = Builder("malformed-floors")   # floor 0's panoramas leave the tables, floor 1's base is negative, floor 2 is sound, floor 3's n_nodes is negative
    for s_ in (31, 32, 33, 34):
        bulk_floor(b, 3, 6, seed=s_)
    c = b.build()
    c["pano_base"] = np.array([10, -1, 6, 9], dtype=np.int32)
    c["n_nodes"] = np.array([3, 3, 3, -3], dtype=np.int32)
    c["malformed"] = True
    out.append(c)

    b = Builder("malformed-extents")   # floor 1's rows run backwards, floor 2's leave the table: none of their rows can be named
    for s_ in (41, 42, 43):
        bulk_floor(b, 3, 5, seed=s_)
    c = b.build()
    c["floor_start"] = np.array([0, 5, 4, 99], dtype=np.int32)
    c["malformed"] = True
    out.append(c)
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES


def case(name):
    return next(c for c in cases() if c["name"] == name)


# ---- the conditions

def check_conditions():
    """-> {wrong kernel: the case that catches it}; asserts the margins and that every wrong kernel is caught."""
    for c in cases():
        (_, w_axis, _), raised, details = expected(c)
        assert raised == c["malformed"], c["name"]
        for r, det in enumerate(details):
            if det is None or det["unfolded"] is None:
                continue
            u = det["unfolded"]
            assert abs(u / 90.0 - round(u / 90.0)) * 90.0 > MARGIN_DEG, (c["name"], r, u)                 # a multiple of 90
            assert abs((u - 45.0) / 90.0 - round((u - 45.0) / 90.0)) * 90.0 > MARGIN_DEG, (c["name"], r, u)   # the fold
            corr = float(w_axis["correction_deg"][GUARD + r])
            assert abs(abs(corr) - MAX_ALLOWED_CORRECTION_DEG) > MARGIN_DEG, (c["name"], r, corr)
    caught = {}
    for wrong in WRONG_KERNELS:
        for c in cases():
            want, _, details = expected(c)
            got, _, _ = expected(c, wrong)
            try:
                worst = compare(c, got, want, details, scale=100.0)
            except AssertionError:
                caught[wrong] = c["name"]   # a status, a count or a copied field
                break
            if max(worst.values()) > 1.0:
                caught[wrong] = c["name"]
                break
        assert wrong in caught, f"no case catches the wrong kernel {wrong}"
    for wrong in INVISIBLE_KERNELS:
        for c in cases():
            (w_rows, w_axis, _), _, _ = expected(c)
            (g_rows, g_axis, _), _, _ = expected(c, wrong)
            assert g_axis["status"].tobytes() == w_axis["status"].tobytes() and g_rows["s"].tobytes() == w_rows["s"].tobytes(), (wrong, c["name"])
            m = w_axis["status"] == APPLIED
            assert np.abs(g_axis["t"][m] - w_axis["t"][m]).max(initial=0.0) <= 1e-9 and np.abs(g_axis["theta_deg"][m] - w_axis["theta_deg"][m]).max(initial=0.0) <= 1e-9
    return caught
