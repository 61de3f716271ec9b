"""Host tests of the floor report (no GPU): the emulator of tests/floor_report_cases.py pinned against a plain dict-and-loop restatement of the
reference's functions, against oracle.layout_oracle.fill_poly bit for bit, and against the numbers the reference's own tests record (each
with that test's own tolerance); the draw against np.random.seed + the reference's call sequence; the fixture and its parser; the stated
conditions on the cases; and eleven emulated WRONG kernels, each of which must fail a named case.

gtsam, gtsfm and cv2 are not installed where this runs: Similarity3.Align of pose pairs is restated as the rules of include/salve_hip.h
(salve_floor_align), and the reference's IoU is unpinned -- the fixture records the EMULATOR's 4707 / 5514 = 0.8536.
"""

import json
import math

import numpy as np
import pytest

from oracle import layout_oracle as lo
from salve_amd import floor_report as fr
from salve_amd.common.sim2 import Sim2
from tests import floor_report_cases as fc

G = fc.GUARD


# ------------------------------------------------------------------------------------------------ the reference, restated with dicts and loops
def _mat(a, b):
    return [[a[0][0] * b[0][0] + a[0][1] * b[1][0], a[0][0] * b[0][1] + a[0][1] * b[1][1]],
            [a[1][0] * b[0][0] + a[1][1] * b[1][0], a[1][0] * b[0][1] + a[1][1] * b[1][1]]]


def _T(a):
    return [[a[0][0], a[1][0]], [a[0][1], a[1][1]]]


def _vec(R, p):
    return [R[0][0] * p[0] + R[0][1] * p[1], R[1][0] * p[0] + R[1][1] * p[1]]


def ref_align(aTi, bTi):
    """gtsfm's align_poses_sim3_ignore_missing over two lists of (R, t) or None -> (aligned list, (R, t, s)): Similarity3.Align of the pose
    pairs -- two Karcher steps from the first pair's aRb, then the scale and translation from the centred translations."""
    pairs = [(a, b) for a, b in zip(aTi, bTi) if a is not None and b is not None]
    n = len(pairs)
    R, t, s = [[1.0, 0.0], [0.0, 1.0]], [0.0, 0.0], 1.0
    if n >= 2:
        rel = [_mat(a[0], _T(b[0])) for a, b in pairs]
        R = rel[0]
        for _ in range(2):
            d = [math.atan2(_mat(_T(R), X)[1][0], _mat(_T(R), X)[0][0]) for X in rel]
            m = sum(d) / n
            R = _mat(R, [[math.cos(m), -math.sin(m)], [math.sin(m), math.cos(m)]])
        ca = [sum(a[1][k] for a, _ in pairs) / n for k in range(2)]
        cb = [sum(b[1][k] for _, b in pairs) / n for k in range(2)]
        x = y = 0.0
        for a, b in pairs:
            rb = _vec(R, [b[1][0] - cb[0], b[1][1] - cb[1]])
            y += (a[1][0] - ca[0]) * rb[0] + (a[1][1] - ca[1]) * rb[1]
            x += rb[0] * rb[0] + rb[1] * rb[1]
        rc = _vec(R, cb)
        s = y / x if x != 0.0 else math.nan
        if s != s or s == 0.0:   # rule 7, this project's own (not pinned against gtsfm's fallback)
            s, t = 1.0, [ca[0] - rc[0], ca[1] - rc[1]]
        else:
            t = [(ca[0] - s * rc[0]) / s, (ca[1] - s * rc[1]) / s]
    aligned = []
    for b in bTi:   # Similarity3.transformFrom(Pose3): (R Rb, s (R tb + t))
        if b is None:
            aligned.append(None)
            continue
        u = _vec(R, b[1])
        aligned.append((_mat(R, b[0]), [s * (u[0] + t[0]), s * (u[1] + t[1])]))
    return aligned, (R, t, s)


def ref_pose_errors(aTi, aligned):
    """ransac.py:88-129 compute_pose_errors_3d"""
    rot, trans = [], []
    for a, b in zip(aTi, aligned):
        if a is None or b is None:
            continue
        E = _mat(_T(a[0]), b[0])
        rot.append(abs(math.degrees(math.atan2(E[1][0], E[0][0]))))
        trans.append(math.hypot(a[1][0] - b[1][0], a[1][1] - b[1][1]))
    return (sum(rot) / len(rot) if rot else math.nan), (sum(trans) / len(trans) if trans else math.nan), rot, trans


def ref_ransac(aTi, bTi, num_iters=1000, delete_frac=0.33):
    """ransac.py:14-85 on the GLOBAL numpy state, as the reference draws"""
    valid = [i for i, b in enumerate(bTi) if b is not None]
    nd = math.ceil(delete_frac * len(valid))
    if len(valid) - nd < 2:
        return ref_align(aTi, bTi)
    best, best_rot, best_trans = None, math.inf, math.inf
    for _ in range(num_iters):
        sub = list(bTi)
        for i in np.random.choice(a=valid, size=nd, replace=False):
            sub[i] = None
        aligned, aSb = ref_align(aTi, sub)
        rot, trans, _, _ = ref_pose_errors(aTi, aligned)   # over the SUBSET's own poses: `aligned` is None where deleted
        if trans <= best_trans and rot <= best_rot:
            best, best_rot, best_trans = aSb, rot, trans
    R, t, s = best
    return [None if b is None else (_mat(R, b[0]), [s * (_vec(R, b[1])[0] + t[0]), s * (_vec(R, b[1])[1] + t[1])]) for b in bTi], best


def ref_report(wSi_list, truth: fr.FloorTruth):
    """from_est_floor_pose_graph without its plots and IoU: (rot, trans in metres, percent, aligned Sim2 by pano id)"""
    n_list = int(truth.pano_ids[-1]) + 1
    gt = {int(p): Sim2(truth.R[k], truth.t[k], float(truth.s[k])) for k, p in enumerate(truth.pano_ids)}
    est = {i: S for i, S in enumerate(wSi_list) if S is not None}
    lift = lambda d: [None if i not in d else ([[float(x) for x in r] for r in d[i].rotation], [float(x) for x in d[i].translation]) for i in range(n_list)]
    _, (R, t, s) = ref_ransac(lift(gt), lift(est))
    a_Sim2_b = Sim2(np.array(R), np.array(t), float(s))
    aligned = {}
    for i, S in est.items():   # apply_Sim3
        c = a_Sim2_b.compose(Sim2(S.rotation, S.translation, 1.0))
        aligned[i] = Sim2(c.rotation, c.translation * c.scale, truth.gt_scale)
    rot, trans, _, _ = ref_pose_errors(lift(gt), lift(aligned))
    return rot, trans * truth.scale_meters_per_coordinate, len(est) / len(gt) * 100, aligned, (R, t, s)


# ------------------------------------------------------------------------------------------------ the 1210 floor and the reference's recorded numbers
def test_1210_floor_gives_the_numbers_the_reference_records(golden_dir):
    d, truth, wSi = fc.golden_1210(golden_dir)
    _, align, iou, _ = fc.emulated_1210(str(golden_dir))
    fo, io = align[4][G], iou[0][G]
    want = d["reference_expects"]
    print(f"1210 floor_02: rot {fo['avg_rot_err']:.4f} trans {fo['avg_trans_err']:.4f} m, {fo['n_est']} of {fo['n_gt']}, IoU {io['inter']} / {io['uni']}")
    assert abs(fo["avg_rot_err"] - want["avg_abs_rot_err"][0]) <= want["avg_abs_rot_err"][1] == 1e-2 and want["avg_abs_rot_err"][0] == 1.37
    assert abs(fo["avg_trans_err"] - want["avg_abs_trans_err"][0]) <= want["avg_abs_trans_err"][1] == 2e-2 and want["avg_abs_trans_err"][0] == 0.19
    assert abs(fo["percent_localized"] - 13 / 19 * 100) <= 1e-2 and (fo["n_est"], fo["n_gt"]) == (13, 19)
    # the emulator's own record (the reference's IoU is unpinned without cv2)
    e = d["emulator"]
    assert (io["n_est"], io["n_gt"], io["inter"], io["uni"]) == (e["iou_n_est"], e["iou_n_gt"], e["iou_inter"], e["iou_union"]) and (io["inter"], io["uni"]) == (4707, 5514)
    assert fo["best"] == e["best"] and abs(fo["avg_rot_err"] - e["avg_rot_err"]) < 1e-12 and abs(fo["avg_trans_err"] - e["avg_trans_err"]) < 1e-12


def test_1210_floor_fails_with_errors_over_all_poses(golden_dir):
    """The mistake of scoring each RANSAC subset against ALL poses gives 1.316 degrees and 0.167 m: outside the reference's tolerances."""
    c = fc.emulated_1210(str(golden_dir))[0]
    fo = fc.emulate_align(c, wrong=("errors-over-all-poses",))[0][4][G]
    print(f"errors over all poses: rot {fo['avg_rot_err']:.4f} trans {fo['avg_trans_err']:.4f}")
    assert abs(fo["avg_rot_err"] - 1.37) > 1e-2 and abs(fo["avg_trans_err"] - 0.19) > 2e-2


def test_1210_emulator_equals_the_plain_restatement(golden_dir):
    _, truth, wSi = fc.golden_1210(golden_dir)
    c, align, _, _ = fc.emulated_1210(str(golden_dir))
    np.random.seed(0)
    rot, trans, pct, aligned, (R, t, s) = ref_report(wSi, truth)
    fo, nodes = align[4][G], align[1][G:-G]
    # The float64 alignment agrees to 1e-9 (the next test); behind it the aligned poses are float32, and numpy's float32 matmul in Sim2.compose may
    # round a product-sum once where the kernel's rule rounds every operation: one float32 ulp of a rotation entry, 6e-8, is 3.4e-6 degrees.
    assert abs(fo["avg_rot_err"] - rot) < 1e-5 and abs(fo["avg_trans_err"] - trans) < 1e-5 and fo["percent_localized"] == pct
    assert np.allclose(fo["R"], [R[0][0], R[0][1], R[1][0], R[1][1]], rtol=0, atol=1e-12) and np.allclose(fo["t"], t, rtol=0, atol=1e-10) and abs(fo["s"] - s) < 1e-10
    for k, p in enumerate(truth.pano_ids):
        assert bool(nodes["localized"][k]) == (int(p) in aligned)
        if int(p) in aligned:   # the float32 poses, bit for bit: both follow Sim2's float32 rules from (nearly) the same float64 transform
            assert np.allclose(nodes["R"][k], aligned[int(p)].rotation.reshape(4), rtol=0, atol=1e-6)
            assert np.allclose(nodes["t"][k], aligned[int(p)].translation, rtol=0, atol=1e-6) and nodes["s"][k] == truth.gt_scale


def test_cases_emulator_equals_the_plain_restatement():
    """Every hypothesis of the edge floors: the emulator's aSb and errors against ref_align + ref_pose_errors on plain lists."""
    c = fc.case("edge-floors")
    hyps = fc.expected_align("edge-floors")[0][0][G:-G]
    checked = 0
    for f, name in enumerate(c["floor_names"]):
        lo_, hi = int(c["node_start"][f]), int(c["node_start"][f + 1])
        a, b = c["truth"][lo_:hi], c["est"][lo_:hi]
        lift = lambda tab, keep: [([[float(r[0]), float(r[1])], [float(r[2]), float(r[3])]], [float(t[0]), float(t[1])]) if (p and k) else None
                                  for r, t, p, k in zip(tab["R"], tab["t"], tab["localized"], keep)]
        for h in range(int(c["hyp_start"][f]), int(c["hyp_start"][f + 1])):
            keep = [(int(c["masks"][h, k >> 5]) >> (k & 31)) & 1 for k in range(hi - lo_)]
            aTi, bTi = lift(a, [1] * len(a)), lift(b, keep)
            aligned, (R, t, s) = ref_align(aTi, bTi)
            rot, trans, _, _ = ref_pose_errors(aTi, aligned)
            got = hyps[h]
            assert np.allclose(got["R"], [R[0][0], R[0][1], R[1][0], R[1][1]], rtol=0, atol=1e-12), (name, h)
            assert np.allclose(got["t"], t, rtol=1e-10, atol=1e-10, equal_nan=True) and (abs(got["s"] - s) <= 1e-10 * abs(s) or (np.isnan(got["s"]) and math.isnan(s))), (name, h)
            for g, w in ((got["rot_err"], rot), (got["trans_err"], trans)):
                assert (np.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-9 * max(1.0, abs(w)), (name, h)
            checked += 1
    assert checked >= 35


def test_two_pose_case_of_the_reference():
    """tests/utils/test_ransac.py: poses at (50, 0) and (0, 10) against (50.1, 0) and (0, 9.9): the translations within 1e-3, the scale within 1e-2."""
    eye = np.tile([1.0, 0.0, 0.0, 1.0], (2, 1))
    at, bt = np.array([[50.0, 0.0], [0.0, 10.0]]), np.array([[50.1, 0.0], [0.0, 9.9]])
    r = fc.align_one(eye, at, eye, bt, np.array([True, True]))
    u = r["s"] * (np.stack([r["R"][0] * bt[:, 0] + r["R"][1] * bt[:, 1], r["R"][2] * bt[:, 0] + r["R"][3] * bt[:, 1]], axis=1) + r["t"])
    print("two-pose case:", u.tolist(), r["s"])
    assert abs(r["s"] - 1.0) <= 1e-2
    assert np.allclose(u[0], [50.0114, 0.0576299], rtol=0, atol=1e-3) and np.allclose(u[1], [-0.0113879, 9.94237], rtol=0, atol=1e-3)


def test_ten_pose_self_alignment_of_the_reference():
    """tests/utils/test_ransac.py: a pose graph of ten aligned to itself by the RANSAC comes back within 1e-3."""
    R5 = [[0.771176, -0.636622, 0.636622, 0.771176], [0.124104, -0.992269, 0.992269, 0.124104], [0.914145, 0.405387, -0.405387, 0.914145],
          [0.105365, -0.994434, 0.994434, 0.105365], [-0.991652, -0.12894, 0.12894, -0.991652]]
    t5 = [[6.94918, 2.4749], [6.06848, 4.57841], [6.47869, 5.29594], [5.59441, 5.22469], [7.21399, 5.41445]]
    truth = fr.FloorTruth("self", "floor_01", np.arange(10), np.array(R5 + R5).reshape(10, 2, 2), np.array(t5 + t5), np.ones(10), [np.zeros((0, 2))] * 10, 1.0, 1.0)
    wSi = [Sim2(truth.R[k], truth.t[k], 1.0) for k in range(10)]
    c = fc.case_from_floors([wSi], [truth], num_iters=1000, seed=0)
    assert len(c["masks"]) == 1000
    bufs, raised = fc.emulate_align(c)
    nodes = bufs[1][G:-G]
    assert not raised and nodes["localized"].all()
    assert np.allclose(nodes["R"].reshape(10, 2, 2), truth.R, rtol=0, atol=1e-3) and np.allclose(nodes["t"], truth.t, rtol=0, atol=1e-3)


# ------------------------------------------------------------------------------------------------ the draw, the fixture, the parser
@pytest.mark.parametrize("seed", [0, 7])
def test_draw_equals_the_reference_call_sequence(seed):
    valid = [np.array([0, 2, 3, 5, 8, 9, 11]), np.array([4]), np.array([1, 6]), np.array([0, 1, 2]), np.arange(40)[::2], np.zeros(0, dtype=np.int64)]
    got = fr.draw_alignment_subsets(valid, num_iters=25, delete_frac=0.33, seed=seed)
    np.random.seed(seed)
    for v, masks in zip(valid, got):
        nd = math.ceil(0.33 * len(v))
        if len(v) - nd < 2:   # no RANSAC: ONE hypothesis keeps all of `valid`, no draw is consumed
            want = [set(v.tolist())]
        else:
            want = [set(v.tolist()) - set(np.random.choice(a=list(v), size=nd, replace=False).tolist()) for _ in range(25)]
        assert masks.shape == (len(want), 8) and masks.dtype == np.uint32
        for m, w in zip(masks, want):
            assert {k for k in range(256) if (int(m[k >> 5]) >> (k & 31)) & 1} == w


def test_fixture_is_data_only_and_the_parser_reads_it(golden_dir, tmp_path):
    path = golden_dir / "zind_1210_floor_02.json"
    assert path.stat().st_size < 64 * 1024
    d = json.loads(path.read_text())   # JSON: numbers, strings, lists and dicts -- nothing a tool reads as code

    def strings(x):
        if isinstance(x, dict):
            for k, v in x.items():
                yield k
                yield from strings(v)
        elif isinstance(x, list):
            for v in x:
                yield from strings(v)
        elif isinstance(x, str):
            yield x

    assert all(len(s) < 200 and "import " not in s and "def " not in s for s in strings(d))
    truth = fr.FloorTruth.from_zind_json(path, "floor_02", building_id="1210")
    want = d["expected_parse"]
    assert [int(p) for p in truth.pano_ids] == sorted(int(k) for k in want) and len(truth.pano_ids) == 19
    assert truth.scale_meters_per_coordinate == d["scale_meters_per_coordinate"]["floor_02"]
    for k, p in enumerate(truth.pano_ids):
        w = want[str(int(p))]
        assert np.array_equal(truth.R[k].reshape(4), np.array(w["R"]).astype(np.float32)) and np.array_equal(truth.t[k], np.array(w["t"]).astype(np.float32))
        assert truth.s[k] == w["s"] and len(truth.room_vertices[k]) == w["n_vertices"]
    first = next(iter(next(iter(next(iter(d["merger"]["floor_02"].values())).values())).values()))
    assert truth.gt_scale == first["floor_plan_transformation"]["scale"]
    raw = first["layout_raw"]["vertices"]
    k0 = int(np.searchsorted(truth.pano_ids, int(first["image_path"].split("_")[-1].split(".")[0])))
    assert np.array_equal(truth.room_vertices[k0], np.array(raw) * [-1.0, 1.0])   # x negated
    with pytest.raises(ValueError):
        fr.FloorTruth.from_zind_json(path, "floor_01")
    # the scale imputation: a floor without one takes the mean of the others', a building without any the data set's average
    p2 = tmp_path / "zind_data.json"
    p2.write_text(json.dumps(dict(d, scale_meters_per_coordinate={"floor_01": 2.0, "floor_02": None, "floor_03": 4.0})))
    assert fr.FloorTruth.from_zind_json(p2, "floor_02").scale_meters_per_coordinate == 3.0
    p2.write_text(json.dumps(dict(d, scale_meters_per_coordinate={"floor_02": None})))
    assert fr.FloorTruth.from_zind_json(p2, "floor_02").scale_meters_per_coordinate == fr.ZIND_AVERAGE_SCALE_METERS_PER_COORDINATE


def test_host_refusals_and_report_json_round_trip(golden_dir):
    _, truth, wSi = fc.golden_1210(golden_dir)
    with pytest.raises(ValueError, match="does not hold"):
        fr.pack_tables([[Sim2(np.eye(2), np.zeros(2), 1.0)]], [truth])   # pano 0 is not on floor_02
    big = fr.FloorTruth("b", "f", np.arange(257), np.tile(np.eye(2), (257, 1, 1)), np.zeros((257, 2)), np.ones(257), [np.zeros((0, 2))] * 257, 1.0, 1.0)
    with pytest.raises(Exception, match="257 panoramas"):
        fr.pack_tables([None], [big])
    rep = fr.FloorReport("1210", "floor_02", 1.5, float("nan"), 50.0, 0.25, np.array([3, 5]), np.array([1.5, np.nan]), np.array([0.2, np.nan]),
                         [None, None, None, Sim2(np.eye(2), np.array([1.0, 2.0]), 0.4)], 3.1, 4, {"R": [1, 0, 0, 1], "t": [0, 0], "s": 1.0}, {"n_hyps": 9})
    back = fr.FloorReport.from_json(json.loads(json.dumps(rep.to_json())))
    assert back.to_json() == rep.to_json() and back.wSi_dict.keys() == {3} and np.isnan(back.avg_abs_trans_err)
    s = fr.summarize([rep, fr.FloorReport("1210", "floor_01", float("nan"), float("nan"), 0.0, 0.0, np.zeros(0), np.zeros(0), np.zeros(0), [], 3.1)])
    assert s["n_floors"] == 2 and s["avg_abs_rot_err"] == {"mean": 1.5, "median": 1.5} and s["floorplan_iou"] == {"mean": 0.125, "median": 0.125}
    assert math.isnan(s["avg_abs_trans_err"]["mean"])


# ------------------------------------------------------------------------------------------------ the raster against the oracle; the stated conditions
RASTER = [c["name"] for c in fc.cases() if not c["launch_checked"] and c["img_h"] * c["img_w"] <= 83 * 45]


@pytest.mark.parametrize("name", RASTER + ["zind-1210"])
def test_emulated_masks_equal_the_oracles_fill_poly(name, golden_dir):
    if name == "zind-1210":
        c, align, iou, bools = fc.emulated_1210(str(golden_dir))
        est = align[1][G:-G]
    else:
        c = fc.case(name)
        est, (iou, _, bools) = fc.raster_est(c), fc.expected_iou(name)
    for f in range(len(c["node_start"]) - 1):
        if iou[0][G + f]["bad"]:   # (a NaN pose: no mask)
            continue
        for tb, table in enumerate((est, c["truth"])):
            img = np.zeros((c["img_h"], c["img_w"]), dtype=np.uint8)
            for i in range(int(c["node_start"][f]), int(c["node_start"][f + 1])):
                v = c["room_xy"][int(c["room_off"][i]):int(c["room_off"][i + 1])]
                if table["localized"][i] and len(v):
                    node = table[i]
                    g = (v @ node["R"].reshape(2, 2).astype(np.float64).T + node["t"].astype(np.float64)) * node["s"] * c["metres"][f]
                    px = lo.to_pixels(g, xmin=-c["off"][0], ymin=-c["off"][1], scale=c["ppm"])
                    assert np.array_equal(px, fc.pose_pixels(v, node, c["metres"][f], c["off"], c["ppm"])[1].astype(np.int64)), (name, f, i)
                    lo.fill_poly(img, px, 1)
            assert np.array_equal(img.astype(bool), bools[f][tb]), (name, f, tb)


def test_stated_conditions_hold_on_every_case(golden_dir):
    worst_sep, worst_half = np.inf, 1.0
    for c in fc.cases():
        if c["launch_checked"]:
            continue
        worst_sep = min(worst_sep, fc.hypothesis_separation(c, fc.expected_align(c["name"])[0][0][G:-G]))
        worst_half = min(worst_half, fc.half_integer_margin(c, fc.raster_est(c)))
    c, align, _, _ = fc.emulated_1210(str(golden_dir))
    worst_sep = min(worst_sep, fc.hypothesis_separation(c, align[0][G:-G]))
    worst_half = min(worst_half, fc.half_integer_margin(c, align[1][G:-G]))
    print(f"smallest relative distance of two hypotheses' errors {worst_sep:.3e}; smallest distance to a half integer {worst_half:.3e}")
    assert worst_sep > 1e-9 and worst_half > 1e-4


def test_polygon_sizes_and_shapes_are_covered():
    c = fc.case("raster-45x83")
    sizes = np.diff(c["room_off"])
    assert {0, 1, 2, 3, 4, 10, 150} <= set(sizes.tolist())
    out = fc.expected_iou("raster-45x83")[0][0][G:-G]
    assert out["n_est"][1] == 0 and out["iou"][1] == 0.0 and out["n_gt"][1] > 0          # the empty estimate
    assert sizes[:c["node_start"][1]].sum() > 1024                                          # more edges than one LDS chunk holds
    assert fc.expected_iou("raster-1x1")[0][0][G]["uni"] == 1


# ------------------------------------------------------------------------------------------------ wrong kernels
def _align_differs(name, wrong):
    got, _ = fc.emulate_align(fc.case(name), wrong=(wrong,))
    return bool(fc.differences(got, fc.expected_align(name)[0], f64_atol=1e-9)[0])


def _iou_differs(name, wrong, est=None):
    c = fc.case(name)
    got = fc.emulate_iou(c, fc.raster_est(c) if est is None else est, wrong=(wrong,))[0]
    return bool(fc.differences(got, fc.expected_iou(name)[0])[0])


@pytest.mark.parametrize("wrong, name", [("errors-over-all-poses", "sizes"), ("pick-lt", "edge-floors"), ("one-karcher-step", "edge-floors"),
                                         ("t-not-divided-by-s", "edge-floors"), ("x-y-exchanged", "edge-floors"), ("float64-aligned-poses", "sizes"),
                                         ("trans-err-not-metres", "one-hypothesis")])
def test_wrong_alignment_kernels_fail(wrong, name):
    assert wrong in fc.WRONG_KERNELS and _align_differs(name, wrong), (wrong, name)


def test_pick_lt_fails_on_the_duplicate_masks():
    """`<` keeps the EARLIER of two equal hypotheses: floor duplicate-masks has its best mask twice."""
    c = fc.case("edge-floors")
    f = c["floor_names"].index("duplicate-masks")
    right, wrong = fc.expected_align("edge-floors")[0][4][G + f], fc.emulate_align(c, wrong=("pick-lt",))[0][4][G + f]
    h0 = int(c["hyp_start"][f])
    assert right["best"] > wrong["best"] >= 0 and np.array_equal(c["masks"][h0 + right["best"]], c["masks"][h0 + wrong["best"]])


def test_one_karcher_step_fails_on_the_floor_with_angles_on_both_sides_of_180():
    c = fc.case("edge-floors")
    f = c["floor_names"].index("both-sides-of-the-first")
    h = int(c["hyp_start"][f])
    a, b = fc.expected_align("edge-floors")[0][0][G + h], fc.emulate_align(c, wrong=("one-karcher-step",))[0][0][G + h]
    assert np.abs(a["R"] - b["R"]).max() > 1e-6


@pytest.mark.parametrize("wrong, name", [("non-zero-winding", "raster-83x45"), ("line-pixels-dropped", "raster-16x16"), ("round-half-away", "raster-half")])
def test_wrong_raster_kernels_fail(wrong, name):
    assert wrong in fc.WRONG_KERNELS
    if name == "raster-half":   # a vertex exactly on a half pixel: 2.5 rounds to 2 (half to even), to 3 away from zero.  Outside the GPU cases by the stated condition.
        node = np.zeros(1, dtype=fc.NODE)
        node["localized"], node["R"], node["s"] = 1, [1, 0, 0, 1], 1.0
        v = np.array([[2.5, 0.5], [6.5, 0.5], [6.5, 4.5], [2.5, 4.5]])
        right, away = fc.pose_pixels(v, node[0], 1.0, (0.0, 0.0), 1.0)[1], fc.pose_pixels(v, node[0], 1.0, (0.0, 0.0), 1.0, wrong=(wrong,))[1]
        assert right.tolist() == [[2, 0], [6, 0], [6, 4], [2, 4]] and away.tolist() == [[3, 1], [7, 1], [7, 5], [3, 5]]
        return
    assert _iou_differs(name, wrong), (wrong, name)


def test_mask_from_unaligned_poses_fails(golden_dir):
    """The estimate's mask must come from the ALIGNED poses: the unaligned table gives other counts on the 1210 floor."""
    assert "mask-from-unaligned-poses" in fc.WRONG_KERNELS
    c, align, iou, _ = fc.emulated_1210(str(golden_dir))
    unaligned = c["est"].copy()
    unaligned["s"] = c["gt_scale"][0]
    got = fc.emulate_iou(c, unaligned)[0][0][G]
    assert (got["inter"], got["uni"]) != (iou[0][G]["inter"], iou[0][G]["uni"])
