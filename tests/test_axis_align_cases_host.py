"""The axis-alignment emulator and its case list, on the CPU: the case list's conditions; the emulator against the closed form, against the
reference's own recorded three-point alignment and against a reference-shaped restatement over salve_amd.common objects; AxisInputs'
refusals, FloorInput's new field and the command line's argument errors.

The closed form: an applied row is R' = Rc R, T = (Rc (s t - c) + c) / s with c the moved W/D/O centre.  The division by s is
Similarity3.Align's own (it returns the T of a = s' (R' b + T), and s' = s here); it is what the rule T = (ca - s' (R cb)) / s' gives, and with
s = 1 -- every hypothesis the exporter writes -- it is the same as Rc (s t - c) + c."""

import json
from pathlib import Path

import numpy as np
import pytest

from salve_amd import pose_graph as pg
from salve_amd.common.pano_data import WDO, PanoData
from salve_amd.common.sim2 import Sim2
from salve_amd.layout import PanoLayouts
from salve_amd.utils import rotation_utils
from tests import axis_align_cases as ac

GOLDEN = Path(__file__).resolve().parent / "golden"


def test_the_case_list_meets_its_conditions():
    caught = ac.check_conditions()
    assert set(caught) == set(ac.WRONG_KERNELS) and len(ac.WRONG_KERNELS) >= 14
    assert sum(len(c["rows"]) for c in ac.cases()) < 1000
    statuses = np.concatenate([ac.expected(c)[0][1]["status"][ac.GUARD:-ac.GUARD] for c in ac.cases()])
    assert {ac.APPLIED, ac.TOO_LARGE, ac.NO_ANGLE, ac.NO_ROOM, ac.MALFORMED} <= set(statuses.tolist())


def test_emulator_equals_the_closed_form_on_every_applied_row():
    """The closed form holds for a ROTATION R.  A row's float32 R is one only to 2^-23 an entry, and what the closest rotation to Rc R then is
    depends on the polygon.  So on every applied row (a) the emulator's geometry is run on the rotation by the row's own float64 angle and
    agrees with the closed form to 1e-9, and (b) the emulator's result for the row as stored agrees with the closed form of that rotation to
    what the float32 entries allow: 2^-22 in R', 2^-22 times (1 + the 12 m the rooms and W/D/Os stay within) in T."""
    n = 0
    rotation = lambda deg: np.array([[np.cos(np.deg2rad(deg)), -np.sin(np.deg2rad(deg))], [np.sin(np.deg2rad(deg)), np.cos(np.deg2rad(deg))]])
    for c in ac.cases():
        if c["name"] == "malformed-extents":   # (its floor table does not say which floor a row belongs to)
            continue
        (rows, axis, _), _, _ = ac.expected(c)
        for r in np.nonzero(axis["status"][ac.GUARD:-ac.GUARD] == ac.APPLIED)[0]:
            rec = axis[ac.GUARD + r]
            R32, t, s, seg, verts = ac.applied_row_inputs(c, r)
            R = rotation(np.rad2deg(np.arctan2(R32[1, 0], R32[0, 0])))
            want_R, want_T = ac.closed_form(R, t, s, seg, rec["correction_deg"])
            theta_deg, T = ac.turn_and_align(R.reshape(4), t, s, seg, verts, rec["correction_deg"])
            assert np.abs(rotation(theta_deg) - want_R).max() <= 1e-9 and np.abs(np.array(T) - want_T).max() <= 1e-9, (c["name"], r)   # (a)
            assert np.abs(rotation(rec["theta_deg"]) - want_R).max() <= 2.0 ** -22 and np.abs(rec["t"] - want_T).max() <= 2.0 ** -22 * 13, (c["name"], r)   # (b)
            assert rows["s"][ac.GUARD + r] == 1.0
            n += 1
    assert n > 300


def test_emulator_reproduces_the_references_three_point_alignment():
    d = json.loads((GOLDEN / "axis_align_compute_i2Ti1.json").read_text())
    pts1, pts2 = np.array(d["pts1"], dtype=np.float64), np.array(d["pts2"], dtype=np.float64)
    theta_deg, T, scale = ac.align_point_pairs([tuple(p) for p in pts2], [tuple(p) for p in pts1])
    th = np.deg2rad(theta_deg)
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    assert np.abs(pts1 @ R.T + np.array(T) - pts2).max() <= 1e-12      # the reference's own assertion: i2Ti1.transformFrom(pts1[i]) == pts2[i]
    want = d["expected_i2Ti1"]
    assert abs(abs(theta_deg) - want["theta_deg"]) <= 1e-12 and np.abs(np.array(T) - want["t"]).max() <= 1e-12 and abs(scale - 1.0) <= 1e-12


# ---- the reference's align_pair_measurement_by_vanishing_angle, restated over salve_amd.common objects (numpy's matrix products, a 3-D
# closest rotation by SVD as gtsam's Rot3::ClosestTo): no code shared with the emulator

def reference_compute_i2Ti1(pts1, pts2):
    a, b = np.c_[pts2, np.zeros(len(pts2))], np.c_[pts1, np.zeros(len(pts1))]   # lifted to the plane z = 0; the pairs are (pt2, pt1)
    ca, cb = a.mean(axis=0), b.mean(axis=0)
    da, db = a - ca, b - cb
    U, _, Vt = np.linalg.svd(da.T @ db)
    aRb = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    rdb = db @ aRb.T
    s = (da * rdb).sum() / (rdb * rdb).sum()
    aTb = (ca - s * (aRb @ cb)) / s
    theta_deg = rotation_utils.rotmat2theta_deg(aRb[:2, :2])
    return rotation_utils.rotmat2d(theta_deg), aTb[:2]


def reference_align_pair(i1, i2, i2Si1, alignment_object, i1_wdo_idx, panos):
    wdo = getattr(panos[i1], alignment_object + "s")[i1_wdo_idx]
    centre_i1 = np.array([wdo.pt1, wdo.pt2]).mean(axis=0)
    centre_i2 = i2Si1.transform_from(centre_i1.reshape(1, 2)).squeeze()
    vertsi1 = panos[i1].room_vertices_local_2d
    vertsi1_i2fr = i2Si1.transform_from(vertsi1)
    i2_theta_i1 = rotation_utils.rotmat2theta_deg(i2Si1.rotation)
    corr = -((panos[i2].vanishing_angle_deg - panos[i1].vanishing_angle_deg) + i2_theta_i1)
    corr = corr % 90
    if corr > 45:
        corr = corr - 90
    if np.absolute(corr) > 15.0:
        return None, corr
    rotmat = rotation_utils.rotmat2d(theta_deg=corr)
    turned = (vertsi1_i2fr - centre_i2).dot(rotmat.T) + centre_i2
    R, t = reference_compute_i2Ti1(vertsi1, turned)
    return Sim2(R=R, t=t, s=1.0), corr


def panos_of_case(c, f):
    base, objects = int(c["pano_base"][f]), {ac.DOOR: "doors", ac.WINDOW: "windows", ac.OPENING: "openings"}
    panos = {}
    for v in range(int(c["n_nodes"][f])):
        p = base + v
        room = c["room_xy"][int(c["room_off"][p]):int(c["room_off"][p + 1])][:-1]   # PanoData holds the room open
        lists = {"doors": [], "windows": [], "openings": []}
        for k in range(int(c["wdo_off"][p]), int(c["wdo_off"][p + 1])):
            lists[objects[int(c["wdo_type"][k])]].append(WDO(None, tuple(c["wdo_xy"][k, 0]), tuple(c["wdo_xy"][k, 1]), 0.0, 1.0, objects[int(c["wdo_type"][k])]))
        panos[v] = PanoData(v, None, room, "", "", lists["doors"], lists["windows"], lists["openings"], float(c["vanishing_deg"][p]))
    return panos


def test_emulator_equals_a_reference_shaped_restatement():
    """The cases both cover: sound tables, every panorama with an angle and a room of three vertices or more."""
    names, n = ("one-row", "65-rows", "room-sizes", "wdo-types", "quadrants", "folds", "scales", "two-floors-and-an-empty-one"), 0
    objects = {ac.DOOR: "door", ac.WINDOW: "window", ac.OPENING: "opening"}
    for name in names:
        c = ac.case(name)
        (rows, axis, _), _, _ = ac.expected(c)
        for f in range(len(c["n_nodes"])):
            panos = panos_of_case(c, f)
            for r in range(int(c["floor_start"][f]), int(c["floor_start"][f + 1])):
                row, rec, out = c["rows"][r], axis[ac.GUARD + r], rows[ac.GUARD + r]
                if rec["status"] == ac.NO_ROOM:
                    continue
                S = Sim2(row["R"].reshape(2, 2), row["t"], float(row["s"]))
                got, corr = reference_align_pair(int(row["i1"]), int(row["i2"]), S, objects[int(c["row_wdo"]["type"][r])], int(c["row_wdo"]["index"][r]), panos)
                assert abs(corr - rec["correction_deg"]) <= 1e-9, (name, r)
                assert (got is None) == (rec["status"] == ac.TOO_LARGE), (name, r)
                if got is not None:
                    assert np.abs(got.rotation.reshape(4) - out["R"]).max() <= 2.0 ** -23 and got.scale == out["s"] == 1.0, (name, r)
                    assert np.abs(got.translation.astype(np.float64) - out["t"]).max() <= 1e-9 + np.spacing(np.float32(np.abs(out["t"]).max())), (name, r)
                    n += 1
    assert n > 80


# ---- the host wrapper

def tiny_axis(angles=(10.0, -5.0, np.nan)):
    room = np.array([[2.0, 2.0], [-2.0, 2.0], [-2.0, -2.0], [2.0, -2.0], [2.0, 2.0]])
    door, window = np.array([[2.0, -0.5], [2.0, 0.5]]), np.array([[-0.5, 2.0], [0.5, 2.0]])
    specs = [(room, [("doors", door), ("windows", window), ("windows", window + 0.1)]), (room, [("doors", door)]), (np.zeros((0, 2)), [])]
    return pg.AxisInputs().add("0001", "floor_01", [4, 7, 9], PanoLayouts.from_specs(specs), angles)


def tiny_meas(uuids, pairs=None):
    n = len(uuids)
    pairs = pairs or [(4, 7)] * n
    return pg.EdgeMeasurements(["0001"] * n, ["floor_01"] * n, [p[0] for p in pairs], [p[1] for p in pairs], [0.9] * n, [1] * n, [1] * n,
                               np.tile(np.eye(2, dtype=np.float32), (n, 1, 1)), np.zeros((n, 2)), np.ones(n), list(uuids), ["identity"] * n)


def test_axis_inputs_tables_and_refusals():
    axis = tiny_axis()
    meas = tiny_meas(["window_1_0", "door_0_0", "window_0_0"], [(4, 9), (4, 7), (7, 9)][:2] + [(4, 7)])
    tabs = axis.tables(meas, meas.compact())
    # rows sorted by (i1, i2): (4, 7) door_0_0, (4, 7) window_0_0, (4, 9) window_1_0; PanoLayouts orders doors, windows, openings
    assert tabs["row_wdo"].tolist() == [(1, 0), (0, 0), (0, 1)] and tabs["pano_base"].tolist() == [0]
    assert tabs["room_off"].tolist() == [0, 5, 10, 10] and tabs["wdo_off"].tolist() == [0, 3, 4, 4] and tabs["wdo_type"].tolist() == [1, 0, 0, 1]
    assert np.array_equal(tabs["vanishing_deg"], np.array([10.0, -5.0, np.nan]), equal_nan=True)
    assert pg.AxisInputs.parse_wdo_pair_uuid("door_3_0") == (1, 3) and pg.AxisInputs.parse_wdo_pair_uuid("opening_0_12") == (2, 0)
    # a W/D/O index the layouts do not hold: the floor, the pair and the uuid are named, and nothing was uploaded (no device is involved here)
    for uuid in ("door_1_0", "window_2_0", "opening_0_0", "door_-1_0"):
        with pytest.raises(ValueError, match=rf"building 0001, floor_01, pair \(4, 7\): .*{uuid}"):
            axis.tables(tiny_meas([uuid]), tiny_meas([uuid]).compact())
    for uuid in ("garage_0_0", "door_0", "door_0_0_identity"):
        with pytest.raises(ValueError, match="wdo_pair_uuid"):
            axis.tables(tiny_meas([uuid]), tiny_meas([uuid]).compact())
    other = tiny_meas(["door_0_0"])
    other.floor_id = ["floor_02"]
    with pytest.raises(ValueError, match="floor_02 is not among the floors"):
        axis.tables(other, other.compact())
    unknown = tiny_meas(["door_0_0"], [(4, 8)])
    with pytest.raises(ValueError, match=r"no layout for panoramas \[8\]"):
        axis.tables(unknown, unknown.compact())
    with pytest.raises(ValueError, match="vanishing angles"):
        tiny_axis(angles=(1.0, 2.0))
    with pytest.raises(ValueError, match="no vanishing angles"):
        tiny_axis(angles=None)
    with pytest.raises(ValueError, match="ascend"):
        pg.AxisInputs().add("0001", "floor_01", [7, 4, 9], tiny_axis().floors[("0001", "floor_01")][1], [0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="random_spanning_trees takes no axis alignment"):
        pg.run(tiny_meas(["door_0_0"]), 0.5, method="random_spanning_trees", axis=axis)


def test_floor_input_carries_the_vanishing_angles():
    from salve_amd import hypotheses
    from salve_amd.common.pano_data import PoseGraph2d

    eye = Sim2(np.eye(2), np.zeros(2), 1.0)
    room = np.array([[1.0, 1.0], [-1.0, 1.0], [-1.0, -1.0]])
    node = lambda i, angle: PanoData(i, eye, room, "", "", [WDO(eye, (1.0, 0.0), (1.0, 0.5), 0.0, 1.0, "doors")], [], [], angle)
    gt = PoseGraph2d("0002", "floor_01", {3: node(3, None), 5: node(5, None)}, 1.0)
    inferred = PoseGraph2d("0002", "floor_01", {3: node(3, 12.5), 5: node(5, None)}, 1.0)
    fi = hypotheses.FloorInput.from_pose_graphs(gt, inferred)
    assert fi.vanishing_angle_deg.dtype == np.float64 and fi.vanishing_angle_deg[0] == 12.5 and np.isnan(fi.vanishing_angle_deg[1])
    plain = hypotheses.FloorInput(fi.building_id, fi.floor_id, fi.pano_ids, fi.layouts, fi.R, fi.t, fi.s, fi.gt_wdo_off, fi.gt_wdo_xy)
    assert plain.vanishing_angle_deg is None   # the trailing field is optional: existing callers are unchanged
    with pytest.raises(ValueError, match="3 vanishing angles for 2 panoramas"):
        hypotheses.FloorInput(fi.building_id, fi.floor_id, fi.pano_ids, fi.layouts, fi.R, fi.t, fi.s, fi.gt_wdo_off, fi.gt_wdo_xy, [0.0, 1.0, 2.0])
    axis = pg.AxisInputs.from_floors([fi])
    assert list(axis.floors) == [("0002", "floor_01")] and axis.floors[("0002", "floor_01")][0].tolist() == [3, 5]
    with pytest.raises(ValueError, match="no vanishing angles"):
        pg.AxisInputs.from_floors([plain])


@pytest.mark.parametrize("argv, message", [
    (["--axis-alignment"], "--axis-alignment needs --mhnet-predictions-data-root and --zind-root"),
    (["--axis-alignment", "--zind-root", "Z"], "--axis-alignment needs --mhnet-predictions-data-root and --zind-root"),
    (["--axis-alignment", "--mhnet-predictions-data-root", "M"], "--axis-alignment needs --mhnet-predictions-data-root and --zind-root"),
    (["--axis-alignment", "--mhnet-predictions-data-root", "M", "--zind-root", "Z", "--method", "random_spanning_trees"],
     "--axis-alignment belongs to --method spanning_tree or pgo"),
    (["--mhnet-predictions-data-root", "M"], "--mhnet-predictions-data-root belongs to --axis-alignment"),
])
def test_command_line_argument_errors(argv, message, capsys, tmp_path):
    with pytest.raises(SystemExit) as e:   # (before a prediction file is read: the directory does not exist)
        pg.main([str(tmp_path / "no_such_directory"), "--hypotheses", str(tmp_path), "--confidence-threshold", "0.5"] + argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_command_line_help_names_the_references_default(capsys):
    with pytest.raises(SystemExit):
        pg.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--axis-alignment" in text and "ON by default there" in text
