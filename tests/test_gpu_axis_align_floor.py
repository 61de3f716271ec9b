"""Axis alignment by vanishing angle on a whole floor, on the GPU: the golden ZInD 0000 floor_01 fixtures (MHNet's rooms and W/D/Os, the
hypotheses the device generates from them) with deterministic synthetic vanishing angles -- every panorama's ground-truth heading folded
into (-45, 45] plus a few degrees of noise, so that a correct hypothesis needs a small correction and a wrong one any.  align_rows gives the
emulator's statuses exactly and its poses within tolerance; solve(axis=) and optimise(axis=) equal solve / optimise on align_rows' table bit
for bit (the device hand-over changes nothing); keep_rows and the random-spanning-trees filter compose; axis=None leaves no trace; the
JSON round-trips; ingest.score_floor passes the inputs through."""

import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib, hypotheses  # noqa: E402
from salve_amd import pose_graph as pg  # noqa: E402
from tests import axis_align_cases as ac  # noqa: E402
from tests import hypotheses_cases as hc  # noqa: E402

DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden"
THRESHOLD = 0.6
OPTS = {"cycle_filter": False}


def synthetic_angles(fi):
    """One angle per panorama: the heading of its ground-truth pose folded into (-45, 45], plus up to 4 degrees of deterministic noise."""
    heading = np.rad2deg(np.arctan2(fi.R[:, 1, 0].astype(np.float64), fi.R[:, 0, 0].astype(np.float64)))
    noisy = heading + 4.0 * np.sin(1.3 * np.arange(len(heading)) + 0.5)
    return (noisy + 45.0) % 90.0 - 45.0


def measurements(h):
    """Every aligned hypothesis and every seventh other one, with deterministic predictions: the aligned ones positive, the others every third."""
    rows = np.array([k for k in range(len(h)) if h.label[k] or k % 7 == 0], dtype=np.int64)
    y_hat = np.array([1 if h.label[k] or k % 3 == 0 else 0 for k in rows])
    prob = 0.5 + 0.5 * ((rows * 37) % 100) / 100.0
    return pg.EdgeMeasurements.from_floor(h, rows, y_hat, prob)


def as_case(meas, axis, name="zind-0000-floor-01"):
    """The measurements as a case of tests/axis_align_cases.py (plumbing: the wrapper's own tables) -> (case, the table order)."""
    floors = meas.compact()
    table, floor_start, n_nodes, _ = pg._device_table(meas, floors, name)
    tabs = axis.tables(meas, floors)
    case = {"name": name, "rows": table.view(ac.ROW), "floor_start": floor_start, "n_nodes": n_nodes, "row_wdo": tabs["row_wdo"].view(ac.WDO),
            "row_wdo_i2": np.zeros(len(table), np.int32), "malformed": False, **{k: tabs[k] for k in ("pano_base", "room_off", "room_xy", "wdo_off",
                                                                                                     "wdo_xy", "wdo_type", "vanishing_deg")}}
    return case, np.concatenate([fl["rows"] for fl in floors])


def check_margins(details, axis_out):
    """The floor's rows keep the margins of axis_align_cases.check_conditions, so no status can flip on a few ulps of atan2f."""
    for r, det in enumerate(details):
        if det is not None and det["unfolded"] is not None:
            u = det["unfolded"]
            assert abs(u / 90.0 - round(u / 90.0)) * 90.0 > ac.MARGIN_DEG and abs((u - 45.0) / 90.0 - round((u - 45.0) / 90.0)) * 90.0 > ac.MARGIN_DEG, (r, u)
            assert abs(abs(float(axis_out["correction_deg"][r])) - ac.MAX_ALLOWED_CORRECTION_DEG) > ac.MARGIN_DEG, r


@pytest.fixture(scope="module")
def floor(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("axis_floor")
    raw, root = hc.expand_fixture(GOLDEN, tmp)
    (fi,) = hypotheses.load_floors(raw, root, ["0000"])
    assert fi.vanishing_angle_deg is not None and np.isnan(fi.vanishing_angle_deg).all()   # the fixture has no vanishing_angle file
    fi.vanishing_angle_deg = synthetic_angles(fi)
    (h,) = hypotheses.generate([fi], DEV)
    meas = measurements(h)
    axis = pg.AxisInputs.from_floors([fi])
    case, order = as_case(meas, axis)
    out_rows, out_axis, out_floors, written, raised, details = ac.emulate(case)
    assert written.all() and not raised
    check_margins(details, out_axis)
    aligned, info = pg.align_rows(meas, axis, DEV)
    return SimpleNamespace(fi=fi, meas=meas, axis=axis, case=case, order=order, want=(out_rows, out_axis, out_floors), details=details, aligned=aligned, info=info)


def test_align_rows_equals_the_emulator(floor):
    want_rows, want_axis, want_floors = floor.want
    meas, aligned, info, order = floor.meas, floor.aligned, floor.info, floor.order
    n = len(meas)
    assert 300 < n < 700 and len(aligned) == n
    assert info["status"][order].tolist() == want_axis["status"].tolist()
    counts = {name: int(want_floors[f"n_{name}"][0]) for name in _lib.AXIS_STATUS_NAMES}
    assert info["counts"] == [counts] and counts["applied"] >= 100 and counts["too_large"] >= 10 and counts["malformed"] == 0
    worst = {"R": 0.0, "t": 0.0, "deg": 0.0, "t64": 0.0}
    for k, r in enumerate(order):   # k: the table's row, r: the measurement
        st = int(want_axis["status"][k])
        for f in ("i1", "i2", "prob", "y_hat", "y_true"):
            assert getattr(aligned, f)[r] == getattr(meas, f)[r]
        if st in (ac.APPLIED, ac.TOO_LARGE):
            worst["deg"] = max(worst["deg"], abs(info["correction_deg"][r] - want_axis["correction_deg"][k]) / ac.E_DEG)
        else:
            assert np.isnan(info["correction_deg"][r])
        if st != ac.APPLIED:   # a bit-identical copy
            assert aligned.R[r].tobytes() == meas.R[r].tobytes() and aligned.t[r].tobytes() == meas.t[r].tobytes() and aligned.s[r] == meas.s[r]
            assert np.isnan(info["theta_deg"][r]) and np.isnan(info["t"][r]).all()
            continue
        tol_R, tol_t, tol_deg, tol_t64 = ac.tolerances(floor.case["rows"][k], floor.details[k]["lever"], want_axis["t"][k])
        d = lambda a, b: float(np.abs(np.asarray(a, dtype=np.float64).reshape(-1) - np.asarray(b, dtype=np.float64).reshape(-1)).max())
        dth = abs(info["theta_deg"][r] - want_axis["theta_deg"][k])
        worst["R"] = max(worst["R"], d(aligned.R[r], want_rows["R"][k]) / tol_R)
        worst["t"] = max(worst["t"], d(aligned.t[r], want_rows["t"][k]) / tol_t)
        worst["deg"] = max(worst["deg"], min(dth, abs(dth - 360.0)) / tol_deg)
        worst["t64"] = max(worst["t64"], d(info["t"][r], want_axis["t"][k]) / tol_t64)
        assert aligned.s[r] == 1.0
    print(f"ZInD 0000 floor_01, {n} rows, {counts}: largest difference / tolerance {worst}")
    assert max(worst.values()) <= 1.0, worst


def strip(doc):
    """A solution's JSON without the keys axis alignment adds."""
    doc = json.loads(json.dumps(doc))
    for d in (doc, doc.get("tree", {})):
        d.get("options", {}).pop("axis_alignment", None)
        for e in d.get("edges", []):
            e.pop("axis_status"), e.pop("axis_correction_deg")
    doc.get("pgo", {}).pop("axis_counts", None)
    return doc


def test_solve_and_optimise_read_the_aligned_table_on_the_device(floor):
    meas, axis, aligned, info = floor.meas, floor.axis, floor.aligned, floor.info
    (sol,) = pg.solve(meas, THRESHOLD, device=DEV, axis=axis, **OPTS)
    (two_step,) = pg.solve(aligned, THRESHOLD, device=DEV, **OPTS)
    assert json.dumps(strip(sol.to_json())) == json.dumps(two_step.to_json())
    assert sol.options["axis_alignment"] is True and "axis_alignment" not in two_step.options and sol.counts["n_chosen"] > 20
    for pair, e in sol.edges.items():
        r = e["row"]
        assert e["axis_status"] == _lib.AXIS_STATUS_NAMES[info["status"][r]]
        assert e["axis_correction_deg"] == (float(info["correction_deg"][r]) if np.isfinite(info["correction_deg"][r]) else None)
        assert sol.i2Si1[pair].rotation.tobytes() == aligned.R[r].tobytes() and sol.i2Si1[pair].translation.tobytes() == aligned.t[r].tobytes()
    assert {e["axis_status"] for e in sol.edges.values()} >= {"applied", "too_large"}
    assert pg.FloorSolution.from_json(json.loads(json.dumps(sol.to_json()))).to_json() == sol.to_json()
    (with_filter,) = pg.solve(meas, THRESHOLD, device=DEV, axis=axis)   # the cycle filter then sees the aligned poses
    (two_step_filter,) = pg.solve(aligned, THRESHOLD, device=DEV)
    assert json.dumps(strip(with_filter.to_json())) == json.dumps(two_step_filter.to_json())

    (pgo,) = pg.optimise(meas, THRESHOLD, device=DEV, axis=axis, **OPTS)
    (pgo_two_step,) = pg.optimise(aligned, THRESHOLD, device=DEV, **OPTS)
    assert json.dumps(strip(pgo.to_json())) == json.dumps(pgo_two_step.to_json())
    assert pgo.record["axis_counts"] == info["counts"][0] and pgo.record["n_factors"] > 20 and "axis_counts" not in pgo_two_step.record
    assert pg.PgoSolution.from_json(json.loads(json.dumps(pgo.to_json()))).to_json() == pgo.to_json()
    (ran,) = pg.run(meas, THRESHOLD, method="pgo", device=DEV, axis=axis, **OPTS)
    assert json.dumps(ran.to_json()) == json.dumps(pgo.to_json())

    # the alignment changes the answer: it is not a no-op on this floor
    (raw,) = pg.solve(meas, THRESHOLD, device=DEV, **OPTS)
    assert json.dumps(raw.to_json()) != json.dumps(two_step.to_json())


def test_without_axis_nothing_changes(floor):
    (sol,) = pg.solve(floor.meas, THRESHOLD, device=DEV, **OPTS)
    (pgo,) = pg.optimise(floor.meas, THRESHOLD, device=DEV, **OPTS)
    (ran,) = pg.run(floor.meas, THRESHOLD, method="pgo", device=DEV, axis=None, **OPTS)
    text = json.dumps([sol.to_json(), pgo.to_json(), ran.to_json()])
    assert "axis" not in text and json.dumps(ran.to_json()) == json.dumps(pgo.to_json())


def test_keep_rows_and_the_edge_filter_compose(floor):
    meas, axis = floor.meas, floor.axis
    keep = np.arange(len(meas)) % 4 != 1
    part, info = pg.align_rows(meas, axis, DEV, keep_rows=keep)
    assert (info["status"][~keep] == -1).all() and info["status"][keep].tolist() == floor.info["status"][keep].tolist()
    assert part.R[keep].tobytes() == floor.aligned.R[keep].tobytes() and part.R[~keep].tobytes() == meas.R[~keep].tobytes()
    (kept,) = pg.solve(meas, THRESHOLD, device=DEV, keep_rows=keep, axis=axis, **OPTS)
    (two_step,) = pg.solve(floor.aligned, THRESHOLD, device=DEV, keep_rows=keep, **OPTS)
    assert json.dumps(strip(kept.to_json())) == json.dumps(two_step.to_json()) and kept.counts["n_rows"] == int(keep.sum())
    # the random-spanning-trees filter samples the RAW rows; the alignment follows it
    sampling = {"num_hypotheses": 6, "sampling_fraction": 0.5, "seed": 2}
    (filtered,) = pg.run(meas, THRESHOLD, method="pgo", filter_by_random_spanning_trees=True, device=DEV, axis=axis, **sampling, **OPTS)
    mask = pg.combined_inlier_mask(pg.sample_trees(meas, THRESHOLD, device=DEV, **sampling))
    (direct,) = pg.optimise(meas, THRESHOLD, keep_rows=mask, device=DEV, axis=axis, **OPTS)
    assert filtered.options.pop("filter_by_random_spanning_trees") == sampling and json.dumps(filtered.to_json()) == json.dumps(direct.to_json())
    with pytest.raises(ValueError, match="random_spanning_trees takes no axis alignment"):
        pg.run(meas, THRESHOLD, method="random_spanning_trees", device=DEV, axis=axis)


def test_score_floor_passes_the_inputs_through(tmp_path):
    from salve_amd import ingest, synthetic
    from salve_amd.models.early_fusion import EarlyFusionCEResnet
    from tests.test_gpu_hypotheses_floor import synthetic_floor_input
    from tests.test_gpu_ingest import make_floor

    raw, depth_root, _, _ = make_floor(tmp_path, n_panos=3, n_hyp=3)
    fi = synthetic_floor_input()
    fi.vanishing_angle_deg = np.array([3.0, -2.0, np.nan])
    (hyps,) = hypotheses.generate([fi], DEV)
    axis = pg.AxisInputs.from_floors([fi])
    torch.manual_seed(3)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"])).eval()
    synthetic.trained_looking_batchnorm(model)
    with torch.no_grad():
        model.fc.bias.copy_(torch.tensor([-20.0, 20.0]))   # every pair a match
    out = ingest.score_floor(model, torch.device(DEV), str(raw), str(depth_root), str(tmp_path / "no_such_directory"), str(tmp_path / "bev"), "0003",
                             "floor_01", str(tmp_path / "preds"), batch_size=4, chunk=4, hypotheses=hyps,
                             pose_graph={"confidence_threshold": 0.5, "cycle_filter": False, "axis": axis})
    sol = out["pose_graph"]
    doc = json.load(open(tmp_path / "preds" / "pose_graph_0003_floor_01.json"))
    assert doc == json.loads(json.dumps(sol.to_json())) and doc["options"]["axis_alignment"] is True and len(doc["edges"]) >= 1
    names = {e["axis_status"] for e in doc["edges"]}
    assert names <= set(_lib.AXIS_STATUS_NAMES) and all("axis_correction_deg" in e for e in doc["edges"])
    for e in doc["edges"]:   # panorama 5 has no angle
        assert (e["axis_status"] == "no_angle") == (5 in (e["i1"], e["i2"])), e
