"""The floor report on whole floors, on the GPU: ZInD building 1210, floor_02 (tests/golden/zind_1210_floor_02.json) end to end through
salve_amd.floor_report.report against the numbers the reference's test records and the emulator's IoU counts; pose_graph.run(..., truth=) and
the command line's --zind-root against the functions they stand for; ingest.score_floor(pose_graph={..., "truth": ...}); and, without the new
keywords, the results and files as they were."""

import json
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import floor_report as fr  # noqa: E402
from salve_amd import pose_graph as pg  # noqa: E402
from salve_amd.common.sim2 import Sim2  # noqa: E402
from tests import floor_report_cases as fc  # noqa: E402
from tests.test_gpu_floor_report import F64_ATOL  # noqa: E402

DEV = "cuda:0"
G = fc.GUARD
OPTS = {"confidence_threshold": 0.5, "cycle_filter": False}
POSE_NAME, REPORT_NAME = "pose_graph_1210_floor_02.json", "floor_report_1210_floor_02.json"


def test_1210_floor_end_to_end(golden_dir):
    d, truth, wSi = fc.golden_1210(golden_dir)
    (rep,) = fr.report([wSi], [truth], device=DEV)
    want = d["reference_expects"]
    print(f"1210 floor_02 on the device: {rep!r}; IoU {rep.counts['iou_inter']} / {rep.counts['iou_union']}")
    assert abs(rep.avg_abs_rot_err - 1.37) <= 1e-2 == want["avg_abs_rot_err"][1]
    assert abs(rep.avg_abs_trans_err - 0.19) <= 2e-2 == want["avg_abs_trans_err"][1]
    assert abs(rep.percent_panos_localized - 13 / 19 * 100) <= 1e-2 and (rep.counts["n_est"], rep.counts["n_gt"], rep.counts["n_hyps"]) == (13, 19, 1000)
    # the emulator: the pick and the IoU counts exactly, the errors within the measured tolerance, the aligned poses within a float32 ulp
    _, align, iou, _ = fc.emulated_1210(str(golden_dir))
    fo, io, nodes = align[4][G], iou[0][G], align[1][G:-G]
    assert rep.best == fo["best"] == d["emulator"]["best"]
    assert abs(rep.avg_abs_rot_err - fo["avg_rot_err"]) <= F64_ATOL and abs(rep.avg_abs_trans_err - fo["avg_trans_err"]) <= F64_ATOL
    assert np.allclose(rep.rotation_errors, align[2][G:-G], rtol=0, atol=F64_ATOL, equal_nan=True)
    assert np.allclose(rep.translation_errors, align[3][G:-G], rtol=0, atol=F64_ATOL, equal_nan=True)
    assert np.isnan(rep.rotation_errors).sum() == 6 and rep.pano_ids.tolist() == truth.pano_ids.tolist()
    assert (rep.counts["iou_n_est"], rep.counts["iou_n_gt"], rep.counts["iou_inter"], rep.counts["iou_union"]) == (io["n_est"], io["n_gt"], io["inter"], io["uni"])
    assert (rep.counts["iou_inter"], rep.counts["iou_union"]) == (4707, 5514) and rep.floorplan_iou == io["iou"]
    for k, p in enumerate(truth.pano_ids):
        S = rep.aligned_wSi_list[int(p)]
        assert (S is not None) == bool(nodes["localized"][k]) == (wSi[int(p)] is not None)
        if S is not None:
            assert np.all(np.abs(S.rotation.reshape(4) - nodes["R"][k]) <= np.spacing(np.abs(nodes["R"][k])))
            assert np.all(np.abs(S.translation - nodes["t"][k]) <= np.spacing(np.abs(nodes["t"][k]))) and S.scale == truth.gt_scale
    assert set(rep.wSi_dict) == {i for i, S in enumerate(wSi) if S is not None}
    assert fr.FloorReport.from_json(json.loads(json.dumps(rep.to_json()))).to_json() == rep.to_json()
    (again,) = fr.report([wSi], [truth], device=DEV)
    assert json.dumps(again.to_json()) == json.dumps(rep.to_json())   # the same bytes on every run


def test_floors_without_a_pose_and_summary(golden_dir):
    """A floor with no pose is reported NaN, NaN, 0, 0 (run_sfm.py:309-311); the summary takes nanmean and nanmedian."""
    _, truth, wSi = fc.golden_1210(golden_dir)
    reps = fr.report([None, wSi, [None] * 35], [truth, truth, truth], num_iters=50, seed=3, device=DEV)
    for r in (reps[0], reps[2]):
        assert np.isnan(r.avg_abs_rot_err) and np.isnan(r.avg_abs_trans_err) and r.percent_panos_localized == 0.0 and r.floorplan_iou == 0.0
        assert r.best is None and r.wSi_dict == {} and r.counts["iou_n_gt"] == 5371
    s = fr.summarize(reps)
    assert s["avg_abs_rot_err"]["mean"] == reps[1].avg_abs_rot_err and s["percent_panos_localized"]["median"] == 0.0
    assert abs(s["floorplan_iou"]["mean"] - reps[1].floorplan_iou / 3) < 1e-15
    with pytest.raises(ValueError, match="does not hold"):
        fr.report([[Sim2(np.eye(2), np.zeros(2), 1.0)]], [truth], device=DEV)


@pytest.fixture(scope="module")
def floor(tmp_path_factory, golden_dir):
    """Prediction and hypothesis files of the 1210 floor: the true relative poses of a chain of its panoramas and two loops, lightly disturbed."""
    tmp = tmp_path_factory.mktemp("floor_report_floor")
    _, truth, _ = fc.golden_1210(golden_dir)
    (tmp / "zind" / "1210").mkdir(parents=True)
    shutil.copy(golden_dir / "zind_1210_floor_02.json", tmp / "zind" / "1210" / "zind_data.json")
    rng = np.random.default_rng(5)
    ids = [int(p) for p in truth.pano_ids[:10]]
    pairs = [(ids[k], ids[k + 1]) for k in range(9)] + [(ids[0], ids[4]), (ids[3], ids[8])]
    wS = {int(p): Sim2(truth.R[k], truth.t[k], 1.0) for k, p in enumerate(truth.pano_ids)}
    fp0, fp1 = [], []
    for k, (i1, i2) in enumerate(pairs):
        rel = wS[i2].inverse().compose(wS[i1])
        th = rng.normal(0, 0.01)
        noise = Sim2(np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]), rng.normal(0, 0.02, 2), 1.0)
        noise.compose(rel).save_as_json(str(tmp / "hyp" / "1210" / "floor_02" / "gt_alignment_approx" / f"{i1}_{i2}__door_0_0_identity.json"))
        stem = f"{tmp}/bev/gt_alignment_approx/1210/pair_{k}___door_0_0_identity_floor_rgb_floor_02_partial_room_01_pano_"
        fp0.append(f"{stem}{i1}.jpg")
        fp1.append(f"{stem}{i2}.jpg")
    (tmp / "preds").mkdir()
    n = len(pairs)
    (tmp / "preds" / "batch_0.json").write_text(json.dumps({"y_hat": [1] * n, "y_true": [1] * n, "y_hat_probs": [0.9] * n, "fp0": fp0, "fp1": fp1}))
    meas = pg.EdgeMeasurements.from_prediction_files(str(tmp / "preds"), str(tmp / "hyp"))
    return tmp, truth, meas


def test_run_takes_the_truth_and_the_command_line_round_trips(floor, capsys):
    tmp, truth, meas = floor
    sols, reps = pg.run(meas, device=DEV, truth=[truth], **OPTS)
    (direct,) = pg.solve(meas, device=DEV, **OPTS)
    assert json.dumps(sols[0].to_json()) == json.dumps(direct.to_json())
    (want,) = fr.report([direct], [truth], device=DEV)
    assert json.dumps(reps[0].to_json()) == json.dumps(want.to_json())
    rep = reps[0]
    assert rep.counts["n_est"] == 10 and abs(rep.percent_panos_localized - 10 / 19 * 100) < 1e-12 and rep.avg_abs_rot_err < 5.0 and rep.avg_abs_trans_err < 1.0
    assert 0.2 < rep.floorplan_iou < 1.0   # (a lightly disturbed chain: sanity only; the values are pinned by the equalities around)
    _, by_key = pg.run(meas, device=DEV, truth={("1210", "floor_02"): truth}, report_options={"num_iters": 1000, "seed": 0}, **OPTS)
    assert json.dumps(by_key[0].to_json()) == json.dumps(rep.to_json())
    _, other = pg.run(meas, device=DEV, truth=[truth], report_options={"num_iters": 20, "seed": 4}, **OPTS)
    assert other[0].counts["n_hyps"] == 20

    assert pg.main([str(tmp / "preds"), "--hypotheses", str(tmp / "hyp"), "--confidence-threshold", "0.5", "--no-cycle-filter", "--device", DEV,
                    "--zind-root", str(tmp / "zind"), "--out", str(tmp / "cli")]) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines[0] == direct.summary() and lines[1] == rep.summary() and json.loads(lines[2]) == json.loads(json.dumps(fr.summarize([rep])))
    assert sorted(f.name for f in (tmp / "cli").iterdir()) == sorted([POSE_NAME, REPORT_NAME])
    doc = json.load(open(tmp / "cli" / REPORT_NAME))
    assert doc == json.loads(json.dumps(rep.to_json())) and fr.FloorReport.from_json(doc).to_json() == rep.to_json()
    assert pg.main([str(tmp / "preds"), "--hypotheses", str(tmp / "hyp"), "--confidence-threshold", "0.5", "--no-cycle-filter", "--device", DEV,
                    "--zind-root", str(tmp / "zind"), "--report-seed", "4", "--report-iters", "20", "--out", str(tmp / "cli20")]) == 0
    capsys.readouterr()
    assert json.load(open(tmp / "cli20" / REPORT_NAME)) == json.loads(json.dumps(other[0].to_json()))


def test_without_the_new_keywords_results_and_files_are_as_before(floor, capsys):
    tmp, truth, meas = floor
    plain = pg.run(meas, device=DEV, **OPTS)
    (direct,) = pg.solve(meas, device=DEV, **OPTS)
    assert isinstance(plain, list) and len(plain) == 1 and json.dumps(plain[0].to_json()) == json.dumps(direct.to_json())
    assert pg.main([str(tmp / "preds"), "--hypotheses", str(tmp / "hyp"), "--confidence-threshold", "0.5", "--no-cycle-filter", "--device", DEV,
                    "--out", str(tmp / "cli_plain")]) == 0
    assert capsys.readouterr().out.strip() == direct.summary()
    assert [f.name for f in (tmp / "cli_plain").iterdir()] == [POSE_NAME]
    pg.write_json(direct, str(tmp / "direct"))
    assert (tmp / "cli_plain" / POSE_NAME).read_bytes() == (tmp / "direct" / POSE_NAME).read_bytes()
    assert sorted(json.load(open(tmp / "cli_plain" / POSE_NAME))) == ["building_id", "counts", "edges", "floor_id", "options", "origin", "pano_ids", "poses"]


def test_score_floor_takes_the_truth(tmp_path):
    """ingest.score_floor(pose_graph={..., "truth": ...}) on the synthetic floor of tests/test_gpu_ingest.py (panoramas 3, 4, 5): the report
    follows the pose graph; without the key the result and the files are as they were."""
    from types import SimpleNamespace

    from salve_amd import ingest, synthetic
    from salve_amd.models.early_fusion import EarlyFusionCEResnet
    from tests.test_gpu_ingest import make_floor

    raw, depth_root, hyp_root, _ = make_floor(tmp_path, n_panos=3, n_hyp=3)
    torch.manual_seed(3)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"])).eval()
    synthetic.trained_looking_batchnorm(model)
    with torch.no_grad():
        model.fc.bias.copy_(torch.tensor([-20.0, 20.0]))   # every pair a match
    square = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])
    truth = fr.FloorTruth("0003", "floor_01", np.array([3, 4, 5]), np.tile(np.eye(2), (3, 1, 1)), np.array([[0.0, 0.0], [1.5, 0.0], [0.0, 2.0]]), np.ones(3),
                          [square] * 3, 2.0, 1.0)
    score = lambda out, pose_graph: ingest.score_floor(model, torch.device(DEV), str(raw), str(depth_root), str(hyp_root), str(tmp_path / "bev"), "0003",
                                                       "floor_01", str(tmp_path / out), batch_size=2, chunk=4, pose_graph=pose_graph)
    plain = score("preds_plain", dict(OPTS))
    with_truth = score("preds_truth", {**OPTS, "truth": truth, "report": {"num_iters": 10, "seed": 2}})
    assert "floor_report" not in plain and sorted(plain) == sorted(k for k in with_truth if k != "floor_report")
    rep = with_truth["floor_report"]
    (want,) = fr.report([with_truth["pose_graph"]], [truth], num_iters=10, seed=2, device=DEV)
    assert json.dumps(rep.to_json()) == json.dumps(want.to_json()) and rep.counts["n_gt"] == 3 and rep.counts["n_est"] == with_truth["pose_graph"].counts["n_localized"]
    name = "floor_report_0003_floor_01.json"
    assert json.load(open(tmp_path / "preds_truth" / name)) == json.loads(json.dumps(rep.to_json()))
    assert sorted(f.name for f in (tmp_path / "preds_truth").iterdir()) == sorted([f.name for f in (tmp_path / "preds_plain").iterdir()] + [name])
    for f in (tmp_path / "preds_plain").iterdir():   # the key changes no other file
        assert f.read_bytes() == (tmp_path / "preds_truth" / f.name).read_bytes(), f.name
