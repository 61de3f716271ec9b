"""`--method pgo` on a whole floor, on the GPU: prediction and hypothesis files of a small synthetic floor (ten panoramas of ZInD 1210's floor_02
truth, noisy relative poses, second hypotheses, loop closures, three confident false positives: tests/pgo_cases.py) go through
`python -m salve_amd.pose_graph ... --method pgo` in a fresh child process; the written files equal what pose_graph.optimise and
floor_report.report return; the report's mean translation error of the optimised poses is below the spanning tree's (the floor was chosen on the
CPU so that it is, with room to spare: pgo_cases.FLOOR_TREE_ERR, FLOOR_PGO_ERR); run(method="pgo") with the random-spanning-trees edge filter
uses the kept rows only; ingest.score_floor(pose_graph={"method": "pgo"}) writes the file the command line writes."""

import json
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import floor_report as fr  # noqa: E402
from salve_amd import pose_graph as pg  # noqa: E402
from salve_amd.common.sim2 import Sim2  # noqa: E402
from tests import floor_report_cases as fc  # noqa: E402
from tests import pgo_cases as pc  # noqa: E402

DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
POSE_NAME, REPORT_NAME = "pose_graph_1210_floor_02.json", "floor_report_1210_floor_02.json"
OPTS = {"confidence_threshold": 0.5, "cycle_filter": False}


@pytest.fixture(scope="module")
def floor(tmp_path_factory, golden_dir):
    tmp = tmp_path_factory.mktemp("pgo_floor")
    _, truth, _ = fc.golden_1210(golden_dir)
    (tmp / "zind" / "1210").mkdir(parents=True)
    shutil.copy(golden_dir / "zind_1210_floor_02.json", tmp / "zind" / "1210" / "zind_data.json")
    meas, _ = pc.floor_measurements(truth)
    doc = {"y_hat": [], "y_true": [], "y_hat_probs": [], "fp0": [], "fp1": []}
    for k, (i1, i2, prob, y_hat, y_true, (x, y, th)) in enumerate(meas):
        label = "gt_alignment_approx" if y_true else "incorrect_alignment"
        Sim2(np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]), np.array([x, y]), 1.0).save_as_json(
            str(tmp / "hyp" / "1210" / "floor_02" / label / f"{i1}_{i2}__door_{k}_0_identity.json"))
        stem = f"{tmp}/bev/{label}/1210/pair_{k}___door_{k}_0_identity_floor_rgb_floor_02_partial_room_01_pano_"
        for key, v in (("y_hat", y_hat), ("y_true", y_true), ("y_hat_probs", prob), ("fp0", f"{stem}{i1}.jpg"), ("fp1", f"{stem}{i2}.jpg")):
            doc[key].append(v)
    (tmp / "preds").mkdir()
    (tmp / "preds" / "batch_0.json").write_text(json.dumps(doc))
    return tmp, truth, pg.EdgeMeasurements.from_prediction_files(str(tmp / "preds"), str(tmp / "hyp"))


def test_the_command_line_in_a_child_process_writes_what_optimise_returns(floor):
    tmp, truth, meas = floor
    (sol,) = pg.optimise(meas, device=DEV, **OPTS)
    child = subprocess.run([sys.executable, "-m", "salve_amd.pose_graph", str(tmp / "preds"), "--hypotheses", str(tmp / "hyp"), "--confidence-threshold", "0.5",
                            "--no-cycle-filter", "--method", "pgo", "--zind-root", str(tmp / "zind"), "--out", str(tmp / "cli"), "--device", DEV],
                           cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    assert sorted(f.name for f in (tmp / "cli").iterdir()) == sorted([POSE_NAME, REPORT_NAME])
    doc = json.load(open(tmp / "cli" / POSE_NAME))
    assert doc == json.loads(json.dumps(sol.to_json())) and pg.json_fname(sol) == POSE_NAME
    back = pg.PgoSolution.from_json(doc)
    assert back.to_json() == sol.to_json() and back.tree.to_json() == sol.tree.to_json()
    lines = child.stdout.strip().split("\n")
    assert lines[0] == sol.summary()

    # the solution itself: the tree as solve returns it, every thresholded prediction between localized panoramas a factor, float32 poses of the float64
    (tree,) = pg.solve(meas, device=DEV, **OPTS)
    assert json.dumps(sol.tree.to_json()) == json.dumps(tree.to_json())
    assert sol.options["method"] == "pgo" and sol.options["robust"] is True and sol.options["cycle_filter"] is False
    n_factors = 1 + int(((meas.y_hat == 1) & (meas.prob >= np.float32(0.5))).sum())
    assert sol.record["n_factors"] == n_factors == 28 and sol.record["n_unknown_nodes"] == tree.counts["n_localized"] == 10
    assert sol.record["cost_final"] < sol.record["cost_initial"] and sol.record["n_downweighted"] >= 3 and sol.record["stop_reason"] in pg._lib.PGO_STOP_NAMES[1:3]
    assert len(sol.wSi_list) == len(tree.wSi_list) and [S is None for S in sol.wSi_list] == [S is None for S in tree.wSi_list]
    for p, S in enumerate(sol.wSi_list):
        if S is not None:
            x, y, th = sol.pose[p]
            assert S.translation.tobytes() == np.array([x, y]).astype(np.float32).tobytes() and S.scale == 1.0
            assert S.rotation.tobytes() == np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]).astype(np.float32).tobytes()

    # the report accepts it as it stands; the optimised poses beat the tree's, as chosen on the CPU
    (rep,) = fr.report([sol], [truth], device=DEV)
    (rep_tree,) = fr.report([tree], [truth], device=DEV)
    assert json.load(open(tmp / "cli" / REPORT_NAME)) == json.loads(json.dumps(rep.to_json())) and lines[1] == rep.summary()
    print(f"mean translation error: spanning tree {rep_tree.avg_abs_trans_err:.4f} m, pgo {rep.avg_abs_trans_err:.4f} m "
          f"(CPU, laid on the truth by the origin, in coordinates: {pc.FLOOR_TREE_ERR}, {pc.FLOOR_PGO_ERR}); rotation {rep_tree.avg_abs_rot_err:.3f} -> "
          f"{rep.avg_abs_rot_err:.3f} degrees")
    assert pc.FLOOR_PGO_ERR < 0.5 * pc.FLOOR_TREE_ERR
    assert rep.avg_abs_trans_err < rep_tree.avg_abs_trans_err and rep.counts["n_est"] == rep_tree.counts["n_est"] == 10
    (again, again_rep) = pg.run(meas, device=DEV, method="pgo", truth=[truth], **OPTS)
    assert json.dumps(again[0].to_json()) == json.dumps(sol.to_json()) and json.dumps(again_rep[0].to_json()) == json.dumps(rep.to_json())


def test_the_optimisers_switches_and_the_edge_filter(floor, capsys):
    tmp, _, meas = floor
    assert pg.main([str(tmp / "preds"), "--hypotheses", str(tmp / "hyp"), "--confidence-threshold", "0.5", "--no-cycle-filter", "--method", "pgo",
                    "--pgo-max-iterations", "2", "--pgo-no-robust", "--out", str(tmp / "cli2"), "--device", DEV]) == 0
    (want,) = pg.optimise(meas, 0.5, robust=False, max_iterations=2, cycle_filter=False, device=DEV)
    assert capsys.readouterr().out.strip() == want.summary()
    assert json.load(open(tmp / "cli2" / POSE_NAME)) == json.loads(json.dumps(want.to_json()))
    assert want.record["n_iterations"] == 2 and want.record["stop_reason"] == "max_iterations" and want.record["n_downweighted"] == 0
    # behind the random-spanning-trees filter the factors are the kept rows only
    sampling = {"num_hypotheses": 8, "sampling_fraction": 0.5, "seed": 1}
    (filtered,) = pg.run(meas, 0.5, method="pgo", filter_by_random_spanning_trees=True, cycle_filter=False, device=DEV, **sampling)
    keep = pg.combined_inlier_mask(pg.sample_trees(meas, 0.5, device=DEV, **sampling))
    (direct,) = pg.optimise(meas, 0.5, keep_rows=keep, cycle_filter=False, device=DEV)
    assert filtered.options.pop("filter_by_random_spanning_trees") == sampling and json.dumps(filtered.to_json()) == json.dumps(direct.to_json())
    assert filtered.tree.counts["n_rows"] == int(keep.sum()) < len(meas) and filtered.record["n_factors"] <= 1 + int(keep.sum())
    # with the cycle filter on, the tree is the filtered one and the factors still every thresholded prediction between its panoramas
    (cyc,) = pg.optimise(meas, 0.5, device=DEV)
    (cyc_tree,) = pg.solve(meas, 0.5, device=DEV)
    assert json.dumps(cyc.tree.to_json()) == json.dumps(cyc_tree.to_json()) and cyc.record["n_unknown_nodes"] == cyc_tree.counts["n_localized"]


def test_score_floor_writes_the_command_lines_file(tmp_path, capsys):
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
    out = ingest.score_floor(model, torch.device(DEV), str(raw), str(depth_root), str(hyp_root), str(tmp_path / "bev"), "0003", "floor_01",
                             str(tmp_path / "preds"), batch_size=2, chunk=4, pose_graph={**OPTS, "method": "pgo", "max_iterations": 20})
    sol = out["pose_graph"]
    name = "pose_graph_0003_floor_01.json"
    assert isinstance(sol, pg.PgoSolution) and sol.record["n_factors"] >= 2 and sol.options["max_iterations"] == 20
    assert json.load(open(tmp_path / "preds" / name)) == json.loads(json.dumps(sol.to_json()))
    assert pg.main([str(tmp_path / "preds"), "--hypotheses", str(hyp_root), "--confidence-threshold", "0.5", "--no-cycle-filter", "--method", "pgo",
                    "--pgo-max-iterations", "20", "--out", str(tmp_path / "cli"), "--device", DEV]) == 0
    capsys.readouterr()
    assert (tmp_path / "cli" / name).read_bytes() == (tmp_path / "preds" / name).read_bytes()
