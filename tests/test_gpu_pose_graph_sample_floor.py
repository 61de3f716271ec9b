"""Random spanning trees behind scoring, on the synthetic floor of tests/test_gpu_pose_graph_floor.py: pose_graph.sample_trees on the files a
score_floor call wrote, and its winner as solve's keep_rows; ingest.score_floor(pose_graph={"method": "random_spanning_trees", ...}) and the
command line's two new switches against the functions they stand for; and, with no new switch or key, the prediction files and the
pose_graph_*.json of the path as it was, byte for byte."""

import json
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import ingest, synthetic  # noqa: E402
from salve_amd import pose_graph as pg  # noqa: E402
from tests.test_gpu_ingest import make_floor  # noqa: E402

DEV = "cuda:0"
OLD = {"confidence_threshold": 0.5, "cycle_filter": False}
SAMPLING = {"num_hypotheses": 5, "sampling_fraction": 0.5, "seed": 1}
NAME = "pose_graph_0003_floor_01.json"


@pytest.fixture(scope="module")
def floor(tmp_path_factory):
    """The floor on disk (three panoramas, the pairs (3, 5), (4, 5), (3, 4)), scored twice by one model that calls every pair a match: with the
    keys the keyword had before into preds_old, with the new method into preds_rst."""
    from salve_amd.models.early_fusion import EarlyFusionCEResnet

    tmp = tmp_path_factory.mktemp("pose_graph_sample_floor")
    raw, depth_root, hyp_root, _ = make_floor(tmp, n_panos=3, n_hyp=3)
    torch.manual_seed(3)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"])).eval()
    synthetic.trained_looking_batchnorm(model)
    with torch.no_grad():
        model.fc.bias.copy_(torch.tensor([-20.0, 20.0]))
    score = lambda out, **kw: ingest.score_floor(model, torch.device(DEV), str(raw), str(depth_root), str(hyp_root), str(tmp / "bev"), "0003", "floor_01",
                                                 str(tmp / out), batch_size=2, chunk=4, **kw)
    old = score("preds_old", pose_graph=OLD)
    rst = score("preds_rst", pose_graph={"confidence_threshold": 0.5, "method": "random_spanning_trees", **SAMPLING})
    meas = pg.EdgeMeasurements.from_prediction_files(str(tmp / "preds_old"), str(hyp_root))
    return SimpleNamespace(tmp=tmp, hyp_root=hyp_root, old=old, rst=rst, meas=meas)


def test_sample_trees_then_solve_keep_rows(floor):
    meas = floor.meas
    (draw,) = pg.draw_hypotheses(meas, 0.5, **SAMPLING)
    assert len(draw.candidates) == 3 and len(draw.subsets) == 3 and all(len(s) == 2 for s in draw.subsets)   # K = 3, m = 2, binom(3, 2) = 3
    (sample,) = pg.sample_trees(meas, 0.5, device=DEV, **SAMPLING)
    assert isinstance(sample, pg.TreeSampleSolution) and sample.best is not None and sample.counts["n_candidates"] == 3 and sample.counts["n_hyps"] == 3
    assert sample.inlier_rows.tolist() == sorted(draw.candidates[draw.subsets[sample.best]].tolist())     # the reference's best_hypothesis
    assert sample.counts["n_localized"] == 3 and sample.origin == 3 and sample.wSi_list[3].scale == 1.0 and len(sample.wSi_list) == 6
    assert all(h["n_localized"] == 3 and h["n_measured"] == 3 and h["n_edges"] == 2 for h in sample.hypotheses)
    assert sample.avg_trans_err == sample.hypotheses[sample.best]["avg_trans_err"] and np.isfinite(sample.avg_rot_err)
    (again,) = pg.sample_trees(meas, 0.5, hypotheses=[draw], device=DEV, **SAMPLING)
    assert again.to_json() == sample.to_json()
    # the winner's rows as the edge filter in front of the first method
    (filtered,) = pg.solve(meas, device=DEV, keep_rows=sample.inlier_mask, **OLD)
    pairs = {(int(meas.i1[r]), int(meas.i2[r])) for r in sample.inlier_rows}
    assert set(filtered.i2Si1) == pairs and len(pairs) == 2 and filtered.counts["n_rows"] == 2 and filtered.counts["n_nodes"] == 3
    assert {e["row"] for e in filtered.edges.values()} == set(sample.inlier_rows.tolist())               # rows are indices into `meas`
    for p, S in enumerate(filtered.wSi_list):   # two edges, one tree: the filtered solve chains what the winner chained
        assert (S is None) == (sample.wSi_list[p] is None)
        if S is not None:
            assert S.rotation.tobytes() == sample.wSi_list[p].rotation.tobytes() and S.translation.tobytes() == sample.wSi_list[p].translation.tobytes()
    (everything,) = pg.solve(meas, device=DEV, keep_rows=np.ones(len(meas), dtype=bool), **OLD)
    (plain,) = pg.solve(meas, device=DEV, **OLD)
    assert everything.to_json() == plain.to_json() == floor.old["pose_graph"].to_json()
    (nothing,) = pg.solve(meas, device=DEV, keep_rows=np.zeros(len(meas), dtype=bool), **OLD)
    assert nothing.wSi_list is None and nothing.counts["n_rows"] == 0 and nothing.counts["n_nodes"] == 3
    with pytest.raises(ValueError, match="keep_rows"):
        pg.solve(meas, device=DEV, keep_rows=np.ones(len(meas) + 1, dtype=bool), **OLD)


def test_score_floor_takes_the_new_keys(floor):
    sol = floor.rst["pose_graph"]
    assert isinstance(sol, pg.TreeSampleSolution) and (sol.building_id, sol.floor_id) == ("0003", "floor_01")
    (again,) = pg.sample_trees(floor.meas, 0.5, device=DEV, **SAMPLING)
    assert again.to_json() == sol.to_json()
    assert json.load(open(floor.tmp / "preds_rst" / NAME)) == json.loads(json.dumps(sol.to_json()))
    assert pg.TreeSampleSolution.from_json(json.load(open(floor.tmp / "preds_rst" / NAME))).to_json() == sol.to_json()


def test_command_line_round_trips_both_switches(floor, capsys):
    common = [str(floor.tmp / "preds_old"), "--hypotheses", str(floor.hyp_root), "--confidence-threshold", "0.5", "--device", DEV, "--num-hypotheses", "5",
              "--seed", "1"]
    assert pg.main(common + ["--method", "random_spanning_trees", "--out", str(floor.tmp / "cli_rst")]) == 0
    sol = floor.rst["pose_graph"]
    assert capsys.readouterr().out.strip() == sol.summary()
    assert [f.name for f in (floor.tmp / "cli_rst").iterdir()] == [NAME]
    assert (floor.tmp / "cli_rst" / NAME).read_bytes() == (floor.tmp / "preds_rst" / NAME).read_bytes()

    assert pg.main(common + ["--filter-by-random-spanning-trees", "--no-cycle-filter", "--out", str(floor.tmp / "cli_filter")]) == 0
    (want,) = pg.run(floor.meas, filter_by_random_spanning_trees=True, device=DEV, **OLD, **SAMPLING)
    assert capsys.readouterr().out.strip() == want.summary()
    doc = json.load(open(floor.tmp / "cli_filter" / NAME))
    assert doc == json.loads(json.dumps(want.to_json())) and doc["options"]["filter_by_random_spanning_trees"] == SAMPLING
    back = pg.FloorSolution.from_json(doc)
    assert back.to_json() == want.to_json() and len(back.i2Si1) == 2 and back.counts["n_rows"] == 2

    with pytest.raises(SystemExit):
        pg.main(common + ["--method", "random_spanning_trees", "--filter-by-random-spanning-trees"])
    capsys.readouterr()
    with pytest.raises(ValueError, match="random_spanning_trees"):
        pg.run(floor.meas, 0.5, method="random_spanning_trees", cycle_filter=False, device=DEV)


def test_without_a_new_switch_the_files_are_as_before(floor, capsys):
    old, rst = floor.tmp / "preds_old", floor.tmp / "preds_rst"
    names = ["batch_0.json", "batch_1.json"]
    assert sorted(f.name for f in old.iterdir()) == sorted(f.name for f in rst.iterdir()) == names + [NAME]
    for n in names:   # the method changes no prediction file
        assert (old / n).read_bytes() == (rst / n).read_bytes(), n
    assert pg.main([str(old), "--hypotheses", str(floor.hyp_root), "--confidence-threshold", "0.5", "--no-cycle-filter", "--out", str(floor.tmp / "cli_old"),
                    "--device", DEV]) == 0
    assert capsys.readouterr().out.strip() == floor.old["pose_graph"].summary()
    assert (floor.tmp / "cli_old" / NAME).read_bytes() == (old / NAME).read_bytes()
    doc = json.load(open(old / NAME))   # the document as it was: these keys and no other
    assert sorted(doc) == ["building_id", "counts", "edges", "floor_id", "options", "origin", "pano_ids", "poses"]
    assert sorted(doc["options"]) == ["confidence_threshold", "cycle_filter", "rot_threshold_deg", "trans_threshold"]
    (direct,) = pg.solve(floor.meas, device=DEV, **OLD)
    (through_run,) = pg.run(floor.meas, device=DEV, **OLD)
    assert json.dumps(direct.to_json()) == json.dumps(through_run.to_json()) == json.dumps(floor.old["pose_graph"].to_json())
