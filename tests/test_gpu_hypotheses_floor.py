"""Alignment hypotheses from the device straight into scoring, on the synthetic floor of tests/test_gpu_ingest.py (panoramas 3, 4, 5) with
W/D/Os from salve_amd.synthetic_layouts: ingest.score_floor(..., hypotheses=generate(...)) writes the prediction files (and the pose graph)
that score_floor writes when it reads write_tree's directory, without touching a hypothesis file; hypotheses=None is the call as it was; and
the command line on the fixture tree (ZInD 0000 floor_01) writes the 2672 files ingest.load_floor_hypotheses reads."""

import inspect
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import hypotheses, ingest, synthetic, synthetic_layouts  # noqa: E402
from salve_amd.layout import PanoLayouts  # noqa: E402
from tests import hypotheses_cases as hc  # noqa: E402
from tests.test_gpu_ingest import make_floor  # noqa: E402

DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden"
OPTIONS = {"confidence_threshold": 0.5, "cycle_filter": False}


def synthetic_floor_input():
    """Panoramas 3, 4, 5 of building 0003: the first three synthetic layouts that carry W/D/Os, two W/D/Os of each at the most (a handful of
    hypotheses), every type present turned into doors and windows alternately so that the pairs share types; near-identity ground truth."""
    specs = [s for s in synthetic_layouts.make_layout_specs(12, seed=0) if len(s[1]) >= 2][:3]
    assert len(specs) == 3
    specs = [(room, [(("doors", "windows")[k % 2], v) for k, (_, v) in enumerate(wdos[:2])]) for room, wdos in specs]
    poses = [(hc.rot(5.0 * k), [0.3 * k, 0.1 * k], 1.0) for k in range(3)]
    gt = [[np.asarray(v).tolist() for _, v in wdos] for _, wdos in specs]
    return hypotheses.FloorInput("0003", "floor_01", np.array([3, 4, 5]), PanoLayouts.from_specs(specs), np.array([p[0] for p in poses]),
                                 np.array([p[1] for p in poses], dtype=np.float32), np.array([p[2] for p in poses]),
                                 np.concatenate([[0], np.cumsum([len(g) for g in gt])]), np.array([s for g in gt for s in g]).reshape(-1, 2, 2))


@pytest.fixture(scope="module")
def floor(tmp_path_factory):
    from salve_amd.models.early_fusion import EarlyFusionCEResnet

    tmp = tmp_path_factory.mktemp("hypotheses_floor")
    raw, depth_root, _, _ = make_floor(tmp, n_panos=3, n_hyp=3)
    tree = tmp / "generated"
    (hyps,) = hypotheses.generate([synthetic_floor_input()], DEV, hypotheses_save_root=str(tree))
    assert 3 <= len(hyps) <= 12 and hyps.pairs is not None and len(hyps.pairs.i1) == 3
    torch.manual_seed(3)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"])).eval()
    synthetic.trained_looking_batchnorm(model)
    with torch.no_grad():
        model.fc.bias.copy_(torch.tensor([-20.0, 20.0]))
    score = lambda out, root, **kw: ingest.score_floor(model, torch.device(DEV), str(raw), str(depth_root), str(root), str(tmp / "bev"), "0003", "floor_01",
                                                       str(tmp / out), batch_size=4, chunk=4, **kw)
    # straight from the device FIRST, while the tree does not exist: nothing can be read from it
    direct = score("preds_direct", tmp / "no_such_directory", hypotheses=hyps, pose_graph=OPTIONS)
    assert not tree.exists() and not (tmp / "no_such_directory").exists()
    assert hypotheses.write_tree([hyps], tree) == len(hyps)
    return SimpleNamespace(tmp=tmp, tree=tree, hyps=hyps, direct=direct, files=score("preds_files", tree, pose_graph=OPTIONS),
                           plain=score("preds_plain", tree, hypotheses=None))


def test_scoring_generated_hypotheses_equals_scoring_their_files(floor):
    back = ingest.load_floor_hypotheses(str(floor.tree), "0003", "floor_01")
    assert back.fpaths == floor.hyps.fpaths and back.R.tobytes() == floor.hyps.R.tobytes() and back.t.tobytes() == floor.hyps.t.tobytes()
    assert back.label.tolist() == floor.hyps.label.tolist() and back.pair_idx.tolist() == floor.hyps.pair_idx.tolist()
    names = sorted(f.name for f in (floor.tmp / "preds_files").iterdir())
    assert names == sorted(f.name for f in (floor.tmp / "preds_direct").iterdir()) and "pose_graph_0003_floor_01.json" in names and len(names) >= 2
    for n in names:
        assert (floor.tmp / "preds_files" / n).read_bytes() == (floor.tmp / "preds_direct" / n).read_bytes(), n
    same = lambda d: json.dumps({k: (v.to_json() if k == "pose_graph" and v is not None else v) for k, v in d.items()}, sort_keys=True, default=str)
    assert same(floor.files) == same(floor.direct)
    scored = sum(len(json.load(open(floor.tmp / "preds_direct" / n))["y_true"]) for n in names if n.startswith("batch_"))
    assert scored == len(floor.hyps)


def test_without_the_keyword_nothing_changes(floor):
    assert inspect.signature(ingest.score_floor).parameters["hypotheses"].default is None
    names = sorted(f.name for f in (floor.tmp / "preds_plain").iterdir())
    assert names and all(n.startswith("batch_") for n in names)
    for n in names:
        assert (floor.tmp / "preds_plain" / n).read_bytes() == (floor.tmp / "preds_files" / n).read_bytes(), n
    assert "pose_graph" not in floor.plain and "rows" not in floor.plain


def test_command_line_writes_the_fixture_floors_2672_files(tmp_path, capsys):
    raw, root = hc.expand_fixture(GOLDEN, tmp_path)
    out = tmp_path / "out"
    assert hypotheses.main(["--raw-dataset-dir", raw, "--mhnet-predictions-data-root", root, "--hypotheses-save-root", str(out), "--buildings", "0000",
                            "--device", DEV]) == 0
    printed = capsys.readouterr().out
    rec = json.loads((GOLDEN / hc.GOLDEN_RESULT).read_text())
    assert f"floor_n_valid_configurations: {rec['n_valid_configurations']}, floor_n_invalid_configurations: {rec['n_invalid_configurations']}" in printed
    assert "GT is-valid frac. over 496 alignment pairs" in printed and "wrote 2672 hypothesis files" in printed
    files = [p for d in hc.LABEL_DIRS for p in (out / "0000" / "floor_01" / d).glob("*.json")]
    assert len(files) == 2672 and len(list((out / "0000" / "floor_01" / "gt_alignment_exact").glob("*.json"))) == len(rec["visibly_adjacent"])
    back = ingest.load_floor_hypotheses(str(out), "0000", "floor_01")
    assert len(back) == 2672 and int(back.label.sum()) == 117
    assert [[hc.LABEL_DIRS[0] if l else hc.LABEL_DIRS[1], Path(fp).name] for l, fp in zip(back.label, back.fpaths)] == hc.recorded_names(rec)
    assert hc.digest([(None, None, None, None, back.R[k].reshape(4), back.t[k]) for k in range(len(back))]) == rec["digest_R_t"]
