"""salve_amd.overlap on hand-made prediction files: the binning of scripts/measure_acc_vs_overlap.py:146-167 (linspace's edges, an IoU of
exactly 1.0, an empty bin), the filters of :67-71, the name parsing of :82-108, the pose errors of :126-143 and the command line."""

import json

import numpy as np
import pytest

from salve_amd import overlap
from salve_amd.common.sim2 import Sim2

ROOT = "/data/bev/incorrect_alignment/0668"


def name(pair_idx, uuid, pano, room=1, floor="floor_02", root=ROOT, surface="floor"):
    return f"{root}/pair_{pair_idx}___{uuid}_{surface}_rgb_{floor}_partial_room_{room:02d}_pano_{pano}.jpg"


def write_preds(d, rows, fname="batch_0.json", with_overlap=True):
    """rows: (y_hat, y_true, prob, fp0, fp1, (intersection, union))"""
    d.mkdir(parents=True, exist_ok=True)
    doc = {"y_hat": [r[0] for r in rows], "y_true": [r[1] for r in rows], "y_hat_probs": [r[2] for r in rows], "fp0": [r[3] for r in rows],
           "fp1": [r[4] for r in rows]}
    if with_overlap:
        doc["overlap"] = [list(r[5]) for r in rows]
    (d / fname).write_text(json.dumps(doc, indent=4))


def row(y_hat, y_true, prob, counts, k=0):
    return (y_hat, y_true, prob, name(k, "door_0_1_identity", 4), name(k, "door_0_1_identity", 7, room=3), counts)


def test_binning_follows_the_reference(tmp_path):
    rows = [row(0, 0, 0.9, (3, 10)),           # 0.3 - 3e-14 lies below linspace's 0.30000000000000004: bin 2
            row(1, 0, 0.9, (0, 10)),           # 0.0: bin 0
            row(0, 0, 0.9, (0, 0)),            # empty union: 0 / 1e-12 = 0.0, bin 0
            row(0, 0, 0.9, (20000, 20000)),    # exactly 1.0 in float64: the last bin, and reported
            row(1, 0, 0.9, (10, 10)),          # 10 / (10 + 1e-12) < 1.0: the last bin, not "full"
            row(0, 0, 0.9, (55, 100)), row(0, 0, 0.9, (59, 100)), row(1, 0, 0.9, (52, 100))]
    write_preds(tmp_path, rows[:4])
    write_preds(tmp_path, rows[4:], "batch_1.json")
    r = overlap.measure_acc_vs_visual_overlap(str(tmp_path), gt_class=0)
    assert np.array_equal(r["bin_edges"], np.linspace(0, 1, 11)) and r["bin_edges"][3] == 0.30000000000000004
    assert r["counts"].tolist() == [2, 0, 1, 0, 0, 3, 0, 0, 0, 2] and r["counts"].dtype == np.int64
    assert r["n_full_overlap"] == 1
    want = np.array([50, np.nan, 100, np.nan, np.nan, 200 / 3, np.nan, np.nan, np.nan, 50], dtype=np.float32)
    assert r["mean_acc"].dtype == np.float32 and np.allclose(r["mean_acc"], want, equal_nan=True)
    assert [e["iou"] for e in r["examples"]][:4] == [3 / (10 + 1e-12), 0.0, 0.0, 1.0] and r["examples"][4]["iou"] < 1.0
    assert [(e["intersection"], e["union"]) for e in r["examples"]] == [x[5] for x in rows]
    assert "avg_rot_err" not in r
    # where the quotient becomes exactly 1.0: from 2^14 pixels on, union + 1e-12 rounds back to union
    assert 16384 / (16384 + 1e-12) == 1.0 and 16383 / (16383 + 1e-12) < 1.0
    # the digitize call itself: the edge 0.30000000000000004 belongs to bin 3, 0.3 to bin 2
    assert np.digitize(0.30000000000000004, np.linspace(0, 1, 11)) - 1 == 3 and np.digitize(0.3, np.linspace(0, 1, 11)) - 1 == 2


def test_class_and_confidence_filters(tmp_path):
    rows = [row(1, 1, 0.95, (8, 10)), row(0, 1, 0.55, (8, 10)), row(0, 0, 0.99, (15, 100)), row(1, 0, 0.60, (15, 100)), row(1, 1, 0.70, (25, 100))]
    write_preds(tmp_path, rows)
    pos = overlap.measure_acc_vs_visual_overlap(str(tmp_path), gt_class=1)
    neg = overlap.measure_acc_vs_visual_overlap(str(tmp_path))          # default: the negatives
    assert pos["counts"].sum() == 3 and neg["counts"].sum() == 2
    assert pos["counts"][7] == 2 and pos["mean_acc"][7] == 50 and pos["counts"][2] == 1 and pos["mean_acc"][2] == 100   # 8 / 10 lies just below the edge 0.8
    assert neg["counts"][0] == 0 and neg["counts"][1] == 2 and neg["mean_acc"][1] == 50
    conf = overlap.measure_acc_vs_visual_overlap(str(tmp_path), gt_class=1, confidence_threshold=0.7)   # prob < threshold is dropped: 0.70 stays
    assert conf["counts"].sum() == 2 and [e["prob"] for e in conf["examples"]] == [0.95, 0.70]
    assert all(e["y_true"] == 1 for e in pos["examples"]) and all(e["y_true"] == 0 for e in neg["examples"])


def test_name_parsing():
    fp0 = "/x/gt_alignment_approx/1398/pair_3412___opening_1_0_rotated_floor_rgb_floor_01_partial_room_10_pano_10.jpg"
    fp1 = "/x/gt_alignment_approx/1398/pair_3412___opening_1_0_rotated_floor_rgb_floor_01_partial_room_01_pano_9.jpg"
    got = overlap.parse_tile_names(fp0, fp1)   # the names sort pano_10 in front of pano_9; the ids are compared as integers
    assert got == {"building_id": "1398", "floor_id": "floor_01", "i1": 9, "i2": 10, "pair_idx": "3412", "wdo_pair_uuid": "opening_1_0",
                   "configuration": "rotated"}
    got = overlap.parse_tile_names(name(54, "door_0_0_identity", 48), name(54, "door_0_0_identity", 51))
    assert got == {"building_id": "0668", "floor_id": "floor_02", "i1": 48, "i2": 51, "pair_idx": "54", "wdo_pair_uuid": "door_0_0",
                   "configuration": "identity"}
    got = overlap.parse_tile_names(name(7, "window_2_3_rotated", 5, surface="ceiling"), name(7, "window_2_3_rotated", 5, surface="ceiling"))
    assert (got["i1"], got["i2"], got["wdo_pair_uuid"], got["configuration"], got["floor_id"]) == (5, 5, "window_2_3", "rotated", "floor_02")
    with pytest.raises(ValueError):
        overlap.parse_tile_names(name(1, "wall_0_0_identity", 1), name(1, "wall_0_0_identity", 2))
    with pytest.raises(ValueError):
        overlap.parse_tile_names(name(1, "door_0_0_mirrored", 1), name(1, "door_0_0_mirrored", 2))


def test_angle_wrap():
    assert overlap.wrap_angle_deg(359.0, 1.0) == 2.0 and overlap.wrap_angle_deg(1.0, 359.0) == 2.0
    assert overlap.wrap_angle_deg(-179.0, 179.0) == 2.0 and overlap.wrap_angle_deg(10.0, 50.0) == 40.0 and overlap.wrap_angle_deg(0.0, 180.0) == 180.0


def rot(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s], [s, c]])


def test_pose_errors_per_bin(tmp_path):
    hyp_root = tmp_path / "hyp"
    rows = [(1, 1, 0.9, name(3, "door_0_1_identity", 7, root="/b/gt_alignment_approx/0668"), name(3, "door_0_1_identity", 4, root="/b/gt_alignment_approx/0668"), (45, 100)),
            (0, 1, 0.9, name(5, "opening_2_0_rotated", 4, root="/b/gt_alignment_approx/0668"), name(5, "opening_2_0_rotated", 9, root="/b/gt_alignment_approx/0668"), (41, 100))]
    write_preds(tmp_path / "preds", rows)
    d = hyp_root / "0668" / "floor_02" / "gt_alignment_approx"
    d.mkdir(parents=True)
    Sim2(rot(1.0), np.array([1.0, 2.0]), 1.0).save_as_json(str(d / "4_7__door_0_1_identity.json"))
    Sim2(rot(170.0), np.array([0.0, 0.0]), 1.0).save_as_json(str(d / "4_9__opening_2_0_rotated.json"))
    asked = []

    def gt(building_id, floor_id, i1, i2):
        asked.append((building_id, floor_id, i1, i2))
        return Sim2(rot(-1.0), np.array([4.0, 6.0]), 1.0) if i2 == 7 else Sim2(rot(-170.0), np.array([0.0, 0.5]), 1.0)

    r = overlap.measure_acc_vs_visual_overlap(str(tmp_path / "preds"), gt_class=1, hypotheses_save_root=str(hyp_root), gt_relative_pose=gt)
    assert asked == [("0668", "floor_02", 4, 7), ("0668", "floor_02", 4, 9)]
    assert np.allclose([e["rot_err"] for e in r["examples"]], [2.0, 20.0]) and np.allclose([e["trans_err"] for e in r["examples"]], [5.0, 0.5])
    assert r["counts"][4] == 2 and np.isclose(r["avg_rot_err"][4], 11.0) and np.isclose(r["avg_trans_err"][4], 2.75) and r["mean_acc"][4] == 50
    assert np.isnan(r["avg_rot_err"][0]) and np.isnan(r["avg_trans_err"][9])
    with pytest.raises(ValueError):
        overlap.measure_acc_vs_visual_overlap(str(tmp_path / "preds"), gt_class=1, hypotheses_save_root=str(hyp_root))


def test_counts_from_tile_files(tmp_path):
    from PIL import Image

    f1 = np.zeros((6, 5, 3), dtype=np.uint8)
    f2 = np.zeros((6, 5, 3), dtype=np.uint8)
    f1[:3, :, 1], f2[2:, :2, 2], f2[0, 4, 0] = 9, 200, 1       # 15 and 9 pixels; 3 in both
    d = tmp_path / "incorrect_alignment" / "0668"
    d.mkdir(parents=True)
    fp0, fp1 = name(2, "door_0_0_identity", 4, root=str(d)).replace(".jpg", ".png"), name(2, "door_0_0_identity", 6, root=str(d)).replace(".jpg", ".png")
    Image.fromarray(f1).save(fp0)
    Image.fromarray(f2).save(fp1)
    assert overlap.counts_from_tiles(fp0, fp1) == (3, 21)
    write_preds(tmp_path / "preds", [(0, 0, 0.8, fp0, fp1, (0, 0))], with_overlap=False)
    r = overlap.measure_acc_vs_visual_overlap(str(tmp_path / "preds"), from_tiles=True)
    assert r["counts"][1] == 1 and r["examples"][0]["iou"] == 3 / (21 + 1e-12)
    with pytest.raises(KeyError, match="overlap"):
        overlap.measure_acc_vs_visual_overlap(str(tmp_path / "preds"))


def test_command_line_prints_one_json_document(tmp_path, capsys):
    write_preds(tmp_path, [row(1, 1, 0.9, (20000, 20000)), row(0, 1, 0.9, (15, 100)), row(0, 0, 0.9, (15, 100))])
    assert overlap.main([str(tmp_path), "--gt-class", "1"]) == 0
    doc = json.loads(capsys.readouterr().out)
    assert set(doc) == {"bin_edges", "counts", "mean_acc", "n_full_overlap"}
    assert doc["counts"] == [0, 1, 0, 0, 0, 0, 0, 0, 0, 1] and doc["n_full_overlap"] == 1
    assert doc["mean_acc"] == [None, 0.0, None, None, None, None, None, None, None, 100.0]
    assert doc["bin_edges"] == np.linspace(0, 1, 11).tolist()
    assert overlap.main([str(tmp_path)]) == 0
    assert json.loads(capsys.readouterr().out)["counts"] == [0, 1, 0, 0, 0, 0, 0, 0, 0, 0]
