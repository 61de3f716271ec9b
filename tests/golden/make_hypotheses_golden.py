"""Writes the fixtures of the alignment-hypothesis tests from ZInD building 0000, floor_01 (32 panoramas) and MHNet's predictions for it:

    python tests/golden/make_hypotheses_golden.py PATH/TO/ZInD/0000/zind_data.json PATH/TO/horizon_net/0000

* zind_0000_floor_01_wdo.json: the `merger` annotation of the floor trimmed to what is read -- per panorama image_path, label, camera_height,
  floor_plan_transformation and layout_raw's vertices, windows, doors, openings -- and the scales.
* mhnet_0000_floor_01.npz: per panorama the prediction file's stem, the image size, floor_boundary (as integers of 1e-6 pixels) and
  wall_features; corners_in_uv and floor_boundary_uncertainty only of the panorama whose first values the reference's own test records.
* hypotheses_0000_floor_01.json: what this project's EMULATOR (tests/hypotheses_cases.py) gives on them, as recorded data: the counts per label,
  the sorted file names (packed: tests/hypotheses_cases.py recorded_names), a digest of R and t, the per-floor counts, the visibly adjacent pairs and the smallest label margin.

The files are DATA only.  The reference's own exporter cannot run where this was written (no gtsam, no shapely): parity with it is unpinned.
"""

import json
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

FLOOR = "floor_01"
RECORDED_STEM = "floor_01_partial_room_09_pano_2"   # the reference's tests/dataset/test_mhnet_prediction.py reads this one


def main(zind_json: str, mhnet_dir: str) -> None:
    from tests import hypotheses_cases as hc

    here = Path(__file__).resolve().parent
    with open(zind_json) as f:
        d = json.load(f)
    floor = {}
    for ck, complete in d["merger"][FLOOR].items():
        floor[ck] = {}
        for pk, partial in complete.items():
            floor[ck][pk] = {k: {"image_path": p["image_path"], "label": p["label"], "camera_height": p["camera_height"],
                                 "floor_plan_transformation": p["floor_plan_transformation"],
                                 "layout_raw": {k2: p["layout_raw"][k2] for k2 in ("vertices", "windows", "doors", "openings")}}
                             for k, p in partial.items()}
    with open(here / hc.GOLDEN_ZIND, "w") as f:
        json.dump({"scale_meters_per_coordinate": d["scale_meters_per_coordinate"], "merger": {FLOOR: floor}}, f, separators=(",", ":"))
    import numpy as np

    def micro(values):   # six decimals -> integers of 1e-6, then differences: small numbers that deflate well; exact, and checked to be
        ints = np.rint(np.asarray(values, dtype=np.float64) * hc.MICRO).astype(np.int64)
        assert (ints / hc.MICRO).tolist() == list(values)
        return np.diff(ints, prepend=0).astype(np.int32)

    panos, boundaries, uncertainty = [], [], None
    for fp in sorted(Path(mhnet_dir).glob("*.json")):
        with open(fp) as f:
            p = json.load(f)["predictions"]
        rec = {"stem": fp.stem, "image_width": p["image_width"], "image_height": p["image_height"], "wall_features": p["wall_features"]}
        boundaries.append(micro(p["room_shape"]["raw_predictions"]["floor_boundary"]))
        if fp.stem == RECORDED_STEM:
            rec["corners_in_uv"] = p["room_shape"]["corners_in_uv"]
            uncertainty = micro(p["room_shape"]["raw_predictions"]["floor_boundary_uncertainty"])
        panos.append(rec)
    np.savez_compressed(here / hc.GOLDEN_MHNET, meta=np.array(json.dumps({"building_id": "0000", "floor_id": FLOOR, "panoramas": panos}, separators=(",", ":"))),
                        floor_boundary=np.stack(boundaries), uncertainty=uncertainty)

    # the emulator's results on the floor as the library's host loaders read it back
    from salve_amd import hypotheses

    with tempfile.TemporaryDirectory() as tmp:
        raw, root = hc.expand_fixture(here, tmp)
        (fi,) = hypotheses.load_floors(raw, root, ["0000"])
    pairs = hc.emulate_floor(hc.floor_dict(fi))
    hyps = hc.expected_hypotheses(pairs)
    out = {"n_panoramas": len(fi.pano_ids), "pano_ids": [int(i) for i in fi.pano_ids], "n_pairs": len(pairs), "n_hypotheses": len(hyps),
           "counts": {hc.LABEL_DIRS[0]: sum(h[0] == 1 for h in hyps), hc.LABEL_DIRS[1]: sum(h[0] == 0 for h in hyps)},
           "n_valid_configurations": sum(p["n_valid"] for p in pairs), "n_invalid_configurations": sum(p["n_rejected"] for p in pairs),
           "n_pruned": sum(p["n_valid"] - len(p["rows"]) for p in pairs),
           "visibly_adjacent": [[p["i1"], p["i2"]] for p in pairs if p["adjacent"]], "min_label_margin": min(m for p in pairs for m in p["margins"]),
           "digest_R_t": hc.digest(hyps), "names": hc.pack_names(hyps),
           "note": "the EMULATOR's values; the reference's exporter is unpinned (gtsam and shapely are not installed where this was written)"}
    with open(here / hc.GOLDEN_RESULT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    assert hc.recorded_names(out) == [[hc.LABEL_DIRS[1 - h[0]], h[7]] for h in hyps]
    for name in (hc.GOLDEN_ZIND, hc.GOLDEN_MHNET, hc.GOLDEN_RESULT):
        print(name, (here / name).stat().st_size, "bytes")
    print({k: out[k] for k in ("n_pairs", "n_hypotheses", "counts", "n_valid_configurations", "n_invalid_configurations", "n_pruned", "min_label_margin")},
          len(out["visibly_adjacent"]), "adjacent pairs")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
