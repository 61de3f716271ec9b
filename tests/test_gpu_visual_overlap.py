"""RenderVerifyPipeline.score(visual_overlap=True) and the drivers on top of it: the counts equal numpy on the very images the verifier's
tiles were made from, in every stream / chunk / precision / tile / JPEG configuration; the logits are those of a run without it; the
prediction files gain exactly one key; and with the JPEG round trip the counts are those of the files the render driver writes."""

import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import ingest, overlap, synthetic  # noqa: E402
from salve_amd.common.sim2 import Sim2  # noqa: E402
from salve_amd.models.early_fusion import EarlyFusionCEResnet  # noqa: E402
from salve_amd.pipeline import RenderVerifyPipeline  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402

DEV = "cuda:0"
N_PANOS, N_HYP = 4, 12


@pytest.fixture(scope="module")
def scene():
    panos = synthetic.make_panos(N_PANOS)
    hyp = synthetic.make_hypotheses(N_HYP, N_PANOS, seed=2)
    hyp.i1[0] = hyp.i2[0] = 1          # hypothesis 0: a panorama against itself at the identity pose
    hyp.R[0], hyp.t[0], hyp.theta_deg[0] = np.eye(2, dtype=np.float32), 0.0, 0.0
    return np.stack([p[0] for p in panos]), np.stack([p[1] for p in panos]), hyp


def model_for(modalities, seed=0):
    torch.manual_seed(seed)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=modalities)).eval()
    synthetic.trained_looking_batchnorm(model)
    return model


def occupancy(ras, bev):
    """bool [n, H, W] from the exported bytes, as the reference takes it from a file: the largest channel is positive."""
    return ras.export_u8(bev).cpu().numpy().max(axis=3) > 0


def numpy_counts(pipe, prepared):
    """int64 [N, S, 2] from the images themselves.  Every posed image is rendered again here, in render order, by the rasteriser's plain
    entry (and sent through the JPEG round trip where the pipeline has one); the chunks whose image buffers the call left intact
    (`bev_index`, `last_chunk_buffer`) are checked to hold exactly these images, so the counts are those of the very images scored."""
    torch.cuda.synchronize()
    S, N = len(pipe.surfaces), prepared["n"]
    imgs, _ = pipe.ras.render(pipe.pano_rgb, pipe.pano_depth, prepared["rows"], N * S)
    if pipe.jpeg_quality is not None:
        imgs = pipe.ras.jpeg_roundtrip(imgs, pipe.jpeg_quality)
    chunks = sorted(pipe.last_chunk_buffer)
    intact = [ci for ci in chunks if all(pipe.last_chunk_buffer[c] != pipe.last_chunk_buffer[ci] for c in chunks if c > ci)]
    assert len(intact) == min(pipe.nbuf, len(chunks))
    for ci in intact:
        n = min(pipe.chunk, N - ci * pipe.chunk)
        held = pipe.bevs[pipe.last_chunk_buffer[ci]][:n * S]
        assert torch.equal(held, imgs[ci * pipe.chunk * S:ci * pipe.chunk * S + n * S]), ci
    posed, ident = occupancy(pipe.ras, imgs), occupancy(pipe.ras, pipe.ref_bev)
    out = np.zeros((N, S, 2), dtype=np.int64)
    for j in range(N):
        ck, k0 = pipe.bev_index(prepared, j)
        for si in range(S):
            a, b = posed[ck * pipe.chunk * S + k0 + si], ident[int(prepared["i2"][j]) * S + si]
            out[j, si] = (a & b).sum(), (a | b).sum()
    return out


SCENARIOS = {
    "three-chunks-three-streams": dict(modalities=["floor_rgb_texture"], chunk=5),
    "one-chunk-one-stream": dict(modalities=["floor_rgb_texture"], chunk=12, overlap=False, streams=1),
    "two-streams": dict(modalities=["floor_rgb_texture"], chunk=5, streams=2),
    "ceiling-and-floor": dict(modalities=["ceiling_rgb_texture", "floor_rgb_texture"], chunk=5),
    "tiles-unfused": dict(modalities=["floor_rgb_texture"], chunk=5, fuse_tiles=False),
    "fp32": dict(modalities=["floor_rgb_texture"], chunk=5, precision="fp32"),
    "jpeg-75": dict(modalities=["ceiling_rgb_texture", "floor_rgb_texture"], chunk=5, jpeg_quality=75),
}


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_counts_equal_numpy_on_the_scored_images(scene, name):
    rgb, depth, hyp = scene
    kw = dict(SCENARIOS[name])
    pipe = RenderVerifyPipeline(model_for(kw.pop("modalities")), torch.device(DEV), **kw)
    pipe.load_panos(rgb, depth)
    prepared = pipe.prepare(hyp)
    with pytest.raises(RuntimeError, match="visual_overlap"):
        pipe.visual_overlap(prepared)
    plain = pipe.score(prepared).clone()
    assert "overlap" not in prepared and "overlap_jobs" not in prepared      # the default path uploads and allocates nothing more
    logits = pipe.score(prepared, visual_overlap=True).clone()
    got = pipe.visual_overlap(prepared)
    pipe.check(name)
    S = len(pipe.surfaces)
    assert got.shape == (N_HYP, S, 2) and got.dtype == np.int64
    assert pipe.valid_mask(prepared).all()      # no dropped row can hide a mismatch
    assert torch.equal(logits, plain)
    want = numpy_counts(pipe, prepared)
    assert np.array_equal(got, want), (got - want)
    assert (got[0, :, 0] == got[0, :, 1]).all() and (got[0, :, 0] > 0).all()      # hypothesis 0: the same image twice
    assert (got[1:, :, 0] < got[1:, :, 1]).all() and (got[:, :, 0] >= 0).all()
    again = pipe.score(prepared, visual_overlap=True)
    assert np.array_equal(pipe.visual_overlap(prepared), got) and torch.equal(again, plain)
    pipe.check(name)


def test_layout_only_is_refused(scene):
    pipe = RenderVerifyPipeline(model_for(["layout"]), torch.device(DEV), chunk=4)
    with pytest.raises(RuntimeError, match="layout"):
        pipe.score({"n": 0}, visual_overlap=True)      # refused before the shard is looked at


# ---------------------------------------------------------------------------------------------- the drivers
def make_floor(root: Path):
    """A synthetic building on disk in the reference's layout (as tests/test_gpu_ingest.py builds one): 2048 x 1024 JPEG panoramas,
    1024 x 512 depth maps, Sim(2) hypothesis files in the two label directories."""
    raw, depth_root, hyp_root = root / "zind", root / "depth", root / "hyp"
    (raw / "0003" / "panos").mkdir(parents=True)
    for i in range(N_PANOS):
        rgb, depth = synthetic.make_pano(i)
        fp = raw / "0003" / "panos" / f"floor_01_partial_room_{N_PANOS - 1 - i:02d}_pano_{i + 8}.jpg"      # pano_10 sorts in front of pano_9
        image_io.write_jpeg(str(fp), np.repeat(np.repeat(rgb, 2, axis=0), 2, axis=1))
        image_io.write_depth_png(str(depth_root / "0003" / f"{fp.stem}.depth.png"), depth)
    hyp = synthetic.make_hypotheses(6, N_PANOS, seed=2)
    for j in range(6):
        d = hyp_root / "0003" / "floor_01" / ("gt_alignment_approx" if j % 3 == 0 else "incorrect_alignment")
        d.mkdir(parents=True, exist_ok=True)
        Sim2(hyp.R[j].astype(np.float64), hyp.t[j].astype(np.float64), 1.0).save_as_json(
            str(d / f"{int(hyp.i1[j]) + 8}_{int(hyp.i2[j]) + 8}__door_{j}_0_{'identity' if j % 2 else 'rotated'}.json"))
    return raw, depth_root, hyp_root


@pytest.fixture(scope="module")
def floor(tmp_path_factory):
    return make_floor(tmp_path_factory.mktemp("overlap_floor"))


def read_preds(d):
    return [json.load(open(f)) for f in sorted(Path(d).glob("batch_*.json"))]


def score(floor, tmp_path, out, model, **kw):
    raw, depth_root, hyp_root = floor
    return ingest.score_floor(model, torch.device(DEV), str(raw), str(depth_root), str(hyp_root), str(tmp_path / "bev"), "0003", "floor_01",
                              str(tmp_path / out), batch_size=4, chunk=4, **kw)


@pytest.mark.parametrize("modalities", [["floor_rgb_texture"], ["ceiling_rgb_texture", "floor_rgb_texture"], ["ceiling_rgb_texture"]])
def test_score_floor_adds_one_key(floor, tmp_path, modalities):
    model = model_for(modalities, seed=3)
    m0 = score(floor, tmp_path, "plain", model)
    m1 = score(floor, tmp_path, "with", model, visual_overlap=True)
    plain, with_ = read_preds(tmp_path / "plain"), read_preds(tmp_path / "with")
    assert len(plain) == len(with_) == 2 and m0 == m1 and m1["num_dropped_no_points_in_window"] == 0
    for a, b in zip(plain, with_):
        assert list(b) == list(a) + ["overlap"]
        assert {k: b[k] for k in a} == a
        assert len(b["overlap"]) == len(b["y_hat"]) and all(len(r) == 2 and 0 <= r[0] <= r[1] and r[1] > 0 for r in b["overlap"])
    # the counts are those of the surface the names carry: the floor where there is one
    rows = [r for b in with_ for r in b["overlap"]]
    if "floor_rgb_texture" in modalities:
        floor_only = read_preds(tmp_path / "with") if modalities == ["floor_rgb_texture"] else None
        if floor_only is None:
            score(floor, tmp_path, "floor", model_for(["floor_rgb_texture"], seed=3), visual_overlap=True)
            floor_only = read_preds(tmp_path / "floor")
        assert rows == [r for b in floor_only for r in b["overlap"]]
    for gt_class in (0, 1):
        r = overlap.measure_acc_vs_visual_overlap(str(tmp_path / "with"), gt_class=gt_class)
        kept = sum(y == gt_class for b in with_ for y in b["y_true"])
        assert int(r["counts"].sum()) == kept == len(r["examples"]) and kept == (2 if gt_class else 4)
        assert all(e["building_id"] == "0003" and e["floor_id"] == "floor_01" and 8 <= e["i1"] < e["i2"] <= 11 for e in r["examples"])


def test_jpeg_counts_equal_those_of_the_written_tiles(floor, tmp_path):
    """jpeg_quality=75: the images counted on the device have been through the reference's JPEG hop, so the counts are those of the
    files the render driver writes under the names in fp0 / fp1 -- ringing around the silhouettes included."""
    from salve_amd import render_dataset

    raw, depth_root, hyp_root = floor
    score(floor, tmp_path, "preds", model_for(["floor_rgb_texture"], seed=3), visual_overlap=True, jpeg_quality=75)
    n = render_dataset.render_pairs(1, str(depth_root), str(tmp_path / "bev"), str(raw), str(hyp_root), None, ["rgb_texture"], None, "0003",
                                    device=DEV, jpeg="host")
    assert n > 0
    lossless = tmp_path / "lossless"
    score(floor, tmp_path, "lossless", model_for(["floor_rgb_texture"], seed=3), visual_overlap=True)
    differs = False
    for gt_class in (0, 1):
        key = overlap.measure_acc_vs_visual_overlap(str(tmp_path / "preds"), gt_class=gt_class)["examples"]
        files = overlap.measure_acc_vs_visual_overlap(str(tmp_path / "preds"), gt_class=gt_class, from_tiles=True)["examples"]
        assert len(key) == len(files) > 0
        assert [(e["intersection"], e["union"]) for e in key] == [(e["intersection"], e["union"]) for e in files]
        plain = overlap.measure_acc_vs_visual_overlap(str(lossless), gt_class=gt_class)["examples"]
        differs |= [(e["intersection"], e["union"]) for e in key] != [(e["intersection"], e["union"]) for e in plain]
    assert differs      # (the round trip does change the masks: the equality above is not that of two lossless routes)
