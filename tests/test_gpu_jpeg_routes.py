"""The JPEG round trip inside the two fused routes on the MI355X.  `RenderVerifyPipeline(jpeg_quality=75)` gives the tiles -- and the
logits -- of the reference's FILE route: render -> export_u8 -> image_io.write_jpeg -> image_io.read_rgb -> the shipped tile transform.
`RenderedTrainSource(jpeg_quality=75)` gives the batches `TrainTransform.apply` makes of the same files at the same draws.  With the
argument unset both routes give what they give without it.  Every comparison is bit-exact; 2 synthetic panoramas, 8 hypotheses."""

import functools
import random
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import layout, synthetic, synthetic_layouts, train_render  # noqa: E402
from salve_amd.common.sim2 import Sim2  # noqa: E402
from salve_amd.models.early_fusion import EarlyFusionCEResnet  # noqa: E402
from salve_amd.models.trainable import _pad8  # noqa: E402
from salve_amd.pipeline import RenderVerifyPipeline  # noqa: E402
from salve_amd.rasteriser import SURFACES, BevRasteriser, pack_hypotheses  # noqa: E402
from salve_amd.transforms import TrainTransform, ValTestTransform  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402

DEV = torch.device("cuda:0")
FLOOR, BOTH = ["floor_rgb_texture"], ["ceiling_rgb_texture", "floor_rgb_texture"]
ALL3 = ["ceiling_rgb_texture", "floor_rgb_texture", "layout"]
P, N, Q = 2, 8, 75
RESIZE, CROP = 234, 224


@functools.lru_cache(maxsize=None)
def _panos():
    panos = [synthetic.make_pano(i) for i in range(P)]
    return np.stack([p[0] for p in panos]), np.stack([p[1] for p in panos])


def _hyp():
    return synthetic.make_hypotheses(N, P, seed=0)


def _file_hop(img: np.ndarray, path) -> np.ndarray:
    image_io.write_jpeg(str(path), img)
    return image_io.read_rgb(str(path))


_FILES = {}


def _file_images(surfaces, tmp_path, with_layouts=False):
    """Per hypothesis its images after the file hop, in the model's channel order (surface-major, (i1, i2) inside a surface, the layout
    pair last): rendered and drawn by the shipped pieces, written and read back as the reference writes and reads them.  Made once per
    modality set and shared."""
    key = (tuple(surfaces), with_layouts)
    if key in _FILES:
        return _FILES[key]
    rgb, depth = _panos()
    hyp = _hyp()
    ras = BevRasteriser(DEV)
    S = len(surfaces)
    surf = [SURFACES[s] for s in surfaces]
    rows = np.concatenate([
        pack_hypotheses(np.repeat(hyp.i1, S), np.tile(surf, N), np.repeat(hyp.R, S, axis=0), np.repeat(hyp.t, S, axis=0), np.ones(N * S)),
        pack_hypotheses(np.repeat(np.arange(P), S), np.tile(surf, P), np.tile(np.eye(2, dtype=np.float32), (P * S, 1, 1)),
                        np.zeros((P * S, 2), np.float32), np.zeros(P * S))])
    bev, _ = ras.render(*ras.upload_panos(rgb, depth), ras.upload_hypotheses(rows), (N + P) * S)
    u8 = ras.export_u8(bev).cpu().numpy()
    if with_layouts:
        pl = synthetic_layouts.make_layouts(P, seed=9)
        specs = [pl.spec(int(hyp.i1[j]), Sim2(hyp.R[j], hyp.t[j], 1.0)) for j in range(N)] + [pl.spec(p) for p in range(P)]
        lay = ras.export_u8(layout.rasterise_layouts(specs, DEV)).cpu().numpy()
    ras.check("file route renders")
    hop = lambda im, name: _file_hop(im, tmp_path / f"{'-'.join(surfaces)}{'-layout' if with_layouts else ''}" / f"{name}.jpg")
    posed = [[hop(u8[j * S + k], f"posed_{j}_{k}") for k in range(S)] for j in range(N)]
    ident = [[hop(u8[(N + p) * S + k], f"ident_{p}_{k}") for k in range(S)] for p in range(P)]
    out = [[im for k in range(S) for im in (posed[j][k], ident[int(hyp.i2[j])][k])] for j in range(N)]
    if with_layouts:
        lay_ident = [hop(lay[N + p], f"layout_ident_{p}") for p in range(P)]
        for j in range(N):
            out[j] += [hop(lay[j], f"layout_posed_{j}"), lay_ident[int(hyp.i2[j])]]
    _FILES[key] = out
    return out


def _model(mods):
    torch.manual_seed(0)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=mods)).eval()
    synthetic.trained_looking_batchnorm(model)
    return model


def _run_pipeline(mods, precision, **kw):
    rgb, depth = _panos()
    pipe = RenderVerifyPipeline(_model(mods), DEV, chunk=N, overlap=False, streams=1, precision=precision, **kw)
    pipe.load_panos(rgb, depth)
    logits = pipe.score(pipe.prepare(_hyp()))
    torch.cuda.synchronize()
    pipe.check("jpeg route")
    return pipe, pipe.tile_bufs[0][:N].clone(), logits.clone()


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
@pytest.mark.parametrize("mods", [FLOOR, BOTH], ids=["floor", "ceiling+floor"])
def test_pipeline_tiles_and_logits_equal_the_file_route(mods, precision, tmp_path):
    surfaces = train_render.train_surfaces(mods)
    images = _file_images(surfaces, tmp_path)
    pipe, tiles, logits = _run_pipeline(mods, precision, jpeg_quality=Q)
    assert pipe.jpeg_quality == Q and pipe.fuse_tiles is False
    C = 6 * len(surfaces)
    vt = ValTestTransform((RESIZE, RESIZE), (CROP, CROP), device=DEV)
    want = torch.stack([torch.cat(vt(*images[j]), 0) for j in range(N)])   # fp32 [N, C, 224, 224]
    if precision == "fp32":
        file_tiles = want.contiguous()
        assert torch.equal(tiles, file_tiles)
        ref_logits = torch.empty_like(logits)
        pipe.engine.forward_nchw(file_tiles, out=ref_logits)
    else:
        file_tiles = torch.zeros_like(tiles)
        file_tiles[..., :C] = want.permute(0, 2, 3, 1).half()
        assert torch.equal(tiles, file_tiles)
        ref_logits = torch.empty_like(logits)
        pipe.engine.forward_nhwc(file_tiles, out=ref_logits)
    torch.cuda.synchronize()
    pipe.check("engine on the file route's tiles")
    assert torch.equal(logits, ref_logits)
    # and the round trip is not a no-op on these renders
    _, lossless, _ = _run_pipeline(mods, precision, fuse_tiles=False)
    assert not torch.equal(tiles, lossless)


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_pipeline_unset_gives_todays_tiles(precision):
    a_pipe, a_tiles, a_logits = _run_pipeline(FLOOR, precision)
    b_pipe, b_tiles, b_logits = _run_pipeline(FLOOR, precision, jpeg_quality=None)
    assert b_pipe.jpeg_quality is None and b_pipe.fuse_tiles == a_pipe.fuse_tiles == (precision == "fp16")
    assert torch.equal(a_tiles, b_tiles) and torch.equal(a_logits, b_logits)


def _epoch(mods, seed, py_seed, B=4, **kw):
    rgb, depth = _panos()
    layouts = synthetic_layouts.make_layouts(P, seed=9) if "layout" in mods else None
    src = train_render.RenderedTrainSource(DEV, mods, batch_size=B, precision="fp32", split="train", seed=seed, layouts=layouts, **kw)
    src.load_panos(rgb, depth)
    src.set_examples(_hyp(), np.arange(N, dtype=np.int64))
    random.seed(py_seed)
    return [(x.clone(), y.clone()) for x, y in src]


@pytest.mark.parametrize("mods,identity", [(FLOOR, "kept"), (FLOOR, "batch"), (BOTH, "kept"), (ALL3, "kept"), (ALL3, "batch")],
                         ids=["floor-kept", "floor-batch", "ceiling+floor-kept", "layouts-kept", "layouts-batch"])
def test_feed_equals_the_transform_of_the_files(mods, identity, tmp_path):
    B, seed = 4, 3
    images = _file_images(train_render.train_surfaces(mods, with_layouts=True), tmp_path, with_layouts="layout" in mods)
    C = 6 * len(mods)
    got = _epoch(mods, seed, 11, B, identity=identity, jpeg_quality=Q)
    tf = TrainTransform((RESIZE, RESIZE), (CROP, CROP), device=DEV)
    gen = torch.Generator()
    gen.manual_seed(seed)
    random.seed(11)
    plan = train_render.plan_epoch(N, B, "train", gen)
    assert len(got) == len(plan) == 2
    for (x, y), idx in zip(got, plan):
        draws = [tf.draw() for _ in idx]
        assert x.shape == (B, CROP, CROP, _pad8(C)) and y[:, 0].cpu().tolist() == idx.tolist()
        for k, (j, draw) in enumerate(zip(idx, draws)):
            want = torch.cat(tf.apply(images[int(j)], *draw), 0).permute(1, 2, 0)
            assert torch.equal(x[k][..., :C], want), (int(j), draw)
            assert bool((x[k][..., C:] == 0.0).all())


@pytest.mark.parametrize("identity", ["kept", "batch"])
def test_feed_unset_gives_todays_batches(identity):
    a = _epoch(BOTH, 3, 11, identity=identity)
    b = _epoch(BOTH, 3, 11, identity=identity, jpeg_quality=None)
    c = _epoch(BOTH, 3, 11, identity=identity, jpeg_quality=Q)
    assert all(torch.equal(u[0], v[0]) and torch.equal(u[1], v[1]) for u, v in zip(a, b))
    assert not all(torch.equal(u[0], v[0]) for u, v in zip(a, c))


def test_sources_that_share_panoramas_must_agree_on_the_round_trip():
    rgb, depth = _panos()
    train = train_render.RenderedTrainSource(DEV, FLOOR, batch_size=4, jpeg_quality=Q)
    train.load_panos(rgb, depth)
    val = train_render.RenderedTrainSource(DEV, FLOOR, batch_size=4, split="val")
    with pytest.raises(RuntimeError, match="jpeg_quality"):
        val.share_panos(train)
