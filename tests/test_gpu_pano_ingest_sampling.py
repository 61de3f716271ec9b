"""ingest.PanoStore.load(decode="device", samplings=jpeg.SAMPLINGS) on the MI355X: 4:2:2, 4:4:4 and greyscale panoramas stay
on the device (jpeg.DEVICE_SAMPLINGS: all of them but 4:4:4) and equal the host route's (Pillow's) pixels behind the same device resize, bit for bit; only what the device still does
not decode -- a progressive file, a three-component file that libjpeg reads as RGB -- takes the host slot; with the default keyword
nothing changes."""

from pathlib import Path

import numpy as np
import pytest

import jpeg_cases as jc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import ingest, jpeg  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402

DEV = "cuda:0"
# tests/test_gpu_pano_ingest.py's mixed set: sizes, tables, restart intervals, and the four files its default route leaves to Pillow
MIXED = [(128, 256, dict(quality=75), "noise"), (256, 512, dict(quality=75), "disc"), (128, 256, dict(quality=90), "noise"),
         (128, 256, dict(quality=75, optimize=True), "disc"), (128, 256, dict(quality=75, restart_marker_rows=1), "noise"),
         (128, 256, dict(quality=75, restart_marker_blocks=3), "disc"), (100, 200, dict(quality=75), "noise"),
         (128, 256, dict(quality=75, progressive=True), "noise"), (128, 256, dict(quality=75, subsampling=0), "disc"),
         (128, 256, dict(quality=75, subsampling=1), "disc"), (128, 256, dict(quality=75, grey=True), "noise"), (128, 256, dict(quality=75), "layout")]


def _write_panos(root: Path, specs, depth_hw):
    """specs: [(h, w, Pillow save arguments, content)] -> ({pano id: path}, depth root); depth maps of depth_hw.  (A copy of
    tests/test_gpu_pano_ingest.py's helper.)"""
    from PIL import Image

    (root / "zind" / "0003" / "panos").mkdir(parents=True)
    fpaths = {}
    rng = np.random.default_rng(0)
    for i, (h, w, save, content) in enumerate(specs):
        save = dict(save)
        fp = root / "zind" / "0003" / "panos" / f"floor_01_partial_room_{i:02d}_pano_{i + 3}.jpg"
        rgb = jc.make_image(content, h, w, seed=i)
        Image.fromarray(rgb[..., 0] if save.pop("grey", False) else rgb).save(str(fp), format="JPEG", **save)
        image_io.write_depth_png(str(root / "depth" / "0003" / f"{fp.stem}.depth.png"), rng.integers(500, 5000, size=depth_hw, dtype=np.uint16))
        fpaths[i + 3] = str(fp)
    return fpaths, str(root / "depth")


def _both(fpaths, depth_root, pano_hw, **kw):
    ids = sorted(fpaths)
    host = ingest.PanoStore(DEV, pano_hw=pano_hw).load(fpaths, depth_root, "0003", ids)
    dev = ingest.PanoStore(DEV, pano_hw=pano_hw).load(fpaths, depth_root, "0003", ids, decode="device", **kw)
    assert dev.index == host.index and dev.fpaths == host.fpaths and dev.rgb.shape == host.rgb.shape == (len(ids), *pano_hw, 3)
    assert torch.equal(dev.rgb, host.rgb) and torch.equal(dev.depth, host.depth)
    return host, dev


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    return _write_panos(tmp_path_factory.mktemp("mixed_panos"), MIXED, (64, 128))


def test_the_mixed_set_with_every_device_sampling_leaves_one_file_to_pillow(mixed):
    fpaths, depth_root = mixed
    wide = dict(restart=True, samplings=jpeg.SAMPLINGS)
    assert [jpeg.parse_file(Path(fpaths[pid]).read_bytes(), **wide).sampling for pid in (11, 12, 13)] == ["4:4:4", "4:2:2", "grey"]
    with pytest.raises(jpeg.Unsupported, match="progressive"):
        jpeg.parse_file(Path(fpaths[10]).read_bytes(), **wide)
    _, dev = _both(fpaths, depth_root, (64, 128), samplings=jpeg.SAMPLINGS)
    assert dev.host_decoded == 1
    _, dev = _both(fpaths, depth_root, (64, 128), samplings=jpeg.DEVICE_SAMPLINGS)      # without 4:4:4: that file goes to Pillow too
    assert dev.host_decoded == 2


def test_the_mixed_set_with_the_default_keyword_is_unchanged(mixed):
    fpaths, depth_root = mixed
    _, dev = _both(fpaths, depth_root, (64, 128))
    assert dev.host_decoded == 4
    _, dev = _both(fpaths, depth_root, (64, 128), samplings=("4:2:0", "4:2:2"))      # a subset: 4:4:4, greyscale and progressive stay on the host
    assert dev.host_decoded == 3
    with pytest.raises(ValueError, match="samplings"):
        ingest.PanoStore(DEV, pano_hw=(64, 128)).load(fpaths, depth_root, "0003", [3], decode="device", samplings=("4:1:1",))


def test_a_keep_rgb_panorama_takes_the_host_slot(tmp_path):
    specs = [(128, 256, dict(quality=75, subsampling=0), "noise"), (128, 256, dict(quality=75, subsampling=0, keep_rgb=True), "disc"),
             (128, 256, dict(quality=75, subsampling=0), "layout")]
    fpaths, depth_root = _write_panos(tmp_path, specs, (64, 128))
    with pytest.raises(jpeg.Unsupported, match="colour space"):
        jpeg.parse_file(Path(fpaths[4]).read_bytes(), restart=True, samplings=jpeg.SAMPLINGS)
    _, dev = _both(fpaths, depth_root, (64, 128), samplings=jpeg.SAMPLINGS)
    assert dev.host_decoded == 1
    want = ingest.resize_rgb_on_device(torch.from_numpy(image_io.read_rgb(fpaths[4])).to(DEV)[None], (64, 128))[0]
    assert torch.equal(dev.rgb[dev.index[4]], want)                    # Pillow's pixels


def test_a_greyscale_panorama_equals_read_rgb3_through_the_device_resize(tmp_path):
    fpaths, depth_root = _write_panos(tmp_path, [(128, 256, dict(quality=75, grey=True), "noise"), (128, 256, dict(quality=90, grey=True, restart_marker_rows=2), "disc")],
                                      (64, 128))
    _, dev = _both(fpaths, depth_root, (64, 128), samplings=jpeg.SAMPLINGS)
    assert dev.host_decoded == 0
    for pid, k in dev.index.items():
        rgb3 = ingest._read_rgb3(fpaths[pid])
        assert rgb3.shape == (128, 256, 3) and np.array_equal(rgb3[..., 0], rgb3[..., 2])
        assert torch.equal(dev.rgb[k], ingest.resize_rgb_on_device(torch.from_numpy(rgb3).to(DEV)[None], (64, 128))[0])


def test_one_full_size_422_panorama(tmp_path):
    """The real ingest shape, once: 1024 x 2048 -> 512 x 1024."""
    fpaths, depth_root = _write_panos(tmp_path, [(1024, 2048, dict(quality=90, subsampling=1), "disc")], (512, 1024))
    p = jpeg.parse_file(Path(fpaths[3]).read_bytes(), restart=True, samplings=jpeg.SAMPLINGS)
    assert (p.h, p.w, p.sampling) == (1024, 2048, "4:2:2")
    _, dev = _both(fpaths, depth_root, (512, 1024), samplings=jpeg.SAMPLINGS)
    assert dev.host_decoded == 0
