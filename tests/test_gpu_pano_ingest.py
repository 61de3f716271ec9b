"""ingest.PanoStore.load(decode="device") on the MI355X: the panoramas' JPEG files decoded by the lane-parallel decoder equal the
host route's (Pillow's) pixels behind the same device resize, bit for bit -- small panoramas, full-size ones, a set that mixes
sizes and tables, files with restart intervals, and files the device does not decode (progressive, greyscale) in the host slot;
score_floor(decode="device") writes score_floor(decode="host")'s prediction files."""

import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import jpeg_cases as jc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import ingest, jpeg  # noqa: E402
from salve_amd.utils import image_io  # noqa: E402

DEV = "cuda:0"


def _write_panos(root: Path, specs, depth_hw):
    """specs: [(h, w, Pillow save arguments, content)] -> ({pano id: path}, depth root); depth maps of depth_hw."""
    from PIL import Image

    (root / "zind" / "0003" / "panos").mkdir(parents=True)
    fpaths = {}
    rng = np.random.default_rng(0)
    for i, (h, w, save, content) in enumerate(specs):
        fp = root / "zind" / "0003" / "panos" / f"floor_01_partial_room_{i:02d}_pano_{i + 3}.jpg"
        rgb = jc.make_image(content, h, w, seed=i)
        Image.fromarray(rgb[..., 0] if save.pop("grey", False) else rgb).save(str(fp), format="JPEG", **save)
        image_io.write_depth_png(str(root / "depth" / "0003" / f"{fp.stem}.depth.png"), rng.integers(500, 5000, size=depth_hw, dtype=np.uint16))
        fpaths[i + 3] = str(fp)
    return fpaths, str(root / "depth")


def _both(fpaths, depth_root, pano_hw):
    ids = sorted(fpaths)
    host = ingest.PanoStore(DEV, pano_hw=pano_hw).load(fpaths, depth_root, "0003", ids)
    dev = ingest.PanoStore(DEV, pano_hw=pano_hw).load(fpaths, depth_root, "0003", ids, decode="device")
    assert dev.index == host.index and dev.fpaths == host.fpaths and dev.rgb.shape == host.rgb.shape == (len(ids), *pano_hw, 3)
    assert torch.equal(dev.rgb, host.rgb) and torch.equal(dev.depth, host.depth)
    return host, dev


def test_four_small_panoramas(tmp_path):
    fpaths, depth_root = _write_panos(tmp_path, [(128, 256, dict(quality=75), c) for c in ("noise", "disc", "layout", "noise")], (64, 128))
    host, dev = _both(fpaths, depth_root, (64, 128))
    assert dev.host_decoded == 0 and host.host_decoded == 0
    for pid, k in dev.index.items():   # and the host route is what it was: Pillow's pixels through the device resize
        want = ingest.resize_rgb_on_device(torch.from_numpy(image_io.read_rgb(fpaths[pid])).to(DEV)[None], (64, 128))[0]
        assert torch.equal(dev.rgb[k], want)


def test_two_full_size_panoramas(tmp_path):
    from tests.test_gpu_ingest import make_floor

    raw, depth_root, _, fpaths = make_floor(tmp_path, n_panos=2, n_hyp=1)
    assert jpeg.parse_file(Path(fpaths[3]).read_bytes())[:2] == (1024, 2048)
    _, dev = _both(ingest.floor_pano_fpaths(str(raw), "0003"), str(depth_root), (512, 1024))
    assert dev.host_decoded == 0


def test_a_set_that_mixes_sizes_tables_and_routes(tmp_path):
    specs = [(128, 256, dict(quality=75), "noise"), (256, 512, dict(quality=75), "disc"), (128, 256, dict(quality=90), "noise"),
             (128, 256, dict(quality=75, optimize=True), "disc"), (128, 256, dict(quality=75, restart_marker_rows=1), "noise"),
             (128, 256, dict(quality=75, restart_marker_blocks=3), "disc"), (100, 200, dict(quality=75), "noise"),
             (128, 256, dict(quality=75, progressive=True), "noise"), (128, 256, dict(quality=75, subsampling=0), "disc"),
             (128, 256, dict(quality=75, subsampling=1), "disc"), (128, 256, dict(quality=75, grey=True), "noise"), (128, 256, dict(quality=75), "layout")]
    fpaths, depth_root = _write_panos(tmp_path, specs, (64, 128))
    for pid, refused in ((10, "progressive"), (11, "sampling"), (12, "sampling"), (13, "component")):
        with pytest.raises(jpeg.Unsupported, match=refused):
            jpeg.parse_file(Path(fpaths[pid]).read_bytes(), restart=True)
    assert len(jpeg.parse_file(Path(fpaths[7]).read_bytes(), restart=True).segments) == 8
    _, dev = _both(fpaths, depth_root, (64, 128))
    assert dev.host_decoded == 4


def test_a_progressive_file_takes_the_host_slot(tmp_path):
    fpaths, depth_root = _write_panos(tmp_path, [(128, 256, dict(quality=75), "noise"), (128, 256, dict(quality=75, progressive=True), "disc"),
                                                 (128, 256, dict(quality=75), "layout")], (64, 128))
    _, dev = _both(fpaths, depth_root, (64, 128))
    assert dev.host_decoded == 1


def test_a_panorama_wider_than_the_device_decodes_takes_the_host_slot(tmp_path):
    """parse_file has no size limit; salve_bev_jpeg_decode_lanes takes 4096 x 4096 at the most."""
    fpaths, depth_root = _write_panos(tmp_path, [(32, 4112, dict(quality=75), "noise"), (128, 256, dict(quality=75), "disc")], (64, 128))
    assert jpeg.parse_file(Path(fpaths[3]).read_bytes(), restart=True).w == 4112 > jpeg.DEVICE_MAX_SIDE
    _, dev = _both(fpaths, depth_root, (64, 128))
    assert dev.host_decoded == 1


def test_a_malformed_file_gets_pillows_verdict(tmp_path):
    """Half a scan: the device reports the image, and the slot is what the host route makes of the file (Pillow raises)."""
    fpaths, depth_root = _write_panos(tmp_path, [(128, 256, dict(quality=75), "noise"), (128, 256, dict(quality=75), "disc")], (64, 128))
    raw = Path(fpaths[4]).read_bytes()
    p = jpeg.parse_file(raw)
    Path(fpaths[4]).write_bytes(raw[:p.scan_offset + p.scan_bytes // 2] + raw[-2:])
    outcomes = []
    for decode in ("host", "device"):
        try:
            outcomes.append(ingest.PanoStore(DEV, pano_hw=(64, 128)).load(fpaths, depth_root, "0003", [3, 4], decode=decode).rgb)
        except OSError as e:
            outcomes.append(type(e))
    assert (torch.equal(*outcomes) if isinstance(outcomes[0], torch.Tensor) else outcomes[0] is outcomes[1])


def test_refusals_and_depth_checks(tmp_path):
    fpaths, depth_root = _write_panos(tmp_path, [(128, 256, dict(quality=75), "noise")], (64, 128))
    with pytest.raises(ValueError, match="decode"):
        ingest.PanoStore(DEV, pano_hw=(64, 128)).load(fpaths, depth_root, "0003", [3], decode="gpu")
    with pytest.raises(ValueError, match="depth map"):
        ingest.PanoStore(DEV, pano_hw=(32, 64)).load(fpaths, depth_root, "0003", [3], decode="device")
    with pytest.raises((ValueError, FileNotFoundError)):
        ingest.PanoStore(DEV, pano_hw=(64, 128)).load(fpaths, str(tmp_path / "nowhere"), "0003", [3], decode="device")


def test_score_floor_writes_the_host_routes_prediction_files(tmp_path):
    from salve_amd.models.early_fusion import EarlyFusionCEResnet
    from tests.test_gpu_ingest import make_floor

    raw, depth_root, hyp_root, _ = make_floor(tmp_path, n_panos=2, n_hyp=3)
    torch.manual_seed(3)
    model = EarlyFusionCEResnet(18, False, 2, SimpleNamespace(modalities=["floor_rgb_texture"])).eval()
    for decode in ("host", "device"):
        ingest.score_floor(model, torch.device(DEV), str(raw), str(depth_root), str(hyp_root), str(tmp_path / "bev"), "0003", "floor_01",
                           str(tmp_path / f"preds_{decode}"), batch_size=2, chunk=2, decode=decode)
    host = sorted((tmp_path / "preds_host").glob("batch_*.json"))
    assert [f.name for f in host] == ["batch_0.json", "batch_1.json"]
    for f in host:
        assert json.load(open(f)) == json.load(open(tmp_path / "preds_device" / f.name)), f.name
