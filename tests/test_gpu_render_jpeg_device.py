"""render_dataset's device JPEG route on the MI355X: render_building_floor_pairs(jpeg="device") writes the same set of files as the
default host route, byte for byte -- texture maps and layout images, also where a forced small slot sends some images through the
overflow fallback --, writes nothing for a pair with an empty render, and nothing at all on a second call."""

from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import render_dataset  # noqa: E402
from salve_amd.jpeg import HEADER_BYTES  # noqa: E402
from tests.test_gpu_ingest import _synthetic_pose_graph, make_floor  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def floor(tmp_path_factory):
    """The synthetic floor of tests/test_gpu_ingest.py: four panoramas, six hypotheses, two surfaces; hypothesis 1's posed render is
    empty (its panorama lies outside the window)."""
    root = tmp_path_factory.mktemp("floor")
    raw, depth_root, hyp_root, _ = make_floor(root, far=(1,))
    return root, str(raw), str(depth_root), str(hyp_root)


def _files(root: Path):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*.jpg"))}


def test_texture_maps_equal_the_host_routes_files(floor):
    root, raw, depth_root, hyp_root = floor

    def run(out, **kw):
        return render_dataset.render_building_floor_pairs(depth_root, str(root / out), hyp_root, raw, "0003", "floor_01", None, ["rgb_texture"],
                                                          device=DEV, **kw)

    n_host = run("bev_host", jpeg="host")
    n_dev = run("bev_device", jpeg="device")
    host, dev = _files(root / "bev_host"), _files(root / "bev_device")
    assert n_host == n_dev == len(host) and 0 < n_host <= 2 * 2 * 5   # six hypotheses, one without points in the window, two surfaces, two tiles
    assert sorted(host) == sorted(dev)
    for name in host:
        assert host[name] == dev[name], name
    assert run("bev_device", jpeg="device") == 0          # idempotent restart: nothing is written again
    assert _files(root / "bev_device") == dev
    # the overflow fallback: a slot that holds some of the scans and not others
    sizes = sorted(len(b) - HEADER_BYTES - 2 for b in host.values())
    stride = (sizes[len(sizes) // 2] + 3) // 4 * 4
    assert sizes[0] < stride < sizes[-1]
    assert run("bev_small", jpeg="device", jpeg_stride=stride) == n_host
    assert _files(root / "bev_small") == host
    assert render_dataset.render_pairs(1, depth_root, str(root / "bev_pairs"), raw, hyp_root, None, ["rgb_texture"], None, "0003", device=DEV,
                                       jpeg="device") == n_host
    assert _files(root / "bev_pairs") == host
    with pytest.raises(ValueError):
        run("bev_bad", jpeg="gpu")


def test_layout_images_equal_the_host_routes_files(floor):
    root, raw, depth_root, hyp_root = floor
    graph = _synthetic_pose_graph([3, 4, 5, 6])

    def run(out, **kw):
        return render_dataset.render_building_floor_pairs(depth_root, "", hyp_root, raw, "0003", "floor_01", str(root / out), ["layout"], device=DEV,
                                                          floor_pose_graph=graph, **kw)

    n_host = run("layout_host")
    n_dev = run("layout_device", jpeg="device")
    host, dev = _files(root / "layout_host"), _files(root / "layout_device")
    assert n_host == n_dev == len(host) and n_host > 0 and host == dev
    assert run("layout_device", jpeg="device") == 0
    sizes = sorted(len(b) - HEADER_BYTES - 2 for b in host.values())
    stride = (sizes[len(sizes) // 2] + 3) // 4 * 4
    if sizes[0] < stride < sizes[-1]:   # (the layouts' scans may all be of one length class; the texture test covers the fallback)
        assert run("layout_small", jpeg="device", jpeg_stride=stride) == n_host
        assert _files(root / "layout_small") == host
