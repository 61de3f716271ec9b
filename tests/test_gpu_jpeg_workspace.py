"""The one workspace per stream that BevRasteriser's three JPEG methods share, on the MI355X: the routes interleaved on one rasteriser,
at two sizes, so that the workspace grows and a smaller call reuses the larger buffer, give what each route gives alone on a rasteriser
of its own; and a side stream gets a workspace of its own.  Everything is compared bit for bit; what the routes compute is
tests/test_gpu_jpeg*.py's business."""

import numpy as np
import pytest

import jpeg_cases as jc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import jpeg  # noqa: E402
from salve_amd.rasteriser import BevRasteriser  # noqa: E402

DEV = torch.device("cuda:0")
QUALITY = 75
CONTENTS = ("noise", "stripes", "layout")
SMALL, LARGE = (17, 9), (33, 47)   # ragged right and bottom MCUs; every route needs more workspace at LARGE than at SMALL


def _images(size):
    h, w = size
    return torch.from_numpy(np.stack([jc.pack_bgr(jc.make_image(c, h, w)) for c in CONTENTS]).astype(np.uint32).view(np.int32)).to(DEV)


def _roundtrip(ras, size, files):
    return (ras.jpeg_roundtrip(_images(size), QUALITY),)


def _encode(ras, size, files):
    return ras.jpeg_encode(_images(size), QUALITY)


def _decode(ras, size, files):
    """(pixels, status) of `files`: whole files of `size` that share their header."""
    parsed = [jpeg.parse_file(f) for f in files]
    p = parsed[0]
    assert (p.h, p.w) == size and len({q.header_key for q in parsed}) == 1
    scans = [f[q.scan_offset:q.scan_offset + q.scan_bytes] for f, q in zip(files, parsed)]
    blob = torch.from_numpy(np.frombuffer(b"".join(scans) + bytes(jpeg.SCAN_PADDING), dtype=np.uint8).copy()).to(DEV)
    nb = np.array([len(s) for s in scans], dtype=np.int64)
    return ras.jpeg_decode(blob, np.cumsum(nb) - nb, nb, p.h, p.w, p.qtab, p.huffman)


ROUTES = {"roundtrip": _roundtrip, "encode": _encode, "decode": _decode}


@pytest.fixture(scope="module")
def alone():
    """(route, size) -> the route's tensors from a rasteriser that has made no other JPEG call; "files", size -> the encoder's files."""
    out = {}
    for size in (SMALL, LARGE):
        scan, nbytes = out["encode", size] = _encode(BevRasteriser(DEV), size, None)
        lens = nbytes.cpu().tolist()
        assert max(lens) <= scan.shape[1]
        files = out["files", size] = [jpeg.file_bytes(scan[i, :n].cpu().numpy().tobytes(), size[0], size[1], QUALITY) for i, n in enumerate(lens)]
        out["roundtrip", size] = _roundtrip(BevRasteriser(DEV), size, None)
        out["decode", size] = _decode(BevRasteriser(DEV), size, files)
        assert out["decode", size][1].cpu().tolist() == [0] * len(CONTENTS)
    return out


def _assert_same(route, got, want):
    if route == "encode":   # (scan, nbytes): a slot's bytes beyond nbytes[i] are not written
        assert torch.equal(got[1], want[1])
        for i, n in enumerate(want[1].cpu().tolist()):
            assert torch.equal(got[0][i, :n], want[0][i, :n]), i
    else:                   # (pixels,) or (pixels, status)
        assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))


def test_interleaved_routes_equal_each_route_alone(alone):
    ras = BevRasteriser(DEV)
    sizes = []
    for route, size in (("roundtrip", SMALL), ("encode", LARGE), ("decode", SMALL), ("roundtrip", LARGE), ("decode", LARGE), ("encode", SMALL)):
        _assert_same(route, ROUTES[route](ras, size, alone["files", size]), alone[route, size])
        assert len(ras._jpeg_ws) == 1
        sizes.append(next(iter(ras._jpeg_ws.values())).numel())
    n = len(CONTENTS)
    need = [getattr(ras.lib, f"salve_bev_jpeg_{r}_workspace_bytes")(n, *s) for r, s in (("roundtrip", SMALL), ("encode", LARGE), ("decode", LARGE))]
    assert need[0] < need[2] < need[1]                       # the order above grows the workspace once ...
    assert sizes == [need[0]] + [need[1]] * 5                # ... and every later call, the smaller ones too, reuses the larger buffer
    ras.check("interleaved JPEG routes")


def test_a_side_stream_has_a_workspace_of_its_own(alone):
    ras = BevRasteriser(DEV)
    _roundtrip(ras, SMALL, None)                             # the default stream's workspace
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        got = {route: fn(ras, LARGE, alone["files", LARGE]) for route, fn in ROUTES.items()}
    side.synchronize()
    for route in ROUTES:
        _assert_same(route, got[route], alone[route, LARGE])
    assert sorted(ras._jpeg_ws) == sorted({side.cuda_stream, torch.cuda.default_stream(DEV).cuda_stream})
    assert ras._jpeg_ws[side.cuda_stream] is not ras._jpeg_ws[torch.cuda.default_stream(DEV).cuda_stream]
    ras.check("JPEG routes on a side stream")
