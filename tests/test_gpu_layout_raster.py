"""`salve_layout_rasterise` on the MI355X against the oracle over its accepted contract (tests/layout_raster_cases.py): every case in
one launch through the C ABI, bit for bit; every pixel of the batch written and nothing around it; the same bits again, through a
slice of the record table and on a side stream; the refusals; one non-square window through the Python wrapper."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import layout_raster_cases as rc  # noqa: E402
from oracle import layout_oracle as lo  # noqa: E402
from salve_amd import _lib, layout, status  # noqa: E402
from salve_amd.common.bevparams import BEVParams  # noqa: E402

DEV = torch.device("cuda:0")
SENTINEL = 0x5A5A5A5A   # no pixel: the kernel's words have a zero top byte
REC_BYTES = _lib.LAYOUT_DTYPE.itemsize


def _ptr(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset)


class _Tables:
    def __init__(self, case):
        rec, poly, segs = case.tables()
        self.n, self.hw = len(rec), case.hw
        self.rec = torch.from_numpy(rec.view(np.uint8)).to(DEV)
        self.poly, self.segs = torch.from_numpy(poly).to(DEV), torch.from_numpy(segs).to(DEV)
        self.word = torch.zeros(1, dtype=torch.int32, device=DEV)

    def run(self, first=0):
        """Images [first, n) in ONE launch into a sentinel-filled buffer with one image in front and one behind -> int32 [n - first + 2, H, W]."""
        n, (H, W) = self.n - first, self.hw
        out = torch.full((n + 2, H, W), SENTINEL, dtype=torch.int32, device=DEV)
        st = _lib.load().salve_layout_rasterise(_ptr(self.rec, first * REC_BYTES), n, _ptr(self.poly), _ptr(self.segs), H, W, _ptr(out[1:]), _ptr(self.word),
                                                ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        assert st == _lib.SALVE_OK, _lib.load().salve_last_error()
        return out


def _check(tab, out, want, what):
    """out: `_Tables.run`'s buffer; want: int32 [n, H, W] words of the oracle."""
    got = out.cpu().numpy()
    assert int(tab.word.item()) == 0, f"{what}: device status word {int(tab.word.item())}"
    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), f"{what}: written outside the batch"
    got = got[1:-1]
    assert got.shape == want.shape
    unwritten = np.argwhere(got == SENTINEL)
    assert len(unwritten) == 0, f"{what}: {len(unwritten)} pixels not written, first (image, row, column) {unwritten[:5].tolist()}"
    if not np.array_equal(got, want):
        bad = [i for i in range(len(want)) if not np.array_equal(got[i], want[i])]
        i = bad[0]
        at = np.argwhere(got[i] != want[i])
        first = [(int(r), int(c), hex(int(got[i][r, c])), hex(int(want[i][r, c]))) for r, c in at[:5]]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} images differ (first {bad[:8]}); image {i}: {len(at)} pixels differ, "
                             f"(row, column, got, want) {first}; top byte set in {int((got >> 24 != 0).sum())} words")


@pytest.mark.parametrize("cid", [c.id for c in rc.cases()])
def test_kernel_equals_oracle_bit_for_bit(cid):
    case = rc.case(cid)
    want = rc.words(rc.expected(case))
    tab = _Tables(case)
    _check(tab, tab.run(), want, cid)
    first = max(1, tab.n // 3)       # through a slice of the record table, as PackedLayouts.rasterise launches
    _check(tab, tab.run(first), want[first:], f"{cid} from record {first}")


@pytest.mark.parametrize("cid", ["chunks-45x83", "polygons-83x45", "workload-501x501"])
def test_same_bits_again_and_on_a_side_stream(cid):
    tab = _Tables(rc.case(cid))
    a, b = tab.run(), tab.run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        c = tab.run()
    side.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and int(tab.word.item()) == 0
    assert bool((a[1:-1] != SENTINEL).all())


def test_refusals_launch_nothing():
    case = rc.case("chunks-45x83")
    tab = _Tables(case)
    H, W = case.hw
    lib = _lib.load()
    out = torch.full((tab.n, H, W), SENTINEL, dtype=torch.int32, device=DEV)

    def call(**kw):
        a = dict(rec=_ptr(tab.rec), n=tab.n, h=H, w=W, out=_ptr(out))
        a.update(kw)
        return lib.salve_layout_rasterise(a["rec"], a["n"], _ptr(tab.poly), _ptr(tab.segs), a["h"], a["w"], a["out"], _ptr(tab.word),
                                          ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))

    for kw in (dict(n=-1), dict(n=65536), dict(rec=None), dict(out=None), dict(h=0), dict(w=0), dict(h=-1), dict(w=-45), dict(h=32001), dict(w=32001)):
        assert call(**kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert lib.salve_last_error().decode() != "", kw
    assert call(n=0) == _lib.SALVE_OK and call(n=0, rec=None, out=None) == _lib.SALVE_OK
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and int(tab.word.item()) == 0
    assert call() == _lib.SALVE_OK
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), rc.words(rc.expected(case))) and int(tab.word.item()) == 0


def _specs_in_pixels(layouts, metres):
    """Layout specs whose vertices land on the given (fractional) pixel positions: `metres` maps a pixel coordinate array to metres."""
    return [(metres(np.asarray(room, dtype=np.float64)), [(kind, metres(np.asarray(v, dtype=np.float64))) for kind, v in wdos]) for room, wdos in layouts]


def test_python_wrapper_with_a_non_square_window():
    """BEVParams(img_h=44, img_w=82) draws 45 x 83 images.  Its window starts at 0 m (half extents int(0.82) = int(0.44) = 0) and the
    oracle's `to_pixels` at -5 m, so the same PIXEL positions -- a third of a pixel off the grid, far from any rounding tie -- are
    written in metres for each: wrapper x = q / 75, oracle x = (q / 50 - 5) / 1.5."""
    bp = BEVParams(img_h=44, img_w=82)
    assert (bp.img_h + 1, bp.img_w + 1) == (45, 83) and bp.xlims == [0, 0] and bp.ylims == [0, 0]
    off = np.array([0.3, -0.3])
    ring = np.array([[6, 5], [70, 4], [76, 30], [40, 28], [38, 52], [4, 40]]) + off          # leaves the window at the top (row 52 > 44)
    layouts = [(np.vstack([ring, ring[:1]]), [("doors", ring[0:2] + [[8, 0], [-30, 0]]), ("windows", ring[2:4] + [[-3, 0], [9, 0]]), ("openings", ring[4:6]),
                                               ("windows", np.array([[-9.0, 20.0], [10.0, 33.0]]) + off)]),
               (np.array([[10, 10], [60, 12], [30, 40], [10, 10]]) + off, []),
               (np.array([[90, -5], [-8, -6], [-7, 60], [95, 55], [90, -5]]) + off, [("doors", np.array([[0, 0], [82, 44]]) + off)])]   # the window covered
    mine = _specs_in_pixels(layouts, lambda q: q / 75.0)
    theirs = _specs_in_pixels(layouts, lambda q: (q / 50.0 - 5.0) / 1.5)
    for (room, wdos), (oroom, owdos) in zip(mine, theirs):   # both chains reach the same integer pixels
        assert np.array_equal(layout.world_to_pixels(bp, room * 1.5), lo.to_pixels(oroom * 1.5))
        assert all(np.array_equal(layout.world_to_pixels(bp, a[1] * 1.5), lo.to_pixels(b[1] * 1.5)) for a, b in zip(wdos, owdos))
    for render_mask in (True, False):
        got = layout.rasterise_layouts(mine, DEV, bev_params=bp, render_mask=render_mask)
        status.check(DEV, "non-square window")
        assert tuple(got.shape) == (3, 45, 83) and got.dtype == torch.int32
        got = got.cpu().numpy()
        for k, (room, wdos) in enumerate(theirs):
            want = rc.words(lo.rasterize_single_layout(room, wdos, img_hw=(45, 83), render_mask=render_mask))
            assert want.any()
            assert np.array_equal(got[k], want), f"layout {k}, render_mask {render_mask}: {int((got[k] != want).sum())} pixels differ"
