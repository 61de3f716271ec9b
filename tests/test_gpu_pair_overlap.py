"""salve_bev_pair_overlap on the GPU through BevRasteriser.pair_overlap: every case of tests/overlap_cases.py bit for bit against the numpy
emulator (guard rows intact, the bad-job status bit raised exactly by the bad-job cases), every documented refusal, and equal bytes on a
second run."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib, status  # noqa: E402
from salve_amd.rasteriser import BevRasteriser  # noqa: E402
from tests import overlap_cases as oc  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ras():
    return BevRasteriser(torch.device(DEV))


_uploaded = {}


def upload(arr: np.ndarray):
    """One device copy per stack (the cases of a geometry share their stacks)."""
    if id(arr) not in _uploaded:
        _uploaded[id(arr)] = (arr, torch.from_numpy(arr.view(np.int32).copy()).to(DEV))   # (the array is kept: its id stays its own)
    return _uploaded[id(arr)][1]


def on_gpu(ras):
    def fn(case, buf):
        a = upload(case["bev_a"])
        b = a if case["bev_b"] is case["bev_a"] else upload(case["bev_b"])
        n = len(case["a_index"])
        jobs = ras.upload_overlap_jobs(case["a_index"], case["b_index"])
        dev = torch.from_numpy(buf).to(DEV)
        got = ras.pair_overlap(a, b, jobs, n, out=dev[oc.GUARD:oc.GUARD + n])
        assert tuple(got.shape) == (n, 4)
        buf[:] = dev.cpu().numpy()
        raised = bool(int(status.word(DEV).item()) & _lib.STATUS_BAD_TILE_JOB)
        if raised:
            with pytest.raises(_lib.SalveHipError, match="pair-overlap job"):
                status.check(DEV, case["name"])
        status.check(DEV, case["name"])   # cleared again (and nothing else was raised)
        return raised
    return fn


@pytest.mark.parametrize("geometry", oc.GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}")
def test_every_case_equals_the_emulator(ras, geometry):
    status.check(DEV, "before the pair-overlap cases")
    mine = [c for c in oc.cases() if (c["h"], c["w"]) == geometry]
    assert mine
    for c in mine:
        buf, raised = oc.run_case(c, on_gpu(ras))
        want, want_raised = oc.expected(c)
        assert torch.equal(torch.from_numpy(buf), torch.from_numpy(want)), c["name"]
        assert raised == want_raised == c["bad"], c["name"]


def test_two_runs_give_equal_bytes_and_a_fresh_output_needs_no_zeroing(ras):
    c = next(c for c in oc.cases() if c["name"] == "501x501-random")
    a, b = upload(c["bev_a"]), upload(c["bev_b"])
    jobs = ras.upload_overlap_jobs(c["a_index"], c["b_index"])
    n = len(c["a_index"])
    first = ras.pair_overlap(a, b, jobs, n)
    second = ras.pair_overlap(a, b, jobs, n, out=torch.full((n, 4), 12345, dtype=torch.int32, device=DEV))
    assert first.dtype == torch.int32 and tuple(first.shape) == (n, 4)
    assert first.cpu().numpy().tobytes() == second.cpu().numpy().tobytes()
    assert torch.equal(first.cpu(), torch.from_numpy(oc.expected(c)[0][oc.GUARD:oc.GUARD + n]))
    status.check(DEV, "two runs")


def test_library_refusals(ras):
    lib = ras.lib
    img = torch.zeros((2, 3, 7), dtype=torch.int32, device=DEV)
    jobs = ras.upload_overlap_jobs([0, 1], [1, 0])
    out = torch.full((3, 4), oc.SENTINEL, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(bev_a=p(img), n_a=2, bev_b=p(img), n_b=2, h=3, w=7, jobs_=p(jobs), n=2, out_=p(out)):
        return lib.salve_bev_pair_overlap(bev_a, n_a, bev_b, n_b, h, w, jobs_, n, out_, status.ptr(DEV), ras._stream())

    refused = [dict(h=0), dict(w=0), dict(h=-3), dict(h=46341, w=46341), dict(h=2 ** 16, w=2 ** 15), dict(n_a=-1), dict(n_b=-1), dict(n=-1),
               dict(bev_a=None), dict(bev_b=None), dict(jobs_=None), dict(out_=None),
               dict(out_=ctypes.c_void_p(out.data_ptr() + 4)), dict(bev_a=ctypes.c_void_p(img.data_ptr() + 2))]
    for kw in refused:
        assert call(**kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert b"salve_bev_pair_overlap" in lib.salve_last_error(), kw
    assert call(n=0) == _lib.SALVE_OK and call(n=0, bev_a=None, bev_b=None, jobs_=None, out_=None) == _lib.SALVE_OK   # launches nothing
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == oc.SENTINEL).all()   # no refused call and no empty one wrote a row
    assert call() == _lib.SALVE_OK
    assert out.cpu().numpy().tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [oc.SENTINEL] * 4]
    status.check(DEV, "refusals")


def test_wrapper_refusals(ras):
    img = torch.zeros((2, 3, 7), dtype=torch.int32, device=DEV)
    jobs = ras.upload_overlap_jobs([0], [1])
    bad = [lambda: ras.pair_overlap(img.float(), img, jobs, 1), lambda: ras.pair_overlap(img, img.cpu(), jobs, 1),
           lambda: ras.pair_overlap(img, img[:, :, :5], jobs, 1), lambda: ras.pair_overlap(img, torch.zeros((2, 7, 3), dtype=torch.int32, device=DEV), jobs, 1),
           lambda: ras.pair_overlap(img, img, jobs, 2), lambda: ras.pair_overlap(img, img, jobs.cpu(), 1),
           lambda: ras.pair_overlap(img, img, jobs, 1, out=torch.zeros((1, 4), dtype=torch.int64, device=DEV)),
           lambda: ras.pair_overlap(img, img, jobs, 1, out=torch.zeros((2, 4), dtype=torch.int32, device=DEV)),
           lambda: ras.pair_overlap(img, img, jobs, 1, out=torch.zeros((1, 8), dtype=torch.int32, device=DEV)[:, ::2]),
           lambda: ras.upload_overlap_jobs([0, 1], [0]), lambda: ras.upload_overlap_jobs([2 ** 31], [0])]
    for f in bad:
        with pytest.raises(_lib.SalveHipError):
            f()
    assert ras.pair_overlap(img, img, jobs, 0).shape == (0, 4)
    status.check(DEV, "wrapper refusals")
