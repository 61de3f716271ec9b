"""salve_floor_align and salve_floor_iou on the GPU, through the C ABI into sentinel-filled buffers: every case of tests/floor_report_cases.py
against the numpy emulator.  Integers are exact -- `best`, n_pairs, the counts, the status bit, inter / union and the masks bit for bit;
salve_floor_iou runs in isolation on the EMULATOR's aligned poses, which makes it exact whatever launch 2 rounds.  The float32 aligned poses
agree within one float32 ulp.  Guard records and records of panoramas in no floor stay untouched; every refusal; equal bytes on a second run.

Float64 outputs differ from the emulator by the device's atan2 / sin / cos against numpy's.  F64_ATOL is four times the largest difference
MEASURED over the cases (profiles/r24_floor_report.txt; the run prints it per case), and by the stated condition may not exceed 1e-9 degrees
or coordinate units: a float32 leak would show as 1e-7.
"""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib, status  # noqa: E402
from tests import floor_report_cases as fc  # noqa: E402

DEV = "cuda:0"
G = fc.GUARD
SALVE_ERR_WORKSPACE = -4
MEASURED_F64_DIFF = 1.421e-14   # profiles/r24_floor_report.txt: two ulps of a rotation error of some 40 degrees
F64_ATOL = 4 * MEASURED_F64_DIFF
assert F64_ATOL <= 1e-9
NAMES = [c["name"] for c in fc.cases()]

_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)
_ptr = lambda t, skip=0: ctypes.c_void_p(t.data_ptr() + skip)
_stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def align(case, bufs, **over):
    """One call of salve_floor_align on `bufs` (the five device byte tensors WITH their guards); `over` replaces arguments by name."""
    lib = _lib.load()
    t = {k: _dev(case[k]) for k in ("node_start", "truth", "est", "hyp_start", "masks", "gt_scale", "metres")}
    a = dict(node_start=_ptr(t["node_start"]), n_floors=len(case["node_start"]) - 1, n_nodes=case["n_nodes"], truth=_ptr(t["truth"]), est=_ptr(t["est"]),
             hyp_start=_ptr(t["hyp_start"]), hyp_mask=_ptr(t["masks"]), n_hyps=len(case["masks"]), gt_scale=_ptr(t["gt_scale"]), metres=_ptr(t["metres"]),
             out_hyps=_ptr(bufs[0], G * fc.HYP_OUT.itemsize), out_nodes=_ptr(bufs[1], G * fc.NODE.itemsize), out_rot=_ptr(bufs[2], G * 8),
             out_trans=_ptr(bufs[3], G * 8), out_floors=_ptr(bufs[4], G * fc.FLOOR_OUT.itemsize), status=status.ptr(DEV), stream=_stream())
    a.update(over)
    rc = lib.salve_floor_align(*a.values())
    torch.cuda.synchronize()
    return rc


def iou(case, est_table, bufs, ws=None, **over):
    """One call of salve_floor_iou on `bufs` = (out, masks) with their guards."""
    lib = _lib.load()
    words = (case["img_w"] + 31) // 32
    t = {k: _dev(case[k]) for k in ("room_xy", "room_off", "node_start", "truth", "metres")}
    t["est"] = _dev(est_table)
    ws_bytes = int(lib.salve_floor_iou_workspace_bytes(len(case["room_xy"]), case["n_nodes"]))
    if ws is None:
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=DEV)
    a = dict(room_xy=_ptr(t["room_xy"]), room_off=_ptr(t["room_off"]), n_room_xy=len(case["room_xy"]), node_start=_ptr(t["node_start"]),
             n_floors=len(case["node_start"]) - 1, n_nodes=case["n_nodes"], est=_ptr(t["est"]), truth=_ptr(t["truth"]), metres=_ptr(t["metres"]),
             img_h=case["img_h"], img_w=case["img_w"], off_x=case["off"][0], off_y=case["off"][1], ppm=case["ppm"], out=_ptr(bufs[0], G * fc.IOU_OUT.itemsize),
             out_masks=_ptr(bufs[1], G * words * 4), workspace=_ptr(ws), workspace_bytes=ws_bytes, status=status.ptr(DEV), stream=_stream())
    a.update(over)
    rc = lib.salve_floor_iou(*a.values())
    torch.cuda.synchronize()
    return rc


def _raised(what):
    raised = bool(int(status.word(DEV).item()) & _lib.STATUS_BAD_FLOOR_TABLE)
    if raised:
        with pytest.raises(_lib.SalveHipError, match="floor-report table"):
            status.check(DEV, what)
    status.check(DEV, what)   # cleared again (and nothing else was raised)
    return raised


def align_on_gpu(case):
    host = fc.fresh_align_buffers(case)
    bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in host]
    assert align(case, bufs) == _lib.SALVE_OK, _lib.load().salve_last_error()
    return [b.cpu().numpy().view(h.dtype) for b, h in zip(bufs, host)], _raised(case["name"])


def iou_on_gpu(case, est):
    host = fc.fresh_iou_buffers(case)
    bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in host]
    assert iou(case, est, bufs) == _lib.SALVE_OK, _lib.load().salve_last_error()
    return [b.cpu().numpy().view(h.dtype) for b, h in zip(bufs, host)], _raised(case["name"])


_ALIGN, _IOU = {}, {}


def align_result(name):
    if name not in _ALIGN:
        _ALIGN[name] = align_on_gpu(fc.case(name))
    return _ALIGN[name]


def iou_result(name):
    if name not in _IOU:
        c = fc.case(name)
        _IOU[name] = iou_on_gpu(c, fc.raster_est(c))
    return _IOU[name]


@pytest.mark.parametrize("name", NAMES)
def test_alignment_equals_the_emulator(name):
    status.check(DEV, "before the floor-report cases")
    got, raised = align_result(name)
    want, want_raised = fc.expected_align(name)
    diffs, worst = fc.differences(got, want, f64_atol=F64_ATOL)
    print(f"{name}: largest float64 difference from the emulator {worst:.3e}")
    assert raised == want_raised and (not raised or fc.case(name)["launch_checked"])
    assert diffs == [], name


@pytest.mark.parametrize("name", NAMES)
def test_iou_equals_the_emulator_bit_for_bit(name):
    status.check(DEV, "before the floor-report cases")
    got, raised = iou_result(name)
    want, want_raised, _ = fc.expected_iou(name)
    assert raised == want_raised
    diffs, worst = fc.differences(got, want, f64_atol=0.0)   # (the IoU is one division of two exact integers)
    assert diffs == [] and worst == 0.0, name


def test_iou_without_masks_gives_the_same_counts():
    c = fc.case("raster-45x83")
    host = fc.fresh_iou_buffers(c)
    bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in host]
    assert iou(c, fc.raster_est(c), bufs, out_masks=ctypes.c_void_p(None)) == _lib.SALVE_OK
    status.check(DEV, "no masks")
    assert bufs[0].cpu().numpy().tobytes() == iou_result("raster-45x83")[0][0].tobytes()
    assert (bufs[1].cpu().numpy() == fc.SENTINEL).all()


def test_two_runs_give_equal_bytes():
    for name in ("thousand-hypotheses", "300-floors", "sizes"):
        first, _ = align_result(name)
        second, _ = align_on_gpu(fc.case(name))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)), name
    for name in ("raster-45x83", "raster-501x501", "300-floors"):
        c = fc.case(name)
        first, _ = iou_result(name)
        second, _ = iou_on_gpu(c, fc.raster_est(c))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)), name


def test_align_refusals():
    lib = _lib.load()
    case = fc.case("sizes")
    bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in fc.fresh_align_buffers(case)]
    untouched = lambda bs: all((b.cpu().numpy() == fc.SENTINEL).all() for b in bs)
    null, odd = ctypes.c_void_p(None), lambda i, by=4: ctypes.c_void_p(bufs[i].data_ptr() + by)
    refused = [dict(n_floors=-1), dict(n_nodes=-1), dict(n_hyps=-1), dict(node_start=null), dict(truth=null), dict(est=null), dict(hyp_start=null),
               dict(hyp_mask=null), dict(gt_scale=null), dict(metres=null), dict(out_hyps=null), dict(out_nodes=null), dict(out_rot=null),
               dict(out_trans=null), dict(out_floors=null), dict(truth=odd(1)), dict(est=odd(1)), dict(out_hyps=odd(0)), dict(out_nodes=odd(1)),
               dict(out_rot=odd(2)), dict(out_trans=odd(3)), dict(out_floors=odd(4)), dict(hyp_mask=odd(0, 2)), dict(node_start=odd(0, 2))]
    for kw in refused:
        assert align(case, bufs, **kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert b"salve_floor_align" in lib.salve_last_error(), kw
    assert align(case, bufs, n_floors=0) == _lib.SALVE_OK   # launches nothing
    assert untouched(bufs)
    status.check(DEV, "refusals")
    assert align(case, bufs) == _lib.SALVE_OK and not untouched(bufs)
    status.check(DEV, "after the refusals")


def test_iou_refusals():
    lib = _lib.load()
    case = fc.case("raster-17x33")
    est = fc.raster_est(case)
    bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in fc.fresh_iou_buffers(case)]
    untouched = lambda bs: all((b.cpu().numpy() == fc.SENTINEL).all() for b in bs)
    null, odd = ctypes.c_void_p(None), lambda i, by=4: ctypes.c_void_p(bufs[i].data_ptr() + by)
    nan, inf = float("nan"), float("inf")
    refused = [dict(n_floors=-1), dict(n_nodes=-1), dict(n_room_xy=-1), dict(img_h=0), dict(img_w=0), dict(img_h=32001), dict(img_w=-5), dict(off_x=nan),
               dict(off_y=inf), dict(ppm=nan), dict(n_floors=2 ** 31 - 1), dict(room_xy=null), dict(room_off=null), dict(node_start=null), dict(est=null),
               dict(truth=null), dict(metres=null), dict(out=null), dict(workspace=null), dict(out=odd(0)), dict(est=odd(0)), dict(room_off=odd(0)),
               dict(out_masks=odd(1, 2)), dict(workspace=odd(0, 8))]
    for kw in refused:
        assert iou(case, est, bufs, **kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert b"salve_floor_iou" in lib.salve_last_error(), kw
    ws_bytes = int(lib.salve_floor_iou_workspace_bytes(len(case["room_xy"]), case["n_nodes"]))
    assert ws_bytes == 16 + 2 * (16 * case["n_nodes"] + 8 * len(case["room_xy"])) and lib.salve_floor_iou_workspace_bytes(-1, 4) == 0
    assert iou(case, est, bufs, workspace_bytes=ws_bytes - 1) == SALVE_ERR_WORKSPACE and b"salve_floor_iou" in lib.salve_last_error()
    assert iou(case, est, bufs, n_floors=0) == _lib.SALVE_OK   # launches nothing
    assert untouched(bufs)
    status.check(DEV, "refusals")
    assert iou(case, est, bufs) == _lib.SALVE_OK and not untouched(bufs)
    status.check(DEV, "after the refusals")
