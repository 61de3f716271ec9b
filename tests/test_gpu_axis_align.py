"""salve_pose_graph_axis_align on the GPU, through the C ABI into sentinel-filled buffers with guards: every case of tests/axis_align_cases.py
against the numpy emulator -- statuses, counts, copied rows and copied fields bit for bit, the aligned poses and the corrections within the
derived tolerances of axis_align_cases (8 float32 ulps of the row angle at 180 degrees, times the lever arm for the translation); guard records
and the rows of floors with a malformed extent intact; the status bit raised exactly by the malformed cases; every documented refusal; equal
bytes on a second run; rows that are not applied bit-identical copies."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib, status  # noqa: E402
from tests import axis_align_cases as ac  # noqa: E402

DEV = "cuda:0"
NAMES = [c["name"] for c in ac.cases()]
TABLES = ("rows", "floor_start", "n_nodes", "row_wdo", "pano_base", "room_off", "room_xy", "wdo_off", "wdo_xy", "wdo_type", "vanishing_deg")


def align(case, bufs, **override):
    """One call of the entry on `bufs` = (out_rows, out_axis, out_floors) device byte tensors WITH their guards; returns its status.
    override: arguments by name (a ctypes pointer for a table, an int for a count)."""
    lib = _lib.load()
    dev = {k: torch.from_numpy(np.ascontiguousarray(case[k]).reshape(-1).view(np.uint8).copy()).to(DEV) for k in TABLES}
    a = {k: (ctypes.c_void_p(t.data_ptr()) if t.numel() else None) for k, t in dev.items()}
    a.update(n_rows=len(case["rows"]), n_floors=len(case["n_nodes"]), n_room_xy=len(case["room_xy"]), n_wdo=len(case["wdo_type"]),
             n_panos=len(case["vanishing_deg"]), status=status.ptr(DEV))
    for k, b, dt in zip(("out_rows", "out_axis", "out_floors"), bufs, (ac.ROW, ac.ROW_OUT, ac.FLOOR_OUT)):
        a[k] = ctypes.c_void_p(b.data_ptr() + ac.GUARD * dt.itemsize)
    a.update(override)
    rc = lib.salve_pose_graph_axis_align(a["rows"], a["n_rows"], a["floor_start"], a["n_nodes"], a["n_floors"], a["row_wdo"], a["pano_base"], a["room_off"],
                                         a["room_xy"], a["n_room_xy"], a["wdo_off"], a["wdo_xy"], a["wdo_type"], a["n_wdo"], a["vanishing_deg"], a["n_panos"],
                                         a["out_rows"], a["out_axis"], a["out_floors"], a["status"],
                                         ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream))
    torch.cuda.synchronize()
    return rc


def on_gpu(case):
    """(the three buffers with their guards as the device left them, was the status bit raised)"""
    host = ac.fresh_buffers(case)
    bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in host]
    assert align(case, bufs) == _lib.SALVE_OK, _lib.load().salve_last_error()
    got = tuple(b.cpu().numpy().view(h.dtype) for b, h in zip(bufs, host))
    raised = bool(int(status.word(DEV).item()) & _lib.STATUS_BAD_AXIS_ROW)
    if raised:
        with pytest.raises(_lib.SalveHipError, match="axis-alignment row"):
            status.check(DEV, case["name"])
    status.check(DEV, case["name"])   # cleared again (and nothing else was raised)
    return got, raised


_RESULTS = {}


def result(name):
    if name not in _RESULTS:
        _RESULTS[name] = on_gpu(ac.case(name))
    return _RESULTS[name]


@pytest.mark.parametrize("name", NAMES)
def test_every_case_equals_the_emulator(name):
    status.check(DEV, "before the axis-alignment cases")
    case = ac.case(name)
    got, raised = result(name)
    want, want_raised, details = ac.expected(case)
    assert raised == want_raised == case["malformed"]
    worst = ac.compare(case, got, want, details)   # (asserts everything exact: statuses, counts, copies, sentinels, guards)
    print(f"{name}: largest difference / tolerance {worst}")
    assert max(worst.values()) <= 1.0, (name, worst)


def test_rows_that_are_not_applied_are_bit_identical_copies():
    seen = set()
    for name in NAMES:
        case = ac.case(name)
        (rows, axis, _), _ = result(name)
        inner_rows, inner_axis = rows[ac.GUARD:-ac.GUARD], axis[ac.GUARD:-ac.GUARD]
        for st in (ac.TOO_LARGE, ac.NO_ANGLE, ac.NO_ROOM, ac.MALFORMED):
            m = (inner_axis["status"] == st) & (inner_axis["reserved"] == 0)
            assert inner_rows[m].tobytes() == case["rows"][m].tobytes(), (name, st)
            if m.any():
                seen.add(st)
        m = (inner_axis["status"] == ac.APPLIED) & (inner_axis["reserved"] == 0)
        for k in ("i1", "i2", "prob", "y_hat"):
            assert inner_rows[k][m].tobytes() == case["rows"][k][m].tobytes(), (name, k)
        assert (inner_rows["s"][m] == 1.0).all()
    assert seen == {ac.TOO_LARGE, ac.NO_ANGLE, ac.NO_ROOM, ac.MALFORMED}


def test_two_runs_give_equal_bytes():
    for name in ("257-rows", "two-floors-and-an-empty-one", "malformed-tables"):
        first, _ = result(name)
        second, _ = on_gpu(ac.case(name))
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes(), name


def test_library_refusals():
    lib = _lib.load()
    case = ac.case("65-rows")
    bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in ac.fresh_buffers(case)]
    untouched = lambda: all((b.cpu().numpy() == ac.SENTINEL).all() for b in bufs)
    null, odd = ctypes.c_void_p(None), lambda k: ctypes.c_void_p(bufs[0].data_ptr() + k)
    refused = [dict(n_rows=-1), dict(n_floors=-1), dict(n_room_xy=-1), dict(n_wdo=-1), dict(n_panos=-1)]
    refused += [{k: null} for k in TABLES + ("out_rows", "out_axis", "out_floors")]
    refused += [{k: odd(4)} for k in ("rows", "room_off", "room_xy", "wdo_off", "wdo_xy", "vanishing_deg", "out_rows", "out_axis")]
    refused += [{k: odd(2)} for k in ("row_wdo", "floor_start", "n_nodes", "pano_base", "out_floors", "status")]
    for kw in refused:
        assert align(case, bufs, **kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert b"salve_pose_graph_axis_align" in lib.salve_last_error(), kw
    assert untouched()
    assert align(case, bufs, n_floors=0) == _lib.SALVE_OK and untouched()   # launches nothing
    status.check(DEV, "refusals")
    assert align(case, bufs, status=None) == _lib.SALVE_OK and not untouched()   # (the status word is optional)
    status.check(DEV, "after the refusals")
