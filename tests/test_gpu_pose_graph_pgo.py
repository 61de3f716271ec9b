"""salve_pose_graph_optimise on the GPU, through the C ABI into sentinel-filled buffers with guards: every case of tests/pgo_cases.py against the
float64 emulator.  The integer outputs -- counts, stop_reason, localized / parent / depth, the status bit -- and lambda (an IEEE sequence with no
rounded input) are compared EXACTLY: tests/test_pgo_cases_host.py shows that no case decides within 1e-6 of a threshold.  The float64 poses and
costs are compared within F64_BOUND, four times the largest difference measured on an MI355X (profiles/r25_pose_graph_pgo.txt), capped at 1e-9
so that a float32 leak (1e-7) cannot hide; the emulator alone moves by at most 1e-11 under an ulp on every sin / cos / atan2.  The float32
records are the float32 of the device's own float64 outputs, exactly.  Guards, the records past n_nodes, and everything else the entry does not
document stay untouched; two runs give the same bytes; every floor of the 70-floor launch has the bytes of its one-floor launch; every
documented refusal refuses."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib, status  # noqa: E402
from tests import pgo_cases as pc  # noqa: E402

DEV = "cuda:0"
SALVE_ERR_WORKSPACE = -4
# The largest difference from the emulator over the case list, measured on an MI355X (profiles/r25_pose_graph_pgo.txt): poses absolutely, costs
# relative to max(1, |cost|).  The bound is 4 x that, and never above 1e-9.
F64_MEASURED = 7.285e-13
F64_BOUND = min(4 * F64_MEASURED, 1e-9)

NAMES = [c["name"] for c in pc.cases()]
G = pc.GUARD


def optimise(case, bufs, ws="own", **override):
    """One call of the entry on `bufs` = (out_nodes, out_pose, out_floors) device byte tensors WITH their guards; returns its status."""
    lib = _lib.load()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(DEV)
    keep = [dev(case["rows"]) if len(case["rows"]) else torch.zeros(8, dtype=torch.uint8, device=DEV), dev(case["floor_start"]), dev(case["n_nodes"]),
            dev(case["init"])]
    P = pc.params(case)
    a = {"rows": ctypes.c_void_p(keep[0].data_ptr()), "n_rows": len(case["rows"]), "n_floors": len(case["n_nodes"]), "max_nodes": case["max_nodes"],
         "init": ctypes.c_void_p(keep[3].data_ptr()), "confidence_threshold": P["confidence_threshold"], "robust": P["robust"], "huber_k": P["huber_k"],
         "odometry_sigmas": P["odometry_sigmas"], "prior_sigmas": P["prior_sigmas"], "max_iterations": P["max_iterations"],
         "relative_error_tol": P["relative_error_tol"], "absolute_error_tol": P["absolute_error_tol"],
         "out_nodes": ctypes.c_void_p(bufs[0].data_ptr() + G * 48), "out_pose": ctypes.c_void_p(bufs[1].data_ptr() + G * 24)}
    a.update(override)
    need = int(lib.salve_pose_graph_optimise_workspace_bytes(max(a["n_floors"], 0), a["max_nodes"]))
    work = torch.empty(max(need, 8), dtype=torch.uint8, device=DEV)
    ws_ptr, ws_bytes = (ctypes.c_void_p(work.data_ptr()), need) if ws == "own" else ws
    sig = lambda s: None if s is None else (ctypes.c_double * 3)(*s)
    rc = lib.salve_pose_graph_optimise(a["rows"], a["n_rows"], ctypes.c_void_p(keep[1].data_ptr()), ctypes.c_void_p(keep[2].data_ptr()), a["n_floors"],
                                       a["max_nodes"], float(a["confidence_threshold"]), a["init"], int(a["robust"]), float(a["huber_k"]),
                                       sig(a["odometry_sigmas"]), sig(a["prior_sigmas"]), int(a["max_iterations"]), float(a["relative_error_tol"]),
                                       float(a["absolute_error_tol"]), a["out_nodes"], a["out_pose"], ctypes.c_void_p(bufs[2].data_ptr() + G * 48),
                                       ws_ptr, ws_bytes, status.ptr(DEV), ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream))
    torch.cuda.synchronize()
    return rc


def on_gpu(case):
    """(the three buffers with their guards as the device left them, was the status bit raised)"""
    host = pc.fresh_buffers(case)
    bufs = [torch.from_numpy(b.view(np.uint8).reshape(-1)).to(DEV) for b in host]
    assert optimise(case, bufs) == _lib.SALVE_OK, _lib.load().salve_last_error()
    got = tuple(b.cpu().numpy().view(h.dtype).reshape(h.shape) for b, h in zip(bufs, host))
    raised = bool(int(status.word(DEV).item()) & _lib.STATUS_BAD_GRAPH_ROW)
    if raised:
        with pytest.raises(_lib.SalveHipError, match="pose-graph rows"):
            status.check(DEV, case["name"])
    status.check(DEV, case["name"])   # cleared again (and nothing else was raised)
    return got, raised


_RESULTS = {}


def result(name):
    if name not in _RESULTS:
        _RESULTS[name] = on_gpu(pc.case(name))
    return _RESULTS[name]


def f64_difference(got, want):
    """The largest difference of two float64 arrays that must be NaN (and sentinel) in the same places; relative to max(1, |want|)."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    m = ~np.isnan(want)
    inf = m & ~np.isfinite(want)
    assert np.array_equal(got[inf], want[inf])
    m &= np.isfinite(want)
    return float((np.abs(got[m] - want[m]) / np.maximum(1.0, np.abs(want[m]))).max()) if m.any() else 0.0


@pytest.mark.parametrize("name", NAMES)
def test_every_case_equals_the_emulator(name):
    status.check(DEV, "before the pgo cases")
    case = pc.case(name)
    (nodes, pose, floors), raised = result(name)
    res = pc.expected(name)
    want_nodes, want_pose, want_floors = pc.expected_buffers(case, res)
    assert raised == any(r["raised"] for r in res) == (name == "70-floors")
    for k in ("n_unknown_nodes", "n_factors", "n_iterations", "n_rejected", "n_downweighted", "stop_reason", "lambda"):
        assert floors[k].tobytes() == want_floors[k].tobytes(), (name, k, floors[k][G:-G], want_floors[k][G:-G])   # (with the guards' bytes)
    for k in ("localized", "parent", "depth", "reserved", "s"):
        assert nodes[k].tobytes() == want_nodes[k].tobytes(), (name, k)
    # the float64 outputs: sentinel bytes where the entry writes nothing (guards, the records past n_nodes), the emulator's within the bound elsewhere
    untouched = want_pose.view(np.uint64) == np.frombuffer(bytes([pc.SENTINEL]) * 8, dtype="<u8")[0]
    assert np.array_equal(pose.view(np.uint64)[untouched], want_pose.view(np.uint64)[untouched]), name
    written = ~untouched
    d_pose = f64_difference(pose[written], want_pose[written])
    d_cost = max(f64_difference(floors[k][G:-G], want_floors[k][G:-G]) for k in ("cost_initial", "cost_final"))
    for k in ("cost_initial", "cost_final"):
        assert floors[k][:G].tobytes() == want_floors[k][:G].tobytes() and floors[k][-G:].tobytes() == want_floors[k][-G:].tobytes()
    # the float32 records: the float32 of the emulator's poses wherever those of the device are (compared exactly against the device's below)
    d_rec = max(float(np.abs(nodes[k][G:-G].astype(np.float64) - want_nodes[k][G:-G].astype(np.float64)).max()) for k in ("R", "t"))
    print(f"{name}: largest difference from the emulator: poses {d_pose:.3e}, costs {d_cost:.3e} (relative to max(1, |cost|)), float32 records {d_rec:.3e}")
    assert max(d_pose, d_cost) <= F64_BOUND, (name, d_pose, d_cost)
    assert d_rec <= 1e-6 * max(1.0, float(np.abs(want_nodes["t"][G:-G]).max()))   # (a float32 ulp of the largest coordinate)


@pytest.mark.parametrize("name", NAMES)
def test_float32_records_are_the_float32_of_the_float64_outputs(name):
    (nodes, pose, _), _ = result(name)
    case = pc.case(name)
    M = case["max_nodes"]
    for f, n in enumerate(case["n_nodes"]):
        n = int(n) if 0 <= n <= M else 0
        rec, p = nodes[G + f * M:G + f * M + n], pose[G + f * M:G + f * M + n]
        loc = rec["localized"] == 1
        assert np.array_equal(np.isnan(p[:, 0]), ~loc) and np.array_equal(np.isnan(p), np.isnan(p[:, :1]).repeat(3, 1))
        assert (rec["R"][~loc] == 0).all() and (rec["t"][~loc] == 0).all() and (rec["s"][~loc] == 0).all() and (rec["parent"][~loc] == -1).all()
        c, s = np.cos(p[loc, 2]).astype(np.float32), np.sin(p[loc, 2]).astype(np.float32)
        assert rec["R"][loc].tobytes() == np.stack([c, -s, s, c], 1).tobytes(), (name, f)
        assert rec["t"][loc].tobytes() == p[loc, :2].astype(np.float32).tobytes() and (rec["s"][loc] == 1.0).all(), (name, f)


def test_two_runs_give_equal_bytes():
    for name in ("far-off-start", "57-nodes", "70-floors"):
        first, _ = result(name)
        second, _ = on_gpu(pc.case(name))
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes(), name


def test_every_floor_of_the_launch_has_the_bytes_of_its_one_floor_launch():
    case = pc.case("70-floors")
    (nodes, pose, floors), _ = result("70-floors")
    M = case["max_nodes"]
    for f in range(len(case["n_nodes"])):
        (n1, p1, f1), raised = on_gpu(pc.single_floor_launch(case, f))
        assert raised == (f in pc.MALFORMED_70), f
        assert n1[G:G + M].tobytes() == nodes[G + f * M:G + (f + 1) * M].tobytes(), f
        assert p1[G:G + M].tobytes() == pose[G + f * M:G + (f + 1) * M].tobytes(), f
        assert f1[G].tobytes() == floors[G + f].tobytes(), f


def test_library_refusals():
    lib = _lib.load()
    case = pc.case("57-nodes")
    host = pc.fresh_buffers(case)
    bufs = [torch.from_numpy(b.view(np.uint8).reshape(-1)).to(DEV) for b in host]
    untouched = lambda: all((b.cpu().numpy() == pc.SENTINEL).all() for b in bufs)
    nan = float("nan")
    refused = [dict(max_nodes=0), dict(max_nodes=-1), dict(max_nodes=257), dict(n_floors=-1), dict(n_rows=-1), dict(confidence_threshold=nan),
               dict(robust=2), dict(robust=-1), dict(huber_k=0.0), dict(huber_k=nan), dict(huber_k=-1.0), dict(odometry_sigmas=(0.2, 0.0, 0.1)),
               dict(odometry_sigmas=(nan, 0.2, 0.1)), dict(prior_sigmas=(0.3, 0.3, -0.1)), dict(prior_sigmas=None), dict(odometry_sigmas=None),
               dict(relative_error_tol=0.0), dict(relative_error_tol=nan), dict(absolute_error_tol=-1e-5), dict(absolute_error_tol=nan),
               dict(max_iterations=-1), dict(rows=ctypes.c_void_p(None)), dict(init=ctypes.c_void_p(None)), dict(out_pose=ctypes.c_void_p(None)),
               dict(out_nodes=ctypes.c_void_p(bufs[0].data_ptr() + 4)), dict(out_pose=ctypes.c_void_p(bufs[1].data_ptr() + 4)),
               dict(init=ctypes.c_void_p(bufs[0].data_ptr() + 4))]
    for kw in refused:
        assert optimise(case, bufs, **kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert b"salve_pose_graph_optimise" in lib.salve_last_error(), kw
    need = int(lib.salve_pose_graph_optimise_workspace_bytes(1, 64))
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert need == 8 * (192 * 193 // 2)
    assert optimise(case, bufs, ws=(ctypes.c_void_p(work.data_ptr()), need - 1)) == SALVE_ERR_WORKSPACE
    assert optimise(case, bufs, ws=(ctypes.c_void_p(None), need)) == SALVE_ERR_WORKSPACE
    assert optimise(case, bufs, ws=(ctypes.c_void_p(work.data_ptr() + 4), need)) == _lib.SALVE_ERR_BAD_ARG
    assert optimise(case, bufs, n_floors=0) == _lib.SALVE_OK   # launches nothing
    assert untouched()
    small = pc.case("triangle-huber")   # max_nodes <= SALVE_PGO_LDS_NODES: no workspace, NULL accepted
    small_bufs = [torch.from_numpy(b.view(np.uint8).reshape(-1)).to(DEV) for b in pc.fresh_buffers(small)]
    assert lib.salve_pose_graph_optimise_workspace_bytes(1, 3) == 0 and optimise(small, small_bufs, ws=(ctypes.c_void_p(None), 0)) == _lib.SALVE_OK
    assert small_bufs[2].cpu().numpy().tobytes() == result("triangle-huber")[0][2].tobytes()
    status.check(DEV, "refusals")
    assert optimise(case, bufs) == _lib.SALVE_OK and not untouched()
    status.check(DEV, "after the refusals")
