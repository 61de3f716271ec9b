"""salve_pose_graph_solve on the GPU, through the C ABI into sentinel-filled buffers: every case of tests/pose_graph_cases.py against the numpy
emulator -- flags, counts, parents, depths, poses and min_trans_err bit for bit, min_rot_err (the one value that carries the device's atan2f)
within MIN_ROT_ERR_RTOL; guard records and the node records past n_nodes intact; the status bit raised exactly by the malformed case; every
documented refusal; equal bytes on a second run."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib, status  # noqa: E402
from tests import pose_graph_cases as pc  # noqa: E402

DEV = "cuda:0"
# min_rot_err = |atan2f(R10, R00)| * (float)(180 / pi) against numpy's arctan2: the largest relative difference over the case list was measured on an
# MI355X as 1.362e-7 (profiles/r19_pose_graph.txt: between one and two float32 ulp); the bound is 4 x that.  (Capped at 1e-5: a few float32 ulp cannot exceed it, a
# larger figure would be a bug.)
MIN_ROT_ERR_MEASURED = 1.362e-7
MIN_ROT_ERR_RTOL = min(4 * MIN_ROT_ERR_MEASURED, 1e-5)

LAUNCHED = [c["name"] for c in pc.cases() if not c["refused"]]


def solve(case, bufs, n_floors=None, max_nodes=None, rows_ptr=None, **scalars):
    """One call of the entry on `bufs` = (out_rows, out_nodes, out_floors) device byte tensors WITH their guards; returns its status."""
    lib = _lib.load()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(DEV)
    rows, floor_start, n_nodes = dev(case["rows"]), dev(case["floor_start"]), dev(case["n_nodes"])
    p = lambda t, dt: ctypes.c_void_p(t.data_ptr() + pc.GUARD * dt.itemsize)
    s = {k: float(case[k]) for k in ("confidence_threshold", "rot_threshold_deg", "trans_threshold")}
    s["cycle_filter"] = case["cycle_filter"]
    s.update(scalars)
    rc = lib.salve_pose_graph_solve(ctypes.c_void_p(rows.data_ptr()) if rows_ptr is None else rows_ptr, len(case["rows"]),
                                    ctypes.c_void_p(floor_start.data_ptr()), ctypes.c_void_p(n_nodes.data_ptr()),
                                    len(case["n_nodes"]) if n_floors is None else n_floors, case["max_nodes"] if max_nodes is None else max_nodes,
                                    s["confidence_threshold"], s["rot_threshold_deg"], s["trans_threshold"], s["cycle_filter"],
                                    p(bufs[0], pc.ROW_OUT), p(bufs[1], pc.NODE_OUT), p(bufs[2], pc.FLOOR_OUT), None, 0, status.ptr(DEV),
                                    ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream))
    torch.cuda.synchronize()
    return rc


def on_gpu(case):
    """(the three buffers with their guards as the device left them, was the status bit raised)"""
    host = pc.fresh_buffers(case)
    bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in host]
    assert solve(case, bufs) == _lib.SALVE_OK, _lib.load().salve_last_error()
    got = tuple(b.cpu().numpy().view(h.dtype) for b, h in zip(bufs, host))
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


def rot_err_difference(got_rows, want_rows):
    """The largest relative difference of min_rot_err where both are finite (where one is +inf, the bit comparison of the others covers it)."""
    g, w = got_rows["min_rot_err"].astype(np.float64), want_rows["min_rot_err"].astype(np.float64)
    assert np.array_equal(np.isfinite(g), np.isfinite(w)) and np.array_equal(g[~np.isfinite(g)], w[~np.isfinite(w)])
    m = np.isfinite(w) & (w != 0)
    assert (g[np.isfinite(w) & (w == 0)] == 0).all()
    return float((np.abs(g[m] - w[m]) / w[m]).max()) if m.any() else 0.0


@pytest.mark.parametrize("name", LAUNCHED)
def test_every_case_equals_the_emulator(name):
    status.check(DEV, "before the pose-graph cases")
    (rows, nodes, floors), raised = result(name)
    (want_rows, want_nodes, want_floors), want_raised, _ = pc.expected(pc.case(name))
    assert raised == want_raised == (name == "malformed-floors")
    assert floors.tobytes() == want_floors.tobytes(), name        # counts and origin, guards
    assert nodes.tobytes() == want_nodes.tobytes(), name          # localized, parent, depth, pose; guards and the records past n_nodes
    for k in ("chosen", "consistent", "n_triplets", "n_consistent", "min_trans_err"):
        assert rows[k].tobytes() == want_rows[k].tobytes(), (name, k)   # (with the guards' bytes)
    d = rot_err_difference(rows[pc.GUARD:-pc.GUARD], want_rows[pc.GUARD:-pc.GUARD])
    print(f"{name}: largest relative difference of min_rot_err {d:.3e}")
    assert d <= MIN_ROT_ERR_RTOL, name
    assert rows[:pc.GUARD].tobytes() == want_rows[:pc.GUARD].tobytes() and rows[-pc.GUARD:].tobytes() == want_rows[-pc.GUARD:].tobytes()


def test_two_runs_give_equal_bytes():
    for name in ("k48-dense", "300-floors", "256-nodes-sparse"):
        first, _ = result(name)
        second, _ = on_gpu(pc.case(name))
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes(), name


def test_library_refusals():
    lib = _lib.load()
    case = pc.case("triangle")
    host = pc.fresh_buffers(case)
    bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in host]
    untouched = lambda: all((b.cpu().numpy() == pc.SENTINEL).all() for b in bufs)
    refused = [dict(max_nodes=0), dict(max_nodes=-1), dict(max_nodes=257), dict(max_nodes=2 ** 31 - 1), dict(n_floors=-1), dict(cycle_filter=2),
               dict(cycle_filter=-1), dict(confidence_threshold=float("nan")), dict(rot_threshold_deg=float("nan")), dict(trans_threshold=float("nan")),
               dict(rows_ptr=ctypes.c_void_p(None)), dict(rows_ptr=ctypes.c_void_p(bufs[0].data_ptr() + 4))]
    for kw in refused:
        assert solve(case, bufs, **kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert b"salve_pose_graph_solve" in lib.salve_last_error(), kw
    big = pc.case("257-nodes")   # a floor of 257 panoramas: refused on the host, nothing launched
    big_bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in pc.fresh_buffers(big)]
    assert solve(big, big_bufs) == _lib.SALVE_ERR_BAD_ARG and b"256" in lib.salve_last_error()
    assert all((b.cpu().numpy() == pc.SENTINEL).all() for b in big_bufs)
    assert solve(case, bufs, n_floors=0) == _lib.SALVE_OK   # launches nothing
    assert untouched()
    assert lib.salve_pose_graph_workspace_bytes(1, 256) == 0
    status.check(DEV, "refusals")
    assert solve(case, bufs) == _lib.SALVE_OK and not untouched()
    status.check(DEV, "after the refusals")


def test_wrapper_equals_the_emulator():
    """salve_amd.pose_graph.solve on the rows of two cases as two floors with scattered pano ids: the dicts it returns are the emulator's."""
    from salve_amd import pose_graph as pg

    names = ("filter-splits-the-component", "k48-dense")
    cols = {k: [] for k in ("building_id", "floor_id", "i1", "i2", "prob", "y_hat", "y_true", "R", "t", "s", "wdo_pair_uuid", "configuration")}
    pano = lambda k: 3 * k + 2   # compact index -> pano id
    for b, name in enumerate(names):
        for r in pc.case(name)["rows"][::-1]:   # (handed over in reverse: the wrapper sorts)
            for k, v in (("building_id", f"000{b}"), ("floor_id", "floor_01"), ("i1", pano(int(r["i1"]))), ("i2", pano(int(r["i2"]))), ("prob", r["prob"]),
                         ("y_hat", r["y_hat"]), ("y_true", 1), ("R", r["R"].reshape(2, 2)), ("t", r["t"]), ("s", r["s"]),
                         ("wdo_pair_uuid", "door_0_0"), ("configuration", "identity")):
                cols[k].append(v)
    sols = pg.solve(pg.EdgeMeasurements(**cols), 0.5, device=DEV)
    assert [s.building_id for s in sols] == ["0000", "0001"]
    for sol, name in zip(sols, names):
        case = pc.case(name)
        (rows, nodes, floors), _, _ = pc.expected(case)
        rows, nodes, fo = rows[pc.GUARD:-pc.GUARD], nodes[pc.GUARD:-pc.GUARD], floors[pc.GUARD]
        chosen = {(pano(int(r["i1"])), pano(int(r["i2"]))) for r in case["rows"][rows["chosen"] == 1]}
        consistent = {(pano(int(r["i1"])), pano(int(r["i2"]))) for r in case["rows"][rows["consistent"] == 1]}
        assert set(sol.i2Si1) == chosen and set(sol.i2Si1_consistent) == consistent and sol.origin == pano(int(fo["origin"]))
        assert sol.counts["n_triplets"] == fo["n_triplets"] and sol.counts["n_localized"] == fo["n_localized"] and sol.counts["n_nodes"] == case["n_nodes"][0]
        assert len(sol.wSi_list) == max(b for _, b in consistent) + 1
        for v in range(int(case["n_nodes"][0])):
            S = sol.wSi_list[pano(v)] if pano(v) < len(sol.wSi_list) else None
            assert (S is not None) == bool(nodes["localized"][v])
            if S is not None:
                assert S.rotation.tobytes() == nodes["R"][v].tobytes() and S.translation.tobytes() == nodes["t"][v].tobytes() and S.scale == nodes["s"][v]
                assert sol.parent[pano(v)] == (pano(int(nodes["parent"][v])) if nodes["parent"][v] >= 0 else -1) and sol.depth[pano(v)] == nodes["depth"][v]
        assert all(S is None for p, S in enumerate(sol.wSi_list) if (p - 2) % 3)
        assert pg.FloorSolution.from_json(sol.to_json()).to_json() == sol.to_json()
    status.check(DEV, "wrapper")
