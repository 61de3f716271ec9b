"""salve_pose_graph_sample_trees on the GPU, through the C ABI into sentinel-filled buffers: every launched case of
tests/pose_graph_sample_cases.py against the numpy emulator -- counts, flags, `best`, inliers, parents, depths, poses and avg_trans_err bit for
bit, avg_rot_err (the one value that carries the device's atan2f) within ROT_ERR_ATOL; guard records and the node records past n_nodes intact;
the status bit raised exactly by the malformed cases; every documented refusal; equal bytes on a second run.

ROT_ERR_ATOL is derived, not measured here: an average of |th_m - th_sim| terms, two angles of at most 180 degrees, each within
tests/test_gpu_pose_graph.py's MIN_ROT_ERR_RTOL = 4 x 1.362e-7 of numpy's: 2 x 180 x 5.45e-7 = 1.96e-4 degrees.  The largest difference the
run measures is printed per case (profiles/r20_pose_graph_sample.txt records it)."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib, status  # noqa: E402
from tests import pose_graph_sample_cases as sc  # noqa: E402

DEV = "cuda:0"
ENTRY = b"salve_pose_graph_sample_trees"
SALVE_ERR_WORKSPACE = -4
LAUNCHED = [c["name"] for c in sc.cases() if not c["refused"]]


def sample(case, bufs, ws=None, **over):
    """One call of the entry on `bufs` = (out_trees, out_inlier, out_nodes, out_floors) device byte tensors WITH their guards; returns its status.
    `over` replaces arguments by name (pointers as ctypes.c_void_p)."""
    lib = _lib.load()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)
    tensors = {k: dev(case[k]) for k in ("rows", "floor_start", "n_nodes", "hyp_start", "masks")}
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    out = lambda t, dt: ctypes.c_void_p(t.data_ptr() + sc.GUARD * np.dtype(dt).itemsize)
    n_hyps, M = len(case["masks"]), over.get("max_nodes", case["max_nodes"])
    ws_bytes = int(lib.salve_pose_graph_sample_workspace_bytes(n_hyps, min(max(M, 0), 256)))
    if ws is None:
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=DEV)
    a = dict(rows=ptr(tensors["rows"]), n_rows=len(case["rows"]), floor_start=ptr(tensors["floor_start"]), n_nodes=ptr(tensors["n_nodes"]),
             n_floors=len(case["n_nodes"]), max_nodes=case["max_nodes"], confidence_threshold=float(case["confidence_threshold"]),
             hyp_start=ptr(tensors["hyp_start"]), hyp_mask=ptr(tensors["masks"]), n_hyps=n_hyps, mask_words=case["mask_words"],
             out_trees=out(bufs[0], sc.TREE_OUT), out_inlier=out(bufs[1], np.int32), out_nodes=out(bufs[2], sc.NODE_OUT),
             out_floors=out(bufs[3], sc.FLOOR_OUT), workspace=ptr(ws), workspace_bytes=ws_bytes, status=status.ptr(DEV),
             stream=ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream))
    a.update(over)
    rc = lib.salve_pose_graph_sample_trees(*a.values())
    torch.cuda.synchronize()
    return rc


def on_gpu(case):
    """(the four buffers with their guards as the device left them, was the status bit raised)"""
    host = sc.fresh_buffers(case)
    bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in host]
    assert sample(case, bufs) == _lib.SALVE_OK, _lib.load().salve_last_error()
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
        _RESULTS[name] = on_gpu(sc.case(name))
    return _RESULTS[name]


@pytest.mark.parametrize("name", LAUNCHED)
def test_every_case_equals_the_emulator(name):
    status.check(DEV, "before the sampled-tree cases")
    got, raised = result(name)
    want, want_raised, _ = sc.expected(sc.case(name))
    for g, w, what in ((got[0], want[0], "trees"), (got[3], want[3], "floors")):
        gr, wr = g["avg_rot_err"][sc.GUARD:-sc.GUARD], w["avg_rot_err"][sc.GUARD:-sc.GUARD]
        m = ~np.isnan(wr) & ~np.isnan(gr)
        print(f"{name}: largest difference of {what}.avg_rot_err {float(np.abs(gr[m] - wr[m]).max()) if m.any() else 0.0:.3e} degrees")
    assert raised == want_raised == (name in sc.LAUNCH_CHECKED)
    assert sc.differences(got, want) == [], name


def test_two_runs_give_equal_bytes():
    for name in ("100-hypotheses", "300-floors", "k-513", "path-256"):
        first, _ = result(name)
        second, _ = on_gpu(sc.case(name))
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes(), name


def test_library_refusals():
    lib = _lib.load()
    case = sc.case("triangle-plus-outlier")
    bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in sc.fresh_buffers(case)]
    untouched = lambda bs: all((b.cpu().numpy() == sc.SENTINEL).all() for b in bs)
    null, odd = ctypes.c_void_p(None), lambda i, by=4: ctypes.c_void_p(bufs[i].data_ptr() + by)
    refused = [dict(max_nodes=0), dict(max_nodes=-1), dict(max_nodes=257), dict(max_nodes=2 ** 31 - 1), dict(n_floors=-1), dict(n_rows=-1),
               dict(n_hyps=-1), dict(mask_words=-1), dict(confidence_threshold=float("nan")), dict(rows=null), dict(floor_start=null), dict(n_nodes=null),
               dict(hyp_start=null), dict(hyp_mask=null), dict(out_trees=null), dict(out_inlier=null), dict(out_nodes=null), dict(out_floors=null),
               dict(workspace=null), dict(rows=odd(0)), dict(out_trees=odd(0)), dict(out_nodes=odd(2)), dict(out_floors=odd(3)), dict(out_inlier=odd(1, 2)),
               dict(hyp_mask=odd(1, 2))]
    for kw in refused:
        assert sample(case, bufs, **kw) == _lib.SALVE_ERR_BAD_ARG, kw
        assert ENTRY in lib.salve_last_error(), kw
    assert sample(case, bufs, workspace_bytes=int(lib.salve_pose_graph_sample_workspace_bytes(len(case["masks"]), case["max_nodes"])) - 1) == SALVE_ERR_WORKSPACE
    assert ENTRY in lib.salve_last_error()
    big = sc.case("257-nodes")   # a floor of 257 panoramas: refused on the host, nothing launched
    big_bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in sc.fresh_buffers(big)]
    assert sample(big, big_bufs) == _lib.SALVE_ERR_BAD_ARG and b"256" in lib.salve_last_error()
    assert untouched(big_bufs)
    assert sample(case, bufs, n_floors=0) == _lib.SALVE_OK and sample(case, bufs, n_hyps=0) == _lib.SALVE_OK   # launch nothing
    assert untouched(bufs)
    assert lib.salve_pose_graph_sample_workspace_bytes(100, 64) == 100 * 64 * sc.NODE_OUT.itemsize
    assert lib.salve_pose_graph_sample_workspace_bytes(0, 64) == 0
    status.check(DEV, "refusals")
    assert sample(case, bufs) == _lib.SALVE_OK and not untouched(bufs)
    status.check(DEV, "after the refusals")


def test_mask_words_zero_selects_nothing():
    """mask_words == 0 (hyp_mask may be null): no hypothesis has an edge, so none is chosen; every output is still written."""
    case = dict(sc.case("triangle-plus-outlier"))
    case["masks"] = np.zeros((len(case["masks"]), 0), dtype=np.uint32)
    case["mask_words"] = 0
    host = sc.fresh_buffers(case)
    bufs = [torch.from_numpy(b.view(np.uint8)).to(DEV) for b in host]
    assert sample(case, bufs, hyp_mask=ctypes.c_void_p(None)) == _lib.SALVE_OK
    got = tuple(b.cpu().numpy().view(h.dtype) for b, h in zip(bufs, host))
    want, raised = sc.run_case(case, sc.emulated())
    assert not raised and sc.differences(got, want) == []
    assert got[3]["best"][sc.GUARD] == -1 and (got[1][sc.GUARD:-sc.GUARD] == 0).all()
    status.check(DEV, "mask_words 0")


def test_wrapper_equals_the_emulator():
    """salve_amd.pose_graph.sample_trees on the rows of two cases as two floors with scattered pano ids and the cases' own hypotheses."""
    from salve_amd import pose_graph as pg

    names = ("last-masked-of-three", "100-hypotheses")
    cols = {k: [] for k in ("building_id", "floor_id", "i1", "i2", "prob", "y_hat", "y_true", "R", "t", "s", "wdo_pair_uuid", "configuration")}
    pano = lambda k: 3 * k + 2   # compact index -> pano id
    for b, name in enumerate(names):
        for r in sc.case(name)["rows"]:
            for k, v in (("building_id", f"000{b}"), ("floor_id", "floor_01"), ("i1", pano(int(r["i1"]))), ("i2", pano(int(r["i2"]))), ("prob", r["prob"]),
                         ("y_hat", r["y_hat"]), ("y_true", 1), ("R", r["R"].reshape(2, 2)), ("t", r["t"]), ("s", r["s"]),
                         ("wdo_pair_uuid", "door_0_0"), ("configuration", "identity")):
                cols[k].append(v)
    meas = pg.EdgeMeasurements(**cols)
    base = np.cumsum([0] + [len(sc.case(n)["rows"]) for n in names])
    draws = [pg.HypothesisDraw(f"000{b}", "floor_01", np.zeros(0, dtype=np.int64), [], sc.case(n)["masks"]) for b, n in enumerate(names)]
    sols = pg.sample_trees(meas, 0.5, hypotheses=draws, device=DEV)
    assert [s.building_id for s in sols] == ["0000", "0001"]
    for b, (sol, name) in enumerate(zip(sols, names)):
        case = sc.case(name)
        (trees, inlier, nodes, floors), _, _ = sc.expected(case)
        trees, inlier, nodes, fo = trees[sc.GUARD:-sc.GUARD], inlier[sc.GUARD:-sc.GUARD], nodes[sc.GUARD:-sc.GUARD], floors[sc.GUARD]
        assert sol.best == fo["best"] >= 0 and sol.counts["n_candidates"] == fo["n_candidates"] and sol.counts["n_hyps"] == len(trees)
        assert sol.inlier_rows.tolist() == (base[b] + np.nonzero(inlier)[0]).tolist() and sol.inlier_mask.sum() == inlier.sum()
        assert sol.avg_trans_err == fo["avg_trans_err"] and abs(sol.avg_rot_err - fo["avg_rot_err"]) <= sc.ROT_ERR_ATOL
        assert [h["n_localized"] for h in sol.hypotheses] == trees["n_localized"].tolist()
        assert len(sol.wSi_list) == pano(int(case["rows"]["i2"][inlier == 1].max())) + 1
        for v in range(int(case["n_nodes"][0])):
            S = sol.wSi_list[pano(v)] if pano(v) < len(sol.wSi_list) else None
            assert (S is not None) == bool(nodes["localized"][v])
            if S is not None:
                assert S.rotation.tobytes() == nodes["R"][v].tobytes() and S.translation.tobytes() == nodes["t"][v].tobytes() and S.scale == nodes["s"][v]
                assert sol.parent[pano(v)] == (pano(int(nodes["parent"][v])) if nodes["parent"][v] >= 0 else -1) and sol.depth[pano(v)] == nodes["depth"][v]
        assert pg.TreeSampleSolution.from_json(sol.to_json()).to_json() == sol.to_json()
    status.check(DEV, "wrapper")
