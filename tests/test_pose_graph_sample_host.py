"""salve_pose_graph_sample_trees without a GPU: the case list keeps its conditions; the emulator of tests/pose_graph_sample_cases.py equals a
dict-and-Sim2 restatement of the reference's ransac_spanning_trees / compute_hypothesis_errors (networkx shortest paths) and reproduces the
records the reference itself left under tests/golden/; pose_graph.draw_hypotheses draws the reference's subsets; numpy's float32 rad2deg
multiplies by the float32 QUOTIENT 180 / pi; every emulated wrong kernel fails a case.

The averages are compared with rtol 1e-5, everything else exactly: the reference averages its translation errors (float32 norms) in float32,
pairwise, and its rotation errors in float64 in list order; the entry sums both in float64 in its own stated order.

The restatement's Sim2 is the reference's class with its two `@` products written out on float32 scalars: numpy hands `@` to a BLAS that may
fuse a product into a sum (tests/test_pose_graph_cases_host.py), and bits are asked here.  The records under tests/golden/ come from the
reference's own class, `@` included, so their poses are compared within that file's few float32 ulp per composition."""

import json
import math
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from salve_amd import pose_graph as pg
from tests import pose_graph_sample_cases as sc
from tests.test_pose_graph_cases_host import assert_poses_close

GOLDEN = sorted((Path(__file__).resolve().parent / "golden").glob("pose_graph_sample_*.json"))
AVG_RTOL = 1e-5


def test_the_case_list_keeps_its_conditions():
    sc.check_conditions()
    names = [c["name"] for c in sc.cases()]
    assert len(set(names)) == len(names) and sum(c["reference"] for c in sc.cases()) >= 10


# ---- the reference's loop, restated on dicts and Sim2 objects (spanning_tree.py:73-141, :144-176, :179-334, :337-384)

F32 = np.float32


class Sim2:
    """salve/common/sim2.py's value type: R, t stored as float32, s a Python float; compose and inverse as :100-130, unfused."""

    def __init__(self, R, t, s):
        self.R_, self.t_, self.s_ = np.asarray(R).astype(F32).reshape(2, 2), np.asarray(t).astype(F32).reshape(2), float(s)

    rotation = property(lambda self: self.R_)
    translation = property(lambda self: self.t_)
    scale = property(lambda self: self.s_)

    @property
    def theta_deg(self):
        return float(np.rad2deg(np.arctan2(self.R_[1, 0], self.R_[0, 0])))

    @staticmethod
    def _matvec(R, v):
        return np.array([R[0, 0] * v[0] + R[0, 1] * v[1], R[1, 0] * v[0] + R[1, 1] * v[1]], dtype=F32)

    def compose(self, S):
        A, B = self.R_, S.R_
        R = np.array([[A[0, 0] * B[0, 0] + A[0, 1] * B[1, 0], A[0, 0] * B[0, 1] + A[0, 1] * B[1, 1]],
                      [A[1, 0] * B[0, 0] + A[1, 1] * B[1, 0], A[1, 0] * B[0, 1] + A[1, 1] * B[1, 1]]], dtype=F32)
        return Sim2(R, self._matvec(A, S.t_) + ((1.0 / S.s_) * self.t_), self.s_ * S.s_)

    def inverse(self):
        Rt = self.R_.T
        return Sim2(Rt, self._matvec(-Rt, self.s_ * self.t_), 1.0 / self.s_)


def wrap_angle_deg(angle1, angle2):
    diff = (angle2 - angle1 + 180) % 360 - 180
    return np.absolute(diff + 360) if diff < -180 else np.absolute(diff)


def greedy_tree(i2Si1_dict):
    import networkx as nx

    edges = i2Si1_dict.keys()
    if len(edges) == 0:
        return None
    G = nx.Graph()
    G.add_edges_from(edges)
    cc_nodes = sorted(max(nx.connected_components(G), key=len))
    wSi_list = [None] * (max(max(a, b) for a, b in edges) + 1)
    origin = cc_nodes[0]
    wSi_list[origin] = Sim2(R=np.eye(2), t=np.zeros(2), s=1.0)
    for dst in cc_nodes[1:]:
        path = nx.shortest_path(G, source=origin, target=dst)
        wSi = Sim2(R=np.eye(2), t=np.zeros(2), s=1.0)
        for i1, i2 in zip(path[:-1], path[1:]):
            wSi = wSi.compose(i2Si1_dict[(i1, i2)].inverse() if i1 < i2 else i2Si1_dict[(i2, i1)])
        wSi_list[dst] = wSi
    return wSi_list


def hypothesis_errors(measurements, wSi_list):
    rot_errors, trans_errors = [], []
    for m in measurements:
        if m.i1 >= len(wSi_list) or m.i2 >= len(wSi_list) or wSi_list[m.i1] is None or wSi_list[m.i2] is None:
            continue
        sim = wSi_list[m.i2].inverse().compose(wSi_list[m.i1])
        rot_errors.append(wrap_angle_deg(sim.theta_deg, m.i2Si1.theta_deg))
        trans_errors.append(np.linalg.norm(sim.translation - m.i2Si1.translation))
    with np.errstate(all="ignore"):
        return (np.mean(rot_errors) if rot_errors else float("nan")), (np.mean(trans_errors) if trans_errors else float("nan"))


def ransac(measurements, hypotheses):
    """(best index, best wSi_list, best_hypothesis as measurement indices) over the given subsets (index lists), as :246-300."""
    best_rot = best_trans = float("inf")
    best_n, best, best_wSi, best_hyp = 0, None, None, None
    for h, idxs in enumerate(hypotheses):
        chosen = [k for k in range(len(measurements)) if k in idxs]
        i2Si1_dict = {}
        for k in chosen:   # randomly overwrite by order
            i2Si1_dict[(measurements[k].i1, measurements[k].i2)] = measurements[k].i2Si1
        wSi_list = greedy_tree(i2Si1_dict)
        if wSi_list is None:
            continue   # (the reference stops in a debugger here)
        rot, trans = hypothesis_errors(measurements, wSi_list)
        n = sum(S is not None for S in wSi_list)
        obj = (best_rot - rot) / 5 + (best_trans - trans) / 1 + 1.33 * (-(best_n - n) / (best_n + 1e-10))
        if obj > 0:
            best_rot, best_trans, best_n, best, best_wSi, best_hyp = rot, trans, n, h, wSi_list, chosen
    return best, best_wSi, best_hyp, best_rot, best_trans


def as_measurements(rows, conf):
    """The candidates of a floor's rows as the reference's measurement objects, and their row indices."""
    idx = np.nonzero(sc.is_candidate(rows, conf))[0]
    return [SimpleNamespace(i1=int(rows["i1"][r]), i2=int(rows["i2"][r]), i2Si1=Sim2(rows["R"][r].reshape(2, 2).copy(), rows["t"][r].copy(), float(rows["s"][r])))
            for r in idx], idx


def assert_floor_equals_restatement(rows, n, conf, masks, nodes, inlier, fo, name):
    meas, idx = as_measurements(rows, conf)
    hyps = [{k for k, r in enumerate(idx) if sc.mask_bit(m, int(r))} for m in masks]
    best, wSi, kept, rot, trans = ransac(meas, hyps)
    assert (best if best is not None else -1) == fo["best"], name
    if best is None:
        assert not inlier.any() and not nodes["localized"].any(), name
        return
    assert sorted(idx[k] for k in kept) == np.nonzero(inlier)[0].tolist(), name
    assert len(wSi) <= n
    for v in range(n):
        S = wSi[v] if v < len(wSi) else None
        assert (S is not None) == bool(nodes["localized"][v]), (name, v)
        if S is not None:
            assert S.rotation.tobytes() == nodes["R"][v].reshape(2, 2).tobytes() and S.translation.tobytes() == nodes["t"][v].tobytes(), (name, v)
            assert S.scale == nodes["s"][v], (name, v)
    np.testing.assert_allclose(fo["avg_rot_err"], rot, rtol=AVG_RTOL, err_msg=name)
    np.testing.assert_allclose(fo["avg_trans_err"], trans, rtol=AVG_RTOL, err_msg=name)


@pytest.mark.parametrize("name", [c["name"] for c in sc.cases() if c["reference"]])
def test_emulator_equals_the_reference_restatement(name):
    pytest.importorskip("networkx")
    case = sc.case(name)
    (trees, inlier, nodes, floors), raised, _ = sc.expected(case)
    assert not raised
    G, M = sc.GUARD, case["max_nodes"]
    for f in range(len(case["n_nodes"])):
        lo, hi, n = int(case["floor_start"][f]), int(case["floor_start"][f + 1]), int(case["n_nodes"][f])
        masks = case["masks"][case["hyp_start"][f]:case["hyp_start"][f + 1]]
        assert_floor_equals_restatement(case["rows"][lo:hi], n, case["confidence_threshold"], masks, nodes[G + f * M:G + f * M + n], inlier[G + lo:G + hi],
                                        floors[G + f], name)


# ---- the reference's own records

def golden_measurements(doc, building="0007", floor="floor_02"):
    m = doc["measurements"]
    n = len(m)
    return pg.EdgeMeasurements(building_id=[building] * n, floor_id=[floor] * n, i1=[x["i1"] for x in m], i2=[x["i2"] for x in m],
                               prob=[x["prob"] for x in m], y_hat=[1] * n, y_true=[1] * n, R=[np.array(x["R"]).reshape(2, 2) for x in m],
                               t=[x["t"] for x in m], s=[x["s"] for x in m], wdo_pair_uuid=["door_0_0"] * n, configuration=["identity"] * n)


@pytest.mark.parametrize("fpath", GOLDEN, ids=lambda p: p.stem)
def test_golden_records_are_reproduced(fpath):
    doc = json.loads(fpath.read_text())
    meas = golden_measurements(doc)
    (draw,) = pg.draw_hypotheses(meas, doc["confidence_threshold"], doc["num_hypotheses"], doc["sampling_fraction"], seed=doc["seed"])
    assert draw.candidates.tolist() == list(range(len(meas)))
    assert [s.tolist() for s in draw.subsets] == doc["hypotheses"]          # the reference's own np.random.choice results
    (fl,) = meas.compact()
    rows = np.zeros(len(meas), dtype=sc.ROW)
    order = fl["rows"]
    rows["i1"], rows["i2"], rows["prob"], rows["y_hat"] = fl["c1"], fl["c2"], meas.prob[order], 1
    rows["R"], rows["t"], rows["s"] = meas.R[order].reshape(-1, 4), meas.t[order], meas.s[order]
    case = sc.make_case(fpath.stem, [(rows, len(fl["pano_ids"]))], [[]])
    case["masks"], case["hyp_start"] = draw.masks, np.array([0, len(draw.masks)], dtype=np.int32)
    (trees, inlier, nodes, floors), raised = sc.run_case(case, sc.emulated())
    G = sc.GUARD
    assert not raised and floors["best"][G] >= 0
    assert sorted(order[np.nonzero(inlier[G:-G])[0]].tolist()) == sorted(doc["best_hypothesis"])
    nodes = nodes[G:-G]
    ids = fl["pano_ids"]
    want = doc["wSi_list"]
    assert len(want) == max(meas.i2[doc["best_hypothesis"]]) + 1
    from salve_amd.common.sim2 import Sim2 as ProjectSim2

    sim = lambda r: None if r is None else ProjectSim2(np.array(r["R"], dtype=np.float32).reshape(2, 2), np.array(r["t"], dtype=np.float32), r["s"])
    by_index = [None] * len(ids)   # the recorded list is by pano id; the emulator's nodes are by compact index
    for p, r in enumerate(want):
        if r is not None:
            by_index[int(np.searchsorted(ids, p))] = sim(r)
    assert {int(ids[v]) for v in np.nonzero(nodes["localized"])[0]} == {p for p, r in enumerate(want) if r is not None}
    assert_poses_close(nodes, by_index, {v: int(nodes["depth"][v]) for v in np.nonzero(nodes["localized"])[0]}, fpath.stem)


def test_golden_records_exist():
    assert len(GOLDEN) >= 2


# ---- draw_hypotheses

def reference_draws(meas_objects, num_hypotheses, sampling_fraction, seed):
    """The reference's own call sequence (spanning_tree.py:213-244) after np.random.seed(seed), on the global generator."""
    import scipy.special

    state = np.random.get_state()
    try:
        np.random.seed(seed)
        K = len(meas_objects)
        m = int(math.ceil(sampling_fraction * K))
        try:
            max_unique = int(scipy.special.binom(K, m))
        except:  # noqa: E722 (the reference's)
            max_unique = 1000
        num = min(max_unique, num_hypotheses)
        capture_distance = np.array([np.absolute(x.i2 - x.i1) for x in meas_objects])
        p = 1 / capture_distance
        p = p / np.sum(p)
        return [np.random.choice(a=K, size=m, replace=False, p=p) for _ in range(num)]
    finally:
        np.random.set_state(state)


def test_draw_hypotheses_equals_the_reference_sequence():
    pytest.importorskip("scipy")
    rng = np.random.default_rng(5)
    cols = {k: [] for k in ("building_id", "floor_id", "i1", "i2", "prob", "y_hat", "y_true", "R", "t", "s", "wdo_pair_uuid", "configuration")}
    for b, n_rows in (("0001", 40), ("0002", 5), ("0003", 3), ("0004", 1300)):   # binom(5, 3) = 10 < 25; binom(1300, 650) overflows: 1000
        for _ in range(n_rows):
            a, c = sorted(rng.choice(60, size=2, replace=False).tolist())
            for k, v in (("building_id", b), ("floor_id", "floor_01"), ("i1", 2 * a + 1), ("i2", 2 * c + 1), ("prob", rng.uniform(0.3, 1.0)),
                         ("y_hat", int(rng.random() < 0.8)), ("y_true", 1), ("R", np.eye(2)), ("t", np.zeros(2)), ("s", 1.0),
                         ("wdo_pair_uuid", "door_0_0"), ("configuration", "identity")):
                cols[k].append(v)
    meas = pg.EdgeMeasurements(**cols)
    thr = 0.55
    for seed, num in ((0, 25), (3, 7)):
        draws = pg.draw_hypotheses(meas, thr, num_hypotheses=num, seed=seed)
        assert [(d.building_id, d.floor_id) for d in draws] == meas.floors()
        for d, fl in zip(draws, meas.compact()):
            cand = [r for r in range(len(meas)) if meas.building_id[r] == d.building_id and meas.y_hat[r] == 1 and meas.prob[r] >= np.float32(thr)]
            assert d.candidates.tolist() == cand
            objs = [SimpleNamespace(i1=int(meas.i1[r]), i2=int(meas.i2[r])) for r in cand]
            want = reference_draws(objs, num, 0.5, seed) if cand else []
            assert len(d.subsets) == len(want) and all(np.array_equal(x, y) for x, y in zip(d.subsets, want))
            assert d.masks.shape == (len(want), (len(fl["rows"]) + 31) // 32)
            for mask, subset in zip(d.masks, want):   # bit k = the floor's k-th sorted row
                rows_set = {int(fl["rows"][k]) for k in range(len(fl["rows"])) if sc.mask_bit(mask, k)}
                assert rows_set == {cand[k] for k in subset}
    assert pg.draw_hypotheses(meas, 2.0)[0].subsets == [] and pg.draw_hypotheses(meas, 2.0)[0].masks.shape[0] == 0   # no candidate: no hypothesis


def _all_candidates(n_rows):
    rng = np.random.default_rng(n_rows)
    pairs = [sorted(rng.choice(50, size=2, replace=False).tolist()) for _ in range(n_rows)]
    return pg.EdgeMeasurements(building_id=["0001"] * n_rows, floor_id=["floor_01"] * n_rows, i1=[a for a, _ in pairs], i2=[b for _, b in pairs],
                               prob=[1.0] * n_rows, y_hat=[1] * n_rows, y_true=[1] * n_rows, R=[np.eye(2)] * n_rows, t=[np.zeros(2)] * n_rows,
                               s=[1.0] * n_rows, wdo_pair_uuid=["door_0_0"] * n_rows, configuration=["identity"] * n_rows)


def test_draw_hypotheses_counts():
    """binom(5, 3) = 10 unique subsets bound the count; where the binomial overflows a float the reference falls back to 1000; min_num_edges."""
    assert len(pg.draw_hypotheses(_all_candidates(5), 0.5, num_hypotheses=25)[0].subsets) == 10
    (big,) = pg.draw_hypotheses(_all_candidates(1300), 0.5, num_hypotheses=1002)
    assert len(big.subsets) == 1000 and all(len(s) == 650 for s in big.subsets[:3])
    (few,) = pg.draw_hypotheses(_all_candidates(30), 0.5, num_hypotheses=4, min_num_edges=7)
    assert len(few.subsets) == 4 and all(len(s) == len(set(s.tolist())) == 7 for s in few.subsets)


def test_numpy_float32_rad2deg_multiplies_by_the_float32_quotient():
    """The constant of phase E: np.rad2deg(x) == x * (float32(180) / float32(pi)) for every one of 2 000 000 float32 angles, and x *
    float32(180 / pi) -- phase B's constant -- equals it for a minority of them only."""
    x = np.random.default_rng(0).uniform(-np.pi, np.pi, size=2_000_000).astype(np.float32)
    want = np.rad2deg(x)
    assert want.dtype == np.float32
    quotient, product = np.float32(180.0) / np.float32(np.pi), np.float32(180.0 / np.pi)
    assert quotient == sc.RAD2DEG_QUOT and float(quotient) == 57.29577636718750 and quotient != product
    assert np.array_equal(x * quotient, want)
    share = float(np.mean(x * product == want))
    print(f"x * float32(180 / pi) equals np.rad2deg(x) for {100 * share:.1f} % of the values")
    assert share < 0.5


# ---- emulated wrong kernels

@pytest.mark.parametrize("wrong", sc.WRONG_KERNELS)
def test_every_emulated_wrong_kernel_fails_a_case(wrong):
    """With the GPU test's comparison (everything bit for bit, avg_rot_err within ROT_ERR_ATOL)."""
    for c in sc.cases():
        if c["refused"] or len(c["masks"]) > 150:
            continue
        got, _ = sc.run_case(c, sc.emulated(wrong))
        diff = sc.differences(got, sc.expected(c)[0])
        if diff:
            print(f"{wrong}: caught by {c['name']} in {diff}")
            return
    pytest.fail(f"no case catches the wrong kernel {wrong}")


def test_the_comparison_accepts_the_emulator_and_an_atan2_sized_difference():
    c = sc.case("100-hypotheses")
    want = sc.expected(c)[0]
    got = tuple(b.copy() for b in want)
    assert sc.differences(got, want) == []
    got[0]["avg_rot_err"][sc.GUARD] += 0.5 * sc.ROT_ERR_ATOL
    assert sc.differences(got, want) == []
    got[0]["avg_rot_err"][sc.GUARD] += sc.ROT_ERR_ATOL
    assert sc.differences(got, want) == ["trees.avg_rot_err"]
    assert sc.ROT_ERR_ATOL == pytest.approx(1.96e-4, rel=1e-2) and 2 * sc.ROT_ERR_ATOL / 5 < sc.OBJ_MARGIN / 10


def test_json_round_trip_and_inlier_mask():
    from salve_amd.common.sim2 import Sim2
    sol = pg.TreeSampleSolution("0001", "floor_01", np.array([2, 5, 8]), {"method": "random_spanning_trees", "confidence_threshold": 0.5}, 1,
                                [None, None, Sim2(np.eye(2), np.zeros(2), 1.0), None, None, Sim2(np.eye(2), np.ones(2), 2.0)], np.array([1, 3]),
                                [{"avg_rot_err": float("nan"), "avg_trans_err": float("nan"), "n_localized": 0, "n_measured": 0, "n_edges": 0, "origin": None},
                                 {"avg_rot_err": 0.25, "avg_trans_err": 0.5, "n_localized": 2, "n_measured": 2, "n_edges": 1, "origin": 2}], 5,
                                {2: -1, 5: 2}, {2: 0, 5: 1}, {"n_nodes": 3, "n_rows": 4, "n_candidates": 3, "n_hyps": 2, "n_improvements": 1, "n_localized": 2,
                                                              "n_inliers": 2}, 2, 0.25, 0.5)
    assert sol.inlier_mask.tolist() == [False, True, False, True, False]
    doc = json.loads(json.dumps(sol.to_json()))   # (strict JSON: no NaN token)
    assert "NaN" not in json.dumps(sol.to_json())
    back = pg.TreeSampleSolution.from_json(doc)
    assert back.to_json() == sol.to_json() and back.wSi_list[5] == sol.wSi_list[5] and back.best == 1
    assert pg.combined_inlier_mask([sol, back]).tolist() == sol.inlier_mask.tolist() and pg.combined_inlier_mask([]) is None
