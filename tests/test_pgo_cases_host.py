"""salve_pose_graph_optimise without a GPU: the emulator of tests/pgo_cases.py reproduces the reference's own recorded case
(tests/algorithms/test_pose2_slam.py::test_planar_slam_pgo_only, under np.isclose's defaults as the reference asserts); its minimum agrees with
an independent minimiser (scipy.optimize.least_squares on a separately written, vectorised statement of the same residuals, each factor scaled
by sqrt(2 rho) / n so that the sum of squares is 2 E); the case list keeps its conditions (no decision within 1e-6 of its threshold, with and
without an ulp on every sin / cos / atan2; the outputs move by at most 1e-11 under that nudge and no count changes); every emulated wrong kernel
fails a case; the new symbols are declared, listed, bound and built; run and the command line refuse what they document; PgoSolution survives
JSON.  gtsam is not installed where this runs: parity with its iterates is unpinned, the objective and its minimum are what is pinned."""

import json
import math
import re
from pathlib import Path

import numpy as np
import pytest

from salve_amd import _lib
from salve_amd import pose_graph as pg
from tests import pgo_cases as pc

ROOT = Path(__file__).resolve().parent.parent
# (max_iterations: the IRLS steps of a floor with Huber-weighted factors converge linearly, a hundred of them need not reach 1e-14)
TIGHT = {"relative_error_tol": 1e-14, "absolute_error_tol": 1e-14, "max_iterations": 3000}
# cases without a minimum to compare: no step is ever taken
NO_MINIMUM = ("stops-at-the-lambda-bound", "non-finite-measurement")


def test_the_case_list_keeps_its_conditions():
    pc.check_conditions()
    names = [c["name"] for c in pc.cases()]
    assert len(set(names)) == len(names)
    sizes = {int(r["floor"]["n_unknown_nodes"]) for c in pc.cases() for r in pc.expected(c["name"])}
    assert {pc.LDS_NODES - 1, pc.LDS_NODES, pc.LDS_NODES + 1, 256, 0, 1} <= sizes
    assert len(pc.case("70-floors")["n_nodes"]) == 70


def test_the_emulator_reproduces_the_references_recorded_case():
    res = pc.expected("reference-recorded")[0]
    assert res["floor"]["n_unknown_nodes"] == 5 and res["floor"]["n_factors"] == 6 and not res["nodes"]["localized"][0]
    assert np.isnan(res["pose"][0]).all()
    for v, want in pc.REFERENCE_EXPECTED.items():
        assert np.isclose(want[2], res["pose"][v][2]), (v, res["pose"][v])          # the reference's two assertions, with their defaults
        assert np.allclose(want[:2], res["pose"][v][:2]), (v, res["pose"][v])
        R = res["nodes"]["R"][v].astype(np.float64)
        assert np.allclose(R, [math.cos(want[2]), -math.sin(want[2]), math.sin(want[2]), math.cos(want[2])], atol=1e-6) and res["nodes"]["s"][v] == 1.0


# ---- the same objective written a second time, vectorised, for scipy

def _problem(rows, n, init, P):
    loc = np.nonzero(init["localized"][:n])[0]
    idx = -np.ones(n, dtype=np.int64)
    idx[loc] = np.arange(len(loc))
    ok = (rows["y_hat"] == 1) & (rows["prob"] >= np.float32(P["confidence_threshold"])) & (idx[rows["i1"]] >= 0) & (idx[rows["i2"]] >= 0)
    r = rows[ok]
    x0 = np.stack([init["t"][loc, 0], init["t"][loc, 1], np.arctan2(init["R"][loc, 2].astype(np.float64), init["R"][loc, 0].astype(np.float64))], 1)
    m = np.stack([r["t"][:, 0], r["t"][:, 1], np.arctan2(r["R"][:, 2].astype(np.float64), r["R"][:, 0].astype(np.float64))], 1).astype(np.float64)
    return loc, idx[r["i1"]], idx[r["i2"]], m, x0.astype(np.float64)


def _scaled_residuals(x, a, b, m, P):
    x = x.reshape(-1, 3)
    wrap = lambda t: np.arctan2(np.sin(t), np.cos(t))
    rot_t = lambda th, v: np.stack([np.cos(th) * v[:, 0] + np.sin(th) * v[:, 1], -np.sin(th) * v[:, 0] + np.cos(th) * v[:, 1]], 1)
    e_xy = rot_t(m[:, 2], rot_t(x[b, 2], x[a, :2] - x[b, :2]) - m[:, :2])
    e = np.concatenate([e_xy, wrap(x[a, 2] - x[b, 2] - m[:, 2])[:, None]], 1) / np.array(P["odometry_sigmas"])
    prior = np.array([[x[0, 0], x[0, 1], wrap(x[0, 2])]]) / np.array(P["prior_sigmas"])
    r = np.concatenate([prior, e], 0)
    nn = np.linalg.norm(r, axis=1)
    k = P["huber_k"]
    rho = np.where((nn <= k) | (not P["robust"]), nn * nn / 2, k * (nn - k / 2))
    scale = np.where(nn > 0, np.sqrt(2 * rho) / np.where(nn > 0, nn, 1.0), 1.0)
    return (r * scale[:, None]).reshape(-1)


def _floors_with_a_minimum():
    out = []
    for c in pc.cases():
        if c["name"] in NO_MINIMUM:
            continue
        for f in range(len(c["n_nodes"])):
            if not pc.floor_is_malformed(c, f) and (len(c["n_nodes"]) == 1 or f % 6 in (2, 5) or f == 12):   # (of the 70 floors: every third, and the lone node)
                out.append((c["name"], f))
    return out


_WORST = {"d0": 0.0}


@pytest.mark.parametrize("name, f", _floors_with_a_minimum())
def test_the_emulators_minimum_is_the_independent_minimisers(name, f):
    from scipy.optimize import least_squares

    c = pc.single_floor_launch(pc.case(name), f) if len(pc.case(name)["n_nodes"]) > 1 else pc.case(name)
    P = pc.params(c, **TIGHT)
    res = pc.emulate(c, **TIGHT)[0]
    n = int(c["n_nodes"][0])
    lo, hi = int(c["floor_start"][0]), int(c["floor_start"][1])
    loc, a, b, m, x0 = _problem(c["rows"][lo:hi], n, c["init"], P)
    if len(loc) == 0:
        assert res["floor"]["stop_reason"] == pc.STOP_EMPTY
        return
    fun = lambda x: _scaled_residuals(x, a, b, m, P)
    assert abs(0.5 * float(fun(x0.reshape(-1)) @ fun(x0.reshape(-1))) - res["floor"]["cost_initial"]) <= 1e-9 * max(1.0, res["floor"]["cost_initial"])
    tightest = dict(method="trf", jac="3-point", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    sol = least_squares(fun, x0.reshape(-1), **tightest)
    # The poses: where two factors on a panorama are both Huber-weighted, rho is a sum of two norms and the minimum is a whole segment (a
    # median), so two minimisers need not meet.  The independent minimiser is therefore also started AT the emulator's minimum: it must stay.
    mine = res["pose"][loc]
    stay = least_squares(fun, mine.reshape(-1), **tightest)
    d0 = float(np.abs(stay.x.reshape(-1, 3) - mine).max())
    if res["floor"]["n_downweighted"] == 0:   # a plain least-squares minimum is isolated: the two runs must meet as well
        d0 = max(d0, float(np.abs(sol.x.reshape(-1, 3) - mine).max()))
    assert abs(stay.cost - res["floor"]["cost_final"]) <= 1e-9 * max(1.0, sol.cost)
    _WORST["d0"] = max(_WORST["d0"], d0)
    print(f"{name}[{f}]: cost {res['floor']['cost_final']:.12g} (scipy {sol.cost:.12g}), largest pose difference {d0:.3e}; worst so far {_WORST['d0']:.3e}")
    assert res["floor"]["stop_reason"] in (pc.STOP_ABSOLUTE, pc.STOP_RELATIVE, pc.STOP_LAMBDA)
    assert abs(sol.cost - res["floor"]["cost_final"]) <= 1e-9 * max(1.0, sol.cost)
    assert d0 <= 4 * pc.D0_MEASURED


# ---- wrong kernels

def _differs(name, variant):
    for want, got in zip(pc.expected(name), pc.emulate(pc.case(name), variant=variant)):
        if want["floor"].tobytes()[:24] != got["floor"].tobytes()[:24]:
            return True
        if np.isfinite(want["pose"]).any() and not np.allclose(want["pose"], got["pose"], rtol=0, atol=1e-6, equal_nan=True):
            return True
    return False


WRONG = [("best-row-only", "several-rows-per-pair"), ("no-prior", "reference-recorded"), ("no-wrap", "branch-cut"),
         ("huber-on-residual-only", "triangle-huber"), ("lambda-not-restored", "far-off-start"), ("measurement-swapped", "reference-recorded"),
         ("unlocalized-not-skipped", "second-component"), ("threshold-gt", "several-rows-per-pair"), ("sigmas-swapped", "triangle-huber"),
         ("stop-on-absolute-decrease", "rejected-steps-inside-the-tolerance")]


@pytest.mark.parametrize("variant, name", WRONG)
def test_every_emulated_wrong_kernel_fails_a_case(variant, name):
    assert variant in pc.WRONG_KERNELS and _differs(name, variant), (variant, name)


def test_every_wrong_kernel_is_tried():
    assert sorted(pc.WRONG_KERNELS) == sorted(v for v, _ in WRONG) and len(WRONG) == 10


def test_robust_off_gives_another_recorded_answer():
    a, b = pc.expected("triangle-huber")[0], pc.expected("triangle-huber-robust-off")[0]
    assert a["floor"]["n_downweighted"] == 1 and b["floor"]["n_downweighted"] == 0
    assert np.abs(a["pose"] - b["pose"]).max() > 1e-2


# ---- the library's surface

def test_the_new_symbols_are_declared_listed_bound_and_built():
    header = (ROOT / "include" / "salve_hip.h").read_text()
    lib = _lib.load()
    for name in ("salve_pose_graph_optimise_workspace_bytes", "salve_pose_graph_optimise"):
        assert re.search(rf"\b{name}\(", header) and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.salve_pose_graph_optimise.argtypes) == 22
    assert (ROOT / "salve_amd" / "csrc" / "pose_graph_pgo.hip").exists()
    body = re.search(r"typedef struct \{([^}]*)\} salve_graph_pgo_floor_out_t;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert tuple(re.findall(r"(\w+)\s*[;,]", body)) == _lib.GRAPH_PGO_FLOOR_OUT_DTYPE.names == pc.PGO_FLOOR_OUT.names
    assert int(re.search(r"#define SALVE_PGO_LDS_NODES (\d+)", header).group(1)) == _lib.PGO_LDS_NODES == pc.LDS_NODES
    for k, stop in enumerate(("EMPTY", "ABSOLUTE", "RELATIVE", "LAMBDA", "MAX_ITERATIONS", "NON_FINITE")):
        assert int(re.search(rf"SALVE_PGO_STOP_{stop} = (\d+)", header).group(1)) == k == getattr(_lib, f"PGO_STOP_{stop}") == getattr(pc, f"STOP_{stop}")
    assert lib.salve_hip_version() == 7 == _lib.EXPECTED_ABI
    # the size query is host code: nothing for floors that fit in LDS, the packed triangle of 3 M unknowns per floor beyond
    ws = lambda F, M: int(lib.salve_pose_graph_optimise_workspace_bytes(F, M))
    assert ws(5, pc.LDS_NODES) == 0 and ws(5, 57) == 5 * 8 * (171 * 172 // 2) and ws(1, 256) == 8 * (768 * 769 // 2) and ws(0, 64) == ws(1, 257) == ws(1, 0) == 0


def _measurements(floors):
    cols = {k: [] for k in ("building_id", "floor_id", "i1", "i2", "prob", "y_hat", "y_true", "R", "t", "s", "wdo_pair_uuid", "configuration")}
    for b, fl, edges in floors:
        for i1, i2, prob in edges:
            for k, v in (("building_id", b), ("floor_id", fl), ("i1", i1), ("i2", i2), ("prob", prob), ("y_hat", 1), ("y_true", 1), ("R", np.eye(2)),
                         ("t", [1.0, 0.0]), ("s", 1.0), ("wdo_pair_uuid", "door_0_0"), ("configuration", "identity")):
                cols[k].append(v)
    return pg.EdgeMeasurements(**cols)


def test_run_and_the_command_line_refuse_what_they_document(tmp_path, capsys):
    meas = _measurements([("0001", "floor_01", [(0, 1, 0.9), (1, 2, 0.9)])])
    with pytest.raises(ValueError, match="unknown method"):
        pg.run(meas, 0.5, method="pose2_slam")
    with pytest.raises(ValueError, match="belong to method pgo"):
        pg.run(meas, 0.5, method="spanning_tree", max_iterations=3)
    with pytest.raises(ValueError, match="belong to method pgo"):
        pg.run(meas, 0.5, method="random_spanning_trees", robust=False)
    with pytest.raises(ValueError, match="max_iterations"):
        pg.run(meas, 0.5, method="pgo", max_iterations=-1)
    for bad in ({"relative_error_tol": 0.0}, {"absolute_error_tol": float("nan")}, {"huber_k": -1.0}, {"odometry_sigmas": (0.2, 0.0, 0.1)},
                {"prior_sigmas": (0.3, 0.3)}):
        with pytest.raises(ValueError, match="pose_graph.optimise"):
            pg.run(meas, 0.5, method="pgo", **bad)
    with pytest.raises(TypeError, match="unknown options"):
        pg.optimise(meas, 0.5, num_hypotheses=3)
    with pytest.raises(ValueError, match="keep_rows"):
        pg.optimise(meas, 0.5, keep_rows=np.ones(5, dtype=bool))
    big = _measurements([("0001", "floor_01", [(k, k + 1, 0.9) for k in range(256)])])
    with pytest.raises(_lib.SalveHipError, match="257 panoramas"):
        pg.optimise(big, 0.5)
    assert pg.optimise(_measurements([]), 0.5) == []
    (tmp_path / "pred").mkdir()
    for argv in (["--method", "spanning_tree", "--pgo-no-robust"], ["--method", "random_spanning_trees", "--pgo-max-iterations", "3"],
                 ["--method", "pgo", "--pgo-max-iterations", "-2"], ["--method", "pose2_slam"]):
        with pytest.raises(SystemExit) as e:
            pg.main([str(tmp_path / "pred"), "--hypotheses", str(tmp_path), "--confidence-threshold", "0.5"] + argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def test_pgo_solution_survives_json():
    sim = lambda th, x, y: pg.Sim2(np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]], dtype=np.float32), np.array([x, y], dtype=np.float32), 1.0)
    tree_opts = {"confidence_threshold": 0.5, "cycle_filter": False, "rot_threshold_deg": 0.5, "trans_threshold": float("inf")}
    edge = {"row": 0, "prob": 0.9, "y_true": 1, "wdo_pair_uuid": "door_0_0", "configuration": "identity", "consistent": False, "n_triplets": 0,
            "n_consistent": 0, "min_rot_err": float("inf"), "min_trans_err": float("inf")}
    tree = pg.FloorSolution("0001", "floor_01", np.array([2, 5]), tree_opts, {(2, 5): sim(0.1, 1.0, 0.0)}, {}, [None, None, sim(0, 0, 0), None, None, sim(-0.1, -1, 0.1)],
                            {(2, 5): edge}, {2: -1, 5: 2}, {2: 0, 5: 1}, {"n_nodes": 2, "n_rows": 1, "n_chosen": 1, "n_triplets": 0, "n_consistent_triplets": 0,
                                                                          "n_consistent_edges": 0, "n_localized": 2}, 2)
    record = {"n_unknown_nodes": 2, "n_factors": 2, "n_iterations": 1, "n_rejected": 0, "n_downweighted": 0, "stop_reason": "absolute_error_tol", "lambda": 1e-6,
              "cost_initial": 0.25, "cost_final": None}
    sol = pg.PgoSolution("0001", "floor_01", np.array([2, 5]), {**tree_opts, "method": "pgo", "robust": True}, tree,
                         [None, None, sim(0, 0, 0), None, None, sim(-0.1, -1.0, 0.125)], {2: (0.0, 0.0, 0.0), 5: (-1.0, 0.125, -0.1)}, record)
    d = json.loads(json.dumps(sol.to_json()))
    back = pg.PgoSolution.from_json(d)
    assert back.to_json() == sol.to_json() and back.pose == sol.pose and back.record == record and back.options["trans_threshold"] == float("inf")
    assert back.tree.to_json() == tree.to_json() and back.origin == 2 and back.counts["n_localized"] == 2
    assert back.wSi_list[5].translation.tobytes() == sol.wSi_list[5].translation.tobytes() and back.wSi_list[3] is None
    assert "pgo over 2 factors" in sol.summary() and "nan" in sol.summary() and pg.json_fname(sol) == "pose_graph_0001_floor_01.json"
