"""Regenerates tests/golden/pose_graph_*.json: inputs and outputs of the REFERENCE's filter_to_SE2_cycle_consistent_edges
(salve/algorithms/cycle_consistency.py:225-303) and greedily_construct_st_Sim2 (salve/algorithms/spanning_tree.py:73-141) on three small
graphs, recorded as data.  tests/test_pose_graph_cases_host.py asks the emulator of tests/pose_graph_cases.py to reproduce them.

    python tests/golden/make_pose_graph_golden.py /path/to/the/reference/checkout

Needs numpy, networkx, scipy and matplotlib.  The reference's two modules are imported as they are; what they import but do not use on this
path is replaced by empty stand-ins: gtsam, gtsfm (but for the one function named below), sklearn, and the reference's own plotting, pose-graph
and evaluation modules.  gtsfm.utils.graph.get_nodes_in_largest_connected_component is the one function of a stand-in that runs; it is
restated here from its documented behaviour: the nodes of the largest connected component of the graph of the given edges.

The graphs have unique shortest paths from their origin, one largest component and one row per pair, so the recorded outputs do not hang on
networkx's iteration order."""

import importlib
import json
import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import pose_graph_cases as pc  # noqa: E402


class _Anything(types.ModuleType):
    """A module whose every attribute is a class nobody instantiates on this path."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def _stand_ins() -> None:
    import networkx as nx

    for name in ("gtsam", "gtsfm", "gtsfm.utils", "gtsfm.utils.geometry_comparisons", "sklearn", "salve.utils.pr_utils", "salve.common.posegraph2d",
                 "salve.common.edge_classification", "salve.utils.graph_rendering_utils"):
        sys.modules[name] = _Anything(name)
    sys.modules["salve.common.posegraph2d"].ENDCOLOR = sys.modules["salve.common.posegraph2d"].REDTEXT = ""
    for name in [m for m in sys.modules if m.startswith("salve.")]:   # `import a.b.c as x` reads c off its (real, namespace) parent package
        parent, leaf = name.rsplit(".", 1)
        setattr(importlib.import_module(parent), leaf, sys.modules[name])
    graph = types.ModuleType("gtsfm.utils.graph")

    def get_nodes_in_largest_connected_component(edges):
        if len(edges) == 0:
            return []
        G = nx.Graph()
        G.add_edges_from(edges)
        return list(max(nx.connected_components(G), key=len))

    graph.get_nodes_in_largest_connected_component = get_nodes_in_largest_connected_component
    sys.modules["gtsfm.utils.graph"] = graph
    sys.modules["gtsfm.utils"].graph = graph
    sys.modules["gtsfm"].utils = sys.modules["gtsfm.utils"]


def graphs():
    """name -> (rows, n): one row per pair (tests/pose_graph_cases.py's builders)."""
    rng = np.random.default_rng(73141)
    fan = pc.FloorBuilder(6, pc.global_poses(rng, 6, scales=True), rng)
    for i in range(1, 6):
        fan.edge(0, i)
    for i in range(1, 5):
        fan.edge(i, i + 1, rot_deg=3.0 if i == 2 else 0.0)
    bridge = pc.FloorBuilder(8, pc.global_poses(rng, 8, scales=True), rng).edge(0, 1).edge(1, 2).edge(0, 2).edge(2, 3).edge(3, 4).edge(3, 5)
    bridge.edge(4, 5).edge(3, 6).edge(5, 6, shift=(0.0, 0.05)).edge(3, 7).edge(4, 7)
    apart = pc.FloorBuilder(6, pc.global_poses(rng, 6), rng).edge(0, 1).edge(2, 3).edge(3, 4).edge(2, 4).edge(4, 5)
    return {"fan": fan.build(), "bridge": bridge.build(), "apart": apart.build()}


def main(reference_root: str) -> None:
    sys.path.insert(0, reference_root)
    _stand_ins()
    import salve.algorithms.cycle_consistency as cycle_consistency
    import salve.algorithms.spanning_tree as spanning_tree
    from salve.common.sim2 import Sim2

    sim = lambda S: None if S is None else {"R": S.rotation.flatten().tolist(), "t": S.translation.flatten().tolist(), "s": S.scale}
    for name, (rows, n) in graphs().items():
        i2Si1 = {(int(r["i1"]), int(r["i2"])): Sim2(r["R"].reshape(2, 2).copy(), r["t"].copy(), float(r["s"])) for r in rows}
        consistent = cycle_consistency.filter_to_SE2_cycle_consistent_edges(i2Si1, two_view_reports_dict=None, visualize=False, verbose=False)
        tree_filtered = spanning_tree.greedily_construct_st_Sim2(consistent, verbose=False)
        tree_all = spanning_tree.greedily_construct_st_Sim2(i2Si1, verbose=False)
        doc = {"n_nodes": n, "SE2_cycle_rot_threshold_deg": 0.5, "SE2_cycle_trans_threshold": 0.01,
               "i2Si1": [{"i1": a, "i2": b, **sim(S)} for (a, b), S in i2Si1.items()],
               "consistent_edges": sorted([a, b] for a, b in consistent),
               "wSi_list_filtered": None if tree_filtered is None else [sim(S) for S in tree_filtered],
               "wSi_list_unfiltered": None if tree_all is None else [sim(S) for S in tree_all]}
        with open(Path(__file__).resolve().parent / f"pose_graph_{name}.json", "w") as f:
            json.dump(doc, f, indent=1)
        print(name, len(i2Si1), "edges,", len(consistent), "consistent")


if __name__ == "__main__":
    main(sys.argv[1])
