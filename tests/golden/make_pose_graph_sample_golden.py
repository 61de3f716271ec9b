"""Regenerates tests/golden/pose_graph_sample_*.json: inputs and outputs of the REFERENCE's ransac_spanning_trees
(salve/algorithms/spanning_tree.py:179-334, with compute_hypothesis_errors and compute_objective_function_improvement) on three small graphs,
recorded as data.  tests/test_pose_graph_sample_host.py asks salve_amd.pose_graph.draw_hypotheses to reproduce the drawn subsets and the
emulator of tests/pose_graph_sample_cases.py to reproduce the winner, its measurements and its poses.

    python tests/golden/make_pose_graph_sample_golden.py /path/to/the/reference/checkout

Needs numpy, networkx, scipy and matplotlib; the stand-ins are make_pose_graph_golden.py's.  A measurement is a plain object with .i1, .i2 and
.i2Si1 (the reference's Sim2).  The subsets are what the reference's own np.random.choice calls return after np.random.seed(seed): the calls
are recorded, not replaced.

The graphs are odd cycles joined at single nodes, several rows per pair, every row noisy: shortest paths are unique in every subgraph, and
the generator takes the first seed at which no drawn subset has two largest components and no scan step lies within 1e-2 of 0."""

import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))

import make_pose_graph_golden as base  # noqa: E402
from tests import pose_graph_cases as pc  # noqa: E402
from tests import pose_graph_sample_cases as sc  # noqa: E402


def graphs():
    """name -> (rows in MEASUREMENT order with compact indices, pano id of every compact index, seed, num_hypotheses, sampling_fraction)."""
    out = {}
    for name, seed, n_tri, tail, per_pair, step, num, fraction in (("chain", 7, 3, 0, 2, 1, 12, 0.5), ("pentagon", 11, 2, 1, 2, 3, 20, 0.6),
                                                                 ("long", 23, 5, 1, 3, 2, 10, 0.7)):
        rng = np.random.default_rng(seed)
        fb = sc._cactus(rng, n_tri, scales=name != "chain", rows_per_pair=per_pair, tail=tail)
        rows = np.array(fb.rows, dtype=pc.ROW)
        rows = rows[rng.permutation(len(rows))]          # measurement order is not pair order
        out[name] = (rows, [step * k + (step - 1) for k in range(fb.n)], seed, num, fraction)
    return out


def main(reference_root: str) -> None:
    sys.path.insert(0, reference_root)
    base._stand_ins()
    import salve.algorithms.spanning_tree as spanning_tree
    from salve.common.sim2 import Sim2

    for name, (rows, pano, first_seed, num, fraction) in graphs().items():
        doc = None
        for seed in range(first_seed, first_seed + 500):   # the first seed whose draws keep the conditions below
            doc = record(spanning_tree, Sim2, name, rows, pano, seed, num, fraction)
            if doc is not None:
                break
        assert doc is not None, name
        with open(HERE / f"pose_graph_sample_{name}.json", "w") as f:
            json.dump(doc, f, indent=1)
        print(name, "seed", seed, len(doc["measurements"]), "measurements,", len(doc["hypotheses"]), "hypotheses,", len(doc["best_hypothesis"]), "kept,",
              sum(S is not None for S in doc["wSi_list"]), "poses", file=sys.stderr)


def record(spanning_tree, Sim2, name, rows, pano, seed, num, fraction):
    sim = lambda S: None if S is None else {"R": S.rotation.flatten().tolist(), "t": S.translation.flatten().tolist(), "s": S.scale}
    meas = [SimpleNamespace(i1=pano[int(r["i1"])], i2=pano[int(r["i2"])], i2Si1=Sim2(r["R"].reshape(2, 2).copy(), r["t"].copy(), float(r["s"])))
            for r in rows]
    drawn, choice = [], np.random.choice

    def recording_choice(*args, **kwargs):
        drawn.append(choice(*args, **kwargs))
        return drawn[-1]

    np.random.seed(seed)
    np.random.choice = recording_choice
    try:
        wSi_list, best = spanning_tree.ransac_spanning_trees(meas, num_hypotheses=num, sampling_fraction=fraction)
    finally:
        np.random.choice = choice
    # the conditions under which the record does not hang on networkx's iteration order or on one ulp of an arctan2
    order = np.lexsort((rows["i2"], rows["i1"]))
    position = {int(r): k for k, r in enumerate(order)}
    recs = []
    for subset in drawn:
        mask = sc.masks_of([[position[int(k)] for k in subset]], len(rows))[0]
        rec, _, det = sc.emulate_hypothesis(rows[order], len(pano), 0.5, mask)
        if det["tied_components"] != 1 or any(k != 1 for k in det["paths"].values()):
            return None
        recs.append(rec)
    if any(abs(o) < 1e-2 for o in sc.scan(recs)[4]):
        return None
    return {"seed": seed, "num_hypotheses": num, "sampling_fraction": fraction, "confidence_threshold": 0.5,
           "measurements": [{"i1": m.i1, "i2": m.i2, "prob": float(r["prob"]), **sim(m.i2Si1)} for m, r in zip(meas, rows)],
           "hypotheses": [[int(k) for k in subset] for subset in drawn],
           "best_hypothesis": [next(k for k, m in enumerate(meas) if m is b) for b in best],
           "wSi_list": [sim(S) for S in wSi_list]}


if __name__ == "__main__":
    main(sys.argv[1])
