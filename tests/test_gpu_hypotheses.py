"""salve_hypotheses_generate on the MI355X against the emulator of tests/hypotheses_cases.py: every synthetic case and the fixture floor
(ZInD 0000 floor_01 with MHNet's predictions) -- the kept rows in candidate order with every float32 of R and t bit for bit, labels, counts,
visibly_adjacent and i2Ti1_gt; written into sentinel-filled buffers, so that nothing outside the reported rows changes; the same bytes on a
second call; and salve_amd.hypotheses.generate's FloorHypotheses in the order ingest.load_floor_hypotheses gives."""

from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from salve_amd import _lib, hypotheses  # noqa: E402
from tests import hypotheses_cases as hc  # noqa: E402

DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden"
CASES = hc.cases()


def on_gpu(packed, min_width_ratio):
    """One launch into sentinel-filled buffers with GUARD records behind them -> (rows, pair_out) as numpy records, guards included."""
    fill = lambda n: torch.full((n,), hc.SENTINEL, dtype=torch.uint8, device=DEV)
    rows_t = fill((packed.n_rows + hc.GUARD) * hc.ROW.itemsize)
    pairs_t = fill((len(packed.pairs) + hc.GUARD) * hc.PAIR_OUT.itemsize)
    hypotheses.launch(packed, DEV, min_width_ratio, out_rows=rows_t, out_pairs=pairs_t)
    torch.cuda.synchronize()
    return rows_t.cpu().numpy().view(hc.ROW), pairs_t.cpu().numpy().view(hc.PAIR_OUT)


def assert_buffers_equal(got, want, what):
    if got.tobytes() == want.tobytes():
        return
    for k in range(len(want)):
        assert got[k].tobytes() == want[k].tobytes(), f"{what} record {k}: got {got[k]}, want {want[k]}"


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cases_equal_the_emulator(case):
    """Raw buffers byte for byte (the sentinel bytes behind n_kept and behind the buffers included), then the assembled floors."""
    assert hc.check_margins(case) >= hc.MIN_MARGIN
    packed = hypotheses.pack([hc.floor_input(f) for f in case["floors"]])
    want_rows, want_pairs, caps = hc.expected_buffers(case)
    assert packed.pairs["capacity"].tolist() == caps and packed.n_rows == sum(caps)
    rows, pairs = on_gpu(packed, case["min_width_ratio"])
    assert_buffers_equal(pairs, want_pairs, "pair")
    assert_buffers_equal(rows, want_rows, "row")
    rows2, pairs2 = on_gpu(packed, case["min_width_ratio"])
    assert rows2.tobytes() == rows.tobytes() and pairs2.tobytes() == pairs.tobytes(), "a second call gives other bytes"
    floors = hypotheses.generate([hc.floor_input(f) for f in case["floors"]], DEV, case["min_width_ratio"], hypotheses_save_root="root")
    assert len(floors) == len(case["floors"])
    for f, got in zip(case["floors"], floors):
        emu = hc.emulate_floor(f, case["min_width_ratio"])
        want = hc.expected_hypotheses(emu)
        assert (got.building_id, got.floor_id, len(got)) == (f["building_id"], f["floor_id"], len(want))
        assert got.label.tolist() == [w[0] for w in want] and got.pair_idx.tolist() == [w[1] for w in want]
        assert got.i1.tolist() == [w[2] for w in want] and got.i2.tolist() == [w[3] for w in want]
        assert got.pair_uuid == [w[6] for w in want]
        assert got.fpaths == [f"root/{f['building_id']}/{f['floor_id']}/{hc.LABEL_DIRS[1 - w[0]]}/{w[7]}" for w in want]
        assert got.R.tobytes() == b"".join(np.asarray(w[4], dtype="<f4").tobytes() for w in want)
        assert got.t.tobytes() == b"".join(np.asarray(w[5], dtype="<f4").tobytes() for w in want)
        assert (got.s == 1.0).all()
        assert got.pairs.i1.tolist() == [p["i1"] for p in emu] and got.pairs.i2.tolist() == [p["i2"] for p in emu]
        assert got.pairs.n_valid.tolist() == [p["n_valid"] for p in emu] and got.pairs.n_rejected.tolist() == [p["n_rejected"] for p in emu]
        assert got.pairs.visibly_adjacent.tolist() == [p["adjacent"] for p in emu]


@pytest.fixture(scope="module")
def fixture_floor(tmp_path_factory):
    raw, root = hc.expand_fixture(GOLDEN, tmp_path_factory.mktemp("hypotheses_fixture"))
    (fi,) = hypotheses.load_floors(raw, root, ["0000"])
    return fi


def test_fixture_floor_equals_the_emulator_and_the_recorded_result(fixture_floor):
    """ZInD 0000 floor_01, 32 panoramas, 496 pairs: the device's raw buffers equal the emulator's, and the assembled floor equals the
    recorded names, counts and digest of tests/golden/hypotheses_0000_floor_01.json."""
    import json

    case = {"name": "fixture", "floors": [hc.floor_dict(fixture_floor)], "min_width_ratio": 0.65}
    assert hc.check_margins(case) >= hc.MIN_MARGIN
    packed = hypotheses.pack([fixture_floor])
    want_rows, want_pairs, _ = hc.expected_buffers(case)
    rows, pairs = on_gpu(packed, 0.65)
    assert_buffers_equal(pairs, want_pairs, "pair")
    assert_buffers_equal(rows, want_rows, "row")
    rec = json.loads((GOLDEN / hc.GOLDEN_RESULT).read_text())
    (got,) = hypotheses.generate([fixture_floor], DEV)
    assert len(got) == rec["n_hypotheses"] == 2672 and int(got.label.sum()) == rec["counts"][hc.LABEL_DIRS[0]]
    assert [[hc.LABEL_DIRS[0] if l else hc.LABEL_DIRS[1], Path(fp).name] for l, fp in zip(got.label, got.fpaths)] == hc.recorded_names(rec)
    assert hc.digest([(None, None, None, None, got.R[k].reshape(4), got.t[k]) for k in range(len(got))]) == rec["digest_R_t"]
    assert hypotheses.floor_summary(got)[:2] == (rec["n_valid_configurations"], rec["n_invalid_configurations"])
    assert [[int(a), int(b)] for a, b, adj in zip(got.pairs.i1, got.pairs.i2, got.pairs.visibly_adjacent) if adj] == rec["visibly_adjacent"]


def test_refusals_before_a_launch():
    lib = _lib.load()
    ok = torch.zeros(64, dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()
    call = lambda **kw: lib.salve_hypotheses_generate(*[kw.get(k, d) for k, d in (
        ("wdo_xy", None), ("wdo_type", None), ("wdo_off", p(ok)), ("n_wdo", 0), ("gt_xy", None), ("gt_off", p(ok)), ("n_gt", 0), ("poses", p(ok)), ("n_panos", 1),
        ("pairs", p(ok)), ("n_pairs", 1), ("max_capacity", 0), ("ratio", 0.65), ("out_rows", None), ("n_rows", 0), ("out_pairs", p(ok)), ("stream", None))])
    assert call(n_pairs=0) == 0
    for bad in (dict(n_pairs=-1), dict(max_capacity=_lib.HYP_MAX_CAPACITY + 1), dict(ratio=float("nan")), dict(pairs=None), dict(out_pairs=p(ok) + 4),
                dict(n_rows=1)):
        assert call(**bad) == -1, bad   # SALVE_ERR_BAD_ARG
    assert (ok == 0).all()
