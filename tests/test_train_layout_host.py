"""Host side of the layout modality in the rendered training feed: the export and the record struct, `PanoLayouts` and its file, the
numpy restatement of salve_layout_pose against `pack_layouts`' tables, the comparator against emulated wrong kernels, and the job /
channel tables of layout batches.  No GPU."""

import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import layout_cases as lc  # noqa: E402
from salve_amd import _lib, layout, synthetic, synthetic_layouts, train_render  # noqa: E402
from salve_amd.common.sim2 import Sim2  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "salve_hip.h").read_text()
LAYOUT, ALL3 = ["layout"], ["ceiling_rgb_texture", "floor_rgb_texture", "layout"]
HW = 501 * 501


# ---------------------------------------------------------------------------------------------------- 1. library
def test_library_exports_layout_pose_and_abi_stays_7():
    lib = _lib.load()
    assert hasattr(lib, "salve_layout_pose") and "salve_layout_pose" in _lib.EXPORTED_SYMBOLS
    assert re.search(r"\bint salve_layout_pose\(", HEADER)
    assert lib.salve_hip_version() == 7 == _lib.EXPECTED_ABI
    assert int(re.search(r"#define SALVE_STATUS_BAD_LAYOUT (\d+)", HEADER).group(1)) == _lib.STATUS_BAD_LAYOUT == 64
    with pytest.raises(_lib.SalveHipError, match="layout image"):
        _lib.check_status_word(_lib.STATUS_BAD_LAYOUT, "x")


def test_pose_record_has_the_headers_layout():
    class Rec(ctypes.Structure):
        _fields_ = [("pano", ctypes.c_int32), ("poly_off", ctypes.c_int32), ("seg_off", ctypes.c_int32), ("reserved", ctypes.c_int32),
                    ("R", ctypes.c_float * 4), ("t", ctypes.c_float * 2), ("s", ctypes.c_double)]

    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} salve_layout_pose_t;", HEADER).group(1), flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n).strip() for d in body.split(";") if d.strip() for n in re.sub(r"^\s*(int32_t|float|double)", "", d.strip()).split(",")]
    assert names == [f[0] for f in Rec._fields_] == list(_lib.LAYOUT_POSE_DTYPE.names)
    assert ctypes.sizeof(Rec) == _lib.LAYOUT_POSE_DTYPE.itemsize == 48
    assert [_lib.LAYOUT_POSE_DTYPE.fields[n][1] for n in names] == [getattr(Rec, n).offset for n in names]


# ---------------------------------------------------------------------------------------------------- 2. PanoLayouts
def _same(a: layout.PanoLayouts, b: layout.PanoLayouts) -> bool:
    return all(np.array_equal(getattr(a, n), getattr(b, n)) and getattr(a, n).dtype == getattr(b, n).dtype for n, _, _ in layout.PanoLayouts.FIELDS)


def test_synthetic_layouts_cover_the_cases():
    specs = synthetic_layouts.make_layout_specs(lc.P, seed=0)
    pl = layout.PanoLayouts.from_specs(specs)
    assert pl.P == lc.P and int(pl.room_count[1]) == 0 and int(pl.wdo_count[1]) == 0          # the empty room
    rooms = np.delete(pl.room_count, 1) - 1                                                  # (stored closed)
    assert rooms.min() >= 4 and rooms.max() <= 12 and len(set(rooms.tolist())) > 3
    assert pl.wdo_count.max() <= 6 and (pl.wdo_count[2::3] == 0).all() and set(pl.wdo_type.tolist()) == {0, 1, 2}
    for p in range(pl.P):   # closed rooms; doors, windows, openings in drawing order
        room, wdos = pl.spec(p)
        assert len(room) == 0 or np.array_equal(room[0], room[-1])
        order = [("doors", "windows", "openings").index(w) for w, _ in wdos]
        assert order == sorted(order)
    assert _same(pl, synthetic_layouts.make_layouts(lc.P, seed=0)) and not _same(pl, synthetic_layouts.make_layouts(lc.P, seed=1))


def test_from_specs_save_load_round_trip(tmp_path):
    pl = synthetic_layouts.make_layouts(9, seed=3)
    pl.save(tmp_path / "layouts.npz")
    back = layout.PanoLayouts.load(tmp_path / "layouts.npz")
    assert _same(pl, back)
    assert _same(train_render.load_render_layouts(str(tmp_path), 9), pl)
    for p in range(9):
        (r0, w0), (r1, w1) = synthetic_layouts.make_layout_specs(9, seed=3)[p], back.spec(p)
        assert np.array_equal(r0, r1) and [a for a, _ in w0] == [a for a, _ in w1] and all(np.array_equal(a[1], b[1]) for a, b in zip(w0, w1))


def test_malformed_layout_files_are_refused_in_one_line(tmp_path):
    pl = synthetic_layouts.make_layouts(5, seed=1)
    tabs = {n: getattr(pl, n) for n, _, _ in layout.PanoLayouts.FIELDS}

    def refused(match, n_panos=5, **changed):
        with open(tmp_path / "layouts.npz", "wb") as f:
            np.savez(f, **{k: v for k, v in {**tabs, **changed}.items() if v is not None})
        with pytest.raises(SystemExit) as e:
            train_render.load_render_layouts(str(tmp_path), n_panos)
        msg = str(e.value)
        assert re.search(match, msg) and "\n" not in msg and "layouts.npz" in msg, msg

    with pytest.raises(SystemExit, match="layouts.npz is missing"):
        train_render.load_render_layouts(str(tmp_path), 5)
    refused("room_off must be a int64 array", room_off=pl.room_off.astype(np.int32))
    refused("room_xy must be a float64 array", room_xy=pl.room_xy.astype(np.float32))
    refused("wdo_type must be a uint8 array", wdo_type=pl.wdo_type.astype(np.int64))
    bad = pl.room_off.copy()
    bad[2] = bad[3] + 1
    refused("room_off must rise", room_off=bad)
    bad = pl.wdo_off.copy()
    bad[-1] += 1
    refused("wdo_off must rise", wdo_off=bad)
    refused("wdo_type must hold one code", wdo_type=np.full_like(pl.wdo_type, 3))
    refused("missing table", wdo_xy=None)
    refused("holds the layouts of 5 panoramas, panos_rgb.npy holds 6", n_panos=6)
    (tmp_path / "layouts.npz").write_bytes(b"not a zip file")
    with pytest.raises(SystemExit) as e:
        train_render.load_render_layouts(str(tmp_path), 5)
    assert "\n" not in str(e.value)


def _stand_in_graph():
    wdo = lambda kind, a, b: SimpleNamespace(type=kind, vertices_local_2d=np.array([a, b], dtype=np.float64))
    node = lambda room, doors=(), windows=(), openings=(): SimpleNamespace(room_vertices_local_2d=np.array(room, dtype=np.float64), doors=list(doors),
                                                                            windows=list(windows), openings=list(openings))
    return SimpleNamespace(nodes={
        3: node([[0, 0], [2, 0], [2, 1.5], [0, 1.5]], doors=[wdo("doors", [0.2, 0], [0.9, 0])], windows=[wdo("windows", [2, 0.3], [2, 1.0])]),
        7: node([[-1, -1], [1, -1], [1, 0], [0, 0], [0, 1], [-1, 1]], windows=[wdo("windows", [-1, -0.5], [-1, 0.5])],
                openings=[wdo("openings", [0, 0.2], [0, 0.8])], doors=[wdo("doors", [-0.5, -1], [0.5, -1]), wdo("doors", [1, -0.8], [1, -0.2])]),
        8: node([[0, 0], [1, 0], [1, 1]]),
    })


def test_from_pose_graph_equals_fused_layouts_identity_specs():
    graph, pano_ids = _stand_in_graph(), [7, 3, 5, 8]   # (panorama 5 is not in the graph: no room)
    table = synthetic.HypothesisTable(np.array([0, 1], np.int32), np.array([1, 3], np.int32), np.tile(np.eye(2, dtype=np.float32), (2, 1, 1)),
                                      np.zeros((2, 2), np.float32), np.zeros(2))
    want = layout.FusedLayouts.from_pose_graph(table, pano_ids, graph)
    pl = layout.PanoLayouts.from_pose_graph(graph, pano_ids)
    assert pl.P == 4 and pl.room_count.tolist() == [7, 5, 0, 4] and pl.wdo_count.tolist() == [4, 2, 0, 0]
    assert [layout.WDO_TYPES[c] for c in pl.wdo_type[:4]] == ["doors", "doors", "windows", "openings"]
    for p, (room, wdos) in enumerate(want.identity):
        r, w = pl.spec(p)
        assert np.array_equal(r, room) and [a for a, _ in w] == [a for a, _ in wdos] and all(np.array_equal(a[1], b[1]) for a, b in zip(w, wdos))
    # and a posed spec is `layout_pair_specs`' first one
    S = Sim2(np.array([[0.0, -1.0], [1.0, 0.0]]), np.array([0.5, -0.25]), 1.25)
    (room1, wdos1), _ = layout.layout_pair_specs(S, graph, 7, 3)
    r, w = pl.spec(0, S)
    assert np.array_equal(r, room1) and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(w, wdos1)) and len(w) == len(wdos1)
    assert lc.tables_equal(layout.pack_layout_tables(want.identity), layout.pose_layouts_numpy(pl, np.arange(4)))


# ---------------------------------------------------------------------------------------------------- 3. the numpy restatement
def test_pose_layouts_numpy_equals_pack_layouts_on_the_seeded_set():
    pl, pano, R, t, s, posed = lc.seeded_set()
    assert pl.P >= 64 and int(posed.sum()) >= 512
    theta = np.degrees(np.arctan2(R[posed][:, 1, 0], R[posed][:, 0, 0])) % 360.0
    assert np.histogram(theta, bins=8, range=(0, 360))[0].min() > 0                       # rotations over the full circle
    assert (s[posed] == 1.0).any() and (s[posed] != 1.0).any()
    assert {1, 2} <= set(pano[posed].tolist())                                            # the empty room and a room without W/D/Os, posed
    want = lc.seeded_host_tables()
    got = layout.pose_layouts_numpy(pl, pano, R, t, s, posed)
    assert lc.tables_equal(want, got)
    rec, poly, seg = got
    assert (poly < 0).any() and (poly > 500).any() and (seg[:, :4] < 0).any()            # parts of rooms outside the window
    assert int(rec["n_poly"].sum()) == len(poly) > 4000 and int(rec["n_seg"].sum()) == len(seg) > 500
    assert rec["n_poly"][0] == 0 and rec["n_seg"][0] == 0 and rec["n_seg"][1] == 0 and rec["n_poly"][1] > 0
    assert set(seg[:, 4].tolist()) == {0x0000ff, 0x00ff00, 0xff0000} and set(seg[:, 5].tolist()) == {8} and not seg[:, 6:].any()
    # the records the device takes carry the same offsets
    recs = layout.pose_records(pl, pano, R, t, s, posed)
    assert np.array_equal(recs["poly_off"], rec["poly_off"]) and np.array_equal(recs["seg_off"], rec["seg_off"])
    assert np.array_equal(recs["R"][~posed], np.tile([1, 0, 0, 1], (lc.P, 1))) and not recs["t"][~posed].any() and (recs["s"][~posed] == 1).all()
    assert np.array_equal(recs["R"][posed], R[posed].reshape(-1, 4)) and np.array_equal(recs["s"][posed], s[posed])


@pytest.mark.parametrize("window", list(lc.WINDOWS))
def test_pose_layouts_numpy_equals_pack_layouts_on_the_strided_set(window):
    """Rooms and W/D/O lists longer than the posing kernel's 64 threads (its loops' second pass), in the default window and a
    non-square one at another resolution."""
    pl, pano, R, t, s, posed = lc.strided_set()
    assert sorted(set(pl.room_count.tolist())) == [1, 63, 64, 65, 130, 200] and sorted(set(pl.wdo_count.tolist())) == [0, 31, 32, 33, 70]
    for p in range(pl.P):   # every panorama with W/D/Os holds all three types
        kinds = set(pl.wdo_type[pl.wdo_off[p]:pl.wdo_off[p + 1]].tolist())
        assert kinds == ({0, 1, 2} if pl.wdo_count[p] else set())
    assert set(pano[posed].tolist()) == set(pano[~posed].tolist()) == set(range(pl.P)) and (s[posed] == 1.0).any() and (s[posed] != 1.0).any()
    theta = np.degrees(np.arctan2(R[posed][:, 1, 0], R[posed][:, 0, 0])) % 360.0
    assert np.histogram(theta, bins=4, range=(0, 360))[0].min() > 0
    bp = lc.window_params(window)
    want = lc.strided_host_tables(window)
    got = layout.pose_layouts_numpy(pl, pano, R, t, s, posed, bev_params=bp)
    assert lc.tables_equal(want, got)
    rec, poly, seg = got
    H, W = (501, 501) if bp is None else (bp.img_h + 1, bp.img_w + 1)
    assert rec["n_poly"].max() == 200 and rec["n_seg"].max() == 70 and len(poly) == int(rec["n_poly"].sum()) and len(seg) == int(rec["n_seg"].sum())
    assert (poly < 0).any() and (poly[:, 0] >= W).any() and (poly[:, 1] >= H).any()      # parts of rooms outside the window
    assert set(seg[:, 4].tolist()) == {0x0000ff, 0x00ff00, 0xff0000} and set(seg[:, 5].tolist()) == {8}
    if bp is not None:   # another window gives other tables
        assert not lc.tables_equal(lc.strided_host_tables("default"), got)


def test_empty_tables_follow_pack_layouts_conventions():
    pl = lc.seeded_set()[0]
    for pano in ([], [1], [1, 1], [2]):   # nothing; the empty room; a room without W/D/Os
        assert lc.tables_equal(layout.pack_layout_tables([pl.spec(p) for p in pano]), layout.pose_layouts_numpy(pl, np.asarray(pano, dtype=np.int64)))
    with pytest.raises(ValueError, match="names panorama 64"):
        layout.pose_records(pl, [0, 64])
    with pytest.raises(ValueError, match="2\\^24"):
        layout.pose_layouts_numpy(pl, [0], np.eye(2)[None], np.array([[3.0e5, 0.0]]), [1.0], [True])


# ---------------------------------------------------------------------------------------------------- 4. the comparator rejects wrong kernels
def test_emulator_without_a_mistake_passes():
    assert lc.tables_equal(lc.seeded_host_tables(), lc.emulate(None, *lc.seeded_set()))
    half = lc.half_pixel_set()
    assert lc.tables_equal(layout.pack_layout_tables(lc.host_specs(half[0], half[1], None, None, None, half[5])), lc.emulate(None, *half))
    assert lc.tables_equal(layout.pose_layouts_numpy(*half), lc.emulate(None, *half))


@pytest.mark.parametrize("variant", lc.VARIANTS)
def test_comparator_rejects_an_emulated_wrong_kernel(variant):
    case = lc.half_pixel_set() if variant == "round half away" else lc.seeded_set()
    want = layout.pose_layouts_numpy(*case) if variant == "round half away" else lc.seeded_host_tables()
    wrong = lc.emulate(variant, *case)
    assert not lc.tables_equal(want, wrong), variant
    if variant == "round half away":   # exactly the ties differ, each by one pixel upwards
        d = wrong[1].astype(np.int64) - want[1]
        assert set(d.reshape(-1).tolist()) == {0, 1} and int(d.sum()) > 0
    if variant == "doors and windows swapped":   # geometry equal, colours not
        assert np.array_equal(want[2][:, :4], wrong[2][:, :4]) and np.array_equal(want[1], wrong[1])


# ---------------------------------------------------------------------------------------------------- 5. job and channel tables
class _TablesOnly(train_render.RenderedTrainSource):
    """The source's table building without a device."""

    def __init__(self, mods, identity, layouts, n_panos, batch_size):
        self.surfaces = train_render.train_surfaces(mods, with_layouts=True)
        self.has_layout, self.layouts, self.identity, self.batch_size, self.pool = True, layouts, identity, batch_size, None
        self.per_sample = len(self.surfaces) + 1
        self.ras = SimpleNamespace(bev_hw=(501, 501))
        self.lay_base = self.layout_bases(n_panos, n_panos)
        self.n_panos = n_panos


def _tables(mods, identity, B=6, n_panos=9):
    pl = synthetic_layouts.make_layouts(n_panos, seed=5)
    hyp = synthetic.make_hypotheses(B, n_panos, seed=4)
    hyp.swap = np.array([0, 1, 1, 0, 1, 0], dtype=bool)
    hyp.i2[:] = [4, 2, 4, 7, 2, 4]   # three distinct second panoramas
    src = _TablesOnly(mods, identity, pl, n_panos, B)
    src.examples = train_render.plan_examples(hyp, np.zeros(B, np.int64), n_panos)
    draws = [(k, 10 - k, bool(k & 1), bool(k & 2)) for k in range(B)]
    return src, hyp, pl, src.batch_tables(np.arange(B), draws)


@pytest.mark.parametrize("identity", ["kept", "batch"])
def test_layout_only_batch_tables(identity):
    B, Pn = 6, 9
    src, hyp, pl, (jobs, aug, rows, recs, n) = _tables(LAYOUT, identity)
    sw = hyp.swap.astype(np.int64)
    assert src.surfaces == [] and src.per_sample == 1 and n == 0 and len(rows) == 0 and jobs.shape == (2, B, 1)
    assert src.lay_base == (0, 0)                                                  # no texture render in front of the layout images
    assert jobs["slot"][0, :, 0].tolist() == jobs["slot"][1, :, 0].tolist() == list(range(B))
    assert jobs["chan"][0, :, 0].tolist() == (3 * sw).tolist() and jobs["chan"][1, :, 0].tolist() == (3 * (1 - sw)).tolist()
    assert jobs["bev_offset"][0, :, 0].tolist() == [k * HW for k in range(B)]
    if identity == "kept":
        assert len(recs) == B and jobs["bev_offset"][1, :, 0].tolist() == [int(p) * HW for p in hyp.i2]
    else:   # the three distinct identity layouts (panoramas 2, 4, 7) behind the six posed ones
        assert len(recs) == B + 3 and recs["pano"][B:].tolist() == [2, 4, 7]
        assert jobs["bev_offset"][1, :, 0].tolist() == [(B + {2: 0, 4: 1, 7: 2}[int(p)]) * HW for p in hyp.i2]
        assert np.array_equal(recs["R"][B:], np.tile([1, 0, 0, 1], (3, 1))) and not recs["t"][B:].any()
    assert recs["pano"][:B].tolist() == hyp.i1.tolist() and np.array_equal(recs["R"][:B], hyp.R.reshape(B, 4)) and np.array_equal(recs["t"][:B], hyp.t)
    assert (recs["s"] == 1.0).all() and np.array_equal(recs["poly_off"], np.cumsum(pl.room_count[recs["pano"]]) - pl.room_count[recs["pano"]])
    assert aug["crop_y"].tolist() == list(range(B)) and aug["flags"].tolist() == [0, 1, 2, 3, 0, 1]


@pytest.mark.parametrize("identity", ["kept", "batch"])
def test_three_modality_batch_tables(identity):
    B, Pn, S = 6, 9, 2
    src, hyp, pl, (jobs, aug, rows, recs, n) = _tables(ALL3, identity)
    sw = hyp.swap.astype(np.int64)
    assert src.surfaces == ["ceiling", "floor"] and src.per_sample == 3 and jobs.shape == (2, B, 3)
    for ab, s_ in ((0, sw), (1, 1 - sw)):   # ceiling pair, floor pair, layout pair: the layout follows the texture maps
        assert jobs["chan"][ab].tolist() == [[3 * int(x), 6 + 3 * int(x), 12 + 3 * int(x)] for x in s_]
        assert (jobs["slot"][ab] == np.arange(B)[:, None]).all()
    U = 0 if identity == "kept" else 3
    n_tex = (B + (min(B, Pn) if identity == "batch" else 0)) * S                   # the array's texture part is sized for B distinct second panoramas
    assert n == (B + U) * S and len(rows) == n and src.lay_base == (n_tex, Pn * S)
    tex = jobs["bev_offset"][:, :, :S]
    assert (tex % HW == 0).all() and sorted((tex[0] // HW).reshape(-1).tolist()) == sorted(set((tex[0] // HW).reshape(-1).tolist()))
    assert int(tex[0].max()) < n * HW                                              # texture jobs stay in front of the layout images
    assert jobs["bev_offset"][0, :, S].tolist() == [(n_tex + k) * HW for k in range(B)]
    if identity == "kept":
        assert jobs["bev_offset"][1, :, S].tolist() == [(Pn * S + int(p)) * HW for p in hyp.i2]
        assert (tex[1] // HW).tolist() == [[int(p) * S, int(p) * S + 1] for p in hyp.i2]
        assert int(tex[1].max()) < Pn * S * HW
    else:
        assert jobs["bev_offset"][1, :, S].tolist() == [(n_tex + B + {2: 0, 4: 1, 7: 2}[int(p)]) * HW for p in hyp.i2]
        assert int(tex[1].max()) < n * HW
    assert len(recs) == B + U
    assert int(jobs["bev_offset"][0].max()) < (n_tex + B + U) * HW                  # every job of the batch's array lies inside what was drawn


def test_layout_needs_layouts_and_the_launch_limit_covers_them():
    for mods in (LAYOUT, ALL3):
        with pytest.raises(RuntimeError, match="layout"):
            train_render.train_surfaces(mods)
    assert train_render.train_surfaces(LAYOUT, with_layouts=True) == [] and train_render.train_surfaces(ALL3, with_layouts=True) == ["ceiling", "floor"]
    pl = synthetic_layouts.make_layouts(4)
    with pytest.raises(RuntimeError, match="65535"):
        train_render.RenderedTrainSource("cuda:0", LAYOUT, batch_size=65536, layouts=pl)
    with pytest.raises(RuntimeError, match="layout images per batch"):
        train_render.RenderedTrainSource("cuda:0", LAYOUT, batch_size=32768, identity="batch", layouts=pl)
    train_render.check_launch(65535, 0, 0, layout=True)
    train_render.check_launch(32767, 0, 32767, layout=True)
    with pytest.raises(RuntimeError, match="layout images"):
        train_render.check_launch(32768, 0, 32768, layout=True)
