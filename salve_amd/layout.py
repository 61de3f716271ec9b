"""Host side of the rasterised-LAYOUT modality: room polygons and W/D/O segments of many
(panorama, pose) pairs packed into flat tables, ONE launch of salve_layout_rasterise for all of them.

Reference: salve/utils/bev_rendering_utils.py:48-251.  Everything up to the integer pixel coordinates is the reference's numpy
(pose `i2Ti1.transform_from`, the x 1.5 HoHoNet -> ZInD factor :127/:149, `bevimg_Sim2_world.transform_from`, `np.round`
:187-188); the pixel arithmetic runs in salve_amd/csrc/layout.hip.  There is no CPU renderer here.
"""

from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from salve_amd import _lib, status
from salve_amd.common.bevparams import DEFAULT_METERS_PER_PX, BEVParams, get_line_width_by_resolution

HOHO_S_ZIND_SCALE_FACTOR = 1.5
RED, GREEN, BLUE, WHITE = (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)
WDO_COLOR_DICT_CV2 = {"windows": RED, "doors": GREEN, "openings": BLUE}   # bev_rendering_utils.py:28-31

# one layout image: (room vertices [K, 2] in metres, already posed; [(W/D/O type, vertices [2, 2] in metres, already posed)])
LayoutSpec = Tuple[np.ndarray, Sequence[Tuple[str, np.ndarray]]]


MAX_LAYOUTS_PER_LAUNCH = 65535   # include/salve_hip.h: salve_layout_rasterise


def world_to_pixels(bev_params: BEVParams, xy: np.ndarray) -> np.ndarray:
    """rasterize_polygon / rasterize_polyline :187-188, :214-215."""
    return np.round(bev_params.bevimg_Sim2_world.transform_from(np.asarray(xy, dtype=np.float64).reshape(-1, 2))).astype(np.int64)


class PackedLayouts:
    """Flat device tables of n layout images (include/salve_hip.h: salve_layout_t records + shared vertex / segment arrays): what
    `salve_layout_rasterise` reads.  Packed once on the host (`pack_layouts`), rasterised in any number of launches over slices of
    the record table (the records carry absolute offsets into the shared arrays)."""

    def __init__(self, rec: np.ndarray, poly: np.ndarray, seg: np.ndarray, hw: Tuple[int, int], device: torch.device) -> None:
        self.n = len(rec)
        self.hw = hw
        self.device = device
        self.rec = torch.from_numpy(rec.view(np.uint8)).to(device)
        self.poly = torch.from_numpy(np.ascontiguousarray(poly)).to(device)
        self.seg = torch.from_numpy(np.ascontiguousarray(seg)).to(device)

    def rasterise(self, lo: int, n: int, out: torch.Tensor) -> torch.Tensor:
        """Images [lo, lo + n) -> out (int32 [>= n, H, W], 0x00BBGGRR, flipped vertically like the texture maps) on the current stream."""
        assert 0 <= lo and lo + n <= self.n and out.is_contiguous() and out.numel() >= n * self.hw[0] * self.hw[1]
        lib = _lib.load()
        rec_bytes = _lib.LAYOUT_DTYPE.itemsize
        H, W = self.hw
        with torch.cuda.device(self.device):
            # salve_layout_rasterise takes at most 65535 images per call (one grid dimension)
            for a in range(lo, lo + n, MAX_LAYOUTS_PER_LAUNCH):
                m = min(MAX_LAYOUTS_PER_LAUNCH, lo + n - a)
                st = lib.salve_layout_rasterise(ctypes.c_void_p(self.rec.data_ptr() + a * rec_bytes), m, ctypes.c_void_p(self.poly.data_ptr()),
                                                ctypes.c_void_p(self.seg.data_ptr()), H, W, ctypes.c_void_p(out[a - lo:].data_ptr()), status.ptr(self.device),
                                                ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
                _lib.check(st, "salve_layout_rasterise")
        return out


def pack_layouts(specs: Sequence[LayoutSpec], device, bev_params: Optional[BEVParams] = None, render_mask: bool = True) -> PackedLayouts:
    """Host side of `rasterise_layouts`: metres -> integer pixels exactly as the reference does (x 1.5, `bevimg_Sim2_world`,
    `np.round`: bev_rendering_utils.py:127, 149, 187-188, 214-215), packed into the kernel's tables and uploaded."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.SalveHipError("layout rasterisation needs a HIP device ('cuda:N'); there is no CPU path")
    bp = bev_params or BEVParams()
    return PackedLayouts(*pack_layout_tables(specs, bp, render_mask), (bp.img_h + 1, bp.img_w + 1), device)


def pack_layout_tables(specs: Sequence[LayoutSpec], bev_params: Optional[BEVParams] = None,
                       render_mask: bool = True) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The host tables of `pack_layouts` before their upload: (salve_layout_t records [n], poly_xy int32 [*, 2], segs int32 [*, 8])."""
    bp = bev_params or BEVParams()
    width = get_line_width_by_resolution(DEFAULT_METERS_PER_PX)
    n = len(specs)
    rec = np.zeros(n, dtype=_lib.LAYOUT_DTYPE)
    polys: List[np.ndarray] = []
    segs: List[Tuple[int, ...]] = []
    n_poly = 0
    for i, (room, wdos) in enumerate(specs):
        room_px = world_to_pixels(bp, np.asarray(room, dtype=np.float64) * HOHO_S_ZIND_SCALE_FACTOR)
        rec[i]["poly_off"], rec[i]["seg_off"] = n_poly, len(segs)
        if render_mask:
            polys.append(room_px)
            n_poly += len(room_px)
            rec[i]["n_poly"] = len(room_px)
        else:
            col = WHITE[0] | (WHITE[1] << 8) | (WHITE[2] << 16)
            for k in range(len(room_px) - 1):
                segs.append((*room_px[k], *room_px[k + 1], col, int(width / 3), 0, 0))
        for wtype, verts in wdos:
            c = WDO_COLOR_DICT_CV2[wtype]
            px = world_to_pixels(bp, np.asarray(verts, dtype=np.float64) * HOHO_S_ZIND_SCALE_FACTOR)
            for k in range(len(px) - 1):
                segs.append((*px[k], *px[k + 1], c[0] | (c[1] << 8) | (c[2] << 16), width, 0, 0))
        rec[i]["n_seg"] = len(segs) - rec[i]["seg_off"]
    poly_np = np.concatenate(polys).astype(np.int32) if polys else np.zeros((1, 2), np.int32)
    seg_np = np.array(segs, dtype=np.int64).astype(np.int32).reshape(-1, 8) if segs else np.zeros((1, 8), np.int32)
    # The kernel clips geometrically (OpenCV's clipLine in 64-bit fixed point; the polygon rules in 64-bit integers): coordinates
    # are NOT clamped per axis -- that would change the slopes of edges that cross the image.  Only absurd values are refused.
    if segs and int(seg_np[:, 5].max()) >= 19:
        raise ValueError("lines of 19 pixels and more need OpenCV's end caps at 18- / 5-degree steps, which the kernel does not draw "
                         "(the reference draws 8- and 2-pixel lines: bevparams.get_line_width_by_resolution(0.02))")
    if max(int(np.abs(poly_np).max(initial=0)), int(np.abs(seg_np[:, :4]).max(initial=0))) > (1 << 24):
        raise ValueError("layout geometry more than 2^24 pixels away from the image: not a room layout")
    return rec, poly_np, seg_np


def rasterise_layouts(specs: Sequence[LayoutSpec], device, bev_params: Optional[BEVParams] = None, render_mask: bool = True) -> torch.Tensor:
    """-> int32 [n, H + 1, W + 1] device tensor holding 0x00BBGGRR, flipped vertically like the texture maps (the format
    BevRasteriser.tiles / export_u8 take).  render_mask=False (a thin contour instead of the filled room, :128-136) draws the
    room boundary as a polyline of a third of the W/D/O width."""
    packed = pack_layouts(specs, device, bev_params, render_mask)
    out = torch.empty((packed.n, *packed.hw), dtype=torch.int32, device=packed.device)
    return packed.rasterise(0, packed.n, out) if packed.n else out


def layout_pair_specs(i2Ti1, floor_pose_graph, i1: int, i2: int) -> Tuple[LayoutSpec, LayoutSpec]:
    """The two layouts of rasterize_room_layout_pair (:48-101): panorama i1's room and W/D/Os moved into i2's frame by i2Ti1
    (:82, :90), panorama i2's as they are (:96).  `floor_pose_graph.nodes[i]` must offer `room_vertices_local_2d` [K, 2] and
    `doors`, `windows`, `openings`: lists of objects with `.type` and `.vertices_local_2d` [2, 2] (salve/common/wdo.py:47-50)."""
    n1, n2 = floor_pose_graph.nodes[i1], floor_pose_graph.nodes[i2]
    close = lambda v: np.vstack([np.asarray(v, dtype=np.float64), np.asarray(v, dtype=np.float64)[0].reshape(-1, 2)])  # :76-77
    room1 = i2Ti1.transform_from(close(n1.room_vertices_local_2d))
    room2 = close(n2.room_vertices_local_2d)
    wdos1 = [(w.type, i2Ti1.transform_from(np.asarray(w.vertices_local_2d, dtype=np.float64))) for w in list(n1.doors) + list(n1.windows) + list(n1.openings)]
    wdos2 = [(w.type, np.asarray(w.vertices_local_2d, dtype=np.float64)) for w in list(n2.doors) + list(n2.windows) + list(n2.openings)]
    return (room1, wdos1), (room2, wdos2)


class FusedLayouts:
    """The layout images the fused render -> verify pipeline needs for a hypothesis table (pipeline.RenderVerifyPipeline.prepare):
    `posed[j]` = panorama i1[j]'s room and W/D/Os under hypothesis j's i2Ti1 (rasterize_room_layout_pair :82, :90), `identity[p]` =
    panorama (store index) p's own layout (:96), the same for every hypothesis that names p as its second panorama."""

    def __init__(self, posed: Sequence[LayoutSpec], identity: Sequence[LayoutSpec]) -> None:
        self.posed, self.identity = list(posed), list(identity)

    @classmethod
    def from_pose_graph(cls, table, pano_ids: Sequence[int], floor_pose_graph, scales: Optional[Sequence[float]] = None) -> "FusedLayouts":
        """table: HypothesisTable whose i1 / i2 index `pano_ids` (ingest.PanoStore order); scales: the hypotheses' Sim(2) scales
        (default 1: alignment hypotheses are SE(2), export_alignment_hypotheses.py)."""
        from salve_amd.common.sim2 import Sim2

        posed = []
        for j in range(len(table)):
            S = Sim2(table.R[j], table.t[j], 1.0 if scales is None else float(scales[j]))
            posed.append(layout_pair_specs(S, floor_pose_graph, int(pano_ids[int(table.i1[j])]), int(pano_ids[int(table.i2[j])]))[0])
        close = lambda v: np.vstack([np.asarray(v, dtype=np.float64), np.asarray(v, dtype=np.float64)[0].reshape(-1, 2)])
        identity = []
        for pid in pano_ids:
            nd = floor_pose_graph.nodes.get(int(pid)) if hasattr(floor_pose_graph.nodes, "get") else floor_pose_graph.nodes[int(pid)]
            if nd is None:    # a panorama no hypothesis names as its second one may be missing from the graph: an empty image
                identity.append((np.zeros((0, 2)), []))
                continue
            identity.append((close(nd.room_vertices_local_2d),
                             [(w.type, np.asarray(w.vertices_local_2d, dtype=np.float64)) for w in list(nd.doors) + list(nd.windows) + list(nd.openings)]))
        return cls(posed, identity)


# ---------------------------------------------------------------------------------------------------- layouts resident on the device
WDO_TYPES = ("windows", "doors", "openings")   # PanoLayouts.wdo_type codes 0, 1, 2
LAYOUTS_FILE = "layouts.npz"
_close = lambda v: np.vstack([np.asarray(v, dtype=np.float64).reshape(-1, 2), np.asarray(v, dtype=np.float64).reshape(-1, 2)[:1]])   # :76-77


def _identity_spec(node) -> LayoutSpec:
    """A pose-graph node's own layout (:96) as `layout_pair_specs` gives it: the closed room; doors, windows, openings."""
    if node is None:
        return np.zeros((0, 2)), []
    return (_close(node.room_vertices_local_2d),
            [(w.type, np.asarray(w.vertices_local_2d, dtype=np.float64)) for w in list(node.doors) + list(node.windows) + list(node.openings)])


class PanoLayouts:
    """The layouts of P panoramas as flat tables, metres in each panorama's own frame: what `salve_layout_pose` keeps resident.
    room_off int64 [P + 1] / room_xy float64 [*, 2]: the rooms, stored CLOSED (first vertex repeated, as `layout_pair_specs` closes
    them); a panorama without a room keeps zero vertices and gives an empty image.  wdo_off int64 [P + 1] / wdo_xy float64 [*, 2, 2] /
    wdo_type uint8 [*] (index into WDO_TYPES): the W/D/Os, per panorama in `layout_pair_specs`' drawing order (doors, windows,
    openings).  Malformed tables raise ValueError."""

    FIELDS = (("room_off", np.int64, 1), ("room_xy", np.float64, 2), ("wdo_off", np.int64, 1), ("wdo_xy", np.float64, 3), ("wdo_type", np.uint8, 1))

    def __init__(self, room_off, room_xy, wdo_off, wdo_xy, wdo_type) -> None:
        given = dict(room_off=room_off, room_xy=room_xy, wdo_off=wdo_off, wdo_xy=wdo_xy, wdo_type=wdo_type)
        for name, dtype, ndim in self.FIELDS:
            a = given[name]
            if not isinstance(a, np.ndarray) or a.dtype != dtype or a.ndim != ndim:
                got = f"{a.dtype} with {a.ndim} dimension(s)" if isinstance(a, np.ndarray) else type(a).__name__
                raise ValueError(f"{name} must be a {np.dtype(dtype).name} array of {ndim} dimension(s), got {got}")
            setattr(self, name, np.ascontiguousarray(a))
        if self.room_xy.shape[1:] != (2,) or self.wdo_xy.shape[1:] != (2, 2):
            raise ValueError(f"room_xy must be [*, 2] and wdo_xy [*, 2, 2], got {self.room_xy.shape} and {self.wdo_xy.shape}")
        if len(self.room_off) < 2 or len(self.room_off) != len(self.wdo_off):
            raise ValueError(f"room_off and wdo_off must both hold P + 1 >= 2 offsets, got {len(self.room_off)} and {len(self.wdo_off)}")
        for name, off, total in (("room_off", self.room_off, len(self.room_xy)), ("wdo_off", self.wdo_off, len(self.wdo_xy))):
            if int(off[0]) != 0 or int(off[-1]) != total or bool((np.diff(off) < 0).any()):
                raise ValueError(f"{name} must rise from 0 to {total} (the rows of its table) without a step back")
        if len(self.wdo_type) != len(self.wdo_xy) or (len(self.wdo_type) and int(self.wdo_type.max()) >= len(WDO_TYPES)):
            raise ValueError(f"wdo_type must hold one code 0..{len(WDO_TYPES) - 1} per row of wdo_xy")
        if not (bool(np.isfinite(self.room_xy).all()) and bool(np.isfinite(self.wdo_xy).all())):
            raise ValueError("room_xy and wdo_xy must be finite")

    @property
    def P(self) -> int:
        return len(self.room_off) - 1

    def __len__(self) -> int:
        return self.P

    @property
    def room_count(self) -> np.ndarray:
        return np.diff(self.room_off)

    @property
    def wdo_count(self) -> np.ndarray:
        return np.diff(self.wdo_off)

    @classmethod
    def from_specs(cls, specs: Sequence[LayoutSpec]) -> "PanoLayouts":
        """One panorama per spec, its room as given (closed already, as `layout_pair_specs` and FusedLayouts.identity hold them)
        and its W/D/Os in the spec's order."""
        rooms = [np.asarray(room, dtype=np.float64).reshape(-1, 2) for room, _ in specs]
        wdos = [[(WDO_TYPES.index(wtype), np.asarray(v, dtype=np.float64)) for wtype, v in w] for _, w in specs]
        for ws in wdos:
            for _, v in ws:
                if v.shape != (2, 2):
                    raise ValueError(f"a W/D/O is a segment of two vertices [2, 2], got {v.shape}")
        flat = [w for ws in wdos for w in ws]
        return cls(np.concatenate([[0], np.cumsum([len(r) for r in rooms])]).astype(np.int64),
                   np.concatenate(rooms).reshape(-1, 2) if rooms else np.zeros((0, 2)),
                   np.concatenate([[0], np.cumsum([len(ws) for ws in wdos])]).astype(np.int64),
                   np.stack([v for _, v in flat]) if flat else np.zeros((0, 2, 2)), np.asarray([c for c, _ in flat], dtype=np.uint8))

    @classmethod
    def from_pose_graph(cls, floor_pose_graph, pano_ids: Sequence[int]) -> "PanoLayouts":
        """Panorama p of the tables = node pano_ids[p] of the graph (the objects FusedLayouts.from_pose_graph takes); a panorama the
        graph does not hold has no room."""
        nodes = floor_pose_graph.nodes
        return cls.from_specs([_identity_spec(nodes.get(int(pid)) if hasattr(nodes, "get") else nodes[int(pid)]) for pid in pano_ids])

    def spec(self, p: int, i2Ti1=None) -> LayoutSpec:
        """Panorama p's layout as the host path takes it (`pack_layouts`): as it is, or moved by `i2Ti1` (a Sim2) exactly as
        `layout_pair_specs` moves panorama 1's (:82, :90)."""
        move = (lambda v: v) if i2Ti1 is None else i2Ti1.transform_from
        room = self.room_xy[self.room_off[p]:self.room_off[p + 1]]
        return (move(room) if len(room) else room,
                [(WDO_TYPES[int(self.wdo_type[k])], move(self.wdo_xy[k])) for k in range(int(self.wdo_off[p]), int(self.wdo_off[p + 1]))])

    def save(self, path) -> None:
        """A plain .npz of the five tables (layouts.npz)."""
        with open(path, "wb") as f:
            np.savez(f, **{name: getattr(self, name) for name, _, _ in self.FIELDS})

    @classmethod
    def load(cls, path) -> "PanoLayouts":
        with np.load(path, allow_pickle=False) as z:
            missing = [name for name, _, _ in cls.FIELDS if name not in z.files]
            if missing:
                raise ValueError(f"missing table(s) {missing}")
            return cls(*[z[name] for name, _, _ in cls.FIELDS])


def pose_records(layouts: PanoLayouts, pano, R=None, t=None, s=None, posed=None) -> np.ndarray:
    """salve_layout_pose_t records of n images: image k draws panorama pano[k] under (R[k], t[k], s[k]) -- or, where posed[k] is
    false, as it is (R = I, t = 0, s = 1).  The output offsets are the running sums of the panoramas' counts."""
    pano = np.asarray(pano).astype(np.int64).reshape(-1)
    n = len(pano)
    if n and (int(pano.min()) < 0 or int(pano.max()) >= layouts.P):
        raise ValueError(f"an image names panorama {int(pano.min()) if int(pano.min()) < 0 else int(pano.max())}; the layout tables hold {layouts.P}")
    rec = np.zeros(n, dtype=_lib.LAYOUT_POSE_DTYPE)
    rec["pano"] = pano
    rec["R"] = np.tile(np.eye(2, dtype=np.float32).reshape(4), (n, 1)) if R is None else np.asarray(R, dtype=np.float32).reshape(n, 4)
    rec["t"] = 0.0 if t is None else np.asarray(t, dtype=np.float32).reshape(n, 2)
    rec["s"] = 1.0 if s is None else np.asarray(s, dtype=np.float64).reshape(n)
    if posed is not None:
        own = ~np.asarray(posed).astype(bool).reshape(n)
        rec["R"][own], rec["t"][own], rec["s"][own] = np.eye(2, dtype=np.float32).reshape(4), 0.0, 1.0
    nv, ns = layouts.room_count[pano], layouts.wdo_count[pano]
    if int(nv.sum()) >= 2 ** 31 or int(ns.sum()) >= 2 ** 31:
        raise ValueError("more than 2^31 vertices or segments in one table")
    rec["poly_off"], rec["seg_off"] = np.cumsum(nv) - nv, np.cumsum(ns) - ns
    return rec


def pose_layouts_numpy(layouts: PanoLayouts, pano, R=None, t=None, s=None, posed=None,
                       bev_params: Optional[BEVParams] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """What `salve_layout_pose` computes, restated in vectorised numpy: (salve_layout_t records [n], poly_xy int32 [*, 2], segs int32
    [*, 8]) -- the three tables `pack_layouts` builds from `layout_pair_specs`-style specs, in its conventions (an all-empty table is
    one row of zeros).  The arithmetic is the device's, elementwise and un-fused, in the host chain's order: x' = x R00 + y R01, + t,
    * s (Sim2.transform_from), * 1.5, + t_bev, * (1 / meters_per_px) (bevimg_Sim2_world, rotation I), np.round, int32.  numpy's `@`
    in the host chain may fuse the first multiply-add: the integer tables are the contract."""
    bp = bev_params or BEVParams()
    rec_in = pose_records(layouts, pano, R, t, s, posed)
    n = len(rec_in)
    pn = rec_in["pano"].astype(np.int64)
    nv, ns = layouts.room_count[pn], layouts.wdo_count[pn]
    bev = bp.bevimg_Sim2_world
    bx, by, bs = float(bev.translation[0]), float(bev.translation[1]), float(bev.scale)

    def gather(off, cnt):   # (image of every output row, its row in the panorama tables)
        img = np.repeat(np.arange(n), cnt)
        return img, off[pn][img] + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))

    def pixels(xy, img):    # xy [m, ..., 2], img [m]
        e = (slice(None),) + (None,) * (xy.ndim - 2)
        Rm, tv, sv = rec_in["R"][img].astype(np.float64), rec_in["t"][img].astype(np.float64), rec_in["s"][img]
        x, y = xy[..., 0], xy[..., 1]
        px = ((((x * Rm[:, 0][e] + y * Rm[:, 1][e]) + tv[:, 0][e]) * sv[e]) * HOHO_S_ZIND_SCALE_FACTOR + bx) * bs
        py = ((((x * Rm[:, 2][e] + y * Rm[:, 3][e]) + tv[:, 1][e]) * sv[e]) * HOHO_S_ZIND_SCALE_FACTOR + by) * bs
        return np.stack([np.round(px), np.round(py)], -1).astype(np.int64)

    v_img, v_row = gather(layouts.room_off, nv)
    s_img, s_row = gather(layouts.wdo_off, ns)
    poly = pixels(layouts.room_xy[v_row], v_img)
    ends = pixels(layouts.wdo_xy[s_row], s_img).reshape(-1, 4)
    if max(int(np.abs(poly).max(initial=0)), int(np.abs(ends).max(initial=0))) > (1 << 24):
        raise ValueError("layout geometry more than 2^24 pixels away from the image: not a room layout")
    width = get_line_width_by_resolution(DEFAULT_METERS_PER_PX)
    seg = np.zeros((len(ends), 8), dtype=np.int64)
    seg[:, :4], seg[:, 4], seg[:, 5] = ends, np.int64(0xff) << (8 * layouts.wdo_type[s_row].astype(np.int64)), width
    rec = np.zeros(n, dtype=_lib.LAYOUT_DTYPE)
    rec["n_poly"], rec["poly_off"], rec["n_seg"], rec["seg_off"] = nv, rec_in["poly_off"], ns, rec_in["seg_off"]
    return (rec, poly.astype(np.int32) if n else np.zeros((1, 2), np.int32), seg.astype(np.int32) if len(seg) else np.zeros((1, 8), np.int32))


class DeviceLayouts:
    """`PanoLayouts` resident on a device, with the output tables of launches of up to `n_max` images: `pose` (salve_layout_pose)
    fills them from a record table, `rasterise` (salve_layout_rasterise) draws them.  Everything runs on the current stream; bad
    records show in the device status word (`status.check`)."""

    def __init__(self, layouts: PanoLayouts, device, n_max: int, bev_params: Optional[BEVParams] = None) -> None:
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SalveHipError("layout posing needs a HIP device ('cuda:N'); there is no CPU path")
        if not 0 < n_max <= MAX_LAYOUTS_PER_LAUNCH:
            raise ValueError(f"a launch poses 1 to {MAX_LAYOUTS_PER_LAUNCH} layout images, got n_max = {n_max}")
        bp = bev_params or BEVParams()
        self.layouts, self.n_max, self.hw = layouts, int(n_max), (bp.img_h + 1, bp.img_w + 1)
        bev = bp.bevimg_Sim2_world
        self.bev = (float(bev.translation[0]), float(bev.translation[1]), float(bev.scale))
        self.width = get_line_width_by_resolution(DEFAULT_METERS_PER_PX)
        up = lambda a, rows: torch.from_numpy(a if len(a) else np.zeros((rows,) + a.shape[1:], a.dtype)).to(self.device)   # (never a null pointer)
        self.room_xy, self.room_off = up(layouts.room_xy, 1), up(layouts.room_off, 1)
        self.wdo_xy, self.wdo_type, self.wdo_off = up(layouts.wdo_xy, 1), up(layouts.wdo_type, 8), up(layouts.wdo_off, 1)
        # capacity: any n_max panoramas fit (the host's running sums never leave it)
        self.poly_cap = max(1, self.n_max * int(layouts.room_count.max(initial=0)))
        self.seg_cap = max(1, self.n_max * int(layouts.wdo_count.max(initial=0)))
        self.rec = torch.zeros(self.n_max * _lib.LAYOUT_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        self.poly = torch.zeros((self.poly_cap, 2), dtype=torch.int32, device=self.device)
        self.seg = torch.zeros((self.seg_cap, 8), dtype=torch.int32, device=self.device)

    def pose(self, recs_dev: torch.Tensor, n: int) -> None:
        """recs_dev: the bytes of n `pose_records` rows on the device (8-byte aligned)."""
        assert 0 <= n <= self.n_max and recs_dev.numel() * recs_dev.element_size() >= n * _lib.LAYOUT_POSE_DTYPE.itemsize
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        L = self.layouts
        with torch.cuda.device(self.device):
            st = _lib.load().salve_layout_pose(p(self.room_xy), p(self.room_off), len(L.room_xy), p(self.wdo_xy), p(self.wdo_type), p(self.wdo_off),
                                               len(L.wdo_xy), L.P, p(recs_dev), n, *self.bev, self.width, p(self.rec), p(self.poly), self.poly_cap,
                                               p(self.seg), self.seg_cap, status.ptr(self.device),
                                               ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _lib.check(st, "salve_layout_pose")

    def rasterise(self, n: int, out: torch.Tensor) -> torch.Tensor:
        """The n images last posed -> out (int32 [>= n, H, W], 0x00BBGGRR, flipped vertically like the texture maps)."""
        H, W = self.hw
        assert 0 <= n <= self.n_max and out.is_contiguous() and out.dtype == torch.int32 and out.numel() >= n * H * W
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        with torch.cuda.device(self.device):
            st = _lib.load().salve_layout_rasterise(p(self.rec), n, p(self.poly), p(self.seg), H, W, p(out), status.ptr(self.device),
                                                    ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _lib.check(st, "salve_layout_rasterise")
        return out

    def draw(self, recs: np.ndarray, out: torch.Tensor) -> torch.Tensor:
        """Upload `pose_records` rows, pose and rasterise them (tests, and the identity images a training source keeps)."""
        n = len(recs)
        if n:
            self.pose(torch.from_numpy(recs.view(np.uint8)).to(self.device), n)
            self.rasterise(n, out)
        return out
