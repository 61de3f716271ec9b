"""Host side of the HIP BEV rasteriser: buffers, tables and launches (no arithmetic on the hot path).

PyTorch is used for device memory and streams only; every computation below the table set-up runs in
salve_amd/csrc/bev_render.hip through the C ABI (include/salve_hip.h).
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from salve_amd import _lib, status
from salve_amd.common.bevparams import BEVParams
from salve_amd.utils import rotation_utils
from salve_amd.utils.hohonet_pano_utils import get_sphere_factors
from salve_amd.utils.normalization_utils import get_imagenet_mean_std

HOHO_S_ZIND_SCALE_FACTOR = 1.5  # applied inside the kernel (reference bev_rendering_utils.py:448-451)
SURFACES = {"floor": 0, "ceiling": 1}
# crop_z_range per surface (reference bev_rendering_utils.py:560-566): lo < z <= hi
Z_RANGES = {"floor": (-float("inf"), -1.0), "ceiling": (0.5, float("inf"))}


def linear_resize_taps(dst: int, src: int) -> np.ndarray:
    """int32 [dst, 4] = (src0, src1, w0, w1): the two source indices and 11-bit fixed-point weights OpenCV's
    uint8 INTER_LINEAR uses for every destination index (float32 source coordinate, weights rounded half to even,
    edge clamps), as called by the reference's Resize transforms (salve/utils/transform.py:256-272)."""
    scale = float(src) / float(dst)
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    below, above = s < 0, s >= src - 1
    f[below] = 0
    s[below] = 0
    f[above] = 0
    s[above] = src - 1
    w1 = np.rint(f * np.float32(2048)).astype(np.int64)
    w0 = np.rint((np.float32(1.0) - f) * np.float32(2048)).astype(np.int64)
    return np.stack([s, np.minimum(s + 1, src - 1), w0, w1], -1).astype(np.int32)


def normalisation_lut() -> np.ndarray:
    """float32 [3, 256]: (v - mean_c) / std_c in float32, i.e. what ToTensor + Normalize produce for a uint8 value
    (salve/utils/transform.py:79-85, 177-202; constants normalization_utils.py:13-26)."""
    mean, std = get_imagenet_mean_std()
    v = np.arange(256, dtype=np.float32)
    return np.stack([(v - np.float32(m)) / np.float32(s) for m, s in zip(mean, std)]).astype(np.float32)


def pack_hypotheses(pano_idx, surface, R, t, apply_pose) -> np.ndarray:
    """Structured array of salve_bev_hyp_t rows."""
    n = len(pano_idx)
    h = np.zeros(n, dtype=_lib.HYP_DTYPE)
    h["pano_idx"] = np.asarray(pano_idx, dtype=np.int32)
    h["surface"] = np.asarray(surface, dtype=np.int32)
    h["R"] = np.asarray(R, dtype=np.float32).reshape(n, 4)
    h["t"] = np.asarray(t, dtype=np.float32).reshape(n, 2)
    h["apply_pose"] = np.asarray(apply_pose, dtype=np.int32)
    return h


@dataclass
class RenderDebug:
    img_xy: Optional[torch.Tensor] = None  # int16 [n, npts, 2]
    keys: Optional[torch.Tensor] = None  # int64 [n, H*W]
    mask: Optional[torch.Tensor] = None  # uint8 [n, H, W]
    stats: Optional[torch.Tensor] = None  # int32 [n, 8]
    in_window: Optional[torch.Tensor] = None  # int32 [n]


class BevRasteriser:
    """Owns the device-side tables and workspace of the rasteriser for one GPU."""

    def __init__(self, device: torch.device, pano_hw: Tuple[int, int] = (512, 1024), bev_params: Optional[BEVParams] = None,
                 crop_ratio: float = 80 / 512, depth_scale: float = 0.001, mask_k: int = 11,
                 resize: int = 234, crop: int = 224) -> None:
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SalveHipError("BevRasteriser needs a HIP device ('cuda:N'); there is no CPU path")
        bp = bev_params or BEVParams()
        H, W = pano_hw
        self.pano_hw = (H, W)
        self.bev_hw = (bp.img_h + 1, bp.img_w + 1)
        self.resize, self.crop = resize, crop
        cfg = _lib.BevConfig()
        cfg.pano_h, cfg.pano_w = H, W
        cfg.crop_rows = int(H * crop_ratio) if crop_ratio > 0 else 0
        cfg.bev_h, cfg.bev_w = self.bev_hw
        cfg.mask_k = mask_k
        cfg.depth_scale = np.float32(depth_scale)
        cfg.win_xmin, cfg.win_xmax = bp.xlims
        cfg.win_ymin, cfg.win_ymax = bp.ylims
        S = bp.bevimg_Sim2_world
        cfg.img_tx, cfg.img_ty = float(S.translation[0]), float(S.translation[1])
        cfg.img_scale = float(S.scale)
        Rm = rotation_utils.rotmat2d(-90)
        for i in range(4):
            cfg.rot_pre[i] = float(Rm.reshape(4)[i])
        cfg.z_lo[0], cfg.z_hi[0] = Z_RANGES["floor"]
        cfg.z_lo[1], cfg.z_hi[1] = Z_RANGES["ceiling"]
        cfg.z_min, cfg.n_slices = -2.0, 4
        self.cfg = cfg
        self.npts = (H - 2 * cfg.crop_rows) * W
        r, zdir, ct, st = get_sphere_factors(H, W)
        self.sphere = torch.from_numpy(np.concatenate([r, zdir, ct, st])).to(self.device)
        self.coef_y = torch.from_numpy(linear_resize_taps(resize, self.bev_hw[0])).to(self.device)
        self.coef_x = torch.from_numpy(linear_resize_taps(resize, self.bev_hw[1])).to(self.device)
        self.lut = torch.from_numpy(normalisation_lut()).to(self.device)
        self._ws_slots = {}   # workspaces by slot: a caller that keeps two batches in flight alternates `ws_slot`
        self.ws_slot = 0
        self.index_builds = 0   # full salve_bev_pano_index_build launches of `pano_index` so far (update_panos makes none)
        self._jpeg_ws = {}      # the JPEG methods' workspace by stream, the largest any of them needed: callers on different streams never share one
        self._jpeg_tables = {}  # quality -> uint16 [2, 64] (host)
        self._jitter_ws = {}    # train_tiles(jitter=)'s grey sums by stream

    # ------------------------------------------------------------------ helpers
    def _stream(self) -> ctypes.c_void_p:
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace(self, n: int) -> torch.Tensor:
        need = self.lib.salve_bev_workspace_bytes(ctypes.byref(self.cfg), n)
        if need == 0:
            _lib.check(-1, "salve_bev_workspace_bytes")
        ws = self._ws_slots.get(self.ws_slot)
        if ws is None or ws.numel() < need:
            if ws is not None:
                # growing a slot: launches issued earlier -- possibly on OTHER streams (the pipeline runs scatter and densify on
                # their own) -- may still read the old buffer, and the caching allocator hands its memory out again as soon as
                # the last reference goes, ordered against the CURRENT stream only.  Growth is rare (a larger batch than any
                # before): wait for the device.
                torch.cuda.synchronize(self.device)
            ws = self._ws_slots[self.ws_slot] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def pano_index(self, pano_depth: torch.Tensor) -> torch.Tensor:
        """The pose-independent panorama index of these depth maps (include/salve_hip.h: salve_bev_pano_index_build), built
        on first use on the current stream and kept with the tensor OBJECT: it lives as long as the tensor does, a slice or a
        copy builds its own.  The key includes the tensor's VERSION counter (torch bumps it on every in-place write: `copy_`,
        `[...] =`, `add_` ...), so depth maps overwritten in place get a fresh index instead of silently rendering with the stale
        one; only writes torch cannot see (a kernel given the raw pointer) need `drop_pano_index`."""
        idx = getattr(pano_depth, "_salve_pano_index", None)
        P = int(pano_depth.shape[0])
        if idx is not None and idx[1] == (pano_depth.data_ptr(), P, pano_depth._version):
            return idx[0]
        assert pano_depth.is_contiguous() and tuple(pano_depth.shape[1:]) == self.pano_hw and pano_depth.element_size() == 2
        if idx is not None:
            # REPLACING an index (the depth maps were written in place): launches issued earlier -- possibly on other streams, the pipeline runs its
            # scatter on one of its own -- may still read the old buffer, and the caching allocator hands its memory out again as soon as the last
            # reference goes, ordered against the current stream only.  Rare (as rare as overwriting depth maps): wait for the device, as the
            # workspace-growth path does.
            torch.cuda.synchronize(self.device)
        nbytes = self.lib.salve_bev_pano_index_bytes(ctypes.byref(self.cfg), P)
        if nbytes == 0:
            _lib.check(-1, "salve_bev_pano_index_bytes")
        buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.index_builds += 1
        with torch.cuda.device(self.device):
            st = self.lib.salve_bev_pano_index_build(ctypes.byref(self.cfg), ctypes.c_void_p(pano_depth.data_ptr()), P,
                                                     ctypes.c_void_p(self.sphere.data_ptr()), ctypes.c_void_p(buf.data_ptr()), nbytes, self._stream())
        _lib.check(st, "salve_bev_pano_index_build")
        pano_depth._salve_pano_index = (buf, (pano_depth.data_ptr(), P, pano_depth._version))
        return buf

    def pano_index_bytes(self, n_panos: int) -> int:
        """Bytes of the panorama index of `n_panos` panoramas."""
        nbytes = int(self.lib.salve_bev_pano_index_bytes(ctypes.byref(self.cfg), n_panos))
        if nbytes == 0:
            _lib.check(-1, "salve_bev_pano_index_bytes")
        return nbytes

    def update_panos(self, pano_rgb: torch.Tensor, pano_depth: torch.Tensor, slots_dev: torch.Tensor, rgb_rows_dev: torch.Tensor,
                     depth_rows_dev: torch.Tensor, index: Optional[torch.Tensor] = None) -> None:
        """Overwrite slots of a resident panorama pool on the current stream: rows k of `rgb_rows_dev` (uint8 [n, H, W, 3]) and
        `depth_rows_dev` (int16 bits [n, H, W]) go to slot slots_dev[k] (device int32 [n], distinct, inside the pool) of `pano_rgb` /
        `pano_depth`, and the panorama index of exactly those slots is rebuilt (include/salve_hip.h: salve_bev_pano_index_update) -- work
        that does not grow with the pool.  The index `pano_index` keeps with the depth tensor is then RE-KEYED to the tensor's new
        version: the next scatter finds it, no full rebuild (which every other in-place write still gets) and no wait for the device.
        A slot outside the pool is reported through the device status word (`check`) by the index update -- and by torch's own
        index check in `index_copy_`.
        It runs on the current stream: a caller with a stream of its own wraps the call in `torch.cuda.stream(...)`.  `index`: the pool's own index
        buffer (what `pano_index` returned for `pano_depth`), for a caller that writes slots from another thread than the one that
        scatters: neither this call nor a `scatter(..., index=)` then LOOKS the index up by the tensor's version, so a scatter issued
        between the slot writes and the re-key can never see a stale key and rebuild the whole pool's index."""
        n = int(slots_dev.shape[0])
        if slots_dev.dtype != torch.int32 or slots_dev.dim() != 1 or not slots_dev.is_contiguous():
            raise _lib.SalveHipError(f"update_panos: slots must be a contiguous int32 vector, got {slots_dev.dtype} {tuple(slots_dev.shape)}")
        if tuple(rgb_rows_dev.shape) != (n,) + tuple(pano_rgb.shape[1:]) or tuple(depth_rows_dev.shape) != (n,) + tuple(pano_depth.shape[1:]) \
                or rgb_rows_dev.dtype != pano_rgb.dtype or depth_rows_dev.dtype != pano_depth.dtype:
            raise _lib.SalveHipError(f"update_panos: {n} slots need rows of {(n,) + tuple(pano_rgb.shape[1:])} {pano_rgb.dtype} and "
                                     f"{(n,) + tuple(pano_depth.shape[1:])} {pano_depth.dtype}, got {tuple(rgb_rows_dev.shape)} {rgb_rows_dev.dtype} and "
                                     f"{tuple(depth_rows_dev.shape)} {depth_rows_dev.dtype}")
        if n == 0:
            return
        P = int(pano_depth.shape[0])
        if n > P:
            raise _lib.SalveHipError(f"update_panos: {n} slots listed, the pool has {P}")
        if index is None:
            index = self.pano_index(pano_depth)   # (the index of the depth maps as they are now: built here on first use)
        elif index.numel() != self.pano_index_bytes(P) or index.device != pano_depth.device:
            raise _lib.SalveHipError(f"update_panos: the index buffer holds {index.numel()} bytes, a pool of {P} slots needs {self.pano_index_bytes(P)}")
        at = slots_dev.to(torch.int64)
        pano_rgb.index_copy_(0, at, rgb_rows_dev)
        pano_depth.index_copy_(0, at, depth_rows_dev)
        with torch.cuda.device(self.device):
            st = self.lib.salve_bev_pano_index_update(ctypes.byref(self.cfg), ctypes.c_void_p(pano_depth.data_ptr()), P,
                                                      ctypes.c_void_p(self.sphere.data_ptr()), ctypes.c_void_p(index.data_ptr()), index.numel(),
                                                      ctypes.c_void_p(slots_dev.data_ptr()), n, status.ptr(self.device), self._stream())
        _lib.check(st, "salve_bev_pano_index_update")
        pano_depth._salve_pano_index = (index, (pano_depth.data_ptr(), P, pano_depth._version))

    @staticmethod
    def drop_pano_index(pano_depth: torch.Tensor) -> None:
        if hasattr(pano_depth, "_salve_pano_index"):
            del pano_depth._salve_pano_index

    def upload_panos(self, rgb: np.ndarray, depth: np.ndarray) -> Tuple[torch.Tensor, torch.Tensor]:
        """rgb uint8 [P,H,W,3], depth uint16 [P,H,W] (host) -> device tensors (depth carried as int16 bits)."""
        assert rgb.dtype == np.uint8 and depth.dtype == np.uint16
        assert rgb.shape[1:3] == self.pano_hw and depth.shape[1:] == self.pano_hw
        d = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(self.device)
        return torch.from_numpy(np.ascontiguousarray(rgb)).to(self.device), d

    def upload_hypotheses(self, hyps: np.ndarray) -> torch.Tensor:
        assert hyps.dtype == _lib.HYP_DTYPE
        return torch.from_numpy(np.ascontiguousarray(hyps).view(np.uint8)).to(self.device)

    # ------------------------------------------------------------------ launches
    def render(self, pano_rgb: torch.Tensor, pano_depth: torch.Tensor, hyps_dev: torch.Tensor, n: int,
               out_bev: Optional[torch.Tensor] = None, debug: bool = False) -> Tuple[torch.Tensor, RenderDebug]:
        """Render n BEV images.  Returns (int32 [n, H, W] holding 0x00BBGGRR, debug buffers)."""
        Hb, Wb = self.bev_hw
        if out_bev is None:
            out_bev = torch.empty((n, Hb, Wb), dtype=torch.int32, device=self.device)
        assert out_bev.is_contiguous() and out_bev.numel() >= n * Hb * Wb
        dbg = RenderDebug()
        if debug:
            dbg.img_xy = torch.empty((n, self.npts, 2), dtype=torch.int16, device=self.device)
            dbg.keys = torch.empty((n, Hb * Wb), dtype=torch.int64, device=self.device)
            dbg.mask = torch.empty((n, Hb, Wb), dtype=torch.uint8, device=self.device)
            dbg.stats = torch.zeros((n, 8), dtype=torch.int32, device=self.device)
            dbg.in_window = torch.zeros(n, dtype=torch.int32, device=self.device)
        ws = self._workspace(n)
        index = self.pano_index(pano_depth)
        P = int(pano_rgb.shape[0])
        ptr = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
        with torch.cuda.device(self.device):
            st = self.lib.salve_bev_render_batch(
                ctypes.byref(self.cfg), ptr(pano_rgb), ptr(pano_depth), P, ptr(self.sphere), ptr(index), ptr(hyps_dev), n,
                ptr(out_bev), ptr(dbg.img_xy), ptr(dbg.keys), ptr(dbg.mask), ptr(dbg.stats), ptr(dbg.in_window), status.ptr(self.device),
                ptr(ws), ws.numel(), self._stream(),
            )
        _lib.check(st, "salve_bev_render_batch")
        return out_bev, dbg

    def scatter(self, pano_rgb: torch.Tensor, pano_depth: torch.Tensor, hyps_dev: torch.Tensor, n: int, out_bev: torch.Tensor,
                in_window: Optional[torch.Tensor] = None, index: Optional[torch.Tensor] = None) -> None:
        """First half of `render`: the sparse images (z-order winners' colours) into `out_bev`, the occupancy bitmaps into the
        workspace.  `in_window` (int32 [n]) receives the number of points inside the window per render (0 => the reference
        writes no tile, bev_rendering_utils.py:279, 623-627).  `index`: the panorama index to use as it is (see `update_panos`);
        default: the one `pano_index` keeps with the depth tensor."""
        ws = self._workspace(n)
        if index is None:
            index = self.pano_index(pano_depth)
        with torch.cuda.device(self.device):
            st = self.lib.salve_bev_scatter(
                ctypes.byref(self.cfg), ctypes.c_void_p(pano_rgb.data_ptr()), ctypes.c_void_p(pano_depth.data_ptr()),
                int(pano_rgb.shape[0]), ctypes.c_void_p(self.sphere.data_ptr()), ctypes.c_void_p(index.data_ptr()),
                ctypes.c_void_p(hyps_dev.data_ptr()), n, ctypes.c_void_p(out_bev.data_ptr()), None, None,
                ctypes.c_void_p(0 if in_window is None else in_window.data_ptr()), status.ptr(self.device),
                ctypes.c_void_p(ws.data_ptr()), ws.numel(), self._stream())
        _lib.check(st, "salve_bev_scatter")

    def densify(self, n: int, out_bev: torch.Tensor) -> torch.Tensor:
        """Second half of `render`: completes the sparse images of `scatter` in place (same `out_bev`, same workspace slot)."""
        ws = self._workspace(n)
        with torch.cuda.device(self.device):
            st = self.lib.salve_bev_densify(ctypes.byref(self.cfg), n, ctypes.c_void_p(out_bev.data_ptr()), None, None,
                                            status.ptr(self.device), ctypes.c_void_p(ws.data_ptr()), ws.numel(), self._stream())
        _lib.check(st, "salve_bev_densify")
        return out_bev

    def densify_tiles(self, n: int, out_bev: torch.Tensor, jobs_a: torch.Tensor, jobs_b: torch.Tensor, tiles_b: torch.Tensor, out: torch.Tensor,
                      out_c: int) -> torch.Tensor:
        """`densify` + `tile_pairs(pretiled=True)` as ONE launch (include/salve_hip.h: salve_bev_densify_tiles): every render's workgroup writes
        its verifier tile as soon as the image is complete.  `jobs_a` / `jobs_b` (upload_tile_jobs, the second with pretiled=True) are indexed by
        RENDER of the launch: destination sample and channel of render r / the pair's pretiled second image and its channel."""
        ws = self._workspace(n)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        with torch.cuda.device(self.device):
            st = self.lib.salve_bev_densify_tiles(ctypes.byref(self.cfg), n, p(out_bev), p(jobs_a), p(jobs_b), p(tiles_b), p(self.coef_y), p(self.coef_x),
                                                  self.resize, self.crop, p(self.lut), p(out), out_c, status.ptr(self.device), p(ws), ws.numel(), self._stream())
        _lib.check(st, "salve_bev_densify_tiles")
        return out_bev

    def render_counted(self, pano_rgb: torch.Tensor, pano_depth: torch.Tensor, hyps_dev: torch.Tensor, n: int,
                       out_bev: torch.Tensor, counts: torch.Tensor) -> None:
        """`render` that also reports, per render, how many points fell inside the window (int32 [n])."""
        ws = self._workspace(n)
        index = self.pano_index(pano_depth)
        ptr = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
        with torch.cuda.device(self.device):
            st = self.lib.salve_bev_render_batch(
                ctypes.byref(self.cfg), ptr(pano_rgb), ptr(pano_depth), int(pano_rgb.shape[0]), ptr(self.sphere), ptr(index), ptr(hyps_dev), n,
                ptr(out_bev), None, None, None, None, ptr(counts), status.ptr(self.device), ptr(ws), ws.numel(), self._stream())
        _lib.check(st, "salve_bev_render_batch")

    def render_points(self, xyz: np.ndarray, rgb_u8: np.ndarray):
        """One BEV image from an explicit world-frame point cloud (host arrays).  Returns (int32 [1,H,W], n_in_window)."""
        xyz_d = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float64)).to(self.device)
        rgb_d = torch.from_numpy(np.ascontiguousarray(rgb_u8, dtype=np.uint8)).to(self.device)
        cnt = torch.zeros(1, dtype=torch.int32, device=self.device)
        Hb, Wb = self.bev_hw
        bev = torch.empty((1, Hb, Wb), dtype=torch.int32, device=self.device)
        ws = self._workspace(1)
        with torch.cuda.device(self.device):
            st = self.lib.salve_bev_scatter_points(ctypes.byref(self.cfg), ctypes.c_void_p(xyz_d.data_ptr()), ctypes.c_void_p(rgb_d.data_ptr()),
                                                   int(xyz_d.shape[0]), ctypes.c_void_p(bev.data_ptr()), ctypes.c_void_p(cnt.data_ptr()),
                                                   ctypes.c_void_p(ws.data_ptr()), ws.numel(), self._stream())
        _lib.check(st, "salve_bev_scatter_points")
        self.densify(1, bev)
        return bev, int(cnt.item())

    def keys_from_pixels(self, xy: torch.Tensor, rgb: torch.Tensor, out_bev: torch.Tensor) -> None:
        """Sparse image of ONE render from explicit integer pixels (int32 [n, 2]) and colours (uint8 [n, 3]) into `out_bev`
        (int32 [1, H, W]); follow with densify(1, out_bev)."""
        ws = self._workspace(1)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        with torch.cuda.device(self.device):
            st = self.lib.salve_bev_keys_from_pixels(ctypes.byref(self.cfg), p(xy), p(rgb), int(xy.shape[0]), p(out_bev), p(ws), ws.numel(), self._stream())
        _lib.check(st, "salve_bev_keys_from_pixels")

    def check(self, what: str) -> None:
        """Raise if a kernel of this device reported a failure (a star walk that did not close leaves an incomplete image).
        Synchronises: call where the host is about to read the images anyway."""
        status.check(self.device, what)

    def export_u8(self, bev: torch.Tensor) -> torch.Tensor:
        """int32 [n,H,W] -> uint8 [n,H,W,3] (the array `render_bev_image` returns)."""
        n, Hb, Wb = bev.shape
        out = torch.empty((n, Hb, Wb, 3), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            st = self.lib.salve_bev_export_u8(ctypes.c_void_p(bev.data_ptr()), n, Hb, Wb, ctypes.c_void_p(out.data_ptr()), self._stream())
        _lib.check(st, "salve_bev_export_u8")
        return out

    JPEG_IMAGES_PER_CALL = 1024   # jpeg_roundtrip, jpeg_encode, jpeg_decode: images per library call (bounds its workspace: 1.5 bytes per padded pixel; jpeg_decode's other samplings up to 3, plus the coefficients)

    def _jpeg_images(self, who: str, t: torch.Tensor, shape=None) -> None:
        """Refuse `t` unless it is a contiguous int32 [n, H, W] tensor on this device (of `shape`, if one is given)."""
        if t.dim() != 3 or t.dtype != torch.int32 or not t.is_contiguous() or t.device != self.device or (shape is not None and tuple(t.shape) != tuple(shape)):
            raise _lib.SalveHipError(f"{who} must be contiguous int32 {'[n, H, W]' if shape is None else tuple(shape)} images on {self.device}, "
                                     f"got {t.dtype} {tuple(t.shape)} on {t.device}")

    def _jpeg_qtab(self, quality: int):
        """libjpeg's tables of `quality`, uint16 [2, 64] on the host, as the argument of a library call."""
        q = int(quality)
        if q not in self._jpeg_tables:
            from salve_amd.jpeg import quality_tables

            self._jpeg_tables[q] = np.ascontiguousarray(quality_tables(q), dtype=np.uint16)
        return self._jpeg_tables[q].ctypes.data_as(ctypes.c_void_p)

    def _jpeg_calls(self, route: str, n: int, h: int, w: int, *more: int):
        """The library calls of one JPEG method on n images: yields (lo, m, workspace pointer, workspace bytes) for images lo .. lo + m - 1,
        at most JPEG_IMAGES_PER_CALL at a time, with this device current.  The three methods share ONE workspace per stream (only one of
        their calls runs on a stream at a time); it grows to the largest need seen."""
        if n == 0:
            return
        per = min(n, self.JPEG_IMAGES_PER_CALL)
        size_fn = f"salve_bev_jpeg_{route}_workspace_bytes"
        need = getattr(self.lib, size_fn)(per, h, w, *more)   # (more: what the route's size query takes behind w)
        if need == 0:
            _lib.check(-1, size_fn)
        key = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._jpeg_ws.get(key)
        if ws is None or ws.numel() < need:   # (allocated under the stream that uses it: the caching allocator orders its reuse against that stream)
            ws = self._jpeg_ws[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            for lo in range(0, n, per):
                yield lo, min(per, n - lo), ctypes.c_void_p(ws.data_ptr()), ws.numel()

    def jpeg_roundtrip(self, bev: torch.Tensor, quality: int = 75, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int32 [n, H, W] images (0x00BBGGRR: BEV renders, layout images) -> what the reference's file hop makes of them: Pillow's
        `save(quality=quality)` and decode (bev_rendering_utils.py:629-630 -> zind_data.py:306-315), bit for bit, on the current stream
        (include/salve_hip.h: salve_bev_jpeg_roundtrip).  `out`: default a new tensor; `out=bev` works in place."""
        self._jpeg_images("jpeg_roundtrip: bev", bev)
        if out is None:
            out = torch.empty_like(bev)
        else:
            self._jpeg_images("jpeg_roundtrip: out", out, bev.shape)
        n, h, w = (int(v) for v in bev.shape)
        for lo, m, ws, ws_bytes in self._jpeg_calls("roundtrip", n, h, w):
            st = self.lib.salve_bev_jpeg_roundtrip(ctypes.c_void_p(bev[lo:].data_ptr()), ctypes.c_void_p(out[lo:].data_ptr()), m, h, w,
                                                   self._jpeg_qtab(quality), ws, ws_bytes, self._stream())
            _lib.check(st, "salve_bev_jpeg_roundtrip")
        return out

    JPEG_STRIDE_FRACTION = 8   # jpeg_encode's default slot: 1 / 8 of salve_bev_jpeg_encode_max_bytes (see its docstring)

    def jpeg_encode(self, bev: torch.Tensor, quality: int = 75, stride: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """int32 [n, H, W] images (0x00BBGGRR) -> (scan uint8 [n, stride], nbytes int32 [n]), both on the device: scan[i, :nbytes[i]] is
        the entropy-coded segment of the file Pillow's `save(path, quality=quality)` writes for image i, byte for byte
        (include/salve_hip.h: salve_bev_jpeg_encode); `salve_amd.jpeg.file_bytes` puts the header and the end marker around it.
        `stride`: bytes per image slot, a multiple of 4.  The default is 1 / 8 of the proven bound for any content (2490 bytes per
        16 x 16 MCU): 318 720 bytes at 501 x 501, where at quality 75 the test table's render-like textured disc needs 66 KB, its layout
        image 14 KB and full-frame noise 154 KB (300 KB at quality 95; the synthetic scenes' renders have not been sized on their own).  An image that needs more reports it: nbytes[i] > stride holds the NEEDED length, its slot
        is incomplete, and the caller encodes that image another way (or again with a larger stride); the other images are whole.
        The bytes of a slot beyond nbytes[i] are not written (the array is not initialised).  On the current stream; batches of at
        most 1024 images per library call, one workspace per stream."""
        self._jpeg_images("jpeg_encode: bev", bev)
        n, h, w = (int(v) for v in bev.shape)
        bound = self.lib.salve_bev_jpeg_encode_max_bytes(h, w)
        if bound == 0:
            _lib.check(-1, "salve_bev_jpeg_encode_max_bytes")
        if stride is None:
            stride = (bound // self.JPEG_STRIDE_FRACTION + 3) // 4 * 4
        stride = int(stride)
        if stride <= 0 or stride % 4:
            raise _lib.SalveHipError(f"jpeg_encode: stride must be a positive multiple of 4, got {stride}")
        scan = torch.empty((n, stride), dtype=torch.uint8, device=self.device)
        nbytes = torch.empty(n, dtype=torch.int32, device=self.device)
        for lo, m, ws, ws_bytes in self._jpeg_calls("encode", n, h, w):
            st = self.lib.salve_bev_jpeg_encode(ctypes.c_void_p(bev[lo:].data_ptr()), m, h, w, self._jpeg_qtab(quality), ctypes.c_void_p(scan[lo:].data_ptr()),
                                                stride, ctypes.c_void_p(nbytes[lo:].data_ptr()), ws, ws_bytes, self._stream())
            _lib.check(st, "salve_bev_jpeg_encode")
        return scan, nbytes

    def jpeg_decode(self, scans: torch.Tensor, scan_offset, scan_bytes, h: int, w: int, qtab: np.ndarray, huffman: np.ndarray,
                    out: Optional[torch.Tensor] = None, stages: int = _lib.JPEG_STAGES_ALL, entropy: str = "image",
                    segments=None, sampling: str = "4:2:0") -> Tuple[torch.Tensor, torch.Tensor]:
        """The entropy-coded scans of n baseline 4:2:0 JPEG files of ONE size that SHARE their tables (`salve_amd.jpeg.parse_file`: equal
        `header_key`) -> (int32 [n, h, w] images holding 0x00BBGGRR, int32 [n] status), both on the device: the pixels Pillow decodes
        from those files, bit for bit (include/salve_hip.h: salve_bev_jpeg_decode; zind_data.py:306-315).
        scans: uint8 device tensor, 1-D; image i is scans[scan_offset[i] : scan_offset[i] + scan_bytes[i]] (HOST integer arrays), as it
        stands in the file (stuffed, padded, no EOI), at any alignment; at least 16 bytes of the tensor lie behind the last scan.
        qtab: uint16 [2, 64] natural order; huffman: uint8 [4, 272] -- `parse_file`'s.  status[i] != 0: image i's scan was malformed
        (jpeg.STATUS_BITS names the bits); its pixels are what had been decoded, the other images are whole.  Nothing is read back here.
        stages: _lib.JPEG_STAGES_ALL (default).  For timing, _lib.JPEG_STAGE_ENTROPY runs the Huffman stage alone (status written, images
        not) and _lib.JPEG_STAGE_INVERSE the inverse stage alone, on the coefficients the entropy stage of the SAME arguments left in
        this stream's workspace (status not written) -- so at most JPEG_IMAGES_PER_CALL images when the stages are called apart, and NO
        other JPEG method (jpeg_roundtrip, jpeg_encode, another jpeg_decode) on this stream between the two: they share the workspace.
        On the current stream; at most JPEG_IMAGES_PER_CALL images per library call, one workspace per stream.
        entropy: "image" (default) is salve_bev_jpeg_decode: one wavefront per image, no restart intervals.  "lanes" is
        salve_bev_jpeg_decode_lanes: a workgroup per SEGMENT with a lane per salve_bev_jpeg_subseq_bytes() bytes, the same pixels and
        the same zero / non-zero status (a failing image's bits and pixels may differ).  segments ("lanes" only): the restart
        intervals, rows (offset in `scans`, bytes, image, first MCU, MCUs) or a _lib.JPEG_SEGMENT_DTYPE array -- `parse_file(data,
        restart=True).segments` rebased to the buffer -- sorted by image, each image's rows tiling its MCUs in order (checked here:
        the device cannot refuse a table it has not read); default one segment per image, scan_offset / scan_bytes.
        sampling: one of jpeg.SAMPLINGS, `parse_file(..., samplings=)`'s `sampling` -- "4:2:2", "4:4:4" and "grey" go through
        salve_bev_jpeg_decode_sampled / _lanes_sampled; MCUs then count in that sampling's MCU (jpeg.MCU_SIZE), and the workspace
        grows to 2 / 3 / 1 bytes per padded pixel plus the coefficients."""
        from salve_amd.jpeg import HUFFMAN_TABLE_BYTES, SCAN_PADDING

        if sampling not in _lib.JPEG_SAMPLINGS:
            raise _lib.SalveHipError(f"jpeg_decode: sampling is one of {tuple(_lib.JPEG_SAMPLINGS)}, got {sampling!r}")

        if entropy not in ("image", "lanes"):
            raise _lib.SalveHipError(f"jpeg_decode: entropy is 'image' or 'lanes', got {entropy!r}")
        if segments is not None and entropy != "lanes":
            raise _lib.SalveHipError("jpeg_decode: a segment table needs entropy='lanes' (salve_bev_jpeg_decode takes no restart intervals)")

        if scans.dim() != 1 or scans.dtype != torch.uint8 or not scans.is_contiguous() or scans.device != self.device:
            raise _lib.SalveHipError(f"jpeg_decode takes the scans as a contiguous 1-D uint8 tensor on {self.device}, got {scans.dtype} {tuple(scans.shape)}")
        off = np.ascontiguousarray(scan_offset, dtype=np.int64).reshape(-1)
        nb = np.ascontiguousarray(scan_bytes, dtype=np.int64).reshape(-1)
        n, h, w = int(off.shape[0]), int(h), int(w)
        if nb.shape[0] != n:
            raise _lib.SalveHipError(f"jpeg_decode: {n} offsets, {nb.shape[0]} lengths")
        if n and (int(off.min()) < 0 or int(nb.min()) < 0 or int(nb.max()) >= 2 ** 31 or int((off + nb).max()) + SCAN_PADDING > scans.numel()):
            raise _lib.SalveHipError(f"jpeg_decode: every scan must lie inside the {scans.numel()} bytes given, with {SCAN_PADDING} bytes of padding behind the last")
        qtab = np.ascontiguousarray(qtab, dtype=np.uint16)
        huffman = np.ascontiguousarray(huffman, dtype=np.uint8)
        if qtab.shape != (2, 64) or huffman.shape != (4, HUFFMAN_TABLE_BYTES):
            raise _lib.SalveHipError(f"jpeg_decode takes qtab [2, 64] and huffman [4, {HUFFMAN_TABLE_BYTES}], got {qtab.shape} and {huffman.shape}")
        if out is None:
            out = torch.empty((n, h, w), dtype=torch.int32, device=self.device)
        else:
            self._jpeg_images("jpeg_decode: out", out, (n, h, w))
        image_status = torch.empty(n, dtype=torch.int32, device=self.device)
        if stages != _lib.JPEG_STAGES_ALL and n > self.JPEG_IMAGES_PER_CALL:
            raise _lib.SalveHipError(f"jpeg_decode: the stages can be called apart for at most {self.JPEG_IMAGES_PER_CALL} images (one workspace), got {n}")
        if entropy == "lanes":
            return self._jpeg_decode_lanes(scans, off, nb, segments, n, h, w, qtab, huffman, out, image_status, int(stages), sampling)
        table = torch.from_numpy(np.concatenate([off.view(np.uint8), nb.astype(np.int32).view(np.uint8)])).to(self.device)   # one upload
        route, more = ("decode", ()) if sampling == "4:2:0" else ("decode_sampled", (_lib.JPEG_SAMPLINGS[sampling],))
        entry = f"salve_bev_jpeg_{route}"
        for lo, m, ws, ws_bytes in self._jpeg_calls(route, n, h, w, *more):
            st = getattr(self.lib, entry)(ctypes.c_void_p(scans.data_ptr()), scans.numel(), ctypes.c_void_p(table.data_ptr() + 8 * lo),
                                          ctypes.c_void_p(table.data_ptr() + 8 * n + 4 * lo), m, h, w, *more, qtab.ctypes.data_as(ctypes.c_void_p),
                                          huffman.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(out[lo:].data_ptr()),
                                          ctypes.c_void_p(image_status[lo:].data_ptr()), ws, ws_bytes, int(stages), self._stream())
            _lib.check(st, entry)
        return out, image_status

    def _jpeg_decode_lanes(self, scans, off, nb, segments, n, h, w, qtab, huffman, out, image_status, stages, sampling="4:2:0"):
        """jpeg_decode(entropy="lanes") behind its argument checks: the segment table checked, rebased per library call, uploaded once."""
        from salve_amd.jpeg import SCAN_PADDING, mcu_grid

        mcus = int(np.prod(mcu_grid(h, w, sampling)))
        if segments is None:
            seg = np.zeros(n, dtype=_lib.JPEG_SEGMENT_DTYPE)
            seg["offset"], seg["bytes"], seg["image"], seg["mcu_count"] = off, nb, np.arange(n), mcus
        else:
            rows = np.asarray(segments)
            if rows.dtype != _lib.JPEG_SEGMENT_DTYPE:
                rows = np.asarray(segments, dtype=np.int64).reshape(-1, 5)
                seg = np.zeros(rows.shape[0], dtype=_lib.JPEG_SEGMENT_DTYPE)
                if rows.size and (np.abs(rows[:, 1:]).max() >= 2 ** 31):
                    raise _lib.SalveHipError("jpeg_decode: a segment's bytes, image or MCUs do not fit 32 bits")
                for k, name in enumerate(_lib.JPEG_SEGMENT_DTYPE.names):
                    seg[name] = rows[:, k]
            else:
                seg = np.ascontiguousarray(rows).reshape(-1)
        if not n <= seg.shape[0] <= _lib.JPEG_MAX_SEGMENTS:
            raise _lib.SalveHipError(f"jpeg_decode: {seg.shape[0]} segments for {n} images: every image has at least one, a call at most {_lib.JPEG_MAX_SEGMENTS}")
        if seg.shape[0]:
            image = seg["image"].astype(np.int64)
            if int(image.min()) < 0 or int(image.max()) >= n:
                raise _lib.SalveHipError(f"jpeg_decode: a segment names an image outside [0, {n})")
            first, count = seg["first_mcu"].astype(np.int64), seg["mcu_count"].astype(np.int64)
            if int(first.min()) < 0 or int(count.min()) < 1 or int((first + count).max()) > mcus:
                raise _lib.SalveHipError(f"jpeg_decode: a segment's MCU range lies outside its image's {mcus} MCUs")
            if int(seg["offset"].min()) < 0 or int(seg["bytes"].min()) < 0 or int((seg["offset"] + seg["bytes"].astype(np.int64)).max()) + SCAN_PADDING > scans.numel():
                raise _lib.SalveHipError(f"jpeg_decode: every segment must lie inside the {scans.numel()} bytes given, with {SCAN_PADDING} bytes of padding behind the last")
            starts = np.flatnonzero(np.r_[True, image[1:] != image[:-1]])            # the first row of each image's run
            expect = np.cumsum(count) - count - np.repeat((np.cumsum(count) - count)[starts], np.diff(np.r_[starts, seg.shape[0]]))
            ends = np.r_[starts[1:], seg.shape[0]] - 1
            tiled = (np.diff(image) >= 0).all() and starts.shape[0] == n and np.array_equal(first, expect) and np.array_equal((first + count)[ends], np.full(n, mcus))
            if not tiled:
                raise _lib.SalveHipError("jpeg_decode: the segments must be sorted by image, and each image's segments must tile its MCUs in order")
        bounds = np.searchsorted(seg["image"], np.arange(0, n + self.JPEG_IMAGES_PER_CALL, self.JPEG_IMAGES_PER_CALL)) if n else np.zeros(1, dtype=np.int64)
        seg = seg.copy()
        seg["image"] %= self.JPEG_IMAGES_PER_CALL          # rebased to its library call's first image
        table = torch.from_numpy(seg.view(np.uint8)).to(self.device) if seg.shape[0] else None   # one upload
        route, more = ("decode", ()) if sampling == "4:2:0" else ("decode_sampled", (_lib.JPEG_SAMPLINGS[sampling],))
        entry = "salve_bev_jpeg_decode_lanes" + ("_sampled" if more else "")
        for k, (lo, m, ws, ws_bytes) in enumerate(self._jpeg_calls(route, n, h, w, *more)):
            s0, s1 = int(bounds[k]), int(bounds[k + 1])
            st = getattr(self.lib, entry)(ctypes.c_void_p(scans.data_ptr()), scans.numel(), ctypes.c_void_p(table.data_ptr() + _lib.JPEG_SEGMENT_DTYPE.itemsize * s0),
                                          s1 - s0, m, h, w, *more, qtab.ctypes.data_as(ctypes.c_void_p), huffman.ctypes.data_as(ctypes.c_void_p),
                                          ctypes.c_void_p(out[lo:].data_ptr()), ctypes.c_void_p(image_status[lo:].data_ptr()), ws, ws_bytes, stages, self._stream())
            _lib.check(st, entry)
        return out, image_status

    def upload_tile_jobs(self, bev_index: Sequence[int], slot: Sequence[int], chan: Sequence[int], pretiled: bool = False) -> torch.Tensor:
        """Tile jobs naming image `bev_index` of a BEV array -- or, with pretiled, of an array of TILE_U8X4 images."""
        Hb, Wb = self.bev_hw
        j = np.zeros(len(slot), dtype=_lib.TILE_JOB_DTYPE)
        j["bev_offset"] = np.asarray(bev_index, dtype=np.int64) * ((self.crop * self.crop) if pretiled else (Hb * Wb))
        j["slot"] = np.asarray(slot, dtype=np.int32)
        j["chan"] = np.asarray(chan, dtype=np.int32)
        return torch.from_numpy(j.view(np.uint8)).to(self.device)

    def tiles(self, bev: torch.Tensor, jobs_dev: torch.Tensor, n_jobs: int, out: torch.Tensor, fmt: int, out_c: int) -> torch.Tensor:
        """Resize -> crop -> normalise into `out` (float32 NCHW or fp16 NHWC, see include/salve_hip.h)."""
        Hb, Wb = self.bev_hw
        with torch.cuda.device(self.device):
            st = self.lib.salve_bev_tiles(
                ctypes.c_void_p(bev.data_ptr()), Hb, Wb, ctypes.c_void_p(jobs_dev.data_ptr()), n_jobs,
                ctypes.c_void_p(self.coef_y.data_ptr()), ctypes.c_void_p(self.coef_x.data_ptr()), self.resize, self.crop,
                ctypes.c_void_p(self.lut.data_ptr()), ctypes.c_void_p(out.data_ptr()), fmt, out_c, self._stream(),
            )
        _lib.check(st, "salve_bev_tiles")
        return out

    def pretile(self, bev: torch.Tensor) -> torch.Tensor:
        """int32 [n, H, W] BEV images -> int32 [n, crop, crop] resized + cropped images (TILE_U8X4), for `tile_pairs(pretiled=True)`."""
        n = int(bev.shape[0])
        out = torch.empty((n, self.crop, self.crop), dtype=torch.int32, device=self.device)
        jobs = self.upload_tile_jobs(np.arange(n), np.arange(n), np.zeros(n, dtype=np.int64))
        return self.tiles(bev, jobs, n, out, _lib.TILE_U8X4, 3)

    def tile_pairs(self, bev_a: torch.Tensor, jobs_a: torch.Tensor, bev_b: torch.Tensor, jobs_b: torch.Tensor, n_pairs: int,
                   out: torch.Tensor, out_c: int, pretiled: bool = False) -> torch.Tensor:
        """Both tiles of every early-fusion pair in one pass (fp16 NHWC; include/salve_hip.h: salve_bev_tile_pairs).  pretiled:
        `bev_b` is `pretile`'s output and `jobs_b` was uploaded with pretiled=True."""
        Hb, Wb = self.bev_hw
        with torch.cuda.device(self.device):
            st = self.lib.salve_bev_tile_pairs(
                ctypes.c_void_p(bev_a.data_ptr()), ctypes.c_void_p(bev_b.data_ptr()), Hb, Wb, ctypes.c_void_p(jobs_a.data_ptr()),
                ctypes.c_void_p(jobs_b.data_ptr()), n_pairs, ctypes.c_void_p(self.coef_y.data_ptr()), ctypes.c_void_p(self.coef_x.data_ptr()),
                self.resize, self.crop, ctypes.c_void_p(self.lut.data_ptr()), ctypes.c_void_p(out.data_ptr()), out_c, 1 if pretiled else 0, self._stream(),
            )
        _lib.check(st, "salve_bev_tile_pairs")
        return out

    def upload_overlap_jobs(self, a_index: Sequence[int], b_index: Sequence[int]) -> torch.Tensor:
        """`pair_overlap`'s job table: job j compares image a_index[j] of its first array with image b_index[j] of its second."""
        a = np.asarray(a_index, dtype=np.int64).reshape(-1)
        b = np.asarray(b_index, dtype=np.int64).reshape(-1)
        if a.shape != b.shape:
            raise _lib.SalveHipError(f"upload_overlap_jobs: {a.shape[0]} first and {b.shape[0]} second images")
        if a.size and (min(int(a.min()), int(b.min())) < -2 ** 31 or max(int(a.max()), int(b.max())) >= 2 ** 31):
            raise _lib.SalveHipError("upload_overlap_jobs: an image index does not fit 32 bits")
        j = np.zeros(a.shape[0], dtype=_lib.OVERLAP_JOB_DTYPE)
        j["a"], j["b"] = a, b
        return torch.from_numpy(j.view(np.uint8)).to(self.device)

    def pair_overlap(self, bev_a: torch.Tensor, bev_b: torch.Tensor, jobs: torch.Tensor, n_jobs: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int32 [n_jobs, 4] = (intersection, union, occupied in a, occupied in b) of the image pairs `jobs` (upload_overlap_jobs) names:
        the pixel counts behind the reference's texture_map_iou (salve/utils/iou_utils.py:14-37; include/salve_hip.h:
        salve_bev_pair_overlap), occupied = a colour byte is non-zero.  bev_a / bev_b: contiguous int32 [n, H, W] images (0x00BBGGRR) of one
        size on this device; they may be the same tensor.  One launch on the current stream, nothing is read back; exact, and the same
        bytes on every run.  A job that names an image outside its array gets the row -1 and is reported through the device status
        word (`check`)."""
        self._jpeg_images("pair_overlap: bev_a", bev_a)
        self._jpeg_images("pair_overlap: bev_b", bev_b, (bev_b.shape[0],) + tuple(bev_a.shape[1:]) if bev_b.dim() == 3 else None)
        n_jobs = int(n_jobs)
        if jobs.dtype != torch.uint8 or jobs.dim() != 1 or not jobs.is_contiguous() or jobs.device != self.device:
            raise _lib.SalveHipError(f"pair_overlap: jobs must be upload_overlap_jobs' contiguous uint8 table on {self.device}, got {jobs.dtype} "
                                     f"{tuple(jobs.shape)} on {jobs.device}")
        if n_jobs < 0 or n_jobs * _lib.OVERLAP_JOB_DTYPE.itemsize > jobs.numel():
            raise _lib.SalveHipError(f"pair_overlap: {n_jobs} jobs asked for, the table holds {jobs.numel() // _lib.OVERLAP_JOB_DTYPE.itemsize}")
        if out is None:
            out = torch.empty((n_jobs, 4), dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or not out.is_contiguous() or out.device != self.device or out.numel() != n_jobs * 4:
            raise _lib.SalveHipError(f"pair_overlap: out must be contiguous int32 [{n_jobs}, 4] on {self.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        n_a, h, w = (int(v) for v in bev_a.shape)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        with torch.cuda.device(self.device):
            st = self.lib.salve_bev_pair_overlap(p(bev_a), n_a, p(bev_b), int(bev_b.shape[0]), h, w, p(jobs), n_jobs, p(out), status.ptr(self.device), self._stream())
        _lib.check(st, "salve_bev_pair_overlap")
        return out

    def train_tiles(self, bev_a: torch.Tensor, bev_b: torch.Tensor, jobs_a: torch.Tensor, jobs_b: torch.Tensor, per_sample: int,
                    aug: torch.Tensor, batch: int, out: torch.Tensor, jitter: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The train transform of a whole batch in one launch (include/salve_hip.h: salve_bev_train_tiles): `out` is the trainable
        model's packed input [batch, crop, crop, Cp], float32 or bfloat16, every channel written (padding channels zero).  bev_a / bev_b:
        int32 [*, H, W] images; jobs_a / jobs_b: `upload_tile_jobs` tables, sample-major [batch][per_sample]; aug: TILE_AUG_DTYPE
        bytes, one draw per sample.  Bad jobs are reported through the device status word (`check`).
        jitter: TILE_JITTER_DTYPE bytes [batch][2 * per_sample] (`train_feed.jitter_table`), one ColorJitter draw per image by channel
        group -- salve_bev_train_tiles_jitter, the photometric augmentation between Resize and Crop (two launches; its workspace is
        kept per stream)."""
        Hb, Wb = self.bev_hw
        if out.dtype not in (torch.float32, torch.bfloat16):
            raise _lib.SalveHipError(f"train_tiles writes float32 or bfloat16, got {out.dtype}")
        if not out.is_contiguous() or tuple(out.shape[:3]) != (batch, self.crop, self.crop):
            raise _lib.SalveHipError(f"train_tiles: out must be contiguous [{batch}, {self.crop}, {self.crop}, Cp], got {tuple(out.shape)}")
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        args = (p(bev_a), int(bev_a.numel() // (Hb * Wb)), p(bev_b), int(bev_b.numel() // (Hb * Wb)), Hb, Wb, p(jobs_a), p(jobs_b), per_sample,
                p(aug), batch, p(self.coef_y), p(self.coef_x), self.resize, self.crop, p(self.lut), p(out),
                _lib.TILE_F32_NHWC if out.dtype == torch.float32 else _lib.TILE_BF16_NHWC, int(out.shape[3]))
        with torch.cuda.device(self.device):
            if jitter is None:
                st, entry = self.lib.salve_bev_train_tiles(*args, status.ptr(self.device), self._stream()), "salve_bev_train_tiles"
            else:
                entry = "salve_bev_train_tiles_jitter"
                need = self.lib.salve_bev_train_tiles_jitter_workspace_bytes(batch, per_sample)
                key = torch.cuda.current_stream(self.device).cuda_stream
                ws = self._jitter_ws.get(key)
                if batch > 0 and (ws is None or ws.numel() < need):   # (allocated under the stream that uses it, as the JPEG workspace)
                    ws = self._jitter_ws[key] = torch.empty(max(need, 4), dtype=torch.uint8, device=self.device)
                st = self.lib.salve_bev_train_tiles_jitter(*args, p(jitter), None if ws is None else p(ws), 0 if ws is None else ws.numel(),
                                                           status.ptr(self.device), self._stream())
        _lib.check(st, entry)
        return out
