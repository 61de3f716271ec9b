"""The step BEFORE the hot path: panoramas and alignment hypotheses from disk to the device.

* `PanoStore` -- the panoramas of one floor, resident on the GPU in the layout the rasteriser reads
  (`u8 [P,512,1024,3]`, `u16 [P,512,1024]`): the RGB JPEG is decoded on the host (Pillow) -- or, with `decode="device"`, on the
  device by the lane-parallel JPEG decoder, the same pixels -- and resized ON THE DEVICE with
  cv2's INTER_LINEAR arithmetic (bev_rendering_utils.py:370-375; `salve_resize_rgb_u8`); the `.depth.png` is the uint16
  millimetre map HoHoNet inference wrote (infer_depth.py:55-62, read at bev_rendering_utils.py:367).
* `load_floor_hypotheses` -- the work list of one (building, floor): `{root}/{building}/{floor}/{label}/{i1}_{i2}__
  {wdo}_{k1}_{k2}_{configuration}.json` files (producer scripts/export_alignment_hypotheses.py:75-90, 234-238), each a
  Sim(2) `{"R": [4], "t": [2], "s": float}` (sim2.py:180-188), enumerated exactly as scripts/render_dataset_bev.py:80-110
  does: labels in the order gt_alignment_approx, incorrect_alignment; files sorted by path; pair_idx restarts per label.
* `score_floor` -- both together through the fused pipeline, producing the prediction files of evaluate.py.
"""

from __future__ import annotations

import ctypes
import glob
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from salve_amd import _lib
from salve_amd.common.sim2 import Sim2
from salve_amd.rasteriser import linear_resize_taps
from salve_amd.synthetic import HypothesisTable
from salve_amd.utils import image_io
from salve_amd.utils.bev_rendering_utils import bev_fname_from_img_fpath

LABEL_TYPES = ("gt_alignment_approx", "incorrect_alignment")  # scripts/render_dataset_bev.py:85 ; is_match = 1, 0


def panoid_from_fpath(fpath: str) -> int:
    """`floor_01_partial_room_04_pano_5.jpg` -> 5 (scripts/render_dataset_bev.py:27-31)."""
    return int(Path(fpath).stem.split("_")[-1])


def floor_pano_fpaths(raw_dataset_dir: str, building_id: str) -> Dict[int, str]:
    """pano id -> JPEG path for a building (scripts/render_dataset_bev.py:77-78)."""
    return {panoid_from_fpath(p): p for p in glob.glob(f"{raw_dataset_dir}/{building_id}/panos/*.jpg")}


def resize_rgb_on_device(rgb_dev: torch.Tensor, out_hw: Tuple[int, int]) -> torch.Tensor:
    """cv2.resize(..., INTER_LINEAR) of uint8 [n,H,W,3] device images (include/salve_hip.h: salve_resize_rgb_u8)."""
    n, H, W, _ = rgb_dev.shape
    h, w = out_hw
    if (H, W) == (h, w):
        return rgb_dev
    lib = _lib.load()
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=rgb_dev.device)
    cy = cx = None
    if not (H == 2 * h and W == 2 * w):
        cy = torch.from_numpy(linear_resize_taps(h, H)).to(rgb_dev.device)
        cx = torch.from_numpy(linear_resize_taps(w, W)).to(rgb_dev.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = lib.salve_resize_rgb_u8(p(rgb_dev.contiguous()), n, H, W, p(out), h, w, p(cy), p(cx),
                                 ctypes.c_void_p(torch.cuda.current_stream(rgb_dev.device).cuda_stream))
    _lib.check(st, "salve_resize_rgb_u8")
    return out


def _read_rgb3(path: str) -> np.ndarray:
    """uint8 [H, W, 3] by Pillow; a greyscale file repeated into three channels."""
    rgb = image_io.read_rgb(path)
    return np.repeat(rgb[:, :, None], 3, axis=2) if rgb.ndim == 2 else rgb


class PanoStore:
    """Panoramas of one floor on the device, addressed by pano id."""

    def __init__(self, device, pano_hw: Tuple[int, int] = (512, 1024)) -> None:
        self.device = torch.device(device)
        self.pano_hw = pano_hw
        self.index: Dict[int, int] = {}
        self.fpaths: List[str] = []
        self.rgb = self.depth = None
        self.host_decoded = 0      # load(decode="device"): the files Pillow decoded
        self._ras = None

    DECODES = ("host", "device")
    READ_THREADS = 16          # decode="device": the pool that reads and parses the files (and inflates the depth PNGs)
    PANOS_PER_CALL = 32        # decode="device": panoramas per jpeg_decode call (its workspace per pixel and panorama: 4.5 bytes for 4:2:0 --
    #                            1.5 of planes, 3 of coefficients -- 6 for 4:2:2, 9 for 4:4:4, 3 for greyscale: 600 MB for 32 4:4:4 panoramas of 2048 x 1024)

    def load(self, img_fpaths: Dict[int, str], depth_save_root: str, building_id: str, pano_ids: Sequence[int], decode: str = "host",
             samplings: Sequence[str] = ("4:2:0",)) -> "PanoStore":
        """Decode -> resize (device).  Depth maps are `{depth_save_root}/{building}/{stem}.depth.png`
        (bev_rendering_utils.py:610-611); one that is missing or of the wrong size raises, as the reference's imread /
        broadcast would.
        decode: "host" (default) decodes every JPEG with Pillow, one after the other, and uploads its pixels.  "device": a thread pool
        reads and parses the files (jpeg.parse_file(restart=True)) and inflates the depth PNGs; the panoramas that share size and
        tables go through BevRasteriser.jpeg_decode(entropy="lanes") together -- only their entropy-coded scans are uploaded -- and a
        file the device does not decode (greyscale, 4:4:4, 4:2:2, progressive ...) or reports as malformed takes Pillow into the same
        slot.  The same `rgb`, bit for bit.
        samplings (decode="device"): the members of jpeg.SAMPLINGS the device decodes; the default is 4:2:0 alone, what Pillow's
        `save()` writes.  With jpeg.DEVICE_SAMPLINGS, 4:2:2 (360-degree cameras) and greyscale files stay on the device as well -- the
        samplings measured faster there; 4:4:4 (editors) is as fast in the reader threads and joins only when named,
        as in jpeg.SAMPLINGS.  A three-component file that libjpeg reads as RGB still goes to Pillow; `host_decoded` counts the rest."""
        if decode not in self.DECODES:
            raise ValueError(f"decode must be one of {self.DECODES}, got {decode!r}")
        samplings = tuple(samplings)
        if not samplings or any(s not in _lib.JPEG_SAMPLINGS for s in samplings):
            raise ValueError(f"samplings must name members of {tuple(_lib.JPEG_SAMPLINGS)}, got {samplings!r}")
        h, w = self.pano_hw
        pids = sorted(set(int(p) for p in pano_ids))
        fps = [img_fpaths[pid] for pid in pids]
        depth_fps = [f"{depth_save_root}/{building_id}/{Path(fp).stem}.depth.png" for fp in fps]
        if decode == "device":
            rgb, depths = self._load_device(fps, depth_fps, samplings)
        else:
            rgbs, depths = [], []
            for fp, dfp in zip(fps, depth_fps):
                rgbs.append(torch.from_numpy(_read_rgb3(fp)).to(self.device)[None])
                depths.append(image_io.read_depth_png(dfp))
                self._check_depth(depths[-1])
            # panoramas of one tour share a size; resize per distinct size so that mixed inputs still work
            rgb = torch.cat([resize_rgb_on_device(t, (h, w)) for t in rgbs], 0).contiguous()
        for k, (pid, fp) in enumerate(zip(pids, fps)):
            self.index[pid] = k
            self.fpaths.append(fp)
        self.rgb = rgb
        self.depth = torch.from_numpy(np.stack(depths).view(np.int16)).to(self.device)
        return self

    def _check_depth(self, depth: np.ndarray) -> None:
        h, w = self.pano_hw
        if depth.shape != (h, w):
            raise ValueError(f"depth map must be {w}x{h}, got {depth.shape[::-1]}")

    def _load_device(self, fps: List[str], depth_fps: List[str], samplings: Tuple[str, ...] = ("4:2:0",)) -> Tuple[torch.Tensor, List[np.ndarray]]:
        """load(decode="device"): (uint8 [P, h, w, 3] on the device, the depth maps)."""
        import concurrent.futures

        from salve_amd import jpeg

        h, w = self.pano_hw

        def read(k: int):
            with open(fps[k], "rb") as f:
                data = f.read()
            try:
                parsed = jpeg.parse_file(data, restart=True, samplings=samplings)
                if max(parsed.h, parsed.w) > jpeg.DEVICE_MAX_SIDE or max(s[1] for s in parsed.segments) > jpeg.DEVICE_MAX_SEGMENT_BYTES:
                    raise jpeg.Unsupported("larger than salve_bev_jpeg_decode_lanes takes")
                return data, parsed, None
            except jpeg.Unsupported:
                return None, None, _read_rgb3(fps[k])

        with concurrent.futures.ThreadPoolExecutor(max_workers=min(self.READ_THREADS, max(1, 2 * len(fps))), thread_name_prefix="salve-panos") as pool:
            reads = [pool.submit(read, k) for k in range(len(fps))]                # both kinds of file are in the pool together
            inflates = [pool.submit(image_io.read_depth_png, p) for p in depth_fps]
            files = [f.result() for f in reads]
            out, pending = self._decode_groups(files)                              # (launched, not waited for: the device decodes while the pool inflates)
            depths = [f.result() for f in inflates]
        for d in depths:
            self._check_depth(d)
        host_route = [k for k, (_, parsed, _) in enumerate(files) if parsed is None]
        for part, st in pending:                       # (one wait, behind the last launch) a scan the device reports: Pillow's verdict counts
            host_route += [k for k, word in zip(part, st.cpu().numpy()) if word]
        for k in host_route:
            rgb = files[k][2] if files[k][2] is not None else _read_rgb3(fps[k])
            out[k] = resize_rgb_on_device(torch.from_numpy(rgb).to(self.device)[None], (h, w))[0]
        self.host_decoded = len(host_route)
        return out, depths

    def _decode_groups(self, files):
        """The parsed files of _load_device, grouped by header, through BevRasteriser.jpeg_decode and the resize -> (uint8 [P, h, w, 3] on
        the device with those slots filled, [(the slots of a call, its status tensor)]).  Nothing is waited for."""
        from salve_amd import jpeg
        from salve_amd.rasteriser import BevRasteriser

        h, w = self.pano_hw
        out = torch.empty((len(files), h, w, 3), dtype=torch.uint8, device=self.device)
        groups: Dict[bytes, List[int]] = {}
        for k, (_, parsed, _) in enumerate(files):
            if parsed is not None:
                groups.setdefault(parsed.header_key, []).append(k)
        if groups and self._ras is None:
            self._ras = BevRasteriser(self.device)
        pending = []
        for members in groups.values():
            first = files[members[0]][1]
            for lo in range(0, len(members), self.PANOS_PER_CALL):
                part = members[lo:lo + self.PANOS_PER_CALL]
                rows, off, nb, at = [], [], [], 0
                for j, k in enumerate(part):
                    parsed = files[k][1]
                    rows += [(at + o - parsed.scan_offset, n, j, m0, mc) for o, n, m0, mc in parsed.segments]
                    off.append(at)
                    nb.append(parsed.scan_bytes)
                    at += parsed.scan_bytes
                blob = np.empty(at + jpeg.SCAN_PADDING, dtype=np.uint8)
                blob[at:] = 0
                for k, o, n in zip(part, off, nb):
                    blob[o:o + n] = np.frombuffer(files[k][0], dtype=np.uint8, count=n, offset=files[k][1].scan_offset)
                img, st = self._ras.jpeg_decode(torch.from_numpy(blob).to(self.device), off, nb, first.h, first.w, first.qtab, first.huffman,
                                                entropy="lanes", segments=rows, sampling=first.sampling)
                out[torch.as_tensor(part, device=self.device)] = resize_rgb_on_device(self._ras.export_u8(img), (h, w))
                pending.append((part, st))
        return out, pending

    def __len__(self) -> int:
        return len(self.index)


@dataclass
class FloorPairs:
    """Per panorama pair (i1 < i2) of a floor what the reference's exporter computes beside the hypothesis files
    (scripts/export_alignment_hypotheses.py:177-208): filled by salve_amd.hypotheses.generate, absent from files."""

    i1: np.ndarray                 # [M] pano ids
    i2: np.ndarray
    n_kept: np.ndarray             # [M] hypotheses of the pair after pruning
    n_valid: np.ndarray            # [M] configurations the width ratio accepted (floor_n_valid_configurations sums them)
    n_rejected: np.ndarray         # [M] ... rejected (floor_n_invalid_configurations)
    visibly_adjacent: np.ndarray   # [M] bool: are_visibly_adjacent on the ground truth's W/D/Os (the pairs of gt_alignment_exact/)
    gt_R: np.ndarray               # [M,2,2] float32: i2Ti1_gt = wTi2.inverse().compose(wTi1)
    gt_t: np.ndarray               # [M,2] float32
    gt_s: np.ndarray               # [M] float64


@dataclass
class FloorHypotheses:
    """Alignment hypotheses of one floor, in the order the reference renders them."""

    building_id: str
    floor_id: str
    i1: np.ndarray          # [N] pano ids (NOT store indices)
    i2: np.ndarray
    R: np.ndarray           # [N,2,2] float32 (Sim2 stores float32, sim2.py:50-52)
    t: np.ndarray           # [N,2] float32
    s: np.ndarray           # [N] float64 (unused by the renderer, which applies R and t * 1.5 only: :447-451)
    label: np.ndarray       # [N] 1 = gt_alignment_approx, 0 = incorrect_alignment
    pair_idx: np.ndarray    # [N] index within its label directory
    pair_uuid: List[str]    # e.g. door_0_0_identity
    fpaths: List[str]
    pairs: Optional[FloorPairs] = None   # salve_amd.hypotheses.generate's: the per-pair counts, visibly_adjacent and i2Ti1_gt

    def __len__(self) -> int:
        return len(self.fpaths)

    def swap(self, img_fpaths: Dict[int, str]) -> np.ndarray:
        """bool [N]: True where the tile of pano i2 sorts BEFORE the tile of pano i1.  The reference's dataset orders the
        two tiles of a pair by file name (salve/dataset/zind_data.py:110 `pair_fpaths.sort()`); the names differ only in
        the pano stem (bev_rendering_utils.py:582-595), e.g. `..partial_room_07_pano_5` > `..partial_room_04_pano_8` and
        `pano_10` < `pano_9` -- not the order of (i1, i2).  The verifier's first image is the one whose name sorts first."""
        return np.array([Path(img_fpaths[int(a)]).stem > Path(img_fpaths[int(b)]).stem for a, b in zip(self.i1, self.i2)], dtype=bool)

    def table(self, store: PanoStore, img_fpaths: Optional[Dict[int, str]] = None) -> HypothesisTable:
        """Rows for pipeline.RenderVerifyPipeline.prepare: pano ids -> store indices, tile order from the file names."""
        ix = lambda ids: np.array([store.index[int(p)] for p in ids], dtype=np.int32)
        if img_fpaths is None:
            img_fpaths = {pid: store.fpaths[k] for pid, k in store.index.items()}
        return HypothesisTable(i1=ix(self.i1), i2=ix(self.i2), R=self.R.astype(np.float32), t=self.t.astype(np.float32),
                               theta_deg=np.degrees(np.arctan2(self.R[:, 1, 0], self.R[:, 0, 0])).astype(np.float64),
                               swap=self.swap(img_fpaths))

    def tile_paths(self, bev_save_root: str, img_fpaths: Dict[int, str], surface_type: str = "floor") -> List[Tuple[str, str]]:
        """(path of pano i1's tile, path of pano i2's tile) per hypothesis: where generate_texture_maps_for_pair writes the
        posed and the identity render (bev_rendering_utils.py:579-595, 629-630)."""
        out = []
        for j in range(len(self)):
            d = f"{bev_save_root}/{LABEL_TYPES[0] if self.label[j] else LABEL_TYPES[1]}/{self.building_id}"
            out.append(tuple(f"{d}/{bev_fname_from_img_fpath(int(self.pair_idx[j]), self.pair_uuid[j], surface_type, img_fpaths[int(p)])}"
                             for p in (self.i1[j], self.i2[j])))
        return out

    def tile_names(self, bev_save_root: str, img_fpaths: Dict[int, str], surface_type: str = "floor") -> List[Tuple[str, str]]:
        """(fp0, fp1) per hypothesis: the same two paths in the SORTED order in which the reference's dataset hands the tiles
        to the verifier and scripts/test.py writes them to the prediction files (zind_data.py:110, 306-315)."""
        return [tuple(sorted(pair)) for pair in self.tile_paths(bev_save_root, img_fpaths, surface_type)]


def load_floor_hypotheses(hypotheses_save_root: str, building_id: str, floor_id: str) -> FloorHypotheses:
    i1, i2, R, t, s, label, pair_idx, uuid, fps = [], [], [], [], [], [], [], [], []
    for label_type in LABEL_TYPES:
        pairs = sorted(glob.glob(f"{hypotheses_save_root}/{building_id}/{floor_id}/{label_type}/*.json"))
        for k, fp in enumerate(pairs):
            stem = Path(fp).stem
            a, b = stem.split("_")[:2]                      # bev_rendering_utils.py:570-571
            S = Sim2.from_json(fp)
            i1.append(int(a)); i2.append(int(b))
            R.append(np.asarray(S.rotation, dtype=np.float32)); t.append(np.asarray(S.translation, dtype=np.float32)); s.append(float(S.scale))
            label.append(1 if label_type == LABEL_TYPES[0] else 0)
            pair_idx.append(k)
            uuid.append(stem.split("__")[-1])               # :577
            fps.append(fp)
    n = len(fps)
    return FloorHypotheses(building_id, floor_id, np.array(i1, dtype=np.int64), np.array(i2, dtype=np.int64),
                           np.array(R, dtype=np.float32).reshape(n, 2, 2), np.array(t, dtype=np.float32).reshape(n, 2),
                           np.array(s, dtype=np.float64), np.array(label, dtype=np.int64), np.array(pair_idx, dtype=np.int64), uuid, fps)


def score_floor(model, device, raw_dataset_dir: str, depth_save_root: str, hypotheses_save_root: str, bev_save_root: str,
                building_id: str, floor_id: str, serialization_save_dir: str, batch_size: int = 64, chunk: Optional[int] = None,
                decode: str = "host", samplings: Sequence[str] = ("4:2:0",), visual_overlap: bool = False, jpeg_quality: Optional[int] = None,
                pose_graph: Optional[Dict[str, Any]] = None, hypotheses: Optional[FloorHypotheses] = None):
    """Disk -> predictions for one floor without writing a tile: the fused counterpart of running
    scripts/render_dataset_bev.py and then scripts/test.py on that floor.  chunk = hypotheses per launch; None: the pipeline picks the
    largest launch that fits the free HBM (pipeline.pick_launch).  decode: PanoStore.load's ("device": the panoramas' JPEG files are
    decoded on the GPU; the same prediction files), and so is samplings (which JPEG samplings stay on the device).
    visual_overlap: evaluate.run_fused_epoch's -- every prediction file also carries "overlap", the pixel counts of the pair's visual overlap
    (what `python -m salve_amd.overlap` bins accuracy by).  jpeg_quality: RenderVerifyPipeline's (75: tiles and counts are those of the
    reference's JPEG files).
    pose_graph: None, or the keyword arguments of salve_amd.pose_graph.solve (confidence_threshold is required; cycle_filter,
    rot_threshold_deg, trans_threshold) and of pose_graph.run (method, filter_by_random_spanning_trees, num_hypotheses, sampling_fraction,
    seed: the best of many random spanning trees, as a method or as an edge filter; method "pgo" with pose_graph.optimise's robust, max_iterations
    and tolerances: the tree refined by pose-graph optimisation, a PgoSolution) -- the floor's pose graph is solved right behind scoring, from the rows still in memory: the result
    gains "pose_graph" (a pose_graph.FloorSolution, or a TreeSampleSolution for method "random_spanning_trees"; None when no hypothesis was scored) and `serialization_save_dir` one more file,
    pose_graph_{building}_{floor}.json, equal to what `python -m salve_amd.pose_graph` makes of the prediction files.  None: launches, files
    and the returned dict are unchanged.  With "truth" (a salve_amd.floor_report.FloorTruth; "report": floor_report.report's num_iters,
    delete_frac, seed) the floor's reconstruction report follows: the result gains "floor_report" and the directory
    floor_report_{building}_{floor}.json.  Without "truth" nothing changes.  With "axis" (a pose_graph.AxisInputs that holds this floor: its inferred
    rooms, W/D/Os and vanishing angles; AxisInputs.from_floors([floor_input]) of the FloorInput that `hypotheses=` was generated from supplies them)
    every relative pose is first aligned by vanishing angle (pose_graph.run's axis=; methods spanning_tree and pgo).
    hypotheses: None, or the floor's FloorHypotheses as salve_amd.hypotheses.generate made them on the device: nothing is read from
    `hypotheses_save_root` then -- the floor goes from layouts to predictions (and with pose_graph= on to the report) without a hypothesis file.
    The prediction files are those of the same rows read from write_tree's directory.  None: launches, files and the returned dict are unchanged."""
    from salve_amd import evaluate
    from salve_amd.pipeline import RenderVerifyPipeline

    if hypotheses is not None and (hypotheses.building_id, hypotheses.floor_id) != (building_id, floor_id):
        raise ValueError(f"hypotheses are those of building {hypotheses.building_id}, {hypotheses.floor_id}, not of {building_id}, {floor_id}")
    hyps = hypotheses if hypotheses is not None else load_floor_hypotheses(hypotheses_save_root, building_id, floor_id)
    if len(hyps) == 0:
        return None
    img_fpaths = floor_pano_fpaths(raw_dataset_dir, building_id)
    store = PanoStore(device).load(img_fpaths, depth_save_root, building_id, np.concatenate([hyps.i1, hyps.i2]), decode=decode, samplings=samplings)
    pipe = RenderVerifyPipeline(model, device, pano_hw=store.pano_hw, chunk=chunk, n_hypotheses=len(hyps), jpeg_quality=jpeg_quality)
    pipe.set_panos(store.rgb, store.depth)
    out = evaluate.run_fused_epoch(pipe, hyps.table(store, img_fpaths), hyps.tile_names(bev_save_root, img_fpaths), hyps.label,
                                   serialization_save_dir, batch_size=batch_size, visual_overlap=visual_overlap, return_rows=pose_graph is not None)
    if pose_graph is None:
        return out
    from salve_amd import pose_graph as pg

    rows = out.pop("rows")
    options = dict(pose_graph)
    truth = options.pop("truth", None)   # a floor_report.FloorTruth: the floor's report follows its pose graph
    report_options = options.pop("report", None) or {}   # floor_report.report's num_iters, delete_frac, seed
    solved = pg.run(pg.EdgeMeasurements.from_floor(hyps, rows["kept"], rows["y_hat"], rows["prob"]), device=device, **options)
    out["pose_graph"] = solved[0] if solved else None
    if solved:
        pg.write_json(solved[0], serialization_save_dir)
    if truth is not None:
        from salve_amd import floor_report

        out["floor_report"] = floor_report.report([solved[0] if solved else None], [truth], device=device, **report_options)[0]
        floor_report.write_json(out["floor_report"], serialization_save_dir)
    return out
