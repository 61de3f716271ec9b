/*
 * salve_hip.h -- C ABI of libsalve_hip.so, the MI355X (gfx950) implementation of SALVe's hot path:
 * the per-hypothesis BEV texture-map rasteriser and the early-fusion ResNet verifier.
 *
 * The reference (zillow/salve @ 2024_10_08) is pure Python and has NO FFI for this path; the boundary it
 * exposes is a set of Python call sites.  Each entry point below names the reference interface it stands
 * behind (paths relative to the reference tree).  The Python facade in salve_amd/ binds these symbols with
 * ctypes and reproduces the reference's signatures, None-returns and exceptions.
 *
 * Conventions
 *   - Every pointer marked "device" is a raw HIP device pointer owned by the caller (PyTorch on the host
 *     side); the library never allocates per call and never frees caller memory.
 *   - All work is enqueued on the given hipStream_t (passed as void*; NULL = the null stream) and is
 *     asynchronous with respect to the host.
 *   - Return value: 0 = OK, negative = salve_status_t; salve_last_error() gives a thread-local message.
 *     No C++ exception crosses this boundary.
 *   - One host thread + one process per GPU is the supported model; handles are not thread-safe.
 */
#ifndef SALVE_HIP_H
#define SALVE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    SALVE_OK = 0,
    SALVE_ERR_BAD_ARG = -1,
    SALVE_ERR_UNSUPPORTED = -2,
    SALVE_ERR_HIP = -3,
    SALVE_ERR_WORKSPACE = -4
} salve_status_t;

#define SALVE_HIP_ABI_VERSION 7  /* 3: device status word (densify, resnet_forward), in-window counts from salve_bev_scatter;
                                     4: salve_bev_tile_pairs; 5: panorama index (salve_bev_pano_index_*), the scatter stage writes the
                                     sparse image into out_bev (no key image in memory, salve_bev_workspace_init is gone), salve_resnet_create
                                     takes its kernel selection as `flags` -- the library reads no environment variable;
                                     6: SALVE_RESNET_CHAIN_STORE_ALL / _NO_TRANSPOSED_TILES / _NO_NEXT_FUSE, out_flags bit 4 (renders densified in the
                                     given order), salve_bev_densify_tiles, a launch of >= 1025 renders keeps its dispatch order in the workspace's key image; unknown
                                     `flags` / `out_flags` bits are refused with SALVE_ERR_BAD_ARG (ABI 5 ignored them);
                                     7: the fp32 verifier handle family salve_resnet_f32_* (the fp16 engine's calls and flags unchanged);
                                        additive within 7: salve_conv_f32_* (training convolutions), salve_bev_tiles_aug, salve_bev_train_tiles and
                                        salve_bev_pano_index_update (with SALVE_STATUS_BAD_PANO_SLOT), salve_layout_pose (with SALVE_STATUS_BAD_LAYOUT),
                                        salve_adam_step, salve_head_* (the training classifier head), salve_bev_jpeg_roundtrip, salve_bev_jpeg_encode
                                        (with salve_bev_jpeg_encode_workspace_bytes / _max_bytes), salve_bev_jpeg_decode (with
                                        salve_bev_jpeg_decode_workspace_bytes and the SALVE_JPEG_* bits of its per-image status),
                                        salve_bev_jpeg_decode_lanes (with salve_bev_jpeg_decode_lanes_workspace_bytes, salve_bev_jpeg_subseq_bytes
                                        and salve_jpeg_segment_t), salve_bev_jpeg_decode_sampled / _lanes_sampled (with their two
                                        _workspace_bytes queries and SALVE_JPEG_SAMPLING_*), salve_bev_train_tiles_jitter (with
                                        salve_bev_train_tiles_jitter_workspace_bytes and salve_tile_jitter_t), salve_bev_pair_overlap (with
                                        salve_overlap_job_t), salve_pose_graph_solve (with salve_pose_graph_workspace_bytes, the salve_graph_*_t
                                        records and SALVE_STATUS_BAD_GRAPH_ROW), salve_pose_graph_sample_trees (with
                                        salve_pose_graph_sample_workspace_bytes, salve_graph_tree_out_t and salve_graph_sample_floor_out_t),
                                        salve_floor_align and salve_floor_iou (with salve_floor_iou_workspace_bytes, the salve_floor_*_out_t
                                        records and SALVE_STATUS_BAD_FLOOR_TABLE), salve_pose_graph_optimise (with
                                        salve_pose_graph_optimise_workspace_bytes, salve_graph_pgo_floor_out_t and SALVE_PGO_*),
                                        salve_pose_graph_axis_align (with salve_axis_wdo_t, salve_axis_row_out_t, salve_axis_floor_out_t, SALVE_AXIS_* and
                                        SALVE_STATUS_BAD_AXIS_ROW) */

/* Device status word: an optional device int32 the caller zeroes once and passes to the launches below.  Kernels OR bits
 * into it when something went wrong that an int return value cannot report (the launch is asynchronous); the caller
 * reads it back at a point where it synchronises anyway.  0 = every launch since the last reset was sound. */
#define SALVE_STATUS_WALK_FAILED 1 /* bev_densify: a Delaunay star did not close -- that render's image is incomplete */
#define SALVE_STATUS_FP16_RANGE 2  /* resnet_forward: an activation exceeded the fp16 range and was saturated (no released
                                      checkpoint does this; a network without normalisation can) */
#define SALVE_STATUS_BAD_HYPOTHESIS 4 /* bev scatter stage: a salve_bev_hyp_t row names a panorama outside [0, n_panos) or a surface
                                         other than 0 / 1 -- that render is an empty image */

#define SALVE_STATUS_LAYOUT_THICKNESS 8 /* layout_rasterise: a segment of thickness >= 19 pixels (OpenCV draws its end caps as 20- / 72-gons,
                                          which are not implemented) -- that segment is not drawn */
#define SALVE_STATUS_BAD_TILE_JOB 16 /* bev_train_tiles: a job names another sample, channels outside the sample, an image outside its array, or
                                        a draw carries unknown flag bits (bev_train_tiles_jitter: or a jitter record is malformed) -- that
                                        sample is not written; bev_pair_overlap: a job names an image outside its array -- its row is -1 */
#define SALVE_STATUS_BAD_PANO_SLOT 32 /* bev_pano_index_update: the slot list names a slot outside [0, n_panos) -- that entry is skipped, the
                                         other listed slots are updated */
#define SALVE_STATUS_BAD_LAYOUT 64 /* layout_pose: an image record names a panorama outside [0, n_panos), offsets outside the output capacities,
                                      or a posed coordinate lies beyond 2^24 pixels -- that image's record is written empty, the others are posed */
#define SALVE_STATUS_BAD_GRAPH_ROW 128 /* pose_graph_solve: a floor's rows are not sorted by (i1, i2), a row has i1 >= i2 or an index outside
                                          [0, n_nodes), the floor's row range is malformed or its n_nodes lies outside [0, max_nodes] -- that
                                          floor's outputs are written EMPTY (no chosen row, nothing localized, origin -1), the others are solved */
#define SALVE_STATUS_BAD_FLOOR_TABLE 256 /* floor_align: a floor's panorama extent or hypothesis extent is malformed (or overlaps a lower floor's) --
                                            that floor is written EMPTY (best -1, NaN errors); floor_iou: a floor's panorama extent or a room's
                                            vertex extent is malformed, or a posed vertex is not finite or lies beyond 2^24 pixels -- that
                                            floor's counts are 0 and its IoU NaN.  The other floors are reported */
#define SALVE_STATUS_BAD_AXIS_ROW 512 /* pose_graph_axis_align: a row names a panorama outside its floor, a W/D/O type outside 0 .. 2 or a W/D/O
                                         its panorama does not hold, a panorama's W/D/O or room extent leaves its table, or the floor's panorama
                                         extent leaves the panorama tables -- that row is copied unchanged with SALVE_AXIS_MALFORMED; or a
                                         floor's row extent is malformed -- none of its rows is written.  The other rows are aligned */

/* Library / ABI version (SALVE_HIP_ABI_VERSION). */
int salve_hip_version(void);
/* Message of the last failing call on this thread ("" if none). */
const char* salve_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * BEV rasteriser.
 * Stands behind salve/utils/bev_rendering_utils.py: get_xyzrgb_from_depth (:347-414), the pose
 * application of render_bev_pair (:443-451), render_bev_image (:254-328) and, underneath it,
 * zorder_utils.choose_elevated_repeated_vals (salve/utils/zorder_utils.py:10-83),
 * interpolation_utils.interp_dense_grid_from_sparse / remove_hallucinated_content
 * (salve/utils/interpolation_utils.py:21-54, 74-122).
 * ------------------------------------------------------------------------------------------------ */

/* The constants the reference hard-codes, gathered in one struct. */
typedef struct {
    int32_t pano_h, pano_w;     /* working pano resolution: 512 x 1024 (bev_rendering_utils.py:373-374) */
    int32_t crop_rows;          /* int(pano_h * crop_ratio) rows dropped top and bottom (:397-401); 80 */
    int32_t bev_h, bev_w;       /* BEVParams.img_h + 1, img_w + 1 (:292-293); 501, 501.  Accepted: 2 <= bev_h, bev_w < 2048 with
                                   ceil(bev_h / 16) * ceil(bev_w / 32) <= 512 (the densify stage's mask pass: one thread per 16 rows of one
                                   32-pixel column word) -- 512 x 512, 1024 x 256, 2047 x 127 and 127 x 2047 are the largest of their
                                   aspect.  Anything else: SALVE_ERR_BAD_ARG from every entry that takes the struct, 0 from its size queries.
                                   (Every accepted image fits the densify stage's LDS block -- two bits per pixel, 4 bytes per row and
                                   12.1 KB, at most 85 KB of the 160 --, so its SALVE_ERR_UNSUPPORTED for an image that does not is never met.) */
    int32_t mask_k;             /* box-filter size of remove_hallucinated_content; 11.  Accepted: odd, 1 .. 17; else SALVE_ERR_BAD_ARG */
    float depth_scale;          /* uint16 depth -> metres, applied in float32 (:367); 0.001f */
    int32_t out_flags;          /* 0 for render_bev_image; 1: no vertical flip, 2: no mask (plain interpolation), 4: the renders of a
                                   launch are densified in the order given (default: the costly ones first -- same images, shorter tail).
                                   Any other bit: SALVE_ERR_BAD_ARG.  The scatter and the densify call of the same renders must be given the
                                   SAME out_flags and n: from 1025 renders per launch the scatter stage leaves a cost per render, and the
                                   densify stage its dispatch order, in the workspace's key image (which the single-render utility paths
                                   salve_bev_scatter_points / salve_bev_keys_from_pixels overwrite) */
    double win_xmin, win_xmax, win_ymin, win_ymax; /* prune_to_2d_bbox window, inclusive (:38-45); -5, 5, -5, 5 */
    double img_tx, img_ty, img_scale; /* bevimg_Sim2_world: (p + t) * s (bevparams.py:69-78); 5, 5, 50 */
    double rot_pre[4];          /* rotmat2d(-90), row-major float64 exactly as numpy computes it (:443) */
    double z_lo[2], z_hi[2];    /* crop_z_range per surface id (lo < z <= hi) (:560-566): floor, ceiling */
    double z_min;               /* z-order slicing: slices of 1 unit on [z_min, z_min + n_slices) */
    int32_t n_slices;           /* (zorder_utils.py:11: zmin -2, zmax 2, 4 slices) */
    int32_t reserved1;
} salve_bev_config_t;

/* One render = one panorama surface under one Sim(2) pose (a row of the reference's work list,
 * scripts/render_dataset_bev.py:91-109). R, t are Sim2's float32 storage (salve/common/sim2.py:50-51). */
typedef struct {
    int32_t pano_idx;   /* which panorama of the batch */
    int32_t surface;    /* 0 = floor, 1 = ceiling */
    float R[4];         /* i2Ti1.rotation, row-major */
    float t[2];         /* i2Ti1.translation (the x1.5 HoHoNet->ZInD factor is applied by the kernel, :448-451) */
    int32_t apply_pose; /* 1: pano-1 of the pair (pose applied), 0: pano-2 (identity) */
    int32_t reserved;
} salve_bev_hyp_t;

/* Bytes of device workspace salve_bev_render_batch needs for n renders (0 on bad config).  The workspace needs no
 * initialisation and carries nothing from one call to the next, except from a scatter-stage call to its densify call. */
size_t salve_bev_workspace_bytes(const salve_bev_config_t* cfg, int32_t n);

/* Panorama index: the pose-INDEPENDENT part of the rasteriser's work, built once per set of panoramas (both surfaces are
 * built) -- the counterpart of get_xyzrgb_from_depth's z filter (bev_rendering_utils.py:408-413), which the reference also
 * evaluates once per panorama and surface, before any pose is applied (:431-446).  The panorama is cut into blocks of
 * 16 x 4 pixels; the index holds, per block, the bounding box of the block's points that pass the surface's z filter, in
 * the frame after the rotmat2d(-90) product (:443-446), 16 bytes per block and surface (180 KB per panorama at 1024 x 512).
 * The render calls use it to visit, per 128 x 128 tile of the output image, only the blocks that can reach the tile under
 * the render's pose.  It must be rebuilt when the depth maps change.
 *   pano_index  device, 16-byte aligned, salve_bev_pano_index_bytes(cfg, n_panos) bytes */
size_t salve_bev_pano_index_bytes(const salve_bev_config_t* cfg, int32_t n_panos);
int salve_bev_pano_index_build(const salve_bev_config_t* cfg, const uint16_t* pano_depth, int32_t n_panos, const double* sphere,
                               void* pano_index, size_t pano_index_bytes, void* stream);
/* Rebuild the index of a LIST of slots of a resident pool of n_panos panoramas (a training run whose panorama set does not fit the
 * device overwrites a few slots per batch).  Contract: pano_index was built or updated for these n_panos slots, and since then only the
 * depth maps of the listed slots have changed; after the call the whole buffer is byte-identical to what salve_bev_pano_index_build
 * writes for the current depth maps.  The work covers the listed slots only (their two range words, block boxes and group boxes): its
 * cost does not depend on n_panos.  Ordered on `stream`; the library allocates nothing.
 *   slots   device int32 [n_slots].  Device memory, so the kernels check every entry before forming an address: a slot outside
 *           [0, n_panos) ORs SALVE_STATUS_BAD_PANO_SLOT into the status word and is skipped.  A slot listed twice is harmless.
 *   status  device int32 status word or NULL
 * SALVE_ERR_BAD_ARG on null or misaligned pointers, n_slots <= 0 or n_slots > n_panos; SALVE_ERR_WORKSPACE on a short index buffer. */
int salve_bev_pano_index_update(const salve_bev_config_t* cfg, const uint16_t* pano_depth, int32_t n_panos, const double* sphere,
                                void* pano_index, size_t pano_index_bytes, const int32_t* slots, int32_t n_slots, int32_t* status,
                                void* stream);

/*
 * Render n BEV texture maps.
 *   pano_rgb    device uint8  [P, pano_h, pano_w, 3]
 *   pano_depth  device uint16 [P, pano_h, pano_w]          (.depth.png payload, millimetres)
 *   sphere      device double [2*pano_h + 2*pano_w]: r[v], zdir[v], cos(theta_u), sin(theta_u), computed on the
 *               host exactly as hohonet_pano_utils.get_uni_sphere_xyz does (salve/utils/hohonet_pano_utils.py:27-43)
 *   pano_index  device: salve_bev_pano_index_build's output for exactly these P panoramas
 *   hyps        device salve_bev_hyp_t [n]
 *   out_bev     device uint32 [n, bev_h, bev_w]: final BEV image (after mask and np.flipud), 0x00BBGGRR
 *   dbg_img_xy  device int16 [n, (pano_h-2*crop_rows)*pano_w, 2] or NULL: BEV pixel (x, y) of every pano point,
 *               (-1, -1) if the point is cropped / pruned (row a4: the bit-exact index contract)
 *   dbg_keys    device uint64 [n, bev_h*bev_w] or NULL: z-order winner per pixel (unflipped):
 *               0 = empty, else ((slice+1) << 45) | (point_index << 24) | 0xBBGGRR
 *   dbg_mask    device uint8 [n, bev_h, bev_w] or NULL: hallucination mask (unflipped; also under out_flags bit 2, which only
 *               keeps the stage from applying it)
 *   dbg_stats   device int32 [n, 8] or NULL: {n_sites, min x, max x, occupied rows, walk iterations, error flag,
 *               sites handed to the general walk, queued triangles}
 *   out_in_window device int32 [n] or NULL: points inside the window per render (0 => the reference returns None, :279,
 *               and generate_texture_maps_for_pair writes no tile for the pair, :623-627)
 *   status      device int32 status word or NULL (SALVE_STATUS_*)
 */
int salve_bev_render_batch(const salve_bev_config_t* cfg, const uint8_t* pano_rgb, const uint16_t* pano_depth,
                           int32_t n_panos, const double* sphere, const void* pano_index, const salve_bev_hyp_t* hyps, int32_t n,
                           uint32_t* out_bev, int16_t* dbg_img_xy, uint64_t* dbg_keys, uint8_t* dbg_mask,
                           int32_t* dbg_stats, int32_t* out_in_window, int32_t* status, void* workspace, size_t workspace_bytes,
                           void* stream);

/* The two halves of salve_bev_render_batch as separate launches (same arguments, same workspace, same out_bev):
 * salve_bev_scatter writes the SPARSE image into out_bev (the z-order winners' colours, :307-308, already flipped) and the
 * occupancy bitmaps into the workspace; salve_bev_densify completes out_bev in place (interpolation + mask).  Used by the
 * benchmark to time the stages on their own; render_batch == scatter followed by densify. */
int salve_bev_scatter(const salve_bev_config_t* cfg, const uint8_t* pano_rgb, const uint16_t* pano_depth, int32_t n_panos,
                      const double* sphere, const void* pano_index, const salve_bev_hyp_t* hyps, int32_t n, uint32_t* out_bev,
                      int16_t* dbg_img_xy, uint64_t* dbg_keys, int32_t* out_in_window, int32_t* status, void* workspace, size_t workspace_bytes,
                      void* stream);
int salve_bev_densify(const salve_bev_config_t* cfg, int32_t n, uint32_t* out_bev, uint8_t* dbg_mask,
                      int32_t* dbg_stats, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* Splat an explicit coloured point cloud -- the `xyzrgb` argument of render_bev_image (bev_rendering_utils.py:254-308):
 * xyz device double [n_points, 3] in the world frame, rgb device uint8 [n_points, 3] (the reference's float colours
 * already truncated to uint8, :307-308).  The scatter stage of ONE render: writes the sparse image into out_bev
 * (uint32 [bev_h, bev_w]) and the bitmaps of render 0 into the workspace; follow with salve_bev_densify(cfg, 1, out_bev, ...).
 * n_in_window (device int32) receives the number of points inside the window (0 => render_bev_image returns None, :279). */
int salve_bev_scatter_points(const salve_bev_config_t* cfg, const double* xyz, const uint8_t* rgb, int32_t n_points,
                             uint32_t* out_bev, int32_t* n_in_window, void* workspace, size_t workspace_bytes, void* stream);

/* Stand-alone forms of the three utilities the reference exposes next to the renderer.
 * salve_zorder_winners: zorder_utils.choose_elevated_repeated_vals (salve/utils/zorder_utils.py:10-83) -- x, y device
 *   int32 [n] pixel coordinates, z device double [n], planes device double [n_slices+1] (np.linspace(zmin, zmax, ..)),
 *   scratch device uint64 [img_h*img_w], valid device uint8 [n] (1 = the point wins its pixel).
 * salve_remove_hallucinated: interpolation_utils.remove_hallucinated_content (salve/utils/interpolation_utils.py:74-122) --
 *   sparse / interp / out device uint8 [H,W,3], scratch device uint8 [H*W].
 * salve_bev_keys_from_pixels: the input side of interpolation_utils.interp_dense_grid_from_sparse (:21-54) -- xy device
 *   int32 [n,2] (x, y) pixels, rgb device uint8 [n,3]; the scatter stage of one render (sparse image into out_bev, last index
 *   wins); follow with salve_bev_densify(cfg, 1, out_bev, ...) using cfg.out_flags = 3 (no flip, no mask) to obtain the
 *   interpolated image. */
int salve_zorder_winners(const int32_t* x, const int32_t* y, const double* z, int32_t n, const double* planes, int32_t n_slices,
                         int32_t img_w, int32_t img_h, uint64_t* scratch, uint8_t* valid, void* stream);
int salve_remove_hallucinated(const uint8_t* sparse, const uint8_t* interp, int32_t H, int32_t W, int32_t K, uint8_t* scratch,
                              uint8_t* out, void* stream);
int salve_bev_keys_from_pixels(const salve_bev_config_t* cfg, const int32_t* xy, const uint8_t* rgb, int32_t n_points, uint32_t* out_bev,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Panorama ingest: n RGB uint8 images [n, src_h, src_w, 3] -> [n, dst_h, dst_w, 3] with the arithmetic of
 * cv2.resize(img, (dst_w, dst_h), interpolation=cv2.INTER_LINEAR), the call every panorama goes through before
 * back-projection (salve/utils/bev_rendering_utils.py:370-375: 2048x1024 JPEG -> 1024x512).  An exact 2x down-scale
 * takes OpenCV's INTER_AREA fast path, (a + b + c + d + 2) >> 2, and needs no tables; any other size uses the 11-bit
 * fixed-point taps coef_y [dst_h, 4], coef_x [dst_w, 4] = {src0, src1, w0, w1} (same layout as salve_bev_tiles). */
int salve_resize_rgb_u8(const uint8_t* src, int32_t n, int32_t src_h, int32_t src_w, uint8_t* dst, int32_t dst_h, int32_t dst_w,
                        const int32_t* coef_y, const int32_t* coef_x, void* stream);

/* Rasterised-LAYOUT modality: n images of a filled room polygon (white) with thick anti-aliased W/D/O segments over it, flipped
 * vertically -- salve/utils/bev_rendering_utils.py:104-156 (rasterize_single_layout; cv2.fillPoly :159-179, cv2.line LINE_AA
 * :210-251).  The host has already applied the pose, the x 1.5 factor, bevimg_Sim2_world and np.round (:187-188, :214-215):
 *   layouts  device salve_layout_t [n]
 *   poly_xy  device int32 [*, 2]: polygon vertices (x, y) in pixels (closing vertex optional)
 *   segs     device int32 [*, 8]: x1, y1, x2, y2, colour 0x00BBGGRR, thickness in pixels, 0, 0
 *   out      device uint32 [n, img_h, img_w], 0x00BBGGRR (the layout of salve_bev_render_batch's out_bev: salve_bev_tiles and
 *            salve_bev_export_u8 take it as is)
 * The pixel rules are OpenCV 4.x's (modules/imgproc/src/drawing.cpp): fillPoly with its defaults for the polygon; for a segment
 * ThickLine with LINE_AA -- an anti-aliased convex quadrilateral (FillConvexPoly: LineAA along the edges, then spans) plus an
 * anti-aliased 12-gon end cap (EllipseEx / ellipse2Poly at 30 degrees) at either end, LineAA's filter and slope tables, every
 * anti-aliased pixel blended twice; thickness <= 1 is one LineAA.  LIMIT: thickness < 19 pixels (the reference draws 8- and
 * 2-pixel lines, bevparams.py:81-99); OpenCV gives thicker lines end caps at 18- / 5-degree steps, which are not implemented -- such
 * a segment is left out and SALVE_STATUS_LAYOUT_THICKNESS is raised in `status` (device int32 status word or NULL).  cv2 is not
 * installed here and the reference's tests pin none of it: the restatement is in oracle/layout_oracle.py ("parity unpinned"), the
 * kernel is bit-exact against it. */
typedef struct {
    int32_t n_poly, poly_off; /* vertex count and first vertex of this image's polygon in poly_xy */
    int32_t n_seg, seg_off;   /* segment count and first segment in segs */
} salve_layout_t;
int salve_layout_rasterise(const salve_layout_t* layouts, int32_t n, const int32_t* poly_xy, const int32_t* segs, int32_t img_h,
                           int32_t img_w, uint32_t* out, int32_t* status, void* stream);

/* The host chain in front of salve_layout_rasterise, on the device (additive within ABI 7): n layout images posed from panorama
 * geometry that stays resident as flat tables, ONE launch per batch.  It stands behind rasterize_room_layout_pair's
 * `i2Ti1.transform_from` of panorama 1's room and W/D/O vertices (salve/utils/bev_rendering_utils.py:82, 90; panorama 2's own
 * layout, :96, is the identity record R = I, t = 0, s = 1), the HoHoNet -> ZInD factor 1.5 (:127, :149), and
 * `bevimg_Sim2_world.transform_from` followed by np.round (:187-188, :214-215).
 *   room_xy / room_off   device double [n_room_xy, 2] in metres in each panorama's own frame, CSR offsets int64 [n_panos + 1]; rooms
 *                        are stored closed (first vertex repeated); a panorama without a room has no vertex and gives an empty image
 *   wdo_xy / wdo_type / wdo_off   device double [n_wdo, 2, 2], uint8 [n_wdo] (0 windows, 1 doors, 2 openings), CSR offsets int64
 *                        [n_panos + 1]; per panorama in drawing order (doors, windows, openings)
 *   recs                 device salve_layout_pose_t [n]: the image's panorama, its pose -- R (row-major) and t are float32 and are widened
 *                        to double, s is a double (Sim2 stores them so) -- and the first vertex / segment of its output; the host
 *                        computes the offsets (a running sum of the panoramas' counts): there is no device scan
 *   bev_tx, bev_ty, bev_scale   -xlims[0], -ylims[0], 1 / meters_per_px of the BEV window;  line_width: W/D/O thickness in pixels
 *   layouts, poly_xy, segs      OUT: exactly the tables salve_layout_rasterise reads (colour 0x00BBGGRR: windows 0x0000ff, doors
 *                        0x00ff00, openings 0xff0000); poly_cap vertices / seg_cap segments of capacity; 8-byte aligned
 * Per coordinate, in fp64, one rounding per operation and in the host's order: x' = x * R00 + y * R01 (y' = x * R10 + y * R11), + t,
 * * s, * 1.5, + bev_t, * bev_scale, round half to even, narrowed to int32.  (numpy's `@` may fuse the first multiply-add; the results
 * can then differ in the last bit of the fp64 intermediate, which changes a pixel coordinate only within an ulp of a half-pixel tie:
 * the contract is the integer tables -- DESIGN.md 4.13.)
 * The record table is device memory, so the kernel checks it before it forms an address: a record whose panorama lies outside
 * [0, n_panos), whose output would leave the capacities, whose panorama's offsets leave the tables, or a coordinate that is not
 * finite or beyond 2^24 pixels (pack_layouts' limit) ORs SALVE_STATUS_BAD_LAYOUT into `status` (device int32 or NULL) and that
 * image's record is written empty (n_poly = n_seg = 0); the other images are written.
 * SALVE_ERR_BAD_ARG on null pointers, misaligned tables, n < 0, n > 65535, n_panos <= 0, non-positive capacities, a non-finite BEV
 * parameter.  The thin-contour variant (render_mask=False) is not posed here. */
typedef struct {
    int32_t pano;               /* panorama whose layout is drawn */
    int32_t poly_off, seg_off;  /* first vertex in poly_xy / first segment in segs of this image */
    int32_t reserved;
    float R[4], t[2];           /* i2Ti1's rotation (row-major) and translation, as Sim2 stores them */
    double s;                   /* i2Ti1's scale */
} salve_layout_pose_t;
int salve_layout_pose(const double* room_xy, const int64_t* room_off, int64_t n_room_xy, const double* wdo_xy, const uint8_t* wdo_type,
                      const int64_t* wdo_off, int64_t n_wdo, int32_t n_panos, const salve_layout_pose_t* recs, int32_t n,
                      double bev_tx, double bev_ty, double bev_scale, int32_t line_width, salve_layout_t* layouts, int32_t* poly_xy,
                      int32_t poly_cap, int32_t* segs, int32_t seg_cap, int32_t* status, void* stream);

/* BEV uint32 -> uint8 [n, bev_h, bev_w, 3], the array render_bev_image returns (bev_rendering_utils.py:328). */
int salve_bev_export_u8(const uint32_t* bev, int32_t n, int32_t bev_h, int32_t bev_w, uint8_t* out, void* stream);

/*
 * Verifier input tiles: Resize (cv2 INTER_LINEAR, uint8 fixed point) -> centre Crop -> ToTensor -> Normalize,
 * i.e. salve/train_utils.py:126-159 with salve/utils/transform.py:256-272, 386-420, 105-123, 177-202.
 *   jobs        device salve_tile_job_t [n_jobs]
 *   coef_y/x    device int32 [resize, 4]: {src0, src1, w0, w1} 11-bit taps per resized row / column
 *   lut         device float [3, 256]: (v - mean_c) / std_c evaluated in float32 on the host
 *   out         SALVE_TILE_F32_NCHW : float [slots, out_c, crop, crop]
 *               SALVE_TILE_F16_NHWC:  fp16  [slots, crop, crop, out_c]
 *               SALVE_TILE_U8X4:      uint32 [slots, crop, crop]
 */
typedef struct {
    int64_t bev_offset; /* element offset of the source image inside `bev` (uint32 units) */
    int32_t slot;       /* destination sample */
    int32_t chan;       /* first of the 3 destination channels */
} salve_tile_job_t;

#define SALVE_TILE_F32_NCHW 0
#define SALVE_TILE_F16_NHWC 1
#define SALVE_TILE_U8X4 2 /* uint32 [slots, crop, crop], 0x00BBGGRR: the Resize + Crop result itself, before ToTensor / Normalize (one
                             image per slot; chan, out_c and lut's values are not used).  For images that many hypotheses share -- the
                             identity render of a pair's second panorama -- so that salve_bev_tile_pairs need not resize them again. */

int salve_bev_tiles(const uint32_t* bev, int32_t bev_h, int32_t bev_w, const salve_tile_job_t* jobs, int32_t n_jobs,
                    const int32_t* coef_y, const int32_t* coef_x, int32_t resize, int32_t crop, const float* lut,
                    void* out, int32_t out_format, int32_t out_c, void* stream);

/* The reference's TRAIN transform (salve/train_utils.py:63-124): Resize -> Crop at a given offset -> RandomHorizontalFlip ->
 * RandomVerticalFlip -> ToTensor -> Normalize, fp32 NCHW only; the draws are the caller's (one per job).  Same 11-bit taps and LUT
 * as salve_bev_tiles: with crop_y = crop_x = (resize - crop) / 2 and flags = 0 the output is bit-identical to salve_bev_tiles'
 * SALVE_TILE_F32_NCHW output.
 *   aug   device salve_tile_aug_t [n_jobs]: crop offsets inside the resized image, 0 <= crop_y, crop_x <= resize - crop (the
 *         kernel clamps them into that range: it never reads outside the taps), flags SALVE_TILE_HFLIP | SALVE_TILE_VFLIP
 *   out   float [slots, out_c, crop, crop] */
typedef struct {
    int32_t crop_y, crop_x; /* top-left corner of the crop inside the resize x resize image */
    int32_t flags;          /* SALVE_TILE_HFLIP (mirror columns) | SALVE_TILE_VFLIP (mirror rows) */
    int32_t reserved;
} salve_tile_aug_t;
#define SALVE_TILE_HFLIP 1
#define SALVE_TILE_VFLIP 2
int salve_bev_tiles_aug(const uint32_t* bev, int32_t bev_h, int32_t bev_w, const salve_tile_job_t* jobs, const salve_tile_aug_t* aug,
                        int32_t n_jobs, const int32_t* coef_y, const int32_t* coef_x, int32_t resize, int32_t crop, const float* lut,
                        float* out, int32_t out_c, void* stream);

/* The TRAIN transform of a whole batch in ONE launch, in the layout and precision the trainable model's stem convolution reads:
 * salve/train_utils.py:63-124 (Resize -> Crop(rand) -> RandomHorizontalFlip -> RandomVerticalFlip -> ToTensor -> Normalize, ONE set of
 * draws per example shared by its 2 / 4 images) followed by the channel concatenation of salve/models/early_fusion.py:52-60, for
 * images that are still in device memory as the rasteriser left them (no JPEG hop: salve/dataset/zind_data.py:306-315 reads them
 * from disk).  Same 11-bit taps and LUT as salve_bev_tiles_aug: the fp32 values are bit-identical to its output, the bf16 values are
 * those rounded once to nearest even.
 *   bev_a / bev_b   two arrays of uint32 0x00BBGGRR images, n_bev_a / n_bev_b images of bev_h x bev_w (as for salve_bev_tile_pairs:
 *                   the batch's posed renders; the identity renders, one per panorama and surface).  Both are only read, so they
 *                   may be the same array or overlap (a batch that renders its identity images behind its posed ones)
 *   jobs_a / jobs_b device salve_tile_job_t [batch][per_sample], sample-major: the per_sample (1..3: one per surface) images of
 *                   sample s from bev_a / bev_b.  .bev_offset = element offset of the image inside its array, .slot = s,
 *                   .chan = first of its 3 channels, a multiple of 3 with chan + 3 <= out_c
 *   aug             device salve_tile_aug_t [batch]: ONE draw per sample; offsets are clamped into [0, resize - crop] as by
 *                   salve_bev_tiles_aug
 *   out             SALVE_TILE_F32_NHWC: float [batch, crop, crop, out_c]; SALVE_TILE_BF16_NHWC: bf16 bit patterns (uint16_t) of the same
 *                   shape; 16-byte aligned.  out_c: a multiple of 8 >= 6 * per_sample (8, 16 or 24).  EVERY channel is written:
 *                   channels no job names (the padding behind the last image) are zero, so `out` needs no memset.
 *   status          device int32 status word or NULL.  The job tables and draws are device memory, so the kernel checks them before
 *                   it forms an address: a job with .slot != s, channels outside [0, out_c), an image outside its array, or a draw
 *                   with unknown flag bits raises SALVE_STATUS_BAD_TILE_JOB and leaves sample s unwritten.
 * SALVE_ERR_BAD_ARG on null pointers, crop <= 0, resize < crop, per_sample outside 1..3, an out_c that is not such a multiple of 8,
 * an unknown format, a misaligned `out`, batch > 65535. */
#define SALVE_TILE_F32_NHWC 3
#define SALVE_TILE_BF16_NHWC 4
int salve_bev_train_tiles(const uint32_t* bev_a, int32_t n_bev_a, const uint32_t* bev_b, int32_t n_bev_b, int32_t bev_h, int32_t bev_w,
                          const salve_tile_job_t* jobs_a, const salve_tile_job_t* jobs_b, int32_t per_sample, const salve_tile_aug_t* aug,
                          int32_t batch, const int32_t* coef_y, const int32_t* coef_x, int32_t resize, int32_t crop, const float* lut,
                          void* out, int32_t out_format, int32_t out_c, int32_t* status, void* stream);

/* salve_bev_train_tiles with the reference's photometric augmentation between Resize and Crop: torchvision's tensor
 * ColorJitter(brightness=0.5, contrast=0.5, saturation=0.5, hue=0.05) on the uint8 resized image (salve/utils/transform.py:619-686; the
 * functional_tensor.py form of torchvision 0.11 / 0.12), every image of a sample with its OWN record.  The arithmetic is DESIGN.md 4.23's,
 * float32 with one rounding per operation; trunc8(v) = v clamped to [0, 255], truncated to a byte:
 *   grey        trunc8((0.2989f r + 0.587f g) + 0.114f b)
 *   brightness  trunc8(b x + b_c 0);  saturation  trunc8(s x + s_c grey(pixel));  contrast  trunc8(c x + c_c m) with
 *               m = (float)S / (float)(resize * resize), S the integer sum of grey over the WHOLE resized image as the operations in front
 *               of contrast in this image's order left it (not the crop), one correctly rounded division
 *   hue         x / 255 -> _rgb2hsv -> h = remainder(h + hue, 1) -> _hsv2rgb -> (byte)(c * 255): not the identity at hue = 0
 * The record's operations run in `order`, the ones whose mask bit is clear skipped.  With every factor 1 and hue disabled the output is
 * salve_bev_train_tiles', bit for bit.  Two launches on `stream` behind a memset of the workspace: the grey sums by integer atomic adds
 * (order-independent: the same input gives the same bytes on every run), then salve_bev_train_tiles' kernel with the chain in front of
 * the table lookup.
 *   jitter      device salve_tile_jitter_t [batch][2 * per_sample]: record [s][g] belongs to the image whose job names channels 3 g ..
 *               3 g + 2 of sample s (x1 .. x6 of the early-fusion concatenation).  Here every job's .chan + 3 <= 6 * per_sample.
 *   workspace   device memory, 4-byte aligned, at least salve_bev_train_tiles_jitter_workspace_bytes(batch, per_sample) bytes (0 for a
 *               batch or per_sample the entry refuses); only this call's launches use it
 *   status      as salve_bev_train_tiles, and: a record whose order is no permutation of 0..3, with mask bits above 15 or with a
 *               non-finite factor or complement raises SALVE_STATUS_BAD_TILE_JOB and leaves sample s unwritten.
 * Refusals: salve_bev_train_tiles', and SALVE_ERR_UNSUPPORTED for resize * resize * 255 >= 2^24 (resize > 256: the grey sum would no
 * longer be an exact float32), SALVE_ERR_BAD_ARG for a null table or workspace, SALVE_ERR_WORKSPACE for a short workspace. */
#define SALVE_JITTER_BRIGHTNESS 0 /* operation codes of salve_tile_jitter_t.order (torchvision's fn_id) and bit numbers of .mask */
#define SALVE_JITTER_CONTRAST 1
#define SALVE_JITTER_SATURATION 2
#define SALVE_JITTER_HUE 3
typedef struct {
    uint8_t order[4];   /* a permutation of the four operation codes, first applied first */
    int32_t mask;       /* bit (1 << code) set: the operation is applied */
    float brightness, contrast, saturation; /* blend factors f */
    float hue;                              /* added to h, in turns */
    float brightness_c, contrast_c, saturation_c; /* (float)(1.0 - (double)f), formed on the host */
    int32_t reserved;
} salve_tile_jitter_t;
size_t salve_bev_train_tiles_jitter_workspace_bytes(int32_t batch, int32_t per_sample);
int salve_bev_train_tiles_jitter(const uint32_t* bev_a, int32_t n_bev_a, const uint32_t* bev_b, int32_t n_bev_b, int32_t bev_h, int32_t bev_w,
                                 const salve_tile_job_t* jobs_a, const salve_tile_job_t* jobs_b, int32_t per_sample, const salve_tile_aug_t* aug,
                                 int32_t batch, const int32_t* coef_y, const int32_t* coef_x, int32_t resize, int32_t crop, const float* lut,
                                 void* out, int32_t out_format, int32_t out_c, const salve_tile_jitter_t* jitter, void* workspace,
                                 size_t workspace_bytes, int32_t* status, void* stream);

/* The visual overlap of image pairs: stands behind salve/utils/iou_utils.py:14-37 (texture_map_iou -> binary_mask_iou), which
 * scripts/measure_acc_vs_overlap.py:77-80 calls on the two tile files of every scored pair.  The images are still in device memory as
 * uint32 0x00BBGGRR, so the reference's occupancy test np.amax(f, axis=2) > 0 is (pixel & 0x00FFFFFF) != 0 -- a stray top byte does not
 * make a pixel occupied -- and the counts are exact integers; IoU = intersection / (union + 1e-12) is left to the caller.
 *   bev_a / bev_b   two arrays of n_bev_a / n_bev_b images of bev_h x bev_w, 4-byte aligned; only read, so they may be the same array
 *   jobs            device salve_overlap_job_t [n_jobs]: job j compares image .a of bev_a with image .b of bev_b
 *   out             device int32 [n_jobs, 4], 16-byte aligned: row j = {intersection, union, occupied_a, occupied_b}, written by ONE
 *                   16-byte store.  No atomics, no zeroing needed, one summation order: the same bytes on every run.
 *   status          device int32 status word or NULL.  The job table is device memory, so the kernel checks it before it forms an
 *                   address: a job whose .a or .b lies outside [0, n_bev_*) reads nothing, writes {-1, -1, -1, -1} and raises
 *                   SALVE_STATUS_BAD_TILE_JOB.
 * One launch on `stream`, one workgroup per job; n_jobs == 0 launches nothing.  SALVE_ERR_BAD_ARG for bev_h or bev_w < 1,
 * bev_h * bev_w >= 2^31, a negative count, and -- with n_jobs > 0 -- a null pointer or a misaligned one. */
typedef struct {
    int32_t a, b; /* image index into bev_a / bev_b */
} salve_overlap_job_t;
int salve_bev_pair_overlap(const uint32_t* bev_a, int32_t n_bev_a, const uint32_t* bev_b, int32_t n_bev_b, int32_t bev_h, int32_t bev_w,
                           const salve_overlap_job_t* jobs, int32_t n_jobs, int32_t* out, int32_t* status, void* stream);

/* The floor pose graph: scored alignment hypotheses -> one global Sim(2) pose per panorama, for any number of floors in ONE launch.  Stands
 * behind the `spanning_tree` method of the reference's scripts/run_sfm.py:112-152 and :440-446 (with and without the cycle filter):
 *   salve/common/edge_classification.py:213-251  get_conf_thresholded_edge_measurements   (phase A: candidate rows)
 *   salve/common/edge_classification.py:254-311  get_most_likely_relative_pose_per_edge   (phase A: the best row of a pair)
 *   salve/algorithms/cycle_consistency.py:26-91   extract_triplets, create_adjacency_list   (phase B: adjacency bitmasks)
 *   salve/algorithms/cycle_consistency.py:172-222 compute_SE2_cycle_error                   (phase B: the error of one 3-cycle)
 *   salve/algorithms/cycle_consistency.py:225-303 filter_to_SE2_cycle_consistent_edges      (phase B: consistent edges)
 *   salve/algorithms/spanning_tree.py:73-141      greedily_construct_st_Sim2                (phases C, D: component, tree, poses)
 * A, best row per pair: a row is a candidate iff y_hat == 1 && prob >= confidence_threshold (a NaN prob never is); a pair's chosen row is
 *    its candidate of largest prob, among equal probs the FIRST in row order (np.argmax; the reference's order among equals is its glob order).
 * B, 3-cycles: for every cycle a < b < c of chosen edges, i0Si0 = (inverse(S_ac).compose(S_bc)).compose(S_ab) under the rules of the
 *    reference's Sim2 (R, t float32, products and sums unfused; (float)(1.0 / s) and (float)s enter the float32 products; scales float64);
 *    rot_err = |atan2f(R10, R00)| * (float)(180 / pi), trans_err = sqrtf(tx * tx + ty * ty); the cycle is consistent iff rot_err <
 *    rot_threshold_deg && trans_err < trans_threshold (NaN never is; trans_threshold = +inf is the rotation-only filter).  An edge is
 *    consistent iff it lies in a consistent cycle.
 * C, component: the graph is the consistent edges (cycle_filter = 1) or the chosen edges (0).  The largest connected component wins, among
 *    equally large ones the one that holds the lowest node (the reference's tie is networkx's iteration order); its lowest node is the origin.
 * D, tree: level-synchronous BFS from the origin; a node's parent is its LOWEST-index neighbour in the previous level; wS_v =
 *    wS_parent.compose(parentS_v), parentS_v = inverse(S_(p, v)) for p < v and S_(v, p) otherwise; the origin is (I, 0, 1).  That is the
 *    reference's left fold along a shortest path, bit for bit where the shortest path is unique; among several the reference takes whichever
 *    networkx's bidirectional search returns.
 *   rows            device salve_graph_row_t [floor_start[n_floors]], 8-byte aligned: one scored hypothesis each.  The rows of floor f are
 *                   floor_start[f] .. floor_start[f + 1] - 1, sorted by (i1, i2), with 0 <= i1 < i2 < n_nodes[f] (compact node indices).
 *   n_rows          the length of `rows`: a floor_start entry outside [0, n_rows] or a decreasing one is a malformed floor
 *   floor_start     device int32 [n_floors + 1];  n_nodes: device int32 [n_floors]
 *   max_nodes       the caller's bound on n_nodes[]: sizes the workgroup's LDS and the stride of out_nodes.  1 .. 256 (SALVE_GRAPH_MAX_NODES);
 *                   more is SALVE_ERR_BAD_ARG before anything is launched.  A floor with n_nodes[f] > max_nodes is a malformed floor.
 *   out_rows        device salve_graph_row_out_t [n_rows], 8-byte aligned: row r's flags and, for a chosen row, its edge's statistics over the
 *                   3-cycles through it (a row that is not chosen, or an edge in no cycle: 0, 0, +inf, +inf)
 *   out_nodes       device salve_graph_node_out_t [n_floors * max_nodes], 8-byte aligned: node v of floor f is record f * max_nodes + v; the
 *                   records v >= n_nodes[f] are NOT written.  A node that is not localized: 0, -1, -1, zeros.
 *   out_floors      device salve_graph_floor_out_t [n_floors]
 *   status          device int32 status word or NULL.  The tables are device memory, so the kernel verifies them before it forms an address
 *                   from them: a malformed floor is written EMPTY and raises SALVE_STATUS_BAD_GRAPH_ROW.
 *   workspace       unused today (salve_pose_graph_workspace_bytes returns 0; NULL is accepted): the floor's graph lives in LDS
 * One launch on `stream`, one workgroup of 256 threads per floor; n_floors == 0 launches nothing.  Every output the call documents is
 * written, none needs zeroing, and no value depends on an arrival order: the same bytes on every run.  SALVE_ERR_BAD_ARG for a negative
 * count, max_nodes outside 1 .. 256, cycle_filter outside {0, 1}, a NaN threshold, and -- with n_floors > 0 -- a null or misaligned pointer
 * (rows and out_rows may be null while n_rows == 0). */
#define SALVE_GRAPH_MAX_NODES 256
typedef struct {
    int32_t i1, i2;  /* compact node indices within the floor, i1 < i2 */
    float prob;      /* probability of the predicted class (the prediction files' y_hat_probs) */
    int32_t y_hat;   /* predicted class */
    float R[4];      /* i2Si1: rotation, row-major */
    float t[2];      /*        translation */
    double s;        /*        scale */
} salve_graph_row_t;
typedef struct {
    int32_t chosen, consistent;    /* 0 / 1 */
    int32_t n_triplets;            /* 3-cycles of chosen edges through this edge */
    int32_t n_consistent;          /* ... of which consistent */
    float min_rot_err, min_trans_err; /* the smallest errors over those cycles (each on its own), +inf without one; a NaN error never lowers them */
} salve_graph_row_out_t;
typedef struct {
    int32_t localized;             /* 0 / 1 */
    int32_t parent, depth;         /* BFS tree: the origin has parent -1 and depth 0 */
    int32_t reserved;              /* written 0 */
    float R[4];                    /* wSi */
    float t[2];
    double s;
} salve_graph_node_out_t;
typedef struct {
    int32_t n_chosen, n_triplets, n_consistent_triplets, n_consistent_edges, n_localized, origin; /* origin: -1 when the graph has no edge */
} salve_graph_floor_out_t;
size_t salve_pose_graph_workspace_bytes(int32_t n_floors, int32_t max_nodes);
int salve_pose_graph_solve(const salve_graph_row_t* rows, int32_t n_rows, const int32_t* floor_start, const int32_t* n_nodes, int32_t n_floors,
                           int32_t max_nodes, float confidence_threshold, float rot_threshold_deg, float trans_threshold, int32_t cycle_filter,
                           salve_graph_row_out_t* out_rows, salve_graph_node_out_t* out_nodes, salve_graph_floor_out_t* out_floors,
                           void* workspace, size_t workspace_bytes, int32_t* status, void* stream);

/* RANSAC over random spanning trees: the `random_spanning_trees` method of the reference's scripts/run_sfm.py and its edge filter
 * --filter_edges_by_random_spanning_trees, for any number of floors and hypotheses in ONE call (two launches on `stream`).  Stands behind
 *   salve/algorithms/spanning_tree.py:179-334  ransac_spanning_trees
 *   salve/algorithms/spanning_tree.py:337-384  compute_hypothesis_errors
 *   salve/algorithms/spanning_tree.py:144-176  compute_objective_function_improvement
 * The subsets are DRAWN BY THE CALLER (salve_amd.pose_graph.draw_hypotheses draws the reference's); the device never draws, so every output
 * is the same bytes on every run.  rows, n_rows, floor_start, n_nodes, max_nodes: exactly salve_pose_graph_solve's, verified the same way.
 *   hyp_start   device int32 [n_floors + 1]: the hypotheses of floor f are hyp_start[f] .. hyp_start[f + 1] - 1
 *   hyp_mask    device uint32 [n_hyps][mask_words]: bit k (word k / 32, bit k % 32) of a hypothesis's mask stands for the floor's row
 *               floor_start[f] + k.  Bits at or beyond the floor's row count and bits on rows that are not candidates are IGNORED; a row
 *               beyond 32 * mask_words has no bit.  May be null while mask_words == 0.
 * Launch 1, one workgroup of 256 threads per hypothesis:
 * A', edges: a row is a candidate iff y_hat == 1 && prob >= confidence_threshold (a NaN prob never is).  Of a pair's contiguous rows the
 *    hypothesis takes the LAST candidate whose mask bit is set -- the reference's dict overwrite in measurement order (:256-258), NOT the
 *    largest prob as salve_pose_graph_solve does.
 * C, D: salve_pose_graph_solve's, over those edges, with its tie rules.  The node records go to the workspace.
 * E, errors against ALL candidate rows of the floor, masked or not.  A row whose two ends are localized is MEASURED:
 *    Z = inverse(wS_i2).compose(wS_i1); th_sim = (double)(atan2f(Z.R10, Z.R00) * C), th_m the same from the row's own R, where C is the
 *    float32 quotient 180.0f / (float)pi = 57.295776 (numpy's float32 rad2deg; not the (float)(180 / pi) of phase B);
 *    d = fmod(th_m - th_sim + 180.0, 360.0), + 360.0 if d < 0; rot_err = fabs(d - 180.0), all float64;
 *    trans_err = (double)sqrtf(dx * dx + dy * dy) on the float32 differences of the two translations.
 *    The sums are float64 in ONE order: thread t adds its rows lo + t, lo + t + 256, ... ascending from 0.0; the 256 partial sums are folded
 *    by halving (p[t] += p[t + 128], then 64, ... 1).  avg = sum / (double)n_measured: NaN without a measured row (np.mean([])), NaN with a
 *    NaN error; every NaN average is written as the quiet NaN 0x7FF8000000000000.  The reference's medians are not computed.
 * Launch 2, one workgroup per floor: one thread scans the floor's hypotheses in order, in float64, from best_rot = best_trans = +inf,
 *    best_n = 0: obj = ((best_rot - rot) / 5 + (best_trans - trans) / 1) + 1.33 * (-(best_n - n) / (best_n + 1e-10)); the hypothesis
 *    replaces the best iff obj > 0 (a NaN never does).  The winner's node records are copied to out_nodes, and out_inlier[r] = 1 for the
 *    rows that are candidates AND in the winner's mask (the reference's best_hypothesis), 0 for every other row of the floor.
 *    A floor without a hypothesis, or whose every hypothesis scores NaN, has best == -1, empty nodes and no inlier (the reference would
 *    crash at len(None): a documented deviation).
 *   out_trees   device salve_graph_tree_out_t [n_hyps], 8-byte aligned.  A hypothesis in no floor's extent: empty, floor == -1.
 *   out_inlier  device int32 [n_rows];  out_nodes: as salve_pose_graph_solve's, the WINNER's;  out_floors: 8-byte aligned
 *   workspace   salve_pose_graph_sample_workspace_bytes(n_hyps, max_nodes) bytes, 8-byte aligned: a node record per hypothesis and node
 * Malformed floors: a bad row extent or node count, rows that break the row contract, a hyp_start extent outside [0, n_hyps] or decreasing,
 * or one that overlaps a LOWER floor's extent (a hypothesis belongs to the lowest floor whose well-formed extent holds it).  Such a floor is
 * written EMPTY (its hypotheses' records too) and raises SALVE_STATUS_BAD_GRAPH_ROW; the other floors are solved.  Every table is verified
 * before an address is formed from it.  n_floors == 0 or n_hyps == 0 launches nothing and writes nothing.
 * SALVE_ERR_BAD_ARG for a negative count, max_nodes outside 1 .. 256, a NaN threshold, and -- with something to launch -- a null or
 * misaligned pointer (rows and out_inlier may be null while n_rows == 0); SALVE_ERR_WORKSPACE for a short workspace. */
typedef struct {
    double avg_rot_err, avg_trans_err; /* mean over the measured rows, degrees and metres */
    int32_t n_localized;               /* the size of the tree's component (the reference's num_poses_estimated) */
    int32_t n_measured;                /* candidate rows with both ends localized */
    int32_t n_edges;                   /* distinct pairs of the hypothesis */
    int32_t origin;                    /* -1: no edge */
    int32_t floor;                     /* the floor it was evaluated for; -1: none */
    int32_t reserved;                  /* written 0 */
} salve_graph_tree_out_t;
typedef struct {
    int32_t best;                      /* index within the floor's hypotheses; -1: none */
    int32_t n_candidates;              /* the reference's K */
    int32_t n_hyps;
    int32_t n_improvements;            /* how often the scan replaced its best */
    double avg_rot_err, avg_trans_err; /* the winner's; NaN without one */
} salve_graph_sample_floor_out_t;
size_t salve_pose_graph_sample_workspace_bytes(int32_t n_hyps, int32_t max_nodes);
int salve_pose_graph_sample_trees(const salve_graph_row_t* rows, int32_t n_rows, const int32_t* floor_start, const int32_t* n_nodes,
                                  int32_t n_floors, int32_t max_nodes, float confidence_threshold, const int32_t* hyp_start,
                                  const uint32_t* hyp_mask, int32_t n_hyps, int32_t mask_words, salve_graph_tree_out_t* out_trees,
                                  int32_t* out_inlier, salve_graph_node_out_t* out_nodes, salve_graph_sample_floor_out_t* out_floors,
                                  void* workspace, size_t workspace_bytes, int32_t* status, void* stream);

/* Pose-graph optimisation: the `pgo` method of the reference's scripts/run_sfm.py (:448-451), a robust Levenberg-Marquardt refinement of a
 * floor's spanning-tree poses over ALL its thresholded predictions, for any number of floors in ONE launch.  Stands behind
 *   salve/algorithms/pose2_slam.py:57-172    planar_slam (optimize_poses_only: no landmark, no bearing-range factor)
 *   salve/algorithms/pose2_slam.py:175-286   execute_planar_slam (without axis alignment)
 * and gtsam's PriorFactorPose2, BetweenFactorPose2, noiseModel.Robust(Huber) and LevenbergMarquardtOptimizer, restated as the rules below.
 * gtsam is not installed where this is built.  Its default build, as far as its source is recalled, linearises the between factor without
 * the chart's derivative and adds a model-fidelity test to the acceptance rule: parity with gtsam's ITERATES and stopping point is therefore
 * UNPINNED.  What is pinned is the objective -- exactly the reference's factor graph -- and that the result minimises it.
 * rows, n_rows, floor_start, n_nodes, max_nodes, confidence_threshold: exactly salve_pose_graph_solve's, verified the same way.
 *   init   device salve_graph_node_out_t [n_floors * max_nodes], 8-byte aligned: the tree's out_nodes (solve and optimise chain on the device).
 * Unknowns: (x, y, theta) in float64 per LOCALIZED node of `init` (localized != 0), in ascending node order; at most 256 nodes, 768 scalars.
 *    Initial value x, y = (double)t[0], (double)t[1], theta = atan2((double)R[2], (double)R[0]).  (The reference goes through theta_deg and
 *    Rot2.fromDegrees: about an ulp apart.  A documented deviation.)  theta is never wrapped: it stays continuous from its initial value.
 * Odometry factors: one per CANDIDATE row (y_hat == 1 && prob >= confidence_threshold; a NaN prob never is) whose two ends are localized
 *    (pose2_slam.py:109-117) -- ALL such rows of a pair, not the most confident one.  m = ((double)t[0], (double)t[1], atan2((double)R[2],
 *    (double)R[0])) of the row's i2Si1; its scale is ignored (the reference builds a Pose2).  Residual of BetweenFactorPose2(X(i2), X(i1), m):
 *    delta = R(theta2)^T (p1 - p2);  e_xy = R(m_theta)^T (delta - m_xy);  e_theta = wrap(theta1 - theta2 - m_theta),
 *    wrap(a) = a - 2 pi ceil((a - pi) / (2 pi)), into (-pi, pi].  Sigmas odometry_sigmas (the reference: 0.2, 0.2, 0.1).
 * Prior factor on the origin, the LOWEST localized node (np.argmax at :102): e = (x, y, wrap(theta)), sigmas prior_sigmas (0.3, 0.3, 0.1).
 * Cost: r = e / sigma, n = ||r||, E = sum rho(n); robust = 1: rho = n^2 / 2 for n <= huber_k, huber_k (n - huber_k / 2) beyond (the
 *    reference's run: 1.345); robust = 0: rho = n^2 / 2 (the reference's unit test).  The sum is float64 in ONE order: thread t of 256 adds the
 *    rho of the floor's rows lo + t, lo + t + 256, ... ascending from 0.0 (thread 0 from the prior's rho); the 256 partial sums are folded by
 *    halving (p[t] += p[t + 128], then 64, ... 1).
 * Step: retraction p += R(theta) d_xy, theta += d_theta (gtsam's default Pose2 chart).  Each factor's exact Jacobian in that chart and its
 *    whitened residual are scaled by sqrt(w), w = 1 for n <= huber_k (or robust = 0), huber_k / n otherwise (IRLS, as gtsam's Robust
 *    linearises).  (J^T J + lambda I) d = -J^T r by a dense float64 Cholesky factorisation of the lower triangle (right-looking, column by
 *    column), a forward and a backward substitution.  A pivot that is not finite and positive is a rejected step.
 *    Order of the sums (no floating-point atomic anywhere): the 3 x 3 block of a pair of nodes is accumulated over the pair's (contiguous) rows
 *    in row order by the thread of the pair's first row; a node's diagonal block and gradient segment by the node's thread over ALL rows of
 *    the floor that touch it, in row order, the prior first.  The same bytes on every run, whichever floors share the launch.
 * LM loop (gtsam's defaults): lambda = 1e-5; at most max_iterations linearisations; a step is ACCEPTED iff E(x + d) is finite and <= E(x):
 *    then lambda /= 10, and the loop stops if the decrease is <= absolute_error_tol, else if decrease / E_old <= relative_error_tol.
 *    Otherwise (REJECTED) lambda *= 10 and the same linearisation is solved again; the loop stops when lambda > 1e5.
 *   out_nodes   device salve_graph_node_out_t [n_floors * max_nodes], 8-byte aligned (records v >= n_nodes[f] NOT written): localized,
 *               parent, depth copied from `init`; R = (float) of (cos, -sin, sin, cos) of theta, t = (float) of x, y; s = 1.0.  A node that
 *               is not localized: the empty record (0, -1, -1, zeros).
 *   out_pose    device double [n_floors * max_nodes][3]: x, y, theta; quiet NaN where not localized; rows v >= n_nodes[f] NOT written
 *   out_floors  device salve_graph_pgo_floor_out_t [n_floors], 8-byte aligned
 *   workspace   salve_pose_graph_optimise_workspace_bytes(n_floors, max_nodes) bytes, 8-byte aligned.  A floor of at most
 *               SALVE_PGO_LDS_NODES localized nodes keeps its system matrix in LDS; a larger one in its slice of the workspace (0 bytes and
 *               NULL accepted while max_nodes <= SALVE_PGO_LDS_NODES).  Both go through the same code.
 * Malformed floors -- a bad extent, a bad row, n_nodes > max_nodes, an `init` record whose parent lies outside [-1, n_nodes) -- are written
 * EMPTY (empty nodes, NaN poses, a zero record with SALVE_PGO_STOP_EMPTY, NaN costs) and raise SALVE_STATUS_BAD_GRAPH_ROW; the other floors are
 * unaffected.  A floor without a localized node is written empty and raises nothing.  A non-finite initial pose or measurement of a factor
 * ends the floor with SALVE_PGO_STOP_NON_FINITE: the initial poses are written, costs NaN.  No address is formed from an unverified index.
 * SALVE_ERR_BAD_ARG for a negative count, max_nodes outside 1 .. 256, a NaN threshold, robust outside {0, 1}, a sigma, huber_k or tolerance
 * that is NaN or not positive, a negative max_iterations, and -- with n_floors > 0 -- a null or misaligned pointer (rows may be null while
 * n_rows == 0); SALVE_ERR_WORKSPACE for a short workspace.  odometry_sigmas and prior_sigmas are HOST double [3]. */
#define SALVE_PGO_LDS_NODES 56
enum {
    SALVE_PGO_STOP_EMPTY = 0,          /* nothing to optimise: malformed floor, or no localized node */
    SALVE_PGO_STOP_ABSOLUTE = 1,       /* an accepted step's decrease <= absolute_error_tol */
    SALVE_PGO_STOP_RELATIVE = 2,       /* ... decrease / E_old <= relative_error_tol */
    SALVE_PGO_STOP_LAMBDA = 3,         /* lambda exceeded 1e5 */
    SALVE_PGO_STOP_MAX_ITERATIONS = 4, /* max_iterations linearisations done */
    SALVE_PGO_STOP_NON_FINITE = 5      /* a non-finite initial pose or measurement */
};
typedef struct {
    int32_t n_unknown_nodes;           /* localized nodes */
    int32_t n_factors;                 /* the prior and the odometry factors */
    int32_t n_iterations;              /* linearisations */
    int32_t n_rejected;                /* rejected steps */
    int32_t n_downweighted;            /* factors with n > huber_k at the final poses (robust = 0: 0) */
    int32_t stop_reason;               /* SALVE_PGO_STOP_* */
    double lambda, cost_initial, cost_final;
} salve_graph_pgo_floor_out_t;
size_t salve_pose_graph_optimise_workspace_bytes(int32_t n_floors, int32_t max_nodes);
int salve_pose_graph_optimise(const salve_graph_row_t* rows, int32_t n_rows, const int32_t* floor_start, const int32_t* n_nodes, int32_t n_floors,
                              int32_t max_nodes, float confidence_threshold, const salve_graph_node_out_t* init, int32_t robust, double huber_k,
                              const double* odometry_sigmas, const double* prior_sigmas, int32_t max_iterations, double relative_error_tol,
                              double absolute_error_tol, salve_graph_node_out_t* out_nodes, double* out_pose,
                              salve_graph_pgo_floor_out_t* out_floors, void* workspace, size_t workspace_bytes, int32_t* status, void* stream);

/* The floor reconstruction report, part 1: the estimated poses of any number of floors aligned to the truth by the reference's RANSAC, and
 * the pose errors, in ONE call (two launches on `stream`).  Stands behind
 *   salve/utils/ransac.py:14-129            ransac_align_poses_sim3_ignore_missing, compute_pose_errors_3d
 *   salve/common/posegraph2d.py:281-383     measure_aligned_abs_pose_error, align_by_Sim3_to_ref_pose_graph, apply_Sim3
 *   gtsfm's align_poses_sim3_ignore_missing and gtsam's Similarity3.Align of pose pairs, restated as the rules below (neither is installed
 *   where this is built; the restatement reproduces the numbers the reference's own tests record -- tests/test_floor_report_host.py).
 * The subsets are DRAWN BY THE CALLER (salve_amd.floor_report.draw_alignment_subsets draws the reference's); the device never draws.
 *   node_start   device int32 [n_floors + 1]: the panoramas of floor f are the records node_start[f] .. node_start[f + 1] - 1 of the two pose
 *                tables, at most 256 (SALVE_GRAPH_MAX_NODES); index k within the floor is the floor's COMPACT panorama index
 *   truth, est   device salve_graph_node_out_t [n_nodes], 8-byte aligned: `localized` (present), R, t (float32) and s are read; the estimate's
 *                s is taken as 1 (PoseGraph2d.from_wSi_list)
 *   hyp_start    device int32 [n_floors + 1]: the hypotheses of floor f are hyp_start[f] .. hyp_start[f + 1] - 1
 *   hyp_mask     device uint32 [n_hyps][8]: bit k of a hypothesis's KEEP mask stands for compact index k; bits at or beyond the floor's
 *                panorama count are ignored
 *   gt_scale, metres_per_coordinate   device float64 [n_floors]: the scale the aligned poses carry, and scale_meters_per_coordinate
 * Launch 1, one wavefront per hypothesis, four per workgroup.  Everything is float64 (R, t widened first), no product is fused into a sum.
 * The hypothesis's PAIRS are the indices whose bit is set and that are present in both tables, ascending; n of them.
 *  1. n < 2: R = I, t = 0, s = 1 (gtsfm's skip rule).  Otherwise:
 *  2. aRb_i = Ra_i * Rb_i^T; R0 = the first pair's.
 *  3. one Karcher step: M_i = R0^T * aRb_i, d_i = atan2(M10, M00), m = (sum d_i) / n, R = R0 * [[cos m, -sin m], [sin m, cos m]];
 *  4. a second step from R.  Exactly two.
 *  5. ca = (sum a_i) / n, cb = (sum b_i) / n (the translations).
 *  6. y = sum (a_i - ca) . (R (b_i - cb)), x = sum |R (b_i - cb)|^2, s = y / x, t = (ca - s * (R cb)) / s: the convention s (R p + t).
 *  7. s NaN or 0 (coincident translations): s = 1, t = ca - R cb.  This rule is this project's own: gtsfm has a fallback there whose text was
 *     not available; NOT pinned against it.
 *  8. errors over the hypothesis's OWN pairs: R_i' = R Rb_i, t_i' = s (R b_i + t); E = Ra_i^T R_i'; rot_i = |atan2(E10, E00)| * (180 / pi);
 *     trans_i = sqrt(dx^2 + dy^2) of a_i - t_i'; the two means are the sums / n (NaN without a pair).
 *  Sums: lane l of the wavefront adds the values of its indices l, l + 64, l + 128, l + 192 in ascending order from 0.0 (pairs only); the 64
 *  partial sums fold by halving (p[l] += p[l + 32], then 16, ... 1).  No floating-point atomic: the same bytes on every run.
 * Launch 2, one workgroup per floor.  Pick: the hypotheses in order from best_rot = best_trans = +inf; one replaces the best iff
 *  trans <= best_trans && rot <= best_rot (of equals the LATER; a NaN never).  Apply: a_Sim2_b = ((float)R, (float)t, s) composed with
 *  (R_i, t_i, 1.0) of every present estimated panorama under the float32 Sim2 rules of salve_pose_graph_solve's phase D; the record written
 *  is (localized 1, parent -1, depth -1, R, t * (float)scale, gt_scale[f]).  Report: over the panoramas present in BOTH tables, rot_i and
 *  trans_i by step 8's formulas on the aligned float32 pose widened (R = I, t = 0, s = 1); thread k holds panorama k's value (0.0 without
 *  one), the 256 values fold by halving (128, 64, ... 1); avg_rot_err = sum / n_both, avg_trans_err = sum / n_both * metres_per_coordinate[f],
 *  percent_localized = n_est / n_gt * 100 (the reference's order of operations).
 *  A floor without a winner (no hypothesis, or every one NaN) is NOT ALIGNED: best -1, empty node records, NaN errors and NaN R, t, s, where
 *  the reference would fail on None -- a documented deviation.
 *   out_hyps        device salve_floor_hyp_out_t [n_hyps], 8-byte aligned.  A hypothesis in no floor's extent: identity, NaN, floor == -1.
 *   out_nodes       device salve_graph_node_out_t [n_nodes]: the aligned estimate; a panorama absent from it: the empty record
 *   out_rot_err, out_trans_err   device float64 [n_nodes]: per panorama (trans in coordinate units, as the reference's arrays), NaN where absent
 *   out_floors      device salve_floor_align_out_t [n_floors], 8-byte aligned
 * Malformed floors: a node extent outside [0, n_nodes], decreasing or longer than 256; a hyp_start extent outside [0, n_hyps] or decreasing,
 * or one that overlaps a LOWER floor's (a hypothesis belongs to the lowest floor whose well-formed extent holds it).  Such a floor is written
 * EMPTY (best -1, n_hyps 0, counts 0, NaN; its node records empty where its node extent is sound) and raises SALVE_STATUS_BAD_FLOOR_TABLE;
 * the other floors are reported.  Every table is verified before an address is formed from it.  Records of panoramas in no floor's extent are
 * not written.  n_floors == 0 launches nothing; n_hyps == 0 skips launch 1 (hyp_mask and out_hyps may then be null).
 * SALVE_ERR_BAD_ARG for a negative count and -- with something to launch -- a null or misaligned pointer. */
#define SALVE_FLOOR_MASK_WORDS 8
typedef struct {
    double R[4], t[2], s;       /* aSb of the hypothesis's own pairs */
    double rot_err, trans_err;  /* the means over its own pairs, degrees and coordinate units; NaN without a pair */
    int32_t n_pairs;
    int32_t floor;              /* the floor it was evaluated for; -1: none */
} salve_floor_hyp_out_t;
typedef struct {
    int32_t best;               /* index within the floor's hypotheses; -1: not aligned */
    int32_t n_hyps;
    int32_t n_est, n_gt;        /* panoramas present in the estimate, in the truth */
    double avg_rot_err;         /* degrees */
    double avg_trans_err;       /* METRES */
    double percent_localized;
    double R[4], t[2], s;       /* the winner's aSb; NaN without one */
} salve_floor_align_out_t;
int salve_floor_align(const int32_t* node_start, int32_t n_floors, int32_t n_nodes, const salve_graph_node_out_t* truth,
                      const salve_graph_node_out_t* est, const int32_t* hyp_start, const uint32_t* hyp_mask, int32_t n_hyps, const double* gt_scale,
                      const double* metres_per_coordinate, salve_floor_hyp_out_t* out_hyps, salve_graph_node_out_t* out_nodes, double* out_rot_err,
                      double* out_trans_err, salve_floor_align_out_t* out_floors, int32_t* status, void* stream);

/* The floor reconstruction report, part 2: the raster IoU of the estimated and the true floor plan of any number of floors in ONE call (two
 * memsets and four launches on `stream`).  Stands behind salve/common/floor_reconstruction_report.py:271-338 (render_raster_occupancy,
 * rasterize_room) and salve/utils/bev_rendering_utils.py:159-193; cv2.fillPoly is restated as oracle/layout_oracle.py's fill_poly, as
 * salve_layout_rasterise's polygon is (parity with cv2 unpinned: it is not installed where this is built).
 *   room_xy, room_off   device float64 [2 * n_room_xy] and int64 [n_nodes + 1]: the LOCAL room vertices (x already negated) of panorama i are
 *                       room_off[i] .. room_off[i + 1] - 1, salve_layout_pose's form, indexed like the pose tables
 *   node_start, est, truth, metres_per_coordinate   as salve_floor_align's; `est` is its out_nodes.  s is read from both tables.
 *   img_h, img_w        the raster, 1 .. 32000 each (the reference: 501 x 501)
 *   offset_x, offset_y, pixels_per_metre   bevimg_Sim2_world: a float32 translation, widened, and a float64 scale (the reference: 25, 25, 10)
 * Launch 1 poses: per table and present panorama g = s_i * (v @ R_i^T + t_i) in float64 with R, t widened, every product and sum on its own;
 *  g * metres_per_coordinate[f]; px = round_half_even((g + offset) * pixels_per_metre) as int32.
 * Launch 2 rasterises: one workgroup per 16 x 16 pixel tile of a floor.  A pixel is occupied in a table iff SOME present panorama's polygon
 *  covers it: even-odd on the 16.16 crossings united with the 8-connected line pixels of every edge (fill_poly).  Counting is by wave
 *  ballots and one INTEGER atomic add per wave and counter: the same bytes on every run.
 * Launch 3: iou = inter / (uni + 1e-12).
 *   out         device salve_floor_iou_out_t [n_floors], 8-byte aligned
 *   out_masks   NULL, or device uint32 [n_floors][2][img_h][(img_w + 31) / 32]: the estimate's mask, then the truth's; pixel (x, y) is bit
 *               x % 32 of word x / 32 of row y (NOT flipped)
 *   workspace   salve_floor_iou_workspace_bytes(n_room_xy, n_nodes) bytes, 16-byte aligned
 * A floor with a malformed node extent (salve_floor_align's rule), or with a posed vertex that is not finite or beyond 2^24 pixels
 * (pack_layouts' limit): bad = 1, counts 0, iou NaN, empty masks, and SALVE_STATUS_BAD_FLOOR_TABLE is raised; the other floors are
 * rasterised.  room_off must ascend within [0, n_room_xy] over ALL n_nodes panoramas (a launch of its own verifies it first): the posed
 * pixels live in the workspace by vertex index, so where two panoramas claim one vertex NO floor is rasterised -- every floor is bad.
 * n_floors == 0 launches nothing.  SALVE_ERR_BAD_ARG for a negative count, an image size outside
 * 1 .. 32000, a non-finite raster parameter, more than 2^31 - 1 tiles (floors x tiles of an image), a null or misaligned pointer (room_xy may be null
 * while n_room_xy == 0); SALVE_ERR_WORKSPACE for a short workspace. */
typedef struct {
    int32_t n_est, n_gt;        /* occupied pixels of the estimate's mask, of the truth's */
    int32_t inter, uni;
    int32_t bad;                /* 0 / 1 */
    int32_t reserved;           /* written 0 */
    double iou;
} salve_floor_iou_out_t;
size_t salve_floor_iou_workspace_bytes(int64_t n_room_xy, int32_t n_nodes);
int salve_floor_iou(const double* room_xy, const int64_t* room_off, int64_t n_room_xy, const int32_t* node_start, int32_t n_floors, int32_t n_nodes,
                    const salve_graph_node_out_t* est, const salve_graph_node_out_t* truth, const double* metres_per_coordinate, int32_t img_h,
                    int32_t img_w, float offset_x, float offset_y, double pixels_per_metre, salve_floor_iou_out_t* out, uint32_t* out_masks,
                    void* workspace, size_t workspace_bytes, int32_t* status, void* stream);

/* Alignment hypotheses: every W/D/O alignment of every panorama pair of any number of floors in ONE launch (additive within ABI 7).  Stands
 * behind the inferred-W/D/O path (`--wdo_source horizon_net`) of the reference's scripts/export_alignment_hypotheses.py:93-273:
 *   salve/utils/wdo_alignment.py:107-284           align_rooms_by_wd (transform_type SE2, use_inferred_wdos_layout)   enumeration, fit, acceptance
 *   salve/utils/se2_estimation.py:11-41            align_points_SE2 (gtsam's Pose2::Align)                           the fit
 *   salve/utils/wdo_alignment.py:394-415           determine_invalid_width_ratio                                     acceptance
 *   salve/common/alignment_hypothesis.py:29-56     prune_to_unique_sim2_objs (Sim2.__eq__, sim2.py)                  pruning
 *   salve/utils/wdo_alignment.py:418-454           obj_almost_equal (rotation_utils.angle_is_equal)                  the label
 *   scripts/export_alignment_hypotheses.py:43-72   are_visibly_adjacent (shapely's hausdorff_distance)               adjacency
 *   scripts/export_alignment_hypotheses.py:205     i2Ti1_gt = wTi2.inverse().compose(wTi1)                           the truth of a pair
 * The host names the pairs: one salve_hyp_pair_t per panorama pair, in any order (the floors, the ascending panorama ids and the pairs the
 * reference leaves out are the host's business).  Per pair the candidates are enumerated doors, windows, openings (wdo_type 1, 0, 2 --
 * salve_layout_pose's codes); within a type i over pano1's objects of the type, j over pano2's (both in table order), and for doors and
 * openings the configuration identity (0) then rotated (1: pano2's two vertices swapped); windows have identity only.  capacity must equal
 * that count: 2 d1 d2 + w1 w2 + 2 o1 o2.
 * Fit, all float64, no product fused into a sum: a = pano2's polygon [p1, p1, p2, p2, p1] (p1 counts three times, p2 twice: the rotation is
 *  the two-point fit's, the translation is not when the widths differ), b = pano1's; ca, cb = (the sum in point order) / 5; over the five
 *  points in order c += db.x da.x + db.y da.y and s += -db.y da.x + db.x da.y; h = sqrt(c c + s s); R = [[c / h, -s / h], [s / h, c / h]],
 *  R = I when h == 0; t = ca - R cb; R and t are rounded to float32 once.  (gtsam takes cos / sin of atan2(s, c): a stated deviation of a
 *  few float64 ulps)
 * Accept: w = sqrt(dx dx + dy dy) of each object; min(w1, w2) / max(w1, w2) >= min_width_ratio (a NaN ratio rejects).
 * Prune, greedily in candidate order over all three types: an accepted candidate x is kept unless |x - k| <= 1e-8 + 1e-5 |k| holds in all four
 *  entries of R and both of t for some k kept before it (float32 values widened to float64; NaN is unequal).
 * Label of a kept row against G = inverse(wS_pano2).compose(wS_pano1) (the float32 Sim(2) arithmetic of salve_pose_graph_solve): 1 iff
 *  |t - G.t| <= 0.35 + 1e-5 |G.t| in both entries, |1 - G.s| <= 0.35 + 1e-5 |G.s|, and the angle difference d = fmod(th_G - th + 180, 360)
 *  (+ 360 when negative) - 180, + 360 if < -180, has |d| <= 7 (doors, windows) or 9 (openings); th = atan2(R10, R00) * (180 / pi) in float64.
 * Adjacency: the pair is visibly adjacent iff some segment of pano1's and some of pano2's GLOBAL ground-truth W/D/Os lie at a Hausdorff
 *  distance < 0.1 (the larger of the two directed maxima over endpoints of the point-to-segment distance, GEOS' rule).
 *   wdo_xy, wdo_type, wdo_off   device float64 [n_wdo][2][2], uint8 [n_wdo], int64 [n_panos + 1]: the inferred W/D/Os, local frames
 *   gt_xy, gt_off               device float64 [n_gt][2][2], int64 [n_panos + 1]: the ground-truth W/D/Os in the GLOBAL frame
 *   poses                       device salve_graph_node_out_t [n_panos]: wS_pano in R, t, s (the other fields are not read)
 *   pairs                       device salve_hyp_pair_t [n_pairs], 8-byte aligned
 *   max_capacity                the caller's bound on pairs[].capacity: sizes the workgroup's LDS (24 bytes per candidate); 0 .. 5120
 *   out_rows                    device salve_hyp_row_t [n_rows]: the kept rows of pair p are row_offset .. row_offset + n_kept - 1, in
 *                               candidate order; the rows behind them up to row_offset + capacity are NOT written
 *   out_pairs                   device salve_hyp_pair_out_t [n_pairs], 8-byte aligned
 * One launch on `stream`, one workgroup of one wavefront per pair; n_pairs == 0 launches nothing.  No floating-point atomic and no atomic append:
 * a kept row's place is its rank in candidate order, so the same bytes on every run.  The tables are device memory, so the kernel verifies a
 * pair before it forms an address from it: with a panorama outside [0, n_panos), an offset table that steps back or leaves its array, more
 * than 32 objects of a type, a capacity other than the candidate count or above max_capacity, or rows outside [0, n_rows], the pair's
 * record is written n_kept = -1 (zeros elsewhere) and none of its rows.  SALVE_ERR_BAD_ARG for a negative count, max_capacity outside
 * 0 .. 5120, a NaN ratio, and -- with n_pairs > 0 -- a null or misaligned pointer (the W/D/O arrays and out_rows may be null while empty). */
#define SALVE_HYP_MAX_WDO_PER_TYPE 32
#define SALVE_HYP_MAX_CAPACITY 5120 /* 2 * 32 * 32 + 32 * 32 + 2 * 32 * 32 */
typedef struct {
    int32_t pano1, pano2;  /* indices into the panorama tables */
    int32_t capacity;      /* the pair's candidate count */
    int32_t reserved;      /* not read */
    int64_t row_offset;    /* the pair's first row in out_rows */
} salve_hyp_pair_t;
typedef struct {
    float R[4];            /* i2Ti1: rotation, row-major */
    float t[2];
    int32_t type;          /* 1 door, 0 window, 2 opening */
    int32_t i, j;          /* the object's rank within its type in pano1, in pano2 */
    int32_t configuration; /* 0 identity, 1 rotated */
    int32_t label;         /* 1 gt_alignment_approx, 0 incorrect_alignment */
    int32_t reserved;      /* written 0 */
} salve_hyp_row_t;
typedef struct {
    int32_t n_kept;           /* -1: a malformed pair */
    int32_t n_valid;          /* accepted candidates, before pruning */
    int32_t n_rejected;       /* candidates the width ratio rejected */
    int32_t visibly_adjacent; /* 0 / 1 */
    float R[4];               /* i2Ti1_gt */
    float t[2];
    double s;
} salve_hyp_pair_out_t;
int salve_hypotheses_generate(const double* wdo_xy, const uint8_t* wdo_type, const int64_t* wdo_off, int64_t n_wdo, const double* gt_xy,
                              const int64_t* gt_off, int64_t n_gt, const salve_graph_node_out_t* poses, int32_t n_panos,
                              const salve_hyp_pair_t* pairs, int64_t n_pairs, int32_t max_capacity, double min_width_ratio,
                              salve_hyp_row_t* out_rows, int64_t n_rows, salve_hyp_pair_out_t* out_pairs, void* stream);

/* Axis alignment by vanishing angle: every scored hypothesis i2Si1 turned about the W/D/O it was aligned on until the two panoramas' vanishing
 * angles agree, for any number of floors in ONE launch (additive within ABI 7).  Stands behind --use_axis_alignment (default True) of the
 * reference's scripts/run_sfm.py:421-426 and salve/algorithms/pose2_slam.py:217-231:
 *   salve/utils/axis_alignment_utils.py:175-263   align_pair_measurement_by_vanishing_angle
 *   salve/utils/axis_alignment_utils.py:266-284   compute_vp_correction
 *   salve/utils/axis_alignment_utils.py:295-323   compute_i2Ti1 (gtsam's Similarity3.Align over point pairs, the degree round trip)
 *   salve/utils/rotation_utils.py:14-42, 87-103   rotmat2d, rotmat2theta_deg, rotate_polygon_about_pt
 *   salve/common/sim2.py:135-160, wdo.py:35-37    Sim2.transform_from, WDO.centroid
 * A pure map over the rows: out_rows[r] is rows[r] with R, t, s replaced where the correction applies; salve_pose_graph_solve and
 * salve_pose_graph_optimise take out_rows in place of rows.  Row r was aligned on W/D/O row_wdo[r] of panorama i1.  Everything is float64 with R
 * and t widened first, no product fused into a sum, every sum in ascending vertex order from 0.0 -- but for the row's own angle:
 *  angle:   theta = (double)(atan2f(R10, R00) * (float)(180 / pi)): float32, as numpy evaluates it on Sim2's float32 entries.
 *  move:    a point p of i1's frame goes to ((p.x R00 + p.y R01) + tx) s, ((p.x R10 + p.y R11) + ty) s (Sim2.transform_from, per entry).
 *  centre:  c = move(((x1 + x2) / 2, (y1 + y2) / 2)) of the W/D/O's two endpoints.
 *  room:    the tables hold rooms CLOSED (layout.PanoLayouts); the polygon used is the OPEN one, all vertices but the last, n of them.
 *  correct: corr = -((vp2 - vp1) + theta); corr = fmod(corr, 90), + 90 when negative (Python's %: [0, 90)); - 90 when > 45.
 *           |corr| > 15 (MAX_ALLOWED_CORRECTION_DEG): SALVE_AXIS_TOO_LARGE, the row stays.
 *  turn:    cs = cos(corr pi / 180), sn = sin(..); a_k = ((d.x cs + d.y (-sn)) + c.x, (d.x sn + d.y cs) + c.y), d = move(v_k) - c; b_k = v_k.
 *  align:   ca = (sum a_k) / n, cb = (sum b_k) / n; H = sum (a_k - ca) (b_k - cb)^T; phi = atan2(H10 - H01, H00 + H11) (the planar closest
 *           rotation); with R = [[cos phi, -sin phi], [sin phi, cos phi]]: x = sum (a_k - ca) . (R (b_k - cb)), y = sum |R (b_k - cb)|^2,
 *           s' = x / y, T = (ca - s' (R cb)) / s' (gtsam's convention s (R p + T)).
 *  result:  theta' = atan2(sin phi, cos phi) (180 / pi) degrees, th = theta' (pi / 180) (rotmat2theta_deg, then Rot2.fromDegrees); the row
 *           written is R = (float)[cos th, -sin th, sin th, cos th], t = (float)T, s = 1.0; i1, i2, prob, y_hat are copied.
 * Analytically R' = Rc R and T = (Rc (s t - c) + c) / s with Rc the rotation by corr.
 * Deviations: a panorama without a finite vanishing angle gives SALVE_AXIS_NO_ANGLE (the reference fails on None); a room of fewer than 3
 * open vertices gives SALVE_AXIS_NO_ROOM (gtsam throws); gtsam is not installed where this was built, so parity with Similarity3.Align's
 * bits (its 3-D closest rotation by SVD) is unpinned.  In both cases, and for SALVE_AXIS_TOO_LARGE, the row is copied bit for bit.
 *   rows, n_rows, floor_start, n_nodes   exactly salve_pose_graph_solve's (compact node indices; here no order among the rows is required and
 *                   there is no max_nodes)
 *   row_wdo         device salve_axis_wdo_t [n_rows]: the type code (0 window, 1 door, 2 opening -- salve_layout_pose's) and the index WITHIN
 *                   the type, in table order, of the W/D/O of panorama i1 (EdgeWDOPair's alignment_object and i1_wdo_idx)
 *   pano_base       device int32 [n_floors]: node v of floor f is panorama pano_base[f] + v of the tables below
 *   room_off, room_xy, n_room_xy   device int64 [n_panos + 1], float64 [n_room_xy][2]: the rooms, closed
 *   wdo_off, wdo_xy, wdo_type, n_wdo   device int64 [n_panos + 1], float64 [n_wdo][2][2], uint8 [n_wdo]: the W/D/Os (any order within a panorama)
 *   vanishing_deg   device float64 [n_panos]: degrees; NaN (or an infinity) = the panorama has none
 *   out_rows        device salve_graph_row_t [n_rows], 8-byte aligned; must not overlap rows
 *   out_axis        device salve_axis_row_out_t [n_rows], 8-byte aligned;  out_floors: device salve_axis_floor_out_t [n_floors]
 *   status          device int32 status word or NULL
 * One launch on `stream`, one workgroup of 256 threads per floor, one thread per row; n_floors == 0 launches nothing.  Every output the call
 * documents is written, none needs zeroing, and the same bytes come out on every run.  The tables are device memory, so the kernel verifies
 * every index and offset before it forms an address from it: a row with a node outside [0, n_nodes[f]), a type outside 0 .. 2, a negative
 * index or one the panorama does not hold, a W/D/O or room extent of panorama i1 that steps back or leaves its table, or a floor whose
 * panoramas leave [0, n_panos) is copied unchanged with SALVE_AXIS_MALFORMED and raises SALVE_STATUS_BAD_AXIS_ROW.  A floor whose row extent
 * is malformed (as salve_pose_graph_solve defines it) has no row that can be named: none is written, its record says bad_extent = 1, and the
 * same bit is raised.  SALVE_ERR_BAD_ARG for a negative count and -- with n_floors > 0 -- a null or misaligned pointer (the row tables may
 * be null while n_rows == 0, the panorama tables while n_panos == 0, room_xy / the W/D/O arrays while empty). */
#define SALVE_AXIS_APPLIED 0
#define SALVE_AXIS_TOO_LARGE 1
#define SALVE_AXIS_NO_ANGLE 2
#define SALVE_AXIS_NO_ROOM 3
#define SALVE_AXIS_MALFORMED 4
#define SALVE_AXIS_N_STATUS 5
typedef struct {
    int32_t type;   /* 0 window, 1 door, 2 opening */
    int32_t index;  /* within the type */
} salve_axis_wdo_t;
typedef struct {
    int32_t status;         /* SALVE_AXIS_* */
    int32_t reserved;       /* written 0 */
    double correction_deg;  /* the folded correction; NaN unless APPLIED or TOO_LARGE */
    double theta_deg;       /* APPLIED: the new rotation angle in degrees and the new translation, before they are rounded; NaN otherwise */
    double t[2];
} salve_axis_row_out_t;
typedef struct {
    int32_t n_applied, n_too_large, n_no_angle, n_no_room, n_malformed;
    int32_t bad_extent;     /* 1: the floor's row extent is malformed, the five counts are 0 */
} salve_axis_floor_out_t;
int salve_pose_graph_axis_align(const salve_graph_row_t* rows, int32_t n_rows, const int32_t* floor_start, const int32_t* n_nodes, int32_t n_floors,
                                const salve_axis_wdo_t* row_wdo, const int32_t* pano_base, const int64_t* room_off, const double* room_xy,
                                int64_t n_room_xy, const int64_t* wdo_off, const double* wdo_xy, const uint8_t* wdo_type, int64_t n_wdo,
                                const double* vanishing_deg, int32_t n_panos, salve_graph_row_t* out_rows, salve_axis_row_out_t* out_axis,
                                salve_axis_floor_out_t* out_floors, int32_t* status, void* stream);

/* The two tiles of an early-fusion pair in ONE pass (the fused render -> verify driver's form of salve_bev_tiles, fp16 NHWC
 * only): pair k takes its first image from bev_a + jobs_a[k].bev_offset and its second from bev_b + jobs_b[k].bev_offset,
 * both go to sample jobs_a[k].slot ( == jobs_b[k].slot), channels jobs_a[k].chan .. + 2 and jobs_b[k].chan .. + 2, which
 * must be the two halves of one group of six channels (min(chan) a multiple of 6, |chan_a - chan_b| == 3: the x1 | x2 of a
 * surface, salve/models/early_fusion.py:52-60 -- either order: salve/dataset/zind_data.py:110).  A thread computes both
 * pixels and writes the six channels (and, for the last group of a sample whose out_c leaves padding channels, the zero
 * padding too) with whole-pixel stores, where two salve_bev_tiles calls write three 2-byte channels each.  Same arithmetic
 * as salve_bev_tiles: bit-identical tiles.  b_pretiled = 1: bev_b holds SALVE_TILE_U8X4 images (uint32 [*, crop, crop]) and
 * jobs_b[k].bev_offset is an element offset into THAT array: the second image of a pair is the identity render of a panorama
 * (bev_rendering_utils.py:455), the same for every hypothesis that names it -- resized and cropped once, only ToTensor +
 * Normalize per pair (the same integer taps, the same table: bit-identical again).  (int return: SALVE_ERR_BAD_ARG on null
 * pointers / bad sizes; the pairing rule is the caller's to keep.) */
int salve_bev_tile_pairs(const uint32_t* bev_a, const uint32_t* bev_b, int32_t bev_h, int32_t bev_w, const salve_tile_job_t* jobs_a,
                         const salve_tile_job_t* jobs_b, int32_t n_pairs, const int32_t* coef_y, const int32_t* coef_x, int32_t resize,
                         int32_t crop, const float* lut, void* out, int32_t out_c, int32_t b_pretiled, void* stream);

/* salve_bev_densify followed by salve_bev_tile_pairs(..., b_pretiled = 1) as ONE launch (the fused render -> verify driver's form since
 * ABI 6): every workgroup of the densify kernel, having finished its render, resizes / crops / normalises it into the verifier's sample
 * while the image is still in the L2 -- a launch of its own reads the 1 MB image back from HBM.  The job tables are indexed by RENDER
 * of the launch (render r = image r of out_bev):
 *   jobs_a[r]   .slot / .chan: destination sample and first channel of render r's tile (.bev_offset is not used); slot < 0: no tile
 *   jobs_b[r]   the pair's second image: .bev_offset = element offset of a SALVE_TILE_U8X4 image inside tiles_b, .chan its first channel
 *               (the two chans are the halves of one group of six, as for salve_bev_tile_pairs)
 * out_bev holds the complete images afterwards, exactly as after salve_bev_densify; `out` the same bits salve_bev_tile_pairs writes.
 * SALVE_ERR_BAD_ARG on null pointers, crop <= 0, resize < crop, an odd out_c or one below 6; SALVE_ERR_UNSUPPORTED when the tile phase's
 * tables (32 bytes per resized row + 3 KB) do not fit the densify kernel's LDS block -- two bits per pixel of the BEV image plus 12.5 KB:
 * resize <= 290 fits every image, 234 at 501 x 501 uses a seventh of it.
 * (bev_rendering_utils.py:254-328 + train_utils.py:126-159 / transform.py:256-272, 386-420, 105-123, 177-202.) */
int salve_bev_densify_tiles(const salve_bev_config_t* cfg, int32_t n, uint32_t* out_bev, const salve_tile_job_t* jobs_a, const salve_tile_job_t* jobs_b,
                            const uint32_t* tiles_b, const int32_t* coef_y, const int32_t* coef_x, int32_t resize, int32_t crop, const float* lut,
                            void* out, int32_t out_c, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Verifier: early-fusion ResNet forward pass (fp16 MFMA, fp32 accumulation).
 * Stands behind salve/models/early_fusion.py:14-83 (EarlyFusionCEResnet), the torchvision trunk
 * selected by salve/models/resnet_factory.py:26-44, and the model build / checkpoint load of
 * salve/train_utils.py:205-242.  The host folds BatchNorm into the convolutions and describes the
 * network as a list of ops over a few activation buffers; the library executes the list.
 * ------------------------------------------------------------------------------------------------ */
#define SALVE_OP_CONV 0       /* out = relu?(conv(in) + bias (+ res)) ; NHWC fp16 */
#define SALVE_OP_MAXPOOL 1    /* 3x3 / stride 2 / pad 1 */
#define SALVE_OP_AVGPOOL_FC 2 /* global average pool + linear layer -> fp32 logits */
#define SALVE_NET_INPUT (-1)  /* buffer id of the network input */
#define SALVE_NO_BUF (-2)     /* "no residual" */

typedef struct {
    int32_t op;
    int32_t in_buf, out_buf, res_buf; /* activation buffer ids (SALVE_NET_INPUT / SALVE_NO_BUF) */
    int32_t Hi, Wi, Cin;              /* input  H, W, channels (channels padded to a multiple of 8) */
    int32_t Ho, Wo, Cout;             /* output H, W, channels (FC: Cout = number of classes) */
    int32_t KH, KW, stride, pad;      /* KW is the PADDED kernel width of the packed weights */
    int32_t relu, reserved;
    int64_t w_off;    /* CONV: element offset into the fp16 weight blob; FC: float offset of the weight in params */
    int64_t b_off;    /* float offset of the bias in params */
    int64_t ktab_off; /* CONV: offset into ktab; one int32 per 8 consecutive k: dy | dx << 8 | channel_offset << 16 */
    /* Optional second, point-wise source of a 1x1 / stride-1 CONV (in2_buf = SALVE_NO_BUF: none): the weight rows are
     * [Cin | Cin2] long and the k-tiles beyond Cin read Cin2 channels of buffer in2 (an [Hi2, Wi2, Cin2] image) at pixel
     * (oy * stride2, ox * stride2).  This is how the projection shortcut of a down-sampling bottleneck block
     * (torchvision `downsample` = 1x1 conv + BN) is folded into the block's last convolution: one GEMM over the
     * concatenated channels instead of a convolution, a tensor written and read back, and a residual add. */
    int32_t in2_buf, Cin2, stride2, Hi2, Wi2, reserved2;
} salve_resnet_op_t;

/* Kernel selection (salve_resnet_create's `flags`; 0 = the product's selection).  Every combination computes the same
 * network in the same k order with fp32 accumulation and one rounding per stored value: the logits are bit-identical, and
 * that is what these bits exist for -- the parity tests run a fused / streaming / 8-phase kernel against the plain
 * implicit-GEMM kernels it replaces.  The library reads NO environment variable (until ABI 4 it did). */
#define SALVE_RESNET_CONV_IGEMM_ONLY 1   /* conv_igemm_kernel for every convolution (no 8-phase kernel) */
#define SALVE_RESNET_CONV8_WHEREVER 2    /* the 8-phase 256 x 256 kernel wherever the shape fits, whatever the launch size */
#define SALVE_RESNET_ROUND_ROBIN_TILES 4 /* natural workgroup order instead of XCD-contiguous tiles */
#define SALVE_RESNET_NO_STEM_FUSE 8      /* 7x7 convolution and max-pool as two launches */
#define SALVE_RESNET_NO_BLOCK_FUSE 16    /* the 56 x 56 bottleneck blocks as three convolutions */
#define SALVE_RESNET_NO_PROJ_FUSE 32     /* ... only the first block of layer 1 (projection shortcut) */
#define SALVE_RESNET_NO_CHAIN 64         /* no expand_chain_kernel */
#define SALVE_RESNET_CHAIN_EXPAND_ONLY 128 /* expand_chain_kernel without the next block's first convolution */
#define SALVE_RESNET_CHAIN_16_WAVES 256  /* its 16-wave / 256-pixel-tile form for the 128-channel shapes */
#define SALVE_RESNET_CHAIN_NO_SPLIT 512  /* its 8-wave form for the 256-channel shapes too */
#define SALVE_RESNET_CHAIN_STORE_ALL 1024 /* every pixel of a stage's last block output is stored (default: only the even rows and columns
                                             that its one reader, the next stage's stride-2 projection shortcut, samples) */
#define SALVE_RESNET_NO_TRANSPOSED_TILES 2048 /* the fused 56 x 56 blocks with a fourth, half-empty tile column of 8 x 16 tiles instead of
                                             the transposed 16 x 8 tiles that cover the last 8 image columns exactly */
#define SALVE_RESNET_NO_NEXT_FUSE 4096   /* the last fused block of layer 1 without the next block's first 1x1 convolution as its fourth GEMM
                                             (with it, that block stores only the even pixels of its own output unless ..._CHAIN_STORE_ALL) */
#define SALVE_RESNET_ALL_FLAGS 8191      /* salve_resnet_create refuses any other bit */

/* Creates a handle that owns device copies of the (host) weight blobs.  NULL on failure.  flags: SALVE_RESNET_* (0). */
void* salve_resnet_create(int32_t num_layers, int32_t in_channels, const salve_resnet_op_t* ops, int32_t n_ops,
                          const void* weights_f16, size_t weights_bytes, const float* params_f32, size_t params_bytes,
                          const int32_t* ktab, size_t ktab_entries, int32_t flags);
void salve_resnet_destroy(void* handle);
int salve_resnet_num_layers(void* handle);
/* Device workspace needed for a batch (activation buffers). */
size_t salve_resnet_workspace_bytes(void* handle, int32_t batch);
/* input: device fp16 [batch, H, W, in_channels] (NHWC); logits: device float [batch, n_classes];
 * status: device int32 status word or NULL (SALVE_STATUS_FP16_RANGE). */
int salve_resnet_forward(void* handle, const void* input, int32_t batch, float* logits, void* workspace,
                         size_t workspace_bytes, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Verifier in fp32 (ABI 7): the reference's own precision, opt-in.
 * The reference evaluates the verifier in float32 with no AMP anywhere (salve/train_utils.py:18-41) through
 * salve/models/early_fusion.py:41-83.  The fp16 engine above stores weights and activations in fp16, which costs an
 * error relative to the logit and a range of 65504.  This second handle family runs the SAME op
 * program (salve_resnet_op_t rows, ktab, in2_buf projection shortcuts) with an fp32 weight blob, fp32 NHWC activations
 * and the exact fp32-input MFMA (v_mfma_f32_32x32x2_f32): one rounding per fp32 operation, no fp16 anywhere, NaN
 * propagated by ReLU / max-pool as torch does, no status bit for large magnitudes.  The fp16 engine and its flags are
 * unchanged.
 *   create:   ops / ktab exactly as for salve_resnet_create; CONV w_off is an element offset into weights_f32 (float
 *             [*], same packing order as the fp16 blob); in_channels = the REAL input channel count (6, 12, 18), whose
 *             padded form (a multiple of 8) must equal the Cin of the convolution that reads SALVE_NET_INPUT.
 *             flags must be 0 (anything else is refused).  NULL on failure (salve_last_error()).
 *   forward:  input = device float NCHW [batch, in_channels, H, W] -- the reference's torch.cat([x1..xn], 1) as it is;
 *             the engine's first launch pads and transposes it to NHWC inside the workspace.  logits: device float
 *             [batch, n_classes].  status: accepted for symmetry with salve_resnet_forward, never written.
 *   workspace_bytes counts the padded input copy and the activation buffers.
 * ------------------------------------------------------------------------------------------------ */
void* salve_resnet_f32_create(int32_t num_layers, int32_t in_channels, const salve_resnet_op_t* ops, int32_t n_ops,
                              const float* weights_f32, size_t weights_bytes, const float* params_f32, size_t params_bytes,
                              const int32_t* ktab, size_t ktab_entries, int32_t flags);
void salve_resnet_f32_destroy(void* handle);
size_t salve_resnet_f32_workspace_bytes(void* handle, int32_t batch);
int salve_resnet_f32_forward(void* handle, const float* input, int32_t batch, float* logits, void* workspace,
                             size_t workspace_bytes, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Verifier in bf16x3 (additive within ABI 7): the fp32 engine's program, input, activations and logits with the
 * convolutions' multiplications on the bf16 matrix cores, opt-in.
 * Everything above about the fp32 engine holds -- fp32 NCHW input, fp32 NHWC activations in the workspace (no storage
 * rounding), fp32 bias / residual / ReLU / pools / head, NaN propagated, no status bit -- except the convolution's products:
 * every fp32 operand x is split into two bf16 pieces,
 *     hi = bf16(x), round to nearest even;   lo = bf16(x - float(hi)), the subtraction being exact in fp32;
 *     NaN -> hi = NaN, lo = 0;   +-inf -> hi = +-inf, lo = 0 (inf - inf is never computed);
 *     a finite x whose rounding would give inf -> hi = the largest finite bf16 of its sign (lo takes the rest),
 * and a product a * w is computed as ah * wh + ah * wl + al * wh by three v_mfma_f32_32x32x16_bf16 into fp32
 * accumulators, in that order per k-step, without atomics or split-K: the same input gives the same bits on every run.
 * Activations are split on their way into LDS, weights once inside create (the caller's blob is the fp32 engine's).
 * bf16 has fp32's exponent range, so the fp32 engine's range is kept.  (An infinite activation can give NaN where one
 * fp32 product gives inf: ah * wl is inf * 0 for a weight whose lo piece is 0, and of the other sign where wl's is.)
 *   Error: a product loses three pieces (al * wl and the residue of each operand after its two pieces), each about
 *          2^-18 |a| |w| (worst case 2^-16: bf16 keeps 8 significand bits; the pieces have mixed signs and average over K).
 *          One convolution output is held to (3 * 2^-18 + 4e-6) * (sum |a| |w| + |bias| (+ |residual|)) of the exact sum,
 *          4e-6 being the allowance of the fp32 accumulation as for the fp32 engine; an engine that loses a cross term
 *          exceeds that 11 x or more.  Logits of the released ResNet-152 configurations (|logit| about 11) stay within
 *          the absolute 1e-3 contract (emulated: 5.3e-5).
 *   create: arguments and refusals of salve_resnet_f32_create, whose checks it runs (refusals of the program carry that
 *           entry's name); flags must be 0.  The handle is used with salve_resnet_f32_workspace_bytes,
 *           salve_resnet_f32_forward and salve_resnet_f32_destroy.
 * ------------------------------------------------------------------------------------------------ */
void* salve_resnet_bf16x3_create(int32_t num_layers, int32_t in_channels, const salve_resnet_op_t* ops, int32_t n_ops,
                                 const float* weights_f32, size_t weights_bytes, const float* params_f32, size_t params_bytes,
                                 const int32_t* ktab, size_t ktab_entries, int32_t flags);

/* ------------------------------------------------------------------------------------------------
 * Training convolutions in fp32 (additive within ABI 7): forward, backward-data and backward-weight of ONE convolution, the
 * hot path of a training step of the verifier (the reference trains in fp32: scripts/train.py and the configs under salve/configs).
 * Everything around them -- BatchNorm with batch statistics, ReLU, residual adds, pooling, the fc layer, the loss and Adam --
 * is the caller's (torch autograd: salve_amd/models/trainable.py).
 *   Layouts: activations NHWC fp32 [batch, H, W, C] (torch's channels_last memory), weights [Cout][KH][KW][Cin] fp32.  Every
 *            pointer is a device pointer, 16-byte aligned.  Cin counts the caller's zero-padded channels: the stem's 6 / 12 / 18
 *            input channels are passed as 8 / 16 / 24.
 *   Shapes:  1 x 1 (pad 0) and 3 x 3 (pad 1) with stride 1 or 2, Cin and Cout 64..2048 in steps of 64; the 7 x 7 / 2 / pad 3 stem
 *            with Cin 8, 16 or 24 and Cout 64..2048 in steps of 64.  Ho, Wo must be the convolution's output size.  Anything
 *            else: SALVE_ERR_BAD_ARG.  The stem's backward-data is SALVE_ERR_UNSUPPORTED: the network input needs no gradient.
 *   Workspace: salve_conv_f32_workspace_bytes(d, pass) bytes of device memory (0 = the descriptor or pass is refused); it holds
 *            nothing from one call to the next.
 *   Results: forward / backward-data are one fp32 fma chain per output; backward-weight splits the batch * Ho * Wo pixels over
 *            workgroups into fp32 partial sums that are added in a fixed order -- no atomics, the same inputs give bit-identical
 *            dW.  All three overwrite their output (no accumulation into it).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t batch, Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, stride, pad;
} salve_conv_desc_t;
#define SALVE_CONV_FWD 0
#define SALVE_CONV_DGRAD 1
#define SALVE_CONV_WGRAD 2
size_t salve_conv_f32_workspace_bytes(const salve_conv_desc_t* d, int32_t pass);
/* y [batch, Ho, Wo, Cout] = conv(x [batch, Hi, Wi, Cin], w): no bias, no activation. */
int salve_conv_f32_forward(const salve_conv_desc_t* d, const float* x, const float* w, float* y, void* ws, size_t ws_bytes, void* stream);
/* dx [batch, Hi, Wi, Cin] = d(sum dy . y) / dx for dy [batch, Ho, Wo, Cout]. */
int salve_conv_f32_backward_data(const salve_conv_desc_t* d, const float* dy, const float* w, float* dx, void* ws, size_t ws_bytes,
                                 void* stream);
/* dw [Cout][KH][KW][Cin] = sum over pixels of dy (x) the input patch. */
int salve_conv_f32_backward_weight(const salve_conv_desc_t* d, const float* x, const float* dy, float* dw, void* ws, size_t ws_bytes,
                                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training convolutions in bf16 (additive within ABI 7): opt-in mixed-precision training.  The same three passes, descriptors,
 * layouts, accepted shapes and refusals as salve_conv_f32_* above, word for word (SALVE_ERR_BAD_ARG for any other shape,
 * SALVE_ERR_UNSUPPORTED for the stem's backward-data, 0 workspace bytes for a refused descriptor or pass).  bf16 values are passed
 * as uint16_t bit patterns (the upper half of the fp32 bits).  The caller keeps fp32 master weights and hands over their bf16
 * copy; the reference trains in fp32, so this is never the default (salve_amd/models/trainable.py: set_train_precision).
 *   Arithmetic: bf16 operands on the bf16 matrix cores (v_mfma_f32_16x16x32_bf16), fp32 accumulation.  forward / backward-data
 *            round each output ONCE to bf16 (round to nearest even, NaN stays NaN); backward-weight writes fp32 dW and never
 *            accumulates in bf16: bf16 x bf16 products are exact in fp32, the pixels are split over workgroups into fp32 partial
 *            sums that are added in a fixed order -- no atomics, the same inputs give bit-identical dW.
 *   All three overwrite their output (no accumulation into it); the workspace holds nothing from one call to the next.
 * ------------------------------------------------------------------------------------------------ */
size_t salve_conv_bf16_workspace_bytes(const salve_conv_desc_t* d, int32_t pass);
/* y [batch, Ho, Wo, Cout] bf16 = conv(x [batch, Hi, Wi, Cin] bf16, w [Cout][KH][KW][Cin] bf16): no bias, no activation. */
int salve_conv_bf16_forward(const salve_conv_desc_t* d, const uint16_t* x, const uint16_t* w, uint16_t* y, void* ws, size_t ws_bytes,
                            void* stream);
/* dx [batch, Hi, Wi, Cin] bf16 = d(sum dy . y) / dx for dy [batch, Ho, Wo, Cout] bf16. */
int salve_conv_bf16_backward_data(const salve_conv_desc_t* d, const uint16_t* dy, const uint16_t* w, uint16_t* dx, void* ws, size_t ws_bytes,
                                  void* stream);
/* dw [Cout][KH][KW][Cin] fp32 = sum over pixels of dy (x) the input patch (bf16 operands). */
int salve_conv_bf16_backward_weight(const salve_conv_desc_t* d, const uint16_t* x, const uint16_t* dy, float* dw, void* ws, size_t ws_bytes,
                                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training BatchNorm with fused ReLU and residual add (additive within ABI 7): opt-in, fp32 and bf16.
 * The reference normalises with torchvision's nn.BatchNorm2d inside its ResNet trunk (salve/models/early_fusion.py:69-76:
 * resnet.bn1 + relu, then layer1..layer4, whose blocks end in bn + identity add + relu) and trains it with batch statistics
 * (scripts/train.py).  These entries compute one BatchNorm2d in train mode -- or, with SALVE_BN_EVAL, on the running
 * statistics -- together with the residual add and the ReLU that follow it, and the matching backward pass
 * (salve_amd/models/trainable.py: BatchNormHipFunction; the default stays torch's BatchNorm).
 *   Layout:  activations [rows, C], rows = batch * H * W, channel innermost (NHWC), fp32 or bf16 bit patterns (uint16_t, the upper
 *            half of the fp32 bits); device pointers, 16-byte aligned.  gamma, beta, running_mean, running_var, save_mean,
 *            save_invstd, dgamma, dbeta: device float [C], always fp32.
 *   Shapes:  C a multiple of 8 from 8 to 4096, rows >= 2; flags a combination of SALVE_BN_*; eps >= 0, momentum in [0, 1].
 *            Anything else, an unknown flag bit included: SALVE_ERR_BAD_ARG, and 0 workspace bytes.
 *   forward, train:  per channel over the rows mean and biased variance, save_mean = mean, save_invstd = 1 / sqrt(var + eps);
 *            running = (1 - momentum) * running + momentum * batch statistic with the UNBIASED variance (torch's definitions;
 *            running_mean / running_var may be NULL: no update).  y = gamma * (x - mean) * invstd + beta, then + residual with
 *            SALVE_BN_ADD, then max(0, .) with SALVE_BN_RELU; the bf16 entry rounds y once.  residual is read only with
 *            SALVE_BN_ADD (else it may be NULL).
 *   forward, eval (SALVE_BN_EVAL):  the same y from running_mean and 1 / sqrt(running_var + eps); nothing else is read or
 *            written (save_mean / save_invstd may be NULL).
 *   backward (train only; with SALVE_BN_EVAL: SALVE_ERR_UNSUPPORTED):  g = dy, or with SALVE_BN_RELU g = dy where the saved
 *            forward output y > 0 and 0 elsewhere (y is read only then).  dbeta = sum g, dgamma = sum g * xhat with
 *            xhat = (x - save_mean) * save_invstd, dx = gamma * save_invstd * (g - dbeta / rows - xhat * dgamma / rows), and with
 *            SALVE_BN_ADD dres = g, the gradient of the residual branch (dres may be NULL otherwise).
 *   Arithmetic: fp32 throughout, also for bf16 activations.  The statistics are Welford sums per thread combined with Chan's
 *            formula in a fixed order (never E[x^2] - E[x]^2); dgamma / dbeta are fp32 partial sums per workgroup added in a
 *            fixed order.  No atomics: the same inputs give bit-identical results.  Element offsets are 64-bit.
 *   Workspace: salve_bn_workspace_bytes(d, pass) bytes of device memory (0 = the descriptor or pass is refused); it holds nothing
 *            from one call to the next.  All outputs are overwritten.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t rows, C, flags;
    float eps, momentum;
} salve_bn_desc_t;
#define SALVE_BN_RELU 1   /* max(0, .) after the normalisation (and after the residual add) */
#define SALVE_BN_ADD 2    /* + residual before the ReLU */
#define SALVE_BN_EVAL 4   /* normalise with the running statistics; forward only */
#define SALVE_BN_FWD 0
#define SALVE_BN_BWD 1
size_t salve_bn_workspace_bytes(const salve_bn_desc_t* d, int32_t pass);
int salve_bn_f32_forward(const salve_bn_desc_t* d, const float* x, const float* residual, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float* y, float* save_mean, float* save_invstd, void* ws, size_t ws_bytes,
                         void* stream);
int salve_bn_f32_backward(const salve_bn_desc_t* d, const float* dy, const float* x, const float* y, const float* gamma, const float* save_mean,
                          const float* save_invstd, float* dx, float* dres, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);
int salve_bn_bf16_forward(const salve_bn_desc_t* d, const uint16_t* x, const uint16_t* residual, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, uint16_t* y, float* save_mean, float* save_invstd, void* ws, size_t ws_bytes,
                          void* stream);
int salve_bn_bf16_backward(const salve_bn_desc_t* d, const uint16_t* dy, const uint16_t* x, const uint16_t* y, const float* gamma,
                           const float* save_mean, const float* save_invstd, uint16_t* dx, uint16_t* dres, float* dgamma, float* dbeta, void* ws,
                           size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Synchronised training BatchNorm: the passes of the entries above as entries of their own (additive within ABI 7): opt-in.
 * `world` data-parallel ranks each hold some rows of one batch; between the passes every rank gathers the others' per-channel
 * results (one all-gather forward, one backward: salve_amd/models/trainable.py: SyncBatchNormHipFunction, --sync-bn), so that
 * every BatchNorm normalises over the rows of ALL ranks.  The kernels are the fused entries' own; no entry adds a pass over x.
 *   Descriptor: salve_bn_desc_t as above, except that rows is THIS RANK's rows and may be 0 or 1 (a rank that got little or none
 *            of a short batch: nothing is launched on the activations, outputs per channel are still written).  SALVE_BN_RELU and
 *            SALVE_BN_ADD as above; SALVE_BN_EVAL: SALVE_ERR_UNSUPPORTED from every entry here (the eval form reads no batch
 *            statistics).  The other refusals are the fused entries'.  world: 1 .. SALVE_BN_MAX_WORLD.
 *   salve_bn_*_stats:  partial float [2][C] = the mean and M2 = sum (x - mean)^2 of this rank's rows: the fused forward's
 *            statistics pass, the same Welford + Chan arithmetic in the same order.  rows == 0 writes zeros.
 *   salve_bn_combine:  partials float [world][2][C], the ranks' `partial` in rank order; rows: HOST int64 [world], the ranks' row
 *            counts (read before the call returns; their sum must be at least 2).  The partials are combined with Chan's formula
 *            in rank order, ranks without rows skipped; mean[C], invstd[C] = 1 / sqrt(M2 / R + eps) over the R rows of all ranks,
 *            running = (1 - momentum) * running + momentum * statistic with the unbiased variance M2 / (R - 1) (running_mean /
 *            running_var may be NULL).  d->rows is not read.  With world == 1 mean, invstd and the running statistics are the
 *            fused forward's save_mean, save_invstd and update, bit for bit.  Every rank that combines the same partials gets the
 *            same bits.
 *   salve_bn_*_apply:  y from x, residual, gamma, beta and the combined mean and invstd: the fused forward's apply pass.
 *   salve_bn_*_backward_reduce:  sums float [2][C] = sum g, sum g * xhat over this rank's rows (g masked by y > 0 with
 *            SALVE_BN_RELU; xhat from the combined mean and invstd): the fused backward's first pass.  sums[0] is this rank's
 *            share of dbeta, sums[1] of dgamma.  rows == 0 writes zeros.
 *   salve_bn_*_backward_apply:  sums float [world][2][C], the ranks' sums in rank order, which the kernel adds in that order
 *            itself; total_rows = R.  dx = gamma * invstd * (g - sum g / R - xhat * sum (g * xhat) / R), dres = g with
 *            SALVE_BN_ADD.  With world == 1 dx and dres are the fused backward's, bit for bit.
 *   Workspace: salve_bn_workspace_bytes(d, SALVE_BN_STATS) for salve_bn_*_stats, (d, SALVE_BN_BWD_REDUCE) for
 *            salve_bn_*_backward_reduce; the other entries take none.  No atomics; element offsets are 64-bit.
 * ------------------------------------------------------------------------------------------------ */
#define SALVE_BN_MAX_WORLD 64
#define SALVE_BN_STATS 16
#define SALVE_BN_BWD_REDUCE 17
int salve_bn_f32_stats(const salve_bn_desc_t* d, const float* x, float* partial, void* ws, size_t ws_bytes, void* stream);
int salve_bn_bf16_stats(const salve_bn_desc_t* d, const uint16_t* x, float* partial, void* ws, size_t ws_bytes, void* stream);
int salve_bn_combine(const salve_bn_desc_t* d, const float* partials, const int64_t* rows, int32_t world, float* running_mean, float* running_var,
                     float* mean, float* invstd, void* stream);
int salve_bn_f32_apply(const salve_bn_desc_t* d, const float* x, const float* residual, const float* gamma, const float* beta, const float* mean,
                       const float* invstd, float* y, void* stream);
int salve_bn_bf16_apply(const salve_bn_desc_t* d, const uint16_t* x, const uint16_t* residual, const float* gamma, const float* beta,
                        const float* mean, const float* invstd, uint16_t* y, void* stream);
int salve_bn_f32_backward_reduce(const salve_bn_desc_t* d, const float* dy, const float* x, const float* y, const float* mean, const float* invstd,
                                 float* sums, void* ws, size_t ws_bytes, void* stream);
int salve_bn_bf16_backward_reduce(const salve_bn_desc_t* d, const uint16_t* dy, const uint16_t* x, const uint16_t* y, const float* mean,
                                  const float* invstd, float* sums, void* ws, size_t ws_bytes, void* stream);
int salve_bn_f32_backward_apply(const salve_bn_desc_t* d, const float* dy, const float* x, const float* y, const float* gamma, const float* mean,
                                const float* invstd, const float* sums, int32_t world, int64_t total_rows, float* dx, float* dres, void* stream);
int salve_bn_bf16_backward_apply(const salve_bn_desc_t* d, const uint16_t* dy, const uint16_t* x, const uint16_t* y, const float* gamma,
                                 const float* mean, const float* invstd, const float* sums, int32_t world, int64_t total_rows, uint16_t* dx,
                                 uint16_t* dres, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Adam over every parameter tensor in one launch, with the bf16 copy of a weight written alongside (additive within ABI 7):
 * opt-in.  The reference trains with torch.optim.Adam(lr, weight_decay) (salve/train_utils.py:173-180) under a poly schedule
 * that changes lr every iteration (scripts/train.py).  This entry performs one step of that optimiser (amsgrad=False,
 * maximize=False, L2 weight decay added to the gradient) for a list of fp32 tensors (salve_amd/optim.py: HipAdam; the default
 * stays torch.optim.Adam).
 *   Table:   device salve_adam_segment_t [n_segments], one record per parameter tensor, 8-byte aligned:
 *              param, grad, exp_avg, exp_avg_sq   device float [n], 4-byte aligned (16-byte aligned tensors take the 16-byte
 *                                                 path); param, exp_avg and exp_avg_sq are updated in place, grad is read only
 *              shadow_bf16                        NULL, or device uint16_t [n]: receives the new param as bf16 bit patterns,
 *                                                 rounded to nearest even (+-inf kept, NaN stored as 0x7FC0)
 *              n                                  elements (64-bit)
 *              step_size                          lr / (1 - beta1^t), t = this tensor's step count after the step
 *              sqrt_bc2                           sqrt(1 - beta2^t)
 *              beta1, beta2, eps, weight_decay    the group's hyperparameters
 *              one_minus_beta1, one_minus_beta2   1 - beta1, 1 - beta2
 *            The scalars are per segment (torch keeps a step count per parameter, groups may differ in lr); the caller computes
 *            each in double and rounds it to float once.  Nothing is a compiled constant: lr changes every step.
 *   Chunks:  device salve_adam_chunk_t [n_chunks], one per workgroup: `segment` indexes the table, `offset` is the first element
 *            of the chunk, a multiple of SALVE_ADAM_CHUNK below that segment's n; the chunk ends SALVE_ADAM_CHUNK elements later
 *            or at n.  A segment of n elements takes ceil(n / SALVE_ADAM_CHUNK) chunks, each listed once (a chunk listed twice
 *            is a race; an element no chunk covers is not updated).
 *   Update:  g += weight_decay * p (skipped for weight_decay == 0); m += (1 - beta1) * (g - m); v = v * beta2 + (1 - beta2) * g * g;
 *            p -= step_size * m / (sqrt(v) / sqrt_bc2 + eps).  fp32, in the operation order of torch's fp32 Adam on the CPU (its
 *            three fused multiply-adds included; sqrt and the divisions correctly rounded), no atomics: the same inputs give
 *            bit-identical outputs.  One launch, whatever n_segments; n_chunks == 0 launches nothing.
 *   Checks:  SALVE_ERR_BAD_ARG on a null table, a null chunk map with n_chunks > 0, negative counts or misaligned tables.  The
 *            tables live on the device, so their contents can be checked only through host_table / host_chunk_map: host copies
 *            of the same bytes (e.g. the staging buffer), either may be NULL.  With host_table, a segment with a null or
 *            misaligned pointer or n < 0 is SALVE_ERR_BAD_ARG; with both, so is a chunk that names a segment outside the table or
 *            an offset that is negative, not a multiple of SALVE_ADAM_CHUNK or not below its segment's n.  On the device a chunk
 *            outside its table or segment is skipped, and no chunk reaches past its segment's n.
 *   The caller owns every buffer; the library allocates nothing and keeps nothing.  The launch is asynchronous on `stream`: the
 *   device tables must stay unchanged until it has run (the host copies are read before the call returns).
 * ------------------------------------------------------------------------------------------------ */
#define SALVE_ADAM_CHUNK 4096   /* elements a workgroup updates */
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    uint16_t* shadow_bf16;
    int64_t n;
    float step_size, sqrt_bc2, beta1, beta2, eps, weight_decay, one_minus_beta1, one_minus_beta2;
} salve_adam_segment_t; /* 80 bytes */
typedef struct {
    int32_t segment, reserved;
    int64_t offset;
} salve_adam_chunk_t; /* 16 bytes */
int salve_adam_step(const salve_adam_segment_t* table, int32_t n_segments, const salve_adam_chunk_t* chunk_map, int32_t n_chunks,
                    const salve_adam_segment_t* host_table, const salve_adam_chunk_t* host_chunk_map, void* stream);

/* ------------------------------------------------------------------------------------------------
 * A flat bucket over any number of fp32 tensors, packed or unpacked in one launch (additive within ABI 7): the buffer that
 * data-parallel training all-reduces once per step (salve_amd/dist_train.py: FlatBucket; the reference wraps its model in
 * nn.DataParallel, salve/train_utils.py:214-215).
 *     salve_flat_pack:    flat[offset_s + i] = tensor_s[i] * scale        salve_flat_unpack:  tensor_s[i] = flat[offset_s + i] * scale
 *   Table:   device salve_flat_segment_t [n_segments], 8-byte aligned, one record per tensor:
 *              tensor   address of device float [n], 4-byte aligned (a 16-byte aligned tensor takes the 16-byte path)
 *              n        elements (64-bit), 0 allowed
 *              offset   the segment's first element in `flat`: a multiple of 4, so that the flat side of every segment is 16-byte
 *                       aligned.  Offsets ascend and segments do not overlap; the elements between offset + n and the next
 *                       segment's offset are padding that neither entry reads or writes.
 *   Chunks:  device salve_adam_chunk_t [n_chunks], one per workgroup of SALVE_ADAM_CHUNK elements, as salve_adam_step takes it: the
 *            segments' chunks in table order, ceil(n / SALVE_ADAM_CHUNK) each, offsets ascending; an empty segment has none.
 *   flat:    device float [flat_elems], 16-byte aligned.
 *   scale:   1.0f copies 32-bit words and multiplies nothing: NaN payloads, infinities, -0 and denormals arrive unchanged.  Any
 *            other value: one fp32 multiply per element.
 *   Checks:  all on the host, before the launch, from host_table / host_chunk_map -- host copies of the same bytes, REQUIRED here
 *            (a segment past flat_elems would write outside the buffer).  SALVE_ERR_BAD_ARG: negative counts; a null or misaligned
 *            table, map or flat buffer; n < 0; an offset that is negative or not a multiple of 4; descending offsets or overlapping
 *            segments; offset + n > flat_elems; a chunk map that is not exactly the table's; a null tensor (or flat) with n > 0; a
 *            tensor address that is not 4-byte aligned.  Nothing is written then.  n_segments == 0: SALVE_OK, nothing is launched.
 *   No atomics; every element is moved by exactly one thread.  The caller owns every buffer.  The launch is asynchronous on
 *   `stream`: the device tables must stay unchanged until it has run.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    uint64_t tensor;
    int64_t n;
    int64_t offset;
} salve_flat_segment_t; /* 24 bytes */
int salve_flat_pack(const salve_flat_segment_t* table, int32_t n_segments, const salve_adam_chunk_t* chunk_map, int32_t n_chunks,
                    const salve_flat_segment_t* host_table, const salve_adam_chunk_t* host_chunk_map, float* flat, int64_t flat_elems, float scale,
                    void* stream);
int salve_flat_unpack(const salve_flat_segment_t* table, int32_t n_segments, const salve_adam_chunk_t* chunk_map, int32_t n_chunks,
                      const salve_flat_segment_t* host_table, const salve_adam_chunk_t* host_chunk_map, float* flat, int64_t flat_elems, float scale,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * The classifier head of a training step with its loss and accuracy counts on the device (additive within ABI 7): opt-in, fp32
 * and bf16.  The reference ends its network in resnet.avgpool, flatten and fc (salve/models/early_fusion.py:78-83), forms
 * softmax probabilities on a clone of the logits and the cross-entropy loss (salve/train_utils.py:18-41), and feeds the arg-max
 * of the probabilities to a per-class accuracy meter on the host (salve/utils/avg_meter.py: intersection / target counts per
 * class).  These entries compute all of that in one forward call and its gradient in one backward call
 * (salve_amd/models/trainable.py: ClassifierHeadHipFunction, salve_amd/evaluate.py: DeviceClassMeter; the default stays torch).
 *   Layout:  x and dx [B, HW, C], the channel innermost (NHWC), fp32 or bf16 bit patterns (uint16_t), device pointers, 16-byte
 *            aligned.  weight [K, C] and bias [K] (fc), pooled [B, C], logits, probs, dlogits [B, K], dw [K, C], db [K]: device
 *            float, always fp32 (weight and pooled 16-byte aligned).  target: device int64 [B].  loss, grad_loss: one device float.
 *   Shapes:  1 <= B <= 65535, 1 <= HW <= 1024, C a multiple of 8 from 8 to 4096, 2 <= K <= 16 (SALVE_HEAD_MAX_CLASSES); flags 0 or
 *            SALVE_HEAD_ACCUMULATE_LOSS.  Anything else, a misaligned or null pointer included: SALVE_ERR_BAD_ARG before any
 *            launch, and 0 workspace bytes for a refused descriptor or pass.
 *   forward: pooled = the mean over HW (summed in fp32, divided by HW once); logits = pooled . weight^T + bias; probs = the
 *            max-subtracted softmax of the logits; loss = the mean over the batch of -log_softmax[target] (cross_entropy's default
 *            reduction).  The meter record (may be NULL: no counts) is updated in place: total[c] += rows whose target is c,
 *            correct[c] += those whose prediction is c too -- the prediction is the arg-max of the probs just written, the first
 *            index winning a tie, as torch.argmax(probs, 1) -- and, with SALVE_HEAD_ACCUMULATE_LOSS only, loss_sum +=
 *            (double)loss * B and loss_rows += B.  A row whose target lies outside [0, K) contributes no loss, no gradient and no
 *            count, increments bad_targets and indexes nothing.  A NaN in x reaches loss and loss_sum as NaN.
 *   backward (from the forward's pooled and probs): dlogits = (probs - onehot(target)) * (*grad_loss / B), dw = dlogits^T . pooled,
 *            db = the column sums of dlogits, dx = (dlogits . weight) / HW broadcast over the HW rows, rounded once for bf16.
 *   Arithmetic: fp32 sums for pooled, logits, dw, db and dx; the few scalars per row (softmax, the row's loss, dlogits) and the sum
 *            of the row losses are formed in double and rounded to fp32 once.  Every reduction (over HW, over C, over B, into the
 *            record) has a fixed order and there are no floating-point atomics: the same inputs give bit-identical results.
 *            Element offsets are 64-bit.
 *   Workspace: salve_head_workspace_bytes(d, pass) bytes of device memory; it holds nothing from one call to the next.  The caller
 *            owns every buffer and zeroes the meter record when a pass begins.  Asynchronous on `stream`; calls on one stream update
 *            the record one after the other.  All other outputs are overwritten.
 * ------------------------------------------------------------------------------------------------ */
#define SALVE_HEAD_MAX_CLASSES 16
typedef struct {
    int32_t B, HW, C, K, flags;
} salve_head_desc_t;
typedef struct {
    int64_t total[SALVE_HEAD_MAX_CLASSES];
    int64_t correct[SALVE_HEAD_MAX_CLASSES];
    double loss_sum;
    int64_t loss_rows;
    int64_t bad_targets;
} salve_head_meter_t; /* 280 bytes */
#define SALVE_HEAD_ACCUMULATE_LOSS 1 /* add this batch to loss_sum / loss_rows (training batches) */
#define SALVE_HEAD_FWD 0
#define SALVE_HEAD_BWD 1
size_t salve_head_workspace_bytes(const salve_head_desc_t* d, int32_t pass);
int salve_head_f32_forward(const salve_head_desc_t* d, const float* x, const float* weight, const float* bias, const int64_t* target, float* pooled,
                           float* logits, float* probs, float* loss, salve_head_meter_t* meter, void* ws, size_t ws_bytes, void* stream);
int salve_head_bf16_forward(const salve_head_desc_t* d, const uint16_t* x, const float* weight, const float* bias, const int64_t* target, float* pooled,
                            float* logits, float* probs, float* loss, salve_head_meter_t* meter, void* ws, size_t ws_bytes, void* stream);
int salve_head_f32_backward(const salve_head_desc_t* d, const float* pooled, const float* probs, const int64_t* target, const float* weight,
                            const float* grad_loss, float* dlogits, float* dw, float* db, float* dx, void* ws, size_t ws_bytes, void* stream);
int salve_head_bf16_backward(const salve_head_desc_t* d, const float* pooled, const float* probs, const int64_t* target, const float* weight,
                             const float* grad_loss, float* dlogits, float* dw, float* db, uint16_t* dx, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The reference's JPEG hop on the device (additive within ABI 7): opt-in.  The reference writes every BEV render and layout image
 * with imageio.imwrite(path.jpg) -- Pillow over libjpeg: baseline, quality 75, 4:2:0 (bev_rendering_utils.py:629-630) -- and its
 * data set decodes the files again (zind_data.py:306-315).  salve_bev_jpeg_roundtrip replaces n images by decode(encode(image))
 * with libjpeg's defaults, bit for bit, without an entropy coder or a file (quantised coefficients of 8-bit baseline data always fit
 * the code range, so the decoded pixels depend on the coefficients alone).
 *   Layout:  bev_in, bev_out: device uint32 [n, h, w] holding 0x00BBGGRR -- salve_bev_densify's out_bev, salve_layout_rasterise's
 *            out, what every tile entry reads.  bev_out == bev_in is allowed (no other overlap); the top byte is written as 0.
 *            qtab: HOST uint16 [2][64], the luma and the chroma quantisation table in natural (row-major) order, read before
 *            the call returns (salve_amd/jpeg.py: quality_tables).
 *   Stages:  RGB -> YCbCr (16-bit fixed point); right / bottom edges replicated to whole blocks as libjpeg does it (chroma: rows to
 *            a whole row group and columns to whole blocks before downsampling, the downsampled rows to whole blocks after it); h2v2
 *            downsampling with the alternating 1, 2 bias; slow-integer forward DCT of the level-shifted samples; quantisation by
 *            q << 3, magnitude rounded half up, sign restored (exact 32-bit integer division); dequantisation; slow-integer inverse
 *            DCT with its range limit; h2v2 "fancy" triangle upsampling (replication where the image is at most 4 pixels wide, as
 *            libjpeg); YCbCr -> RGB with the range limit.  Integer arithmetic only, no atomics, one writer per output: the same
 *            inputs give the same bits.  Offsets are 64-bit.
 *   Checks:  SALVE_ERR_BAD_ARG (and 0 workspace bytes from the size query) on null pointers, n <= 0, n > 65535, h or w outside
 *            [1, 4096], a table entry outside [1, 255], images that are not 4-byte aligned, a workspace smaller than
 *            salve_bev_jpeg_roundtrip_workspace_bytes(n, h, w) or not 16-byte aligned.
 *   Workspace: the decoded luma and half-resolution chroma planes, 1.5 bytes per pixel of the images rounded up to whole 16 x 16
 *            MCUs; it holds nothing from one call to the next.  Two launches, asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------------ */
size_t salve_bev_jpeg_roundtrip_workspace_bytes(int32_t n, int32_t h, int32_t w);
int salve_bev_jpeg_roundtrip(const uint32_t* bev_in, uint32_t* bev_out, int32_t n, int32_t h, int32_t w, const uint16_t* qtab, void* ws,
                             size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The reference's JPEG FILES from the device (additive within ABI 7): opt-in.  salve_bev_jpeg_encode leaves, for each of n images,
 * the entropy-coded scan of the file Pillow's `save(path, quality=q)` writes (libjpeg: baseline, 4:2:0, the standard Huffman
 * tables of ITU-T T.81 Annex K, one interleaved scan, no restart interval), byte for byte: the forward chain of
 * salve_bev_jpeg_roundtrip (the same device functions), then jchuff.c's encode_one_block -- DC differences per component in scan
 * order, (run, size) symbols in zigzag order with ZRL and EOB, bits most significant first, the last byte padded with 1-bits, a
 * 0x00 stuffed behind every 0xFF.  The file is header + scan + FF D9; the 623 header bytes depend on h, w and the tables only and
 * are the host's (salve_amd/jpeg.py: file_header, file_bytes).
 *   bev         device uint32 [n, h, w] holding 0x00BBGGRR, as for salve_bev_jpeg_roundtrip; only read
 *   qtab        HOST uint16 [2][64], luma and chroma table in natural order, read before the call returns
 *   scan        device bytes: image i's scan starts at scan + i * scan_stride (stuffed and padded; no header, no EOI)
 *   scan_bytes  device int32 [n]: the scan's length in bytes
 *   Capacity:   salve_bev_jpeg_encode_max_bytes(h, w) bounds the scan of ANY content: a block codes to at most 11 + 11 bits of DC
 *               (the longest DC code plus category 11's value bits) and 63 x (16 + 10) bits of AC (the longest AC code plus category
 *               10's value bits per coefficient; with table entries >= 1, 8-bit samples give no larger category, and a ZRL's 11 bits
 *               per 16 zeros and the EOB cost less than the coefficients they replace), 1660 bits; six blocks per 16 x 16 MCU are 1245
 *               bytes, and stuffing at most doubles them: 2490 bytes per MCU, rounded up to a multiple of 4.  A caller may pass a
 *               SMALLER scan_stride (real scans are a small fraction of the bound).  If image i needs more than scan_stride bytes,
 *               scan_bytes[i] still holds the NEEDED length, nothing is written outside the image's slot, no status bit is set and
 *               the other images are complete: the caller sees scan_bytes[i] > scan_stride and encodes that image another way.
 *               Bytes of a slot beyond the scan's length are not written.
 *   Checks:     SALVE_ERR_BAD_ARG (and 0 from the two size queries) on null pointers, n <= 0, n > 65535, h or w outside [1, 4096],
 *               a table entry outside [1, 255], bev or scan_bytes not 4-byte aligned, a workspace smaller than
 *               salve_bev_jpeg_encode_workspace_bytes(n, h, w) or not 16-byte aligned, scan_stride 0 or not a multiple of 4.
 *   Workspace:  per block 128 bytes of coefficients (int16, zigzag order, MCU-interleaved) and a 4-byte length / bit offset; the
 *               unstuffed bit stream at its bound (1245 bytes per MCU); a counter per 1024 bytes of it.  About 2.1 MB per 501 x 501
 *               image.  It needs no initialisation and holds nothing from one call to the next.
 *   Eight launches, asynchronous on `stream`.  32-bit integer arithmetic, vector stores and vector atomics (bit-wise OR into zeroed
 *   words: no dependence on order): the same input gives the same bytes.
 * ------------------------------------------------------------------------------------------------ */
size_t salve_bev_jpeg_encode_workspace_bytes(int32_t n, int32_t h, int32_t w);
size_t salve_bev_jpeg_encode_max_bytes(int32_t h, int32_t w);
int salve_bev_jpeg_encode(const uint32_t* bev, int32_t n, int32_t h, int32_t w, const uint16_t* qtab, uint8_t* scan, size_t scan_stride,
                          int32_t* scan_bytes, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The tile data set's JPEG FILES decoded on the device, in whole batches (additive within ABI 7): opt-in.  The reference trains and
 * evaluates from rendered tiles on disk and decodes every file with Pillow (zind_data.py:306-315).  salve_bev_jpeg_decode decodes n
 * images of ONE size that SHARE their tables -- baseline: 8-bit, three components, 4:2:0, one interleaved scan (MCU = Y0 Y1 Y2 Y3 Cb
 * Cr), no restart interval -- to the pixels Pillow's decoder gives (libjpeg: slow-integer inverse DCT, fancy upsampling), bit for bit.
 * The host parses the headers (salve_amd/jpeg.py: parse_file) and hands over the entropy-coded scans as they stand in the files.
 *   scans        device bytes, scans_size of them.  Image i is the stuffed, padded scan at scans + scan_offset[i], scan_bytes[i] long:
 *                no header, no EOI, any byte alignment.  The caller leaves SALVE_JPEG_SCAN_PADDING (16) bytes behind the last scan:
 *                scan_offset[i] + scan_bytes[i] + 16 <= scans_size for every image, else the image is not read at all and reports
 *                SALVE_JPEG_BAD_SLOT.  (The decoder itself reads no byte at or behind scan_offset[i] + scan_bytes[i].)
 *   scan_offset  device int64 [n];  scan_bytes  device int32 [n] (0 is allowed: the image reports SALVE_JPEG_TRUNCATED)
 *   qtab         HOST uint16 [2][64]: the luma and the chroma quantisation table of the files' DQT segments in NATURAL order
 *   huffman      HOST bytes [4][272]: DC luma, AC luma, DC chroma, AC chroma, each the 16 BITS and 256 HUFFVAL bytes of a DHT segment
 *                (HUFFVAL zero-filled behind its last symbol).  Both are read before the call returns.
 *   bev_out      device uint32 [n, h, w], 0x00BBGGRR: what every tile entry reads
 *   image_status device int32 [n]: 0, or the SALVE_JPEG_* bits of what was wrong with the image's scan.  Always written.
 *   Entropy stage (ITU-T T.81 F.2.2), one wavefront per image: the lanes stage the scan into LDS in coalesced runs; the 0x00 stuffed
 *                behind a 0xFF is dropped inline; the symbol loop is wave-uniform; codes are looked up in a 9-bit look-ahead table in
 *                LDS, longer ones by the maxcode walk; DC category plus value bits with the EXTEND rule and a predictor per component
 *                across the whole scan; (run, size) symbols with ZRL and EOB in zigzag order; every block leaves as one coalesced
 *                128-byte store of int16 coefficients into the workspace.
 *   Inverse stage: dequantisation and the two inverse DCT passes into the planes of salve_bev_jpeg_roundtrip, then its pixel launch
 *                unchanged (the same device functions).  The blocks of an edge MCU that lie outside the image are decoded and ignored.
 *   Malformed input: no scan makes the kernels read or write out of bounds, loop without end or fault.  The byte position is bounded
 *                by scan_bytes[i], the coefficient index by 63, the DC category by 11 and the predictor by +-2047; a code that is not
 *                in the table is rejected; every turn of the symbol loop consumes at least one bit or ends.  Each failure sets a bit:
 *                  SALVE_JPEG_BAD_CODE      a bit pattern that is no code of its table
 *                  SALVE_JPEG_COEF_OVERRUN  a run that passes coefficient 63
 *                  SALVE_JPEG_TRUNCATED     the scan ended before the last MCU
 *                  SALVE_JPEG_DC_RANGE      a DC category above 11 or a DC predictor outside +-2047
 *                  SALVE_JPEG_LEFTOVER      more than 7 bits left behind the last MCU, or pad bits that are not all 1
 *                  SALVE_JPEG_MARKER        0xFF followed by anything but 0x00 inside the scan, or as its last byte
 *                  SALVE_JPEG_BAD_SLOT      offset / length outside the scan buffer and its padding
 *                A failing image keeps the coefficients it had decoded, every later one is zero, and it still goes through the inverse
 *                stage; the other images of the call are unaffected, and the device status word is not touched.
 *   Parity with Pillow is claimed for streams whose coefficients came from an 8-bit image (every real encoder's output); for other
 *                well-formed streams the output is deterministic only.
 *   Checks:      SALVE_ERR_BAD_ARG (and 0 from the size query) on null pointers, n <= 0, n > 65535, h or w outside [1, 4096], a
 *                quantisation entry outside [1, 255], a BITS array that over-subscribes the code space or sums past 256, scans_size
 *                below 16, scan_offset not 8-byte or scan_bytes / bev_out / image_status not 4-byte aligned, a workspace smaller than
 *                salve_bev_jpeg_decode_workspace_bytes(n, h, w) or not 16-byte aligned.
 *   Workspace:   the planes (1.5 bytes per pixel of the images rounded up to whole 16 x 16 MCUs) and 768 bytes of coefficients per
 *                MCU: 1.2 MB per 501 x 501 image.  It needs no initialisation and holds nothing from one call to the next.
 *   stages:      SALVE_JPEG_STAGES_ALL for a decode.  SALVE_JPEG_STAGE_ENTROPY alone runs the first launch only (scans -> coefficients in
 *                the workspace, image_status written; bev_out untouched); SALVE_JPEG_STAGE_INVERSE alone runs the other two on the
 *                coefficients the last entropy stage left in the SAME workspace for the same n, h, w (image_status untouched): a caller
 *                can put events between the stages (tools/measure/bench_tile_files.py), and nothing else may write that workspace
 *                between them -- with BevRasteriser, whose JPEG methods share one workspace per stream: no other JPEG call on that
 *                stream.  Any other value: SALVE_ERR_BAD_ARG.
 *   Three launches, asynchronous on `stream`.  Integer arithmetic and plain stores only, one writer per output: the same input
 *   gives the same bits.  Offsets are 64-bit.
 * ------------------------------------------------------------------------------------------------ */
#define SALVE_JPEG_SCAN_PADDING 16
#define SALVE_JPEG_STAGE_ENTROPY 1u
#define SALVE_JPEG_STAGE_INVERSE 2u
#define SALVE_JPEG_STAGES_ALL 3u
#define SALVE_JPEG_BAD_CODE 1u
#define SALVE_JPEG_COEF_OVERRUN 2u
#define SALVE_JPEG_TRUNCATED 4u
#define SALVE_JPEG_DC_RANGE 8u
#define SALVE_JPEG_LEFTOVER 16u
#define SALVE_JPEG_MARKER 32u
#define SALVE_JPEG_BAD_SLOT 64u
size_t salve_bev_jpeg_decode_workspace_bytes(int32_t n, int32_t h, int32_t w);
int salve_bev_jpeg_decode(const uint8_t* scans, size_t scans_size, const int64_t* scan_offset, const int32_t* scan_bytes, int32_t n, int32_t h,
                          int32_t w, const uint16_t* qtab, const uint8_t* huffman, uint32_t* bev_out, int32_t* image_status, void* ws,
                          size_t ws_bytes, uint32_t stages, void* stream);

/* ------------------------------------------------------------------------------------------------
 * salve_bev_jpeg_decode with a LANE-PARALLEL entropy stage, and with restart intervals (additive within ABI 7): opt-in.
 * salve_bev_jpeg_decode runs one wavefront per image whose symbol loop is scalar: its time is the latency of ONE image whatever the
 * batch, and a panorama's scan of several hundred KB takes far longer than on the host.  Here a workgroup of 256 lanes takes one
 * SEGMENT -- a whole scan, or one restart interval of it -- and every lane decodes salve_bev_jpeg_subseq_bytes() bytes of the
 * stuffed stream at once: self-synchronising Huffman decoding (Weissenberger and Schmidt; salve_amd/csrc/jpeg_entropy_lanes.h has
 * the passes, their bounds and what a wrong guess may meet).  Everything else is salve_bev_jpeg_decode's: the arguments, the
 * inverse stage (the same two launches on the same coefficients), image_status, `stages`, the workspace's layout.
 *   segments     device salve_jpeg_segment_t [n_segments], 8-byte aligned, in place of scan_offset / scan_bytes: the segment's bytes
 *                scans + offset .. + bytes (stuffed, no RSTn marker, any alignment; offset + bytes + 16 <= scans_size), the image it
 *                belongs to, its first MCU in the image's scan order and its MCUs.  An image without restart markers is ONE segment
 *                (first_mcu 0, mcu_count = the image's MCUs); the DC predictors start at 0 in every segment (T.81 E.1.4).  The
 *                segments of an image must tile its MCUs; their order in the table is free.  The table is on the device, so the
 *                library cannot read it: BevRasteriser.jpeg_decode checks the tiling on the host before the upload.  Whatever the
 *                table says, the kernel reads no byte outside scans[0 .. scans_size) and writes no coefficient outside its image:
 *                a segment outside the buffer, or whose MCU range is not inside the image, decodes nothing and reports
 *                SALVE_JPEG_BAD_SLOT to its image; a segment whose image is outside [0, n) is ignored; an MCU no segment names
 *                decodes as zeros (mid grey) WITHOUT a status bit.
 *   image_status 0 for an image whose segments are all well-formed, non-zero exactly when salve_bev_jpeg_decode would report the
 *                same bytes (one segment) -- the OR over the image's segments of: too few blocks SALVE_JPEG_TRUNCATED, blocks or
 *                more than 7 bits left over (or pad bits that are not 1) SALVE_JPEG_LEFTOVER, a DC value outside +-2047 after the
 *                scan SALVE_JPEG_DC_RANGE, and BAD_CODE / COEF_OVERRUN / MARKER for what the TRUE pass met.  The bits may differ from
 *                salve_bev_jpeg_decode's, and so may a failing image's pixels (deterministic, otherwise unspecified: this decoder
 *                does not stop at the first error).  The other images do not notice.
 *   Checks:      salve_bev_jpeg_decode's, and SALVE_ERR_BAD_ARG (0 from the size query) for n_segments outside [n, 2^24], a null or
 *                misaligned segment table.
 *   Workspace:   salve_bev_jpeg_decode's bytes (the lanes keep their state in LDS); no initialisation by the caller -- the call
 *                itself clears the coefficients (the lanes store the non-zero ones only) and image_status (the segments OR into it).
 *   Two clears and three launches, asynchronous on `stream`.  Integer arithmetic; plain stores, and one vector atomic OR per failing
 *   segment into the zeroed status word (no dependence on order): the same input gives the same bits.
 * ------------------------------------------------------------------------------------------------ */
#define SALVE_JPEG_MAX_SEGMENTS (1 << 24)
typedef struct salve_jpeg_segment_t {
    int64_t offset;     /* first byte of the segment in `scans` */
    int32_t bytes;
    int32_t image;      /* 0 .. n - 1 */
    int32_t first_mcu;  /* in the image's scan order */
    int32_t mcu_count;
} salve_jpeg_segment_t;
size_t salve_bev_jpeg_decode_lanes_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t n_segments);
int32_t salve_bev_jpeg_subseq_bytes(void);
int salve_bev_jpeg_decode_lanes(const uint8_t* scans, size_t scans_size, const salve_jpeg_segment_t* segments, int32_t n_segments, int32_t n,
                                int32_t h, int32_t w, const uint16_t* qtab, const uint8_t* huffman, uint32_t* bev_out, int32_t* image_status,
                                void* ws, size_t ws_bytes, uint32_t stages, void* stream);

/* ------------------------------------------------------------------------------------------------
 * salve_bev_jpeg_decode and salve_bev_jpeg_decode_lanes for 4:2:2, 4:4:4 and greyscale files as well (additive within ABI 7): opt-in.
 * The tile data set is always 4:2:0; panoramas come from cameras (4:2:2), editors (4:4:4) and scanners (one component).  The two
 * entries below are the two above with ONE more argument, `sampling`, behind w; with SALVE_JPEG_SAMPLING_420 they ARE the two above
 * (the same launches, the same bits).  Everything not named here is as documented there.
 *   sampling     the frame's sampling factors, and with them the MCU -- its blocks in scan order and its size in pixels:
 *                  SALVE_JPEG_SAMPLING_420   Y 2x2, Cb 1x1, Cr 1x1   Y0 Y1 Y2 Y3 Cb Cr (6 blocks)   16 x 16
 *                  SALVE_JPEG_SAMPLING_422   Y 2x1, Cb 1x1, Cr 1x1   Y0 Y1 Cb Cr (4)                16 wide x 8 high
 *                  SALVE_JPEG_SAMPLING_444   Y 1x1, Cb 1x1, Cr 1x1   Y Cb Cr (3)                      8 x 8
 *                  SALVE_JPEG_SAMPLING_GREY  one component           Y (1): the scan is not interleaved, its blocks count
 *                                                                    ceil(w / 8) x ceil(h / 8) in raster order                8 x 8
 *                An image's MCUs -- what a segment's first_mcu / mcu_count count, and a restart interval -- are
 *                ceil(w / MCU width) * ceil(h / MCU height).  A DC predictor per component, restarted per segment.
 *   qtab, huffman as above: [luma, chroma] and [DC luma, AC luma, DC chroma, AC chroma]; a greyscale call reads the luma ones only,
 *                but all of them are checked: the caller repeats the luma tables in the chroma slots (salve_amd/jpeg.py: parse_file).
 *   Pixels:      entropy decoding, dequantisation and the inverse DCT are the same; 4:2:2 chroma is upsampled as libjpeg's
 *                h2v1_fancy_upsample does (along the row only: (3 near + far + 1) >> 2 to the left, + 2 to the right, the two end
 *                pixels copied; a row of at most two chroma samples is replicated), 4:4:4 has none; the colour conversion is the
 *                same; greyscale leaves Y | Y << 8 | Y << 16.  Bit for bit Pillow's pixels (mode L repeated into three channels).
 *                The caller decides that a three-component file IS YCbCr (libjpeg reads some 1x1 1x1 1x1 files as RGB:
 *                salve_amd/jpeg.py has the rule).
 *   Workspace:   per image, the component planes back to back, each rounded up to whole MCUs -- 1.5 / 2 / 3 / 1 bytes per
 *                MCU-rounded pixel for 4:2:0 / 4:2:2 / 4:4:4 / greyscale -- then 128 bytes of coefficients per block
 *                (6 / 4 / 3 / 1 blocks per MCU); the `_workspace_bytes` queries say how much.
 *   Checks:      those of the entries above, and SALVE_ERR_BAD_ARG (0 from the size queries) for a `sampling` that is none of the
 *                four.  The bounds hold for every sampling: no byte read at or behind a scan's or segment's end, no coefficient
 *                written outside the image's MCUs * blocks * 64.
 * ------------------------------------------------------------------------------------------------ */
#define SALVE_JPEG_SAMPLING_420 0
#define SALVE_JPEG_SAMPLING_422 1
#define SALVE_JPEG_SAMPLING_444 2
#define SALVE_JPEG_SAMPLING_GREY 3
size_t salve_bev_jpeg_decode_sampled_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t sampling);
size_t salve_bev_jpeg_decode_lanes_sampled_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t n_segments, int32_t sampling);
int salve_bev_jpeg_decode_sampled(const uint8_t* scans, size_t scans_size, const int64_t* scan_offset, const int32_t* scan_bytes, int32_t n,
                                  int32_t h, int32_t w, int32_t sampling, const uint16_t* qtab, const uint8_t* huffman, uint32_t* bev_out,
                                  int32_t* image_status, void* ws, size_t ws_bytes, uint32_t stages, void* stream);
int salve_bev_jpeg_decode_lanes_sampled(const uint8_t* scans, size_t scans_size, const salve_jpeg_segment_t* segments, int32_t n_segments,
                                        int32_t n, int32_t h, int32_t w, int32_t sampling, const uint16_t* qtab, const uint8_t* huffman,
                                        uint32_t* bev_out, int32_t* image_status, void* ws, size_t ws_bytes, uint32_t stages, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SALVE_HIP_H */
