/*
 * street_crafter_amd -- C ABI of the MI355X (gfx950) Gaussian-splat hot path.
 *
 * This is the drop-in boundary: plain pointers + sizes, no torch types.  Every pointer is a
 * DEVICE pointer unless its name ends in _host.  `stream` is a hipStream_t passed as void*.
 * Every entry point returns 0 on success, a hipError_t (>0) from the runtime, or a negative
 * SC_E* code for an argument the library rejects before launching anything.
 *
 * What each entry point replaces (reference = zzz5y/street_crafter, paths under /root/reference):
 *   sc_projection_fwd/bwd   gsplat.rendering.fully_fused_projection
 *                           called at street_gaussian/models/street_gaussian_renderer.py:219-232
 *   sc_isect_*              gsplat.rendering.isect_tiles           renderer.py:243-252
 *   sc_isect_offsets        gsplat.rendering.isect_offset_encode   renderer.py:253
 *   sc_sh_fwd/bwd           gsplat.rendering.spherical_harmonics   renderer.py:259
 *   sc_rasterize_fwd/bwd    gsplat.rendering.rasterize_to_pixels   renderer.py:267-280
 *                           (backward reached from train.py:236; absgrad read at
 *                            street_gaussian/models/street_gaussian_model.py:505-506)
 *   sc_knn3_mean_dist2      simple_knn._C.distCUDA2
 *                           street_gaussian/models/gaussian_model.py:65,
 *                           gaussian_model_actor.py:139, data_processor/utils/render_utils.py:125
 *   sc_point_project        diff_point_rasterization.PointRasterizer (forward)
 *   sc_point_rasterize_fwd  data_processor/utils/render_utils.py:129-176 (the LiDAR condition render)
 *   sc_point_assemble_project  the frame assembly + visibility filter in front of it, from resident sweeps
 *                           (waymo_render_lidar_pcd.py:207-267, pointcloud_processor/waymo_processor.py:199-226)
 *   sc_loss_fwd/bwd         street_gaussian/utils/loss_utils.py ssim / l1_loss (train.py:168-188)
 *   sc_depth_trim_fwd/bwd   the trimmed LiDAR depth loss (train.py:211-218)
 *   sc_acc_reg_fwd/bwd      the sky loss (train.py:194-196) and the object accumulation loss (train.py:205-206)
 *   sc_frame_tail_fwd/bwd   the pixel-wise tail between the rasterizer and the losses: depth division, sky composite,
 *                           colour correction, permute to planes (street_gaussian_renderer.py:282-300 and :116-132,
 *                           street_gaussian/models/color_correction.py:135-138)
 *   sc_cubemap_fwd/bwd      nvdiffrast.torch.texture(boundary_mode='cube') and the body of SkyCubeMap.forward
 *                           (street_gaussian/models/sky_cubemap.py:92-127; texture calls at :102, :120, :205)
 *   sc_lpips_prep/head_*    the arithmetic of lpips(image * mask, gt * mask) around its convolutions (train.py:172,185;
 *                           street_gaussian/utils/lpipsPyTorch/modules/lpips.py:30-36, networks.py:50-63, utils.py:6-8)
 *   sc_conv*, sc_maxpool2d_*  the convolution stack between the two (networks.py:53-63 over torchvision's alexnet /
 *                           vgg16 features), forward and data gradient; opt-in
 *   sc_resize_fwd/mask/bwd  DiffusionRunner.preprocess_tensor (street_gaussian/utils/diffusion_utils.py:99-115) and the
 *                           row slice after it (train.py:160-169): crop + torchvision Resize in one launch
 *   sc_adam_step            optimizer.step() of every sub-model (street_gaussian_model.py:467-484)
 *   sc_densify_stats        set_max_radii2D + add_densification_stats (street_gaussian_model.py:486-533)
 *   sc_densify_plan/apply   densify_and_prune of every sub-model (street_gaussian_model.py:535-549,
 *                           gaussian_model.py:363-547)
 *   sc_compose_fwd/bwd      StreetGaussianModel.parse_camera + the five get_* properties (street_gaussian_model.py:
 *                           202-407; gaussian_model_actor.py:67-76, gaussian_model_sky.py:62-76)
 *   sc_actor_poses_fwd/bwd  ActorPose.get_tracking_rotation / get_tracking_translation of every visible actor
 *                           (street_gaussian/models/actor_pose.py:83-144): the pose inputs of sc_compose_fwd
 *   sc_voxel_downsample_*   open3d voxel_down_sample(0.1) of the concatenated LiDAR sweeps
 *                           (street_gaussian/pointcloud_processor/base_processor.py:82-85)
 *   sc_radius_outlier_mask  open3d remove_radius_outlier(nb_points=10, radius=0.5)  (base_processor.py:86)
 *   sc_point_bounds_*       the min / max of get_Sphere_Norm (street_gaussian/datasets/base_readers.py:81-82)
 *   sc_gaussian_init        the arithmetic of GaussianModel.create_from_pcd (street_gaussian/models/gaussian_model.py:59-80)
 *                           and GaussianModelActor.create_from_pcd (gaussian_model_actor.py:128-157)
 * The CUDA sources of gsplat / simple-knn are not vendored in the reference;
 * semantics follow SURVEY.md Appendix A and are pinned by oracle/ + tests/golden/.
 *
 * Layouts: all float tensors fp32, row-major, innermost dimension contiguous:
 *   means[N,3] quats[N,4](wxyz) scales[N,3] viewmats[C,4,4](world->cam) Ks[C,3,3]
 *   radii i32[C,N]  means2d[C,N,2]  depths[C,N]  conics[C,N,3]  compensations[C,N]
 *   isect_ids i64[I] = (cam << (32+tile_bits)) | (tile << 32) | depth_bits ; flatten_ids i32[I] = cam*N+n
 *   isect_offsets i32[C,tile_h,tile_w] ; colors[C,N,D] ; opacities[C,N]
 *   render_colors[C,H,W,D] render_alphas[C,H,W,1] last_ids i32[C,H,W]
 */
#ifndef STREET_CRAFTER_AMD_H
#define STREET_CRAFTER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sc_stream_t;

#define SC_OK 0
#define SC_EINVAL (-1)      /* bad size / null pointer / unsupported parameter */
#define SC_EWORKSPACE (-2)  /* workspace too small */
#define SC_EUNSUPPORTED (-3)

/* ---- library info ------------------------------------------------------------------- */
const char* sc_version(void);
const char* sc_error_string(int code);
/* compiled-for architecture string, e.g. "gfx950" */
const char* sc_target_arch(void);
/* host-side spin until *addr == value (acquire); returns 0, or 1 after timeout_us microseconds (< 0: never).
 * For the sequence number sc_isect_bin_count publishes into host-mapped memory (meta_mirror[4]); a ctypes host
 * calls it without holding the GIL, so other host threads keep launching meanwhile. */
int sc_wait_i64(const int64_t* addr, int64_t value, int64_t timeout_us);

/* ---- a1: projection (renderer.py:219-232) -------------------------------------------- */
int sc_projection_fwd(const float* means, const float* quats, const float* scales,
                      const float* viewmats, const float* Ks, int C, int N, int width, int height,
                      float eps2d, float near_plane, float far_plane, float radius_clip,
                      int32_t* radii, float* means2d, float* depths, float* conics,
                      float* compensations /* nullable */, sc_stream_t stream);

/* VJP of sc_projection_fwd w.r.t. means/quats/scales (camera tensors carry no grad at the
 * reference's call site).  v_compensations nullable.  Outputs are OVERWRITTEN (summed over C). */
int sc_projection_bwd(const float* means, const float* quats, const float* scales,
                      const float* viewmats, const float* Ks, int C, int N, int width, int height,
                      float eps2d, const int32_t* radii, const float* conics,
                      const float* compensations /* nullable */,
                      const float* v_means2d, const float* v_depths, const float* v_conics,
                      const float* v_compensations /* nullable */,
                      float* v_means, float* v_quats, float* v_scales, sc_stream_t stream);

/* sc_projection_bwd with the cameras' gradient as well (gsplat's v_viewmats; camera-pose optimisation).  Inputs as
 * sc_projection_bwd.  v_means / v_quats / v_scales: each nullable (not written then; with all three null the chain to
 * the Gaussians is not computed); what is written is bit-equal to sc_projection_bwd's (it is that kernel's launch).
 * v_viewmats [C,4,4], required, OVERWRITTEN: for every (c, n) with radii > 0, with v_pc = dL/d(W m + t) and the
 * symmetric vSc = dL/d(W Sigma W^T),
 *     v_viewmats[c][:3,:3] += v_pc m^T + 2 vSc W Sigma        v_viewmats[c][:3,3] += v_pc
 * and the bottom row is +0.  Ks gets no gradient (as in gsplat).  No float atomics: one partial row of 12 floats per
 * (camera, block of 256 Gaussians) in `workspace` (sc_projection_bwd_cam_workspace_bytes: the rows and 40 N bytes for
 * per-Gaussian outputs left null; 16-B aligned; 0 bytes and nullable when C == 0 or N == 0), added per camera in a
 * fixed order in double: the same bits from run to run.  A row with radii <= 0 contributes by selection, whatever its
 * leaves hold; a camera that sees nothing, and N == 0, give 16 exact +0.  SC_EINVAL: negative C / N, width or
 * height <= 0, a null required pointer, a misaligned workspace. */
int64_t sc_projection_bwd_cam_workspace_bytes(int C, int N);
int sc_projection_bwd_cam(const float* means, const float* quats, const float* scales,
                          const float* viewmats, const float* Ks, int C, int N, int width, int height,
                          float eps2d, const int32_t* radii, const float* conics,
                          const float* compensations /* nullable */,
                          const float* v_means2d, const float* v_depths, const float* v_conics,
                          const float* v_compensations /* nullable */,
                          float* v_means /* nullable */, float* v_quats /* nullable */, float* v_scales /* nullable */,
                          float* v_viewmats, void* workspace, sc_stream_t stream);
/* VJP of sc_camera_centers (c = -R^T t): v_viewmats[c][:3,3] = -R v_c, v_viewmats[c][:3,:3] = -t v_c^T, bottom row 0.
 * v_centers [C,3]; v_viewmats [C,4,4] is OVERWRITTEN.  One launch, one thread per camera. */
int sc_camera_centers_bwd(const float* viewmats, const float* v_centers, int C, float* v_viewmats, sc_stream_t stream);

/* ---- a3: tile intersection (renderer.py:243-252) -------------------------------------- */
/* workspace bytes needed by sc_isect_count/sc_isect_emit for CN = C*N gaussians */
size_t sc_isect_workspace_bytes(int64_t CN);
/* pass 1: tiles_per_gauss[C,N] and the total number of intersections (device int64). */
int sc_isect_count(const float* means2d, const int32_t* radii, int C, int N,
                   int tile_size, int tile_width, int tile_height,
                   int32_t* tiles_per_gauss, int64_t* total_dev, void* workspace, size_t ws_bytes,
                   sc_stream_t stream);
/* pass 2: unsorted keys/values in emission order (gaussian-major, row-major over the rect).
 * Must be called with the workspace left by sc_isect_count. */
int sc_isect_emit(const float* means2d, const int32_t* radii, const float* depths, int C, int N,
                  int tile_size, int tile_width, int tile_height,
                  const int32_t* tiles_per_gauss, int64_t n_isects,
                  int64_t* isect_ids, int32_t* flatten_ids, void* workspace, size_t ws_bytes,
                  sc_stream_t stream);

/* stable LSD radix sort of (u64 key, i32 value) pairs over key bits [0, end_bit). In place:
 * on return keys/vals hold the sorted result.  tmp_* are scratch of the same size. */
size_t sc_radix_sort_workspace_bytes(int64_t n);
int sc_radix_sort_pairs_u64_i32(uint64_t* keys, int32_t* vals, uint64_t* tmp_keys, int32_t* tmp_vals,
                                int64_t n, int end_bit, void* workspace, size_t ws_bytes,
                                sc_stream_t stream);

/* Fused tile-bucketed path: produces exactly what count + emit + stable sort + offset-encode
 * produce (bit-identical isect_ids / flatten_ids / offsets): Gaussians are bucketed by SUPER-TILE
 * (2x2 tiles), each super-tile is sorted once in LDS and its up-to-4 per-tile lists are emitted by
 * a stable filter.  Two calls because the caller must size the outputs in between:
 *   sc_isect_bin_count : tiles_per_gauss, per-tile offsets (= isect_offset_encode result) and
 *                        meta_dev[0] = total intersections I, [1] = largest per-tile count,
 *                        [2] = total (Gaussian, super-tile) records, [3] = largest super-tile
 *   sc_isect_bin_sort  : isect_ids / flatten_ids, sorted.  `capacity` = elements the output buffers
 *                        were sized for, `rec_capacity` = records the workspace was sized for,
 *                        `super_capacity` = largest super-tile the caller provisioned LDS for.  The
 *                        kernels read meta_dev themselves and do NOTHING when meta_dev[0] > capacity,
 *                        meta_dev[2] > rec_capacity or meta_dev[3] > super_capacity, so a caller may
 *                        launch with predicted sizes before it has read meta_dev back (no GPU idle
 *                        bubble) and retry with exact sizes if the prediction was too small.
 *                        Elements [I, capacity) of isect_ids / flatten_ids are not written (nor is any element
 *                        by a launch that does nothing); no store lands outside the I entries.
 *                        A super-tile bucket of up to 3584 records is sorted by one workgroup in LDS; when
 *                        super_capacity is larger, longer buckets are first cut into depth ranges that fit
 *                        (only they pay for it).
 * Both return SC_EUNSUPPORTED when C*tile_width*tile_height > 36864 (a 3840x2160 frame has 32400 tiles), C*N >= 2^28 or
 * super_capacity > 220 000; the caller then takes the count/emit/radix-sort route.
 */
/* n_records < 0: bytes of the count-phase workspace (shared by both calls; holds the visible Gaussians'
 * rectangle / depth / id, 16 B each, in spatial order); n_records >= 0: bytes of the sort-phase workspace for that many records. */
size_t sc_isect_bin_workspace_bytes(int64_t CN, int C, int tile_width, int tile_height, int64_t n_records);
/* meta_mirror (nullable): HOST-MAPPED pinned int64[5] (hipHostMalloc; torch pin_memory).  When given,
 * the device stores meta[0..3] there and then `seq` into meta_mirror[4] with system-scope release, so
 * the host can poll meta_mirror[4] == seq instead of enqueuing a D2H copy + event (which costs a copy
 * kernel and a barrier bubble in the middle of the frame). */
int sc_isect_bin_count(const float* means2d, const int32_t* radii, const float* depths, int C, int N,
                       int tile_size, int tile_width, int tile_height,
                       int32_t* tiles_per_gauss, int32_t* isect_offsets, int64_t* meta_dev /* [4] */,
                       int64_t* meta_mirror /* [5], nullable */, int64_t seq,
                       void* workspace, size_t ws_bytes,
                       const int32_t* tile_work /* nullable: [sc_view_slots()][C*tile_width*tile_height], see
                           sc_rasterize_fwd */,
                       const float* viewmats /* nullable (= slot 0): [C,4,4] world->camera, the frame's cameras: which
                           bank of tile_work this call uses is looked up from camera 0's forward axis, see VIEW SLOTS */,
                       int32_t* view_registry /* nullable (= slot 0): int32[sc_view_registry_words()], VIEW SLOTS */,
                       int32_t* tile_order /* nullable: out, the rasterizer's dispatch list built from tile_work:
                           sc_tile_order_len(C*tile_width*tile_height) items, see sc_rasterize_fwd */,
                       sc_stream_t stream);
/* VIEW SLOTS.  The rasterizer's work hint (tile_work) only helps the frame that finds it if it was left by the
 * same view; a street rig renders front / front-left / front-right in turn.  tile_work therefore has sc_view_slots()
 * banks of C*tile_width*tile_height words, and sc_isect_bin_count chooses the bank on the DEVICE (no host round
 * trip, no extra launch): camera 0's forward axis (row 2 of the world->camera rotation of viewmats [C,4,4]) is
 * matched against `view_registry` (persistent, caller-owned, zero-initialised int32[sc_view_registry_words()], one
 * per device); a slot within ~7 degrees is reused and follows the camera, otherwise the least recently used one
 * is taken over.  The slot is stored in tile_order's last word, where the rasterizer finds the bank to report
 * into.  Scheduling only: any slot renders the same image. */
int sc_view_slots(void);
int sc_view_registry_words(void);
/* Records of the largest super-tile bucket one workgroup of sc_isect_bin_sort sorts in LDS (3584).  A caller that
 * predicts `super_capacity` with head-room should not let the head-room alone cross this value: above it every call
 * also launches the split kernel and the segment workgroups, whether or not a bucket is that large. */
int sc_isect_bin_bucket_capacity(void);
/* The RANGE PLAN by which sc_isect_bin_sort cuts a bucket of more than sc_isect_bin_bucket_capacity() records into depth
 * ranges, callable on the host (no device is touched; the kernel runs the same formulae, csrc/isect_split_plan.h).
 *   sc_isect_split_limits   : out[0] = ranges one bucket may be cut into (the kernel's tables), [1] = largest bucket the
 *                             split takes (= largest super_capacity), [2] = cap, records of one range (= the bucket
 *                             capacity), [3] = light_max, a bin above it is a group of its own, [4] = target, [5] = bins
 *   sc_isect_split_seg_bound: segments a launch provisions for rec_capacity = n_records and nsb super-tiles
 *   sc_isect_split_bins     : bins[i] = histogram bin of keys[i] (60-bit: depth bits << 28 | flat id) in a bucket whose
 *                             smallest / largest key are lo / hi
 *   sc_isect_split_plan     : bin_counts[out[5]] -> range_of_bin[out[5]] (-1: empty bin) and the number of ranges
 */
int sc_isect_split_limits(int64_t* out /* [6] */);
int64_t sc_isect_split_seg_bound(int64_t n_records, int nsb);
int sc_isect_split_bins(const uint64_t* keys, int64_t n, uint64_t lo, uint64_t hi, int32_t* bins);
int sc_isect_split_plan(const uint32_t* bin_counts, int cap, int32_t* range_of_bin, int32_t* n_ranges);
int sc_isect_bin_sort(const float* means2d, const int32_t* radii, const float* depths, int C, int N,
                      int tile_size, int tile_width, int tile_height,
                      const int32_t* isect_offsets, const int64_t* meta_dev,
                      void* count_workspace /* the one sc_isect_bin_count filled: its scratch counters are
                                               consumed by the first launch whose capacities suffice */,
                      int64_t capacity, int64_t rec_capacity, int64_t super_capacity,
                      int64_t* isect_ids /* nullable */, int32_t* flatten_ids,
                      void* workspace, size_t ws_bytes, sc_stream_t stream);
/* isect_ids from the sorted lists: isect_ids[k] = (camera << (32 + tile_bits)) | (tile << 32) | bits(depths[
 * flatten_ids[k]]) for every k in tile's range of isect_offsets.  Lets a caller skip the 8 B x I key array in
 * sc_isect_bin_sort (isect_ids = NULL) and produce it only if somebody asks for it. */
int sc_isect_ids_rebuild(const int32_t* flatten_ids, const int32_t* isect_offsets, const float* depths,
                         int C, int N, int tile_width, int tile_height, int64_t n_isects,
                         int64_t* isect_ids, sc_stream_t stream);
/* Re-zero the sort phase's bucket cursors / fallback flags inside `count_workspace`: call before a
 * SECOND sc_isect_bin_sort of the same count phase (retry after an under-predicted capacity). */
int sc_isect_bin_reset_cursors(void* count_workspace, int64_t CN, int C, int tile_width, int tile_height,
                               sc_stream_t stream);

/* ---- a4: offsets (renderer.py:253) ---------------------------------------------------- */
int sc_isect_offsets(const int64_t* isect_ids, int64_t n_isects, int C, int tile_width,
                     int tile_height, int32_t* offsets, sc_stream_t stream);

/* ---- a6: spherical harmonics (renderer.py:259) ---------------------------------------- */
/* M rows; dirs[M,3], coeffs[M,K,3] (K >= (degree+1)^2 coefficients per row, row stride K),
 * masks uint8[M] nullable; colors[M,3].  Masked-out rows are written as 0. */
int sc_sh_fwd(int degree, const float* dirs, const float* coeffs, const uint8_t* masks,
              int64_t M, int K, float* colors, sc_stream_t stream);
/* v_dirs nullable. v_coeffs[M,K,3] fully written (zeros beyond the used bases / masked rows). */
int sc_sh_bwd(int degree, const float* dirs, const float* coeffs, const uint8_t* masks,
              int64_t M, int K, const float* v_colors, float* v_coeffs, float* v_dirs,
              sc_stream_t stream);

/* ---- a9: rasterize (renderer.py:267-280) ---------------------------------------------- */
/* D = number of colour channels, 1..32 (3 and 4 have dedicated kernels).
 * backgrounds[C,D] nullable; tile_masks uint8[C,tile_h,tile_w] nullable (0 = skip tile). */
int sc_rasterize_fwd(const float* means2d, const float* conics, const float* colors,
                     const float* opacities, const float* backgrounds, const uint8_t* tile_masks,
                     int C, int N, int D, int width, int height, int tile_size,
                     int tile_width, int tile_height,
                     const int32_t* isect_offsets, const int32_t* flatten_ids, int64_t n_isects,
                     float* render_colors, float* render_alphas,
                     int32_t* last_ids /* nullable: only the backward pass reads it */,
                     const int32_t* tile_order /* nullable: the DISPATCH LIST buffer (sc_tile_order_len(C*tile_width*
                         tile_height) items; the forward reads its leading part), one item per workgroup in launch order (longest-running first: the launch's makespan is one
                         tile's serial walk plus the throughput part).  item = flat tile << 2 | kind: kind 0 = the whole
                         tile, 1 / 2 = its upper / lower 16 x 8 half (a tile whose walk would be the launch's tail is
                         shared by two waves); negative = no work.  Every tile must appear exactly once as kind 0 or
                         once as each of kinds 1 and 2 (a tile that does not appear is not rendered).
                         sc_isect_bin_count builds it */,
                     int32_t* tile_work /* nullable: [sc_view_slots()][C*tile_width*tile_height]; the bank named by
                         tile_order's last word (0..sc_view_slots()-1, clamped) receives the list entries every tile
                         walked: the scheduling hint the NEXT frame of that view has its tile_order built from
                         (persistent, caller-owned, zero-initialised; stale or half-updated values are fine).  Without
                         tile_order: bank 0 */,
                     sc_stream_t stream);
/* number of int32 items in the dispatch-list buffer for `total_tiles` tiles: the forward's list (total_tiles +
 * total_tiles / 8 + 8 items: every tile + room for the split ones, padded with -1), then a whole-tile list in the
 * same order (total_tiles items `tile << 2`), one word that says whether that second list was built: it is only
 * under sc_set_option raster_bwd_split 0 (set BEFORE the frame's sc_isect_bin_count), for a backward that takes
 * whole tiles; by default sc_rasterize_bwd follows the forward's list, half tiles included -- and, last, the view
 * slot of the call (see VIEW SLOTS).  The forward's list, the word and the view slot are always written; the whole-tile
 * list is not written at all unless it is built.  Tiles of equal work class take their slots through an integer
 * atomic: a list holds the same items from run to run, not necessarily in the same sequence. */
int sc_tile_order_len(int total_tiles);
/* Gradient outputs must be ZERO-FILLED by the caller (the kernel accumulates with atomics).
 * v_means2d_abs nullable (absgrad).
 * Every shape sc_rasterize_fwd takes is taken here: tile_size 1..32 (a tile whose pixel count is not a multiple of 64,
 * e.g. 12 x 12, runs in whole waves), D 1..32 (the generic kernel stages 40 + 4 D bytes of LDS per splat and sizes its
 * batches to 64 KiB: 1024 splats per batch at tile 32 up to D = 6, 384 at D = 32). */
int sc_rasterize_bwd(const float* means2d, const float* conics, const float* colors,
                     const float* opacities, const float* backgrounds, const uint8_t* tile_masks,
                     int C, int N, int D, int width, int height, int tile_size,
                     int tile_width, int tile_height,
                     const int32_t* isect_offsets, const int32_t* flatten_ids, int64_t n_isects,
                     const float* render_alphas, const int32_t* last_ids,
                     const float* v_render_colors, const float* v_render_alphas,
                     float* v_means2d_abs, float* v_means2d, float* v_conics, float* v_colors,
                     float* v_opacities, const int32_t* tile_order /* nullable, as sc_rasterize_fwd */,
                     sc_stream_t stream);

/* ---- a14: simple_knn.distCUDA2 --------------------------------------------------------- */
size_t sc_knn_workspace_bytes(int64_t n);
int sc_knn3_mean_dist2(const float* points, int64_t n, float* out, void* workspace,
                       size_t ws_bytes, sc_stream_t stream);

/* ---- LiDAR condition render, diff_point_rasterization.PointRasterizer
 *      (data_processor/utils/render_utils.py:129-176; contract: street_crafter_amd/lidar_condition.py render_points)
 * Hard-disc point splats, blended front to back.  The tile binning between the two calls is sc_isect_count /
 * sc_isect_emit / sc_radix_sort_pairs_u64_i32 / sc_isect_offsets with C = 1 and tile_size 16.
 * sc_point_project: one camera.  points [N,3] world; colors [N,3]; viewmat double [4,4] world->cam (row-major, p_cam =
 *   viewmat @ [p,1]); u = fx x/z + cx, v = fy y/z + cy (pixel centres at +0.5).  Camera transform, u, v and r are
 *   evaluated in fp64 and rounded once to fp32 (world coordinates of tens of metres lose ~1e-4 px in fp32); the knn
 *   radius rule stays fp32, as render_points evaluates it.  Alpha per point = opacities[n]
 *   (nullable) or occ, in (0, 1].  World radius by radius_mode:
 *     0: scale                                              1: scale * z / focal_r * 0.5 * min(H, W)  (ndc scale)
 *     2: min(sqrt(max(radius_in[n], 1e-7)) * knn_scale_down, scale)   radius_in = distCUDA2 of the points (knn scale)
 *     3: radius_in[n] * scale                               (per-point world radius x scale_modifier)
 *   pixel radius r = world_r * focal_r / z.  A point is kept iff max(near_plane, 0) < z < far_plane, its centre and
 *   radius are finite in fp32, r >= 0 and its alpha lies in (0, 1].  Outputs: radii i32[N] = max(ceil(min(r, 2^30)), 1)
 *   for a kept point and 0 for a culled one (a kept point of r = 0 is listed with radius 1 and covers exactly the pixel
 *   whose centre it sits on, 0 <= 0; means2d, depths are 0 for a culled point), means2d [N,2],
 *   depths [N] -- the layout sc_isect_count / sc_isect_emit read -- and records [N,8] (16-B aligned) = (u, v, r^2, z,
 *   r, g, b, alpha), what sc_point_rasterize_fwd gathers.  SC_EINVAL: N < 0, an empty image, an unknown mode, occ outside
 *   (0, 1] without opacities, a missing radius_in for modes 2 / 3, focal_r <= 0, scale < 0, a null pointer.
 * sc_point_rasterize_fwd: one 64-lane wave per 16 x 4 strip of a 16 x 16 tile (sc_set_option "point_raster_waves").
 *   Per pixel the covering points (dx^2 + dy^2 <= r^2) of
 *   the tile's depth-sorted list, while hits < max_hit:  c += T a rgb,  d += T a z,  T *= 1 - a;  then
 *   rgb = c + T * background (nullable: black), alpha = 1 - T, depth = d.  rgb channel k of pixel p at
 *   out_rgb[p * pix_stride + k * ch_stride], alpha at out_alpha[p * alpha_stride], depth (nullable) at out_depth[p]:
 *   interleaved [H,W,4] is (pix_stride 4, ch_stride 1, out_alpha = out_rgb + 3, alpha_stride 4), planes [3,H,W] +
 *   [H,W] are (1, H*W, separate plane, 1).  SC_EINVAL: max_hit < 1, tile_width / tile_height other than the 16-pixel
 *   grid of the image, a stride < 1, n_isects outside [0, 2^31), a null pointer, records not 16-B aligned. */
int sc_point_project(const float* points, const float* colors, const float* opacities /* nullable */, float occ,
                     const float* radius_in /* nullable for modes 0 / 1 */, int N, const double* viewmat, double fx,
                     double fy, double cx, double cy, double focal_r, int width, int height, double near_plane,
                     double far_plane, int radius_mode, double scale, float knn_scale_down, int32_t* radii,
                     float* means2d, float* depths, float* records, sc_stream_t stream);
int sc_point_rasterize_fwd(const float* records, int N, int width, int height, int tile_width, int tile_height,
                           const int32_t* isect_offsets, const int32_t* flatten_ids, int64_t n_isects, int max_hit,
                           const float* background /* nullable [3] */, float* out_rgb, int64_t pix_stride,
                           int64_t ch_stride, float* out_alpha, int64_t alpha_stride,
                           float* out_depth /* nullable */, sc_stream_t stream);

/* ---- LiDAR condition frame from RESIDENT sweeps: frame assembly + visibility filter + sc_point_project in one launch
 *      (data_processor/waymo_processor/waymo_render_lidar_pcd.py:207-267 per frame x camera x shift, and
 *      WaymoPointCloudProcessor.render_condition, street_gaussian/pointcloud_processor/waymo_processor.py:199-226;
 *      contract: lidar_condition.assemble_frame / filter_visible; host side: street_crafter_amd/lidar_sequence.py)
 * xyz double [n_resident,3] and rgb float [n_resident,3] stay on the device for the whole sequence, every track's frames
 * contiguous in frame order, so a window of a track is one range.  A frame is one small block of 8-byte words, the same
 * bytes at frame_host (host memory: validated here) and frame_dev (device memory, 8-B aligned: read by the kernel; the
 * caller copies it there on `stream` before the call):
 *   words [0,16)  view     double [4,4] world->camera of the points MOVED BY -origin (rows 0..2 read), as sc_point_project
 *   words [16,19) origin   double [3]; word 19 unused
 *   words [20,32) filt_m   double [3,4] world->camera of the unmoved world points (the visibility filter)
 *   words [32,41) filt_k   double [3,3] intrinsics (the visibility filter); words [41,48) unused
 *   then n_poses x double [3,4] actor poses, then n_segments x sc_point_segment.
 * Segment s puts resident rows [src_begin, src_begin + count) at output rows [out_begin, out_begin + count), through
 * pose slot `pose` (-1: none).  Per output row i, all in fp64, left to right, without contraction:
 *   w = p, or w_r = P[r][0] x + P[r][1] y + P[r][2] z + P[r][3];
 *   filter == 1: cam = filt_m [w,1], pix = filt_k cam; the row is kept iff cam_z > 1e-3, 0 <= pix_0 / pix_2 < width and
 *     0 <= pix_1 / pix_2 < height (lidar_condition.filter_visible); a dropped row is ALL ZERO in radii, means2d, depths
 *     and records (a culled point to the tile binning); nothing is compacted;
 *   q = (float)(w - origin); then exactly sc_point_project on q under `view` with alpha occ and the colour rgb[row]:
 *     radii, means2d, depths, records as there (radius modes 0, 1, 2; radius_in [N] indexed by OUTPUT row);
 *   points_world (nullable) [N,3] = (float)w.
 * radii, means2d, depths, records all NULL with points_world given: only points_world is written (the knn radius
 * rule's first step).  The segment search keeps the first sc_point_assemble_lds_segments() output begins in LDS and
 * reads later ones from global memory.  Nothing waits for the device.
 * SC_EINVAL, nothing launched, no GPU needed: N, n_segments, n_poses or n_resident < 0; a negative count; segments whose
 *   output ranges do not tile [0, N) in order; a pose slot outside [-1, n_poses); a resident range outside
 *   [0, n_resident]; filter other than 0 / 1; an empty image, a radius mode other than 0..2, occ outside (0, 1], mode 2
 *   without radius_in, focal_r <= 0, scale < 0; frame_host NULL with segments; and, for N > 0, a null xyz / rgb /
 *   frame_dev, only some of the four projection outputs, no output at all, records not 16-B aligned, frame_dev not 8-B
 *   aligned.  N == 0 with a valid table: SC_OK. */
#define SC_POINT_FRAME_HEADER_WORDS 48
typedef struct {
    int64_t src_begin;
    int32_t out_begin;
    int32_t count;
    int32_t pose;               /* -1: no pose */
    int32_t reserved;
} sc_point_segment;
int sc_point_assemble_lds_segments(void);
int sc_point_assemble_project(const double* xyz, const float* rgb, int64_t n_resident, const void* frame_host,
                              const void* frame_dev, int n_segments, int n_poses, int N, int filter, float occ,
                              const float* radius_in /* nullable for modes 0 / 1 */, double fx, double fy, double cx,
                              double cy, double focal_r, int width, int height, double near_plane, double far_plane,
                              int radius_mode, double scale, float knn_scale_down, int32_t* radii, float* means2d,
                              float* depths, float* records, float* points_world /* nullable */, sc_stream_t stream);

/* ---- photometric loss of the training step: loss_utils.ssim + loss_utils.l1_loss
 *      (street_gaussian/utils/loss_utils.py:21-37, 95-131; called at train.py:168-188, both branches)
 * One pass computes, per image b of a batch, with x = where(mask, img1, 0), y = where(mask, img2, 0):
 *   ssim_out[b] = mean over C*H*W of the SSIM map (Gaussian window 11, sigma 1.5, zero padding 5, C1 = 0.01^2,
 *   C2 = 0.03^2), ssim_out[B] = the mean over all B images; l1_out[b] = mean of |img1 - img2| over the (pixel, channel)
 *   entries the mask keeps (NaN when it keeps none, as torch's mean of an empty selection); kept_out[b] (nullable) = that
 *   entry count.  Sums are deterministic (per-block slab in `workspace`, summed in a fixed order): no float atomics.
 * Strided input: strides_host[11] (host memory, elements, >= 0) = img1 (batch, channel, row, column), img2 (the same
 *   four), mask (batch, row, column).  The mask is u8 [mask_batch, mask_height, mask_width] (mask_batch 1 or B, the
 *   rest H, W), broadcast over channels; mask NULL keeps every pixel.  So the rasterizer's [H,W,4] image viewed as
 *   [3,H,W] (strides 1 / 4W / 4 in the last three) and a row crop img[:, upper:, :] are read without a copy.
 * Gradient maps (nullable; all [B,C,H,W] contiguous, scaled by 1/(C*H*W)): map_b = dS/dE[x^2], map_c = dS/dE[xy], with
 *   map_a1 = dS/dmu1 and / or map_a2 = dS/dmu2 -- b and c together with at least one of a1 / a2, or none.
 * sc_loss_bwd (gather form, no atomics): grad1 = g_ssim[b] (G*a1 + 2 x G*b + y G*c) + g_l1[b] sign(x - y) / kept[b],
 *   grad2 = g_ssim[b] (G*a2 + 2 y G*b + x G*c) + g_l1[b] sign(y - x) / kept[b], both zero where the mask is false,
 *   written contiguous [B,C,H,W] (either nullable, not both).  g_ssim / g_l1 [B] are device memory (nullable: that term
 *   is absent); neither call synchronises with the host.
 * SC_EINVAL (nothing launched): a size <= 0, window != 11, a negative stride, a mask shape that does not broadcast, an
 *   incomplete map set, a null required pointer.  SC_EWORKSPACE: workspace_bytes < sc_loss_workspace_bytes (0 for bad
 *   sizes). */
size_t sc_loss_workspace_bytes(int batch, int channels, int height, int width);
int sc_loss_fwd(const float* img1, const float* img2, const uint8_t* mask /* nullable */, const int64_t* strides_host,
                int batch, int channels, int height, int width, int mask_batch, int mask_height, int mask_width,
                int window, float* ssim_out, float* l1_out, int64_t* kept_out /* nullable */,
                float* map_a1, float* map_a2, float* map_b, float* map_c, void* workspace, size_t workspace_bytes,
                sc_stream_t stream);
int sc_loss_bwd(const float* img1, const float* img2, const uint8_t* mask /* nullable */, const int64_t* strides_host,
                int batch, int channels, int height, int width, int mask_batch, int mask_height, int mask_width,
                int window, const float* map_a1, const float* map_a2, const float* map_b, const float* map_c,
                const float* g_ssim, const float* g_l1, const int64_t* kept, float* grad1, float* grad2,
                sc_stream_t stream);

/* ---- trimmed LiDAR depth loss of the training step (train.py:211-218)
 * kept = (lidar_depth > 0) && mask (mask NULL: all true), e = fabsf(depth - lidar_depth) in fp32, n = #kept,
 * k = (int64)(keep * (double)n) (Python's int(keep * n)).  value_out = the mean of the k smallest e, NaN ordered above
 * +inf (torch.topk(largest=False)); NaN when k == 0, as the reference's mean of an empty tensor.  The selection is a
 * radix select over the fp32 error bits, all on the device: the value is (sum of e < t + (k - below) t) / k, summed in
 * double and rounded once, t = the k-th smallest error.  threshold_out (nullable) = t (NaN when k == 0);
 * counts_out (nullable) = {n, k, below}, below = #(e < t).  Deterministic: no float atomics.
 * Strided input: strides_host[6] (host memory, elements, >= 0) = depth (row, column), lidar_depth (row, column), mask
 *   (row, column): [1,H,W] tensors (the leading size-1 dimension carries no stride), read through the strides.
 * sc_depth_trim_bwd reads the state the forward left in `workspace` (keep it unchanged between the two calls) and writes
 *   grad_depth = sign(d - l) * (g * (1 / (float)k)) on the selected pixels and +0 elsewhere, grad_lidar the negation,
 *   contiguous [H,W] (either nullable, not both).  grad_value [1] is device memory.  Selected: every pixel with e < t,
 *   then the first k - below pixels with e == t in row-major order.
 * SC_EINVAL (nothing launched): H or W <= 0, H*W >= 2^31, keep outside (0, 1], a negative stride, a null required
 *   pointer.  SC_EWORKSPACE: workspace_bytes < sc_depth_trim_workspace_bytes (0 for bad sizes). */
size_t sc_depth_trim_workspace_bytes(int height, int width);
int sc_depth_trim_fwd(const float* depth, const float* lidar_depth, const uint8_t* mask /* nullable */,
                      const int64_t* strides_host, int height, int width, double keep, float* value_out,
                      float* threshold_out /* nullable */, int64_t* counts_out /* nullable [3] */, void* workspace,
                      size_t workspace_bytes, sc_stream_t stream);
int sc_depth_trim_bwd(const float* depth, const float* lidar_depth, const uint8_t* mask /* nullable */,
                      const int64_t* strides_host, int height, int width, const float* grad_value,
                      const void* workspace, size_t workspace_bytes, float* grad_depth, float* grad_lidar,
                      sc_stream_t stream);

/* ---- sky and object accumulation losses of the training step (train.py:194-196 sky, train.py:205-206 object)
 * a = clamp(acc, 1e-6f, 0x1.ffffdep-1f); per mask channel c, with L = -log(1 - a) and E = -(a log a + (1 - a) log(1 - a)):
 *   mode 0 (sky):    where(mask, L, E)       mode 1 (object): where(mask, E, L)
 * value_out = the mean over mask_channels * H * W (the reference's where broadcasts a [Cm,H,W] mask over acc [1,H,W]),
 * summed in double per block, the slab added in a fixed order.  acc is fp32 [1,H,W], mask u8 [Cm,H,W] (required).
 * strides_host[5] (host memory, elements, >= 0) = acc (row, column), mask (channel, row, column).
 * sc_acc_reg_bwd: grad_acc [H,W] contiguous = g / (Cm H W) * sum_c (L chosen ? 1 / (1 - a) : log(1 - a) - log a) where
 *   1e-6f <= acc <= 0x1.ffffdep-1f (clamp's gradient passes at the bounds), 0 elsewhere (NaN included).
 * SC_EINVAL (nothing launched): H or W <= 0, H*W >= 2^31, mask_channels < 1, mode other than 0 / 1, a negative stride,
 *   a null required pointer.  SC_EWORKSPACE: workspace_bytes < sc_acc_reg_workspace_bytes (0 for bad sizes). */
size_t sc_acc_reg_workspace_bytes(int height, int width);
int sc_acc_reg_fwd(const float* acc, const uint8_t* mask, const int64_t* strides_host, int mask_channels, int height,
                   int width, int mode, float* value_out, void* workspace, size_t workspace_bytes, sc_stream_t stream);
int sc_acc_reg_bwd(const float* acc, const uint8_t* mask, const int64_t* strides_host, int mask_channels, int height,
                   int width, int mode, const float* grad_value, float* grad_acc, sc_stream_t stream);

/* ---- frame tail of the training step (street_gaussian_renderer.py:282-300, :116-132; color_correction.py:135-138)
 * Per pixel, with c = render_colors (D = channels, 3 or 4; dense [H,W,D], or with colors_planar = 1 dense [D,H,W], the
 * storage sc_rasterize_fwd_planar leaves behind a [H,W,D] view), a = render_alphas [H,W] (dense), s = sky
 * (nullable; three channels read through sky_strides_host[3] = channel, row, column strides in elements, >= 0, host
 * memory) and A = affine (nullable; 12 floats, row-major [3,4], DEVICE memory).  Every product, sum and quotient is a
 * separately rounded fp32 operation, in this order:
 *     keep  = 1 - a
 *     v_j   = c_j + s_j * keep                               (v_j = c_j without sky)
 *     rgb_i = ((A_i0 v_0 + A_i1 v_1) + A_i2 v_2) + A_i3      (rgb_i = v_i without affine)
 *     depth = c_3 / max(a, 1e-10f)
 * rgb [3,H,W] contiguous planes; depth [H,W] contiguous (nullable; D == 4 only).  clamp = 1 (cfg.mode != 'train'): c_j
 * and s_j are clamped to [0,1] before the composite and rgb_i after the affine; the depth is not touched.
 * sc_frame_tail_bwd, with g = grad_rgb [3,H,W] and h = grad_depth [H,W] (contiguous, either nullable, not both; an absent
 * one counts as zero), the clamp = 0 form only:
 *     gv_j          = (A_0j g_0 + A_1j g_1) + A_2j g_2       (gv_j = g_j without affine)
 *     grad_colors_j = gv_j                                   grad_colors_3 = h / max(a, 1e-10f)
 *     grad_sky_j    = gv_j * keep
 *     grad_alphas   = -((gv_0 s_0 + gv_1 s_1) + gv_2 s_2) - [a >= 1e-10f] (h c_3) / (max(a, 1e-10f))^2
 *     grad_affine_ij = sum over pixels of g_i v_j            grad_affine_i3 = sum over pixels of g_i
 *   grad_colors [H,W,D], grad_alphas [H,W], grad_sky ([3,H,W] planes when grad_sky_planar, else [H,W,3]) and grad_affine
 *   [12] are contiguous and each nullable: only those given are computed and written (at least one).  grad_sky and
 *   grad_affine need grad_rgb and their input.  v is recomputed, never stored.
 *   The twelve sums are deterministic (no float atomics): a lane adds at most 16 pixels serially in fp32, a block of 256
 *   lanes finishes with an 8-level tree and stores its 12 partials into `workspace`; a one-block second launch adds the
 *   block partials in float64 and rounds once.  No term passes through more than 24 fp32 additions at any frame size.
 * Four consecutive pixels per lane, 16-byte accesses; an array whose address is not 16-byte aligned, the last H*W mod 4
 * pixels and a sky that is neither [H,W,4]-strided, [H,W,3] nor [3,H,W] dense take scalar accesses with the same results.
 * SC_EINVAL (nothing launched): H or W <= 0, H*W >= 2^31, channels other than 3 / 4, a flag other than 0 / 1, a depth
 *   pointer with channels == 3,
 *   a negative stride, a null required pointer, a gradient asked for without its inputs.  SC_EWORKSPACE: grad_affine asked
 *   for with workspace_bytes < sc_frame_tail_workspace_bytes (0 for bad sizes). */
size_t sc_frame_tail_workspace_bytes(int height, int width);
int sc_frame_tail_fwd(const float* colors, int channels, int colors_planar, const float* alphas, const float* sky /* nullable */,
                      const int64_t* sky_strides_host, const float* affine /* nullable */, int height, int width,
                      int clamp, float* rgb, float* depth /* nullable */, sc_stream_t stream);
int sc_frame_tail_bwd(const float* colors, int channels, int colors_planar, const float* alphas, const float* sky /* nullable */,
                      const int64_t* sky_strides_host, const float* affine /* nullable */, int height, int width,
                      const float* grad_rgb, const float* grad_depth, float* grad_colors, float* grad_alphas,
                      float* grad_sky, int grad_sky_planar, float* grad_affine, void* workspace, size_t workspace_bytes,
                      sc_stream_t stream);

/* ---- sky cube map (street_gaussian/models/sky_cubemap.py:92-127; nvdiffrast.torch.texture in cube mode at :102, :120
 *      and :205; reached from street_gaussian_renderer.py:123-126 and :156-159)
 * Seamless bilinear sampling of tex fp32 [6,R,R,C] (contiguous; faces +x -x +y -y +z -z; 2 <= R <= 16384; C 1..4), one
 * sample per direction.  The major axis is z if |z| > max(|x|,|y|), else y if |y| > |x|, else x; face coordinates s, t in
 * [-1,1] follow the OpenGL table (+x: -z/|x|, -y/|x|; -x: z/|x|, -y/|x|; +y: x/|y|, z/|y|; -y: x/|y|, -z/|y|;
 * +z: x/|z|, -y/|z|; -z: -x/|z|, -y/|z|).  The texel position is ((s+1)/2 R - 0.5, (t+1)/2 R - 0.5), s along the last
 * spatial axis; the taps are floor and floor + 1 in each axis.  A tap outside [0,R-1] in one axis is the texel whose cell
 * contains that tap's centre on the extended face plane, re-indexed with the same rule (the adjacent edge texel); a tap
 * outside in both axes is dropped and the other three weights are renormalised.  A direction that is all zero or not
 * finite gives zeros and no gradient.  Directions need not be normalised.
 * Directions: dirs [n,3], or (dirs null) generated per pixel i = y * width + x from ray_matrix_host (HOST memory, 9
 *   floats, row-major M = R^T K^-1): d = M (x + px, y + py, 1), (px, py) = perturb[i] ([n,2], nullable: 0.5, 0.5).  This
 *   is get_rays_torch (street_gaussian/utils/graphics_utils.py:200-221) with the camera origin cancelled.
 * Pixel mask (at most one of the two, both nullable): mask u8 [n] non-zero, or acc fp32 [n] as (1 - acc) > 1e-3 in fp32
 *   (sky_cubemap.py:88).  A sample outside the mask gets `fill` in every channel and no gradient.
 * flags: SC_CUBE_SIGMOID applies 1 / (1 + exp(-v)) to each tap (the stored map holds logits, sky_cubemap.py:102);
 *   SC_CUBE_CLAMP clamps the result to [0,1]; SC_CUBE_PLANAR writes out [C,n] instead of [n,C].
 * sc_cubemap_bwd: grad_out in out's layout; grad_tex [6,R,R,C] is OVERWRITTEN (zeroed, then fp32 atomic adds of
 *   weight * grad * activation' per tap; zeros when no sample is inside the mask).  The sum order is not fixed.
 * Nothing waits for the device.  SC_EINVAL (nothing launched): R or C out of range, n < 0 or >= 2^38, unknown flag bits,
 *   both or neither of dirs / ray_matrix_host, perturb without ray_matrix_host, width <= 0 or n not a multiple of width
 *   with ray_matrix_host, both mask and acc, a null required pointer.  n == 0: SC_OK. */
#define SC_CUBE_SIGMOID 1
#define SC_CUBE_CLAMP 2
#define SC_CUBE_PLANAR 4
int sc_cubemap_fwd(const float* tex, int resolution, int channels, const float* dirs /* nullable */,
                   const float* ray_matrix_host /* nullable */, const float* perturb /* nullable */,
                   const uint8_t* mask /* nullable */, const float* acc /* nullable */, int64_t n, int width, int flags,
                   float fill, float* out, sc_stream_t stream);
int sc_cubemap_bwd(const float* tex, int resolution, int channels, const float* dirs /* nullable */,
                   const float* ray_matrix_host /* nullable */, const float* perturb /* nullable */,
                   const uint8_t* mask /* nullable */, const float* acc /* nullable */, int64_t n, int width, int flags,
                   float fill, const float* grad_out, float* grad_tex, sc_stream_t stream);

/* ---- perceptual loss: the arithmetic of lpips(image * mask, gt * mask) around the network's convolutions
 *      (train.py:172,185; lpipsPyTorch/modules/lpips.py:30-36 LPIPS.forward, networks.py:50-63 z_score and the taps,
 *      utils.py:6-8 normalize_activation).  The convolutions, ReLU and max-pool stay with the caller.
 * PREP.  sc_lpips_prep_fwd: out [3,H,W] contiguous, out_c = (where(mask, img_c, 0) - mean_c) / std_c, every operation
 *   rounded separately, IEEE division: for finite images bit-identical to torch's ((img * mask) - mean) / std.  img is
 *   fp32 [3,H,W] read through strides_host[5] (host memory, elements, >= 0) = img (channel, row, column), mask (row,
 *   column); mask u8 [1,H,W] non-zero = keep, NULL keeps every pixel (its two strides are then not looked at).
 *   mean_host / std_host: three host floats each.  sc_lpips_prep_bwd: grad_img [3,H,W] contiguous = grad_out_c / std_c
 *   where the mask keeps the pixel, +0 elsewhere (the image strides are not looked at): autograd's two roundings.
 *   SC_EINVAL (nothing launched): H or W <= 0, a negative stride, a null required pointer, std_c == 0.
 * HEAD.  For n_taps <= SC_LPIPS_MAX_TAPS taps l with features fx_l, fy_l fp32 [C_l, P_l] (pixel stride 1, channel
 *   strides stride_x, stride_y >= P_l, independent of one another) and weights w_l [C_l]:
 *     n(f)_p = sqrtf(sum_c f_cp^2)      fh_cp = f_cp / (n_p + 1e-10f)
 *     d_l = (1 / P_l) sum_p sum_c w_lc (fhx_cp - fhy_cp)^2          out[l] = d_l, out[n_taps] = d_0 + ... + d_{n_taps-1}
 *   The difference is formed before it is squared: fx == fy gives exactly 0.  Sums are deterministic: one double per
 *   workgroup in `workspace`, added in a fixed order, no float atomics.  norm_x / norm_y (nullable, [P_l]) receive n(fx),
 *   n(fy): the backward reads them.  Features so small that f^2 underflows in fp32 are outside the contract.
 *   sc_lpips_head_bwd, with g = *grad_value (device memory, no host round trip), r = 1 / (n + 1e-10f), u_c = fhx_c - fhy_c,
 *   a_c = 2 g w_c u_c / P_l:
 *     grad_fx_k = r a_k - fx_k (r^2 / n) sum_c a_c fx_c      (the second term taken as 0 where n == 0)
 *   and grad_fy the mirror image with -a_c; both [C_l, P_l] contiguous, either nullable per tap (a tap with neither is
 *   skipped); norm_x and norm_y of a tap that is not skipped are required.  Every element has one writer: no atomics.
 *   n == 0 is a DEVIATION from the reference on purpose: autograd of sqrt at 0 gives NaN in the feature gradients of a
 *   pixel whose features are all zero (a ReLU's backward behind the tap drops it again, anything else spreads it); this
 *   returns the finite limit of the closed form along f -> 0.
 *   The table is HOST memory and travels to the kernels by value.  Nothing waits for the device.
 *   SC_EINVAL (nothing launched): n_taps <= 0 or > SC_LPIPS_MAX_TAPS, a null table, channels or pixels <= 0, a channel
 *   stride < pixels, a null required pointer, more than 2^31 - 1 workgroups of 64 pixels.  SC_EWORKSPACE: workspace null,
 *   not 8-byte aligned or smaller than sc_lpips_head_workspace_bytes (0 for a bad table). */
#define SC_LPIPS_MAX_TAPS 8
typedef struct {
    const float* fx;
    const float* fy;
    const float* weight;
    float* norm_x;          /* forward: nullable output; backward: input */
    float* norm_y;
    float* grad_fx;         /* backward only, nullable */
    float* grad_fy;
    int64_t stride_x;       /* channel strides, elements */
    int64_t stride_y;
    int32_t channels;
    int32_t pixels;
} sc_lpips_tap;
int sc_lpips_prep_fwd(const float* img, const uint8_t* mask /* nullable */, const int64_t* strides_host, int height,
                      int width, const float* mean_host, const float* std_host, float* out, sc_stream_t stream);
int sc_lpips_prep_bwd(const float* grad_out, const uint8_t* mask /* nullable */, const int64_t* strides_host, int height,
                      int width, const float* std_host, float* grad_img, sc_stream_t stream);
size_t sc_lpips_head_workspace_bytes(const sc_lpips_tap* taps_host, int n_taps);
int sc_lpips_head_fwd(const sc_lpips_tap* taps_host, int n_taps, float* out /* [n_taps + 1] */, void* workspace,
                      size_t workspace_bytes, sc_stream_t stream);
int sc_lpips_head_bwd(const sc_lpips_tap* taps_host, int n_taps, const float* grad_value, sc_stream_t stream);

/* ---- perceptual loss: the convolution stack between the prep and the head (lpipsPyTorch/modules/networks.py:53-63,
 *      the loop `x = layer(x)` over torchvision's alexnet / vgg16 features; reached from train.py:172,185).  Opt-in: the
 *      default route of street_crafter_amd/lpips.py runs these layers on torch.  The weights are frozen (networks.py
 *      set_requires_grad(False)), so the backward is the data gradient only.
 * All tensors fp32 planes, contiguous: x [cin,h,w], y [cout,oh,ow], weight [cout,cin,kh,kw] as torch holds it.
 * Geometry: kh, kw in 1..11, strides in 1..4, zero padding 0 <= p < k, no dilation, no groups, up to 32767 channels;
 *   oh = (h + 2 py - kh) / sy + 1 (floor; 0 when the padded input is smaller than the kernel), ow alike, and the caller's
 *   oh, ow must be these numbers.  Edges are handled in the kernels: no padded copy of anything.
 * PACK.  sc_conv_pack_fwd / sc_conv_pack_dgrad write the weights once per criterion into the layout the MFMA kernel
 *   reads (K-major, zero filled to its tile multiples, followed by one int32 per k naming (channel, ky, kx)); `packed`
 *   16-byte aligned, sc_conv_pack_bytes(cin, cout, kh, kw, dgrad) bytes (0 for a geometry outside the limits).  The
 *   dgrad form has the channel roles swapped and the taps flipped.
 * sc_conv2d_relu_fwd: y = conv(x) + bias (bias nullable), then max(y, 0) when relu = 1; one writer per element, the
 *   pre-activation never reaches memory.  Implicit GEMM on v_mfma_f32_16x16x4_f32: float32 with one rounding per product-sum,
 *   in a fixed order over k = (c kh + ky) kw + kx (within gamma(K) sum |x||w| of the exact sum, gamma(n) = n u / (1 - n u),
 *   u = 2^-24, whatever the order), then ONE rounded add of the bias.
 * sc_conv2d_dgrad (stride 1 only): grad_in [cin,h,w] = conv_transpose(g', weight) (+ add), g' = grad_out where
 *   relu_out > 0 else +0 (relu_out [cout,oh,ow] is the SAVED ReLU output of this convolution; NULL: no mask); `add`
 *   (nullable, [cin,h,w]: the gradient the head hands back for this tensor when it is a tap) is ONE rounded add after
 *   the sum.  The same MFMA kernel over the dgrad pack, padding k - 1 - p.
 * sc_conv2d_dgrad_strided (any stride in 1..4): the same result by gather on the VALU, one thread per element of
 *   grad_in over the (channel, oy, ox) that read it, in increasing order, fmaf; reads `weight` itself, not a pack.
 * sc_maxpool2d_fwd / _bwd: window kh x kw (1..16), strides >= 1, no padding, no dilation, floor mode:
 *   oh = (h - kh) / sy + 1 (0 when h < kh).  The maximum is the FIRST one in row-major window order under torch's
 *   comparison (v > best || isnan(v)).  The backward is a gather: every element of x looks at the windows that cover it,
 *   recomputes each window's arg-max and adds grad_out of those that chose it, in increasing (oy, ox) order from +0, then
 *   `add` (nullable, as above): bit-equal to torch's CPU autograd.  No index tensor.
 * No atomics, no split of K across workgroups: bit-identical from run to run.  Nothing waits for the device.  A pack is
 *   written on the stream handed to sc_conv_pack_*: the calls that read it must run on that stream or after it.
 * SC_EINVAL (nothing launched): a negative size, a geometry outside the limits above, oh / ow that do not follow from
 *   it, more than 2^31 - 1 elements in a tensor, relu not 0 / 1, a null required pointer or an unaligned pack while
 *   there is work.  SC_EWORKSPACE: packed_bytes too small.  0 without a launch for empty work (no channel on either
 *   side or no output position in the forward; no element of grad_in in a backward). */
size_t sc_conv_pack_bytes(int cin, int cout, int kh, int kw, int dgrad);
int sc_conv_pack_fwd(const float* weight, int cin, int cout, int kh, int kw, void* packed, size_t packed_bytes,
                     sc_stream_t stream);
int sc_conv_pack_dgrad(const float* weight, int cin, int cout, int kh, int kw, void* packed, size_t packed_bytes,
                       sc_stream_t stream);
int sc_conv2d_relu_fwd(const float* x, const void* packed, size_t packed_bytes, const float* bias /* nullable */, int cin,
                       int h, int w, int cout, int kh, int kw, int sy, int sx, int py, int px, int oh, int ow, int relu,
                       float* y, sc_stream_t stream);
int sc_conv2d_dgrad(const float* grad_out, const float* relu_out /* nullable */, const void* packed_dgrad,
                    size_t packed_bytes, const float* add /* nullable */, int cin, int h, int w, int cout, int kh, int kw,
                    int py, int px, int oh, int ow, float* grad_in, sc_stream_t stream);
int sc_conv2d_dgrad_strided(const float* grad_out, const float* relu_out /* nullable */, const float* weight,
                            const float* add /* nullable */, int cin, int h, int w, int cout, int kh, int kw, int sy,
                            int sx, int py, int px, int oh, int ow, float* grad_in, sc_stream_t stream);
int sc_maxpool2d_fwd(const float* x, int channels, int h, int w, int kh, int kw, int sy, int sx, int oh, int ow, float* y,
                     sc_stream_t stream);
int sc_maxpool2d_bwd(const float* grad_out, const float* x, const float* add /* nullable */, int channels, int h, int w,
                     int kh, int kw, int sy, int sx, int oh, int ow, float* grad_in, sc_stream_t stream);

/* ---- crop + separable resize of the novel-view training inputs (street_gaussian/utils/diffusion_utils.py:99-115,
 *      called at train.py:160-161 and diffusion_utils.py:193,287-290; the row slice of train.py:164-169)
 * What torchvision's Resize does to a tensor, torch.nn.functional.interpolate(mode="bilinear", align_corners=False) with
 * or without antialias, as one weighted gather per output: out[b,c,r,ox] = a * sum_jy wy[jy] (sum_jx wx[jx]
 * x[b,c,ys+jy,xs+jx]) + b for the output row oy = r + row_begin; only rows oy >= row_begin exist in out
 * ([B,C,h_out - row_begin,w_out], contiguous).  The sums run in table order, x inside y, in fp32.
 * TAP TABLES (DEVICE memory, built by the caller: street_crafter_amd/resize.py tap_table): for an axis with n entries,
 *   idx int32 [2n+1] = start[n] then offset[n+1], w fp32 [offset[n]]; entry i reads start[i] .. start[i] + (offset[i+1] -
 *   offset[i]) - 1 with the weights w[offset[i] ..].  Forward tables have one entry per OUTPUT index and start in the
 *   (cropped) input; the transposed tables of sc_resize_bwd have one entry per cropped INPUT index and start in the output
 *   (the contiguous run of outputs that read it).  No tap bound.  The tables are trusted; image indices read through them
 *   are clamped to the image.
 * x: fp32, the first element of the CROPPED region, read in place through strides_host = {batch, channel, row, column}
 *   element strides (>= 0); in_h x in_w is the cropped size.  SC_RESIZE_PACKED4 promises that 16 bytes can be read at
 *   every pixel (channel stride 1, column stride 4, channels <= 4, everything 16-byte aligned: the rasterizer's
 *   [H,W,4] output); all channels of a tap are then one load.
 * SC_RESIZE_AFFINE applies a, b (else they are ignored and the sum is stored as it is).
 * sc_resize_mask_fwd: x u8 (bool) with the same geometry, out u8 = 1 iff any tap of the two tables is non-zero.
 * sc_resize_bwd: grad_out in out's layout; grad_x fp32 [B,C,height,width] contiguous, EVERY element written once:
 *   a * sum over the transposed tables' outputs with oy >= row_begin inside the crop (top, left, in_h, in_w), +0
 *   elsewhere and where no output contributes.  No memset, no atomics: bit-identical from run to run.
 * Nothing waits for the device.  SC_EINVAL (nothing launched): a size <= 0, batch * channels > 65535, row_begin outside
 *   [0, h_out), a negative stride, unknown flag bits, SC_RESIZE_PACKED4 on a layout that is not the one above, a crop
 *   outside the image, a null pointer. */
#define SC_RESIZE_AFFINE 1
#define SC_RESIZE_PACKED4 2
int sc_resize_fwd(const float* x, const int64_t* strides_host, int batch, int channels, int in_h, int in_w,
                  const int32_t* ty_idx, const float* ty_w, const int32_t* tx_idx, const float* tx_w, int h_out, int w_out,
                  int row_begin, int flags, float a, float b, float* out, sc_stream_t stream);
int sc_resize_mask_fwd(const uint8_t* x, const int64_t* strides_host, int batch, int channels, int in_h, int in_w,
                       const int32_t* ty_idx, const int32_t* tx_idx, int h_out, int w_out, int row_begin, uint8_t* out,
                       sc_stream_t stream);
int sc_resize_bwd(const float* grad_out, int batch, int channels, int height, int width, int top, int left, int in_h,
                  int in_w, const int32_t* uy_idx, const float* uy_w, const int32_t* ux_idx, const float* ux_w, int h_out,
                  int w_out, int row_begin, int flags, float a, float* grad_x, sc_stream_t stream);

/* ---- the tail of the training step: optimizer.step() of every sub-model (train.py:319, street_gaussian_model.py:
 *      467-484; torch.optim.Adam(l, lr=0.0, eps=1e-15), gaussian_model.py:305) in one call
 * Multi-tensor Adam, torch's non-amsgrad, no-weight-decay formula, per element in fp32:
 *   m' = m + (1 - b1) (g - m)      v' = b2 v + (1 - b2) g^2      p' = p - step_size * m' / (sqrt(v') / bias2_sqrt + eps)
 * param, exp_avg, exp_avg_sq are updated in place.  step_size = lr / (1 - b1^t) and bias2_sqrt = sqrt(1 - b2^t) are the
 * caller's (computed in double, as torch does) and per tensor: a parameter skipped for a missing grad keeps its own t.
 * table_host is HOST memory; it travels to the kernel by value in the kernel arguments, sc_adam_max_tensors() entries
 * per launch (more entries: more launches inside the call): no host-to-device copy, no workspace, no synchronisation.
 * Tensors whose four pointers are 16-byte aligned move as 16-byte vectors with a scalar tail; others element by
 * element.  numel == 0 is legal (its pointers are not looked at).  Tensors of one call must not overlap.
 * n_tensors == 0: returns 0, nothing launched.  SC_EINVAL (nothing launched): n_tensors < 0, a null table with
 * n_tensors > 0, a negative numel, a null pointer in an entry with numel > 0. */
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    float step_size;
    float bias2_sqrt;
} sc_adam_tensor;
int sc_adam_max_tensors(void);
int sc_adam_step(const sc_adam_tensor* table_host, int n_tensors, float one_minus_beta1, float beta2,
                 float one_minus_beta2, float eps, sc_stream_t stream);

/* ---- densification statistics of one render (train.py:283-290; street_gaussian_model.py:486-533 set_max_radii2D +
 *      add_densification_stats; in-repo statement: street_crafter_amd/densify_stats.py DensificationStats)
 * grad [N,2] = viewspace_points.grad, absgrad [N,2] (nullable) = .absgrad, radii [N] int32 (radii_is_float == 0) or
 * fp32, visible u8 [N].  Each segment is one sub-model: rows [start, end) of the render, accumulators of end - start
 * rows.  For every row i of a segment with visible[i], r = i - start:
 *   max_radii[r] = max(max_radii[r], (float)radii[i]) (NaN propagates, as torch.max);   denom[r] += 1;
 *   with absgrad:    grad_accum[r,0] += ||(absgrad[i] * 0.5) * (W, H)||,  grad_accum[r,1] += ||(grad[i] * 0.5) * (W, H)||
 *                    (half_width = 0.5 W, half_height = 0.5 H)
 *   without absgrad: grad_accum[r,0] += ||grad[i]||,  grad_accum[r,1] += 0
 * Invisible rows and rows outside every segment are not written.  Segments travel by value in the kernel arguments
 * (segments_host is HOST memory); one launch for up to 64 non-empty segments.  No atomics (accumulators of different
 * segments must not overlap), no synchronisation.
 * n_segments == 0, or every segment empty: returns 0, nothing launched.  SC_EINVAL (nothing launched): N < 0,
 * n_segments < 0, a null segments_host, a segment with start < 0, start > end, end > N or a null accumulator, a null
 * grad, radii or visible when some segment is not empty. */
typedef struct {
    int64_t start, end;
    float* grad_accum; /* [n,2] */
    float* denom;      /* [n,1] */
    float* max_radii;  /* [n] */
} sc_stats_segment;
int sc_densify_stats(const float* grad, const float* absgrad /* nullable */, const void* radii, int radii_is_float,
                     const uint8_t* visible, int64_t N, float half_width, float half_height,
                     const sc_stats_segment* segments_host, int n_segments, sc_stream_t stream);

/* ---- densify and prune of any number of sub-models (train.py:292-299; StreetGaussianModel.densify_and_prune,
 *      street_gaussian_model.py:535-549; per sub-model gaussian_model.py:363-547 densify_and_clone / densify_and_split /
 *      prune_points with prune_optimizer / cat_optimizer, gaussian_model_bkgd.py:100-157, gaussian_model_actor.py:201-272)
 * Two calls, because the caller sizes the new tensors in between from ONE read of the counters.
 *
 * sc_densify_plan: which rows the new population consists of.  Per original row i of a job, from that row's data alone:
 *   g = grad_accum[i, grad_col] / denom[i] (NaN -> 0); hot = g >= max_grad; s = exp(scaling[i]);
 *   small = max(s) <= dense_size (= percent_dense * extent); clone = hot && small; split = hot && !small.
 *   Four candidate rows ("slots"): 0 the original (exists when !split), 1 its clone (clone), 2 / 3 the split children
 *   k = 0 / 1 (split).  A child has xyz' = xyz + R(q / |q|) (split_noise[k,i] * s) (R: the w-x-y-z matrix of
 *   general_utils.py:125-146) and raw scaling' = log(s / 1.6f); everything else of a child, and all of a clone, is the
 *   parent's raw row.  An existing candidate c is pruned when
 *     sigmoid(opacity[i]) < min_opacity, or
 *     prune_big != 0 and max(exp(scaling_c)) > big_size (= extent * percent_big_ws; for a child the exp of the fresh raw
 *       value) -- with region 1 (sphere: region_a = centre, region_b[0] = radius; gaussian_model_bkgd.py:126-129) only
 *       where !(|xyz_c - centre| > radius) --, or
 *     prune_big != 0 and region 2 (box: region_a = min_xyz, region_b = max_xyz; gaussian_model_actor.py:231-251) and one
 *       of the two samples xyz_c + R (box_noise[slot,i,m] * s_c), m = 0 / 1, is not inside [min_xyz, max_xyz], or
 *     slot 0 and max_screen_size > 0 and max_radii[i] > max_screen_size.
 *   Output order is the reference's (repeat + appended rows + mask): surviving originals in row order, surviving clones in
 *   source-row order, surviving children 0, surviving children 1.  Written per job: src_row i32 / slot u8, n' entries
 *   (capacity 2 n: a row leaves at most two rows, itself and its clone or its two children); child_xyz / child_scaling
 *   [2,n,3], rows of split parents only; counters i32[8] = {points_total (= n), points_clone, points_split,
 *   points_below_min_opacity, points_big_ws, points_pruned, n', 0}, the reference's counts over the population after the
 *   split (a split parent is not a pruned point).  counters must be ZERO-FILLED by the caller.
 *   Three launches per sc_densify_max_jobs() non-empty jobs (the table travels by value in the kernel arguments): keep
 *   flags + totals per block of sc_densify_scan_block() rows, an exclusive scan of the totals laid out [slot][block], the
 *   emission.  No workgroup waits for another; the counters are integer atomics: every output is the same from run to run.
 *   No synchronisation with the host.
 * sc_densify_apply: dst[r,:] = src[src_row[r],:] for r < n_out, for the parameter and (when given) both Adam moments of
 *   every group; moments of rows with slot != 0 are zeros; rows with slot 2 / 3 of a group with `child` take
 *   child[slot - 2, src_row[r], :] (the plan's child_xyz / child_scaling) as parameter.  width (floats per row) is
 *   arbitrary, 0 included; a group whose width is a multiple of 4 and whose pointers are 16-byte aligned moves as 16-byte
 *   vectors, others element by element.  n_out == 0 and n == 0 are legal.  sc_densify_max_groups() groups per launch.
 * n_jobs / n_groups == 0: returns 0, nothing launched.  SC_EINVAL (nothing launched): a negative count, a null table, a
 *   job with n < 0 or n >= 2^29, grad_col / region outside their range, max_grad not > 0, a null counters, a null pointer
 *   in a job with n > 0 (box_noise only where it is read), a workspace that is not 16-byte aligned, a group with n, n_out or width < 0, n_out > 2 n, one moment
 *   pointer without the other three, a null pointer in a group with n_out * width > 0.  SC_EWORKSPACE: workspace_bytes <
 *   sc_densify_plan_workspace_bytes (0 for a bad table). */
typedef struct {
    int64_t n;
    const float* xyz;         /* [n,3] */
    const float* scaling;     /* [n,3] raw */
    const float* rotation;    /* [n,4] raw, wxyz */
    const float* opacity;     /* [n] raw */
    const float* grad_accum;  /* [n,2] */
    const float* denom;       /* [n] */
    const float* max_radii;   /* [n] */
    const float* split_noise; /* [2,n,3] standard normal */
    const float* box_noise;   /* [4,n,2,3] standard normal; read only when prune_big != 0 and region == 2 */
    int32_t* src_row;         /* out [2n] */
    uint8_t* slot;            /* out [2n] */
    float* child_xyz;         /* out [2,n,3] */
    float* child_scaling;     /* out [2,n,3] */
    int32_t* counters;        /* in/out [8] */
    float max_grad, dense_size, min_opacity, big_size, max_screen_size;
    float region_a[3], region_b[3];
    int32_t grad_col;         /* 0, or 1 for the densify_grad_abs_* variants */
    int32_t prune_big;
    int32_t region;           /* 0 none, 1 sphere, 2 box */
} sc_densify_job;
typedef struct {
    const float* src_param;       /* [n,width] */
    const float* src_exp_avg;     /* nullable, with the three other moment pointers */
    const float* src_exp_avg_sq;
    float* dst_param;             /* [n_out,width] */
    float* dst_exp_avg;
    float* dst_exp_avg_sq;
    const float* child;           /* nullable: [2,n,width] */
    const int32_t* src_row;       /* [n_out] */
    const uint8_t* slot;          /* [n_out] */
    int64_t n, n_out;
    int32_t width;
    int32_t reserved;
} sc_densify_group;
int sc_densify_scan_block(void);
int sc_densify_max_jobs(void);
int sc_densify_max_groups(void);
size_t sc_densify_plan_workspace_bytes(const sc_densify_job* jobs_host, int n_jobs);
int sc_densify_plan(const sc_densify_job* jobs_host, int n_jobs, void* workspace, size_t workspace_bytes,
                    sc_stream_t stream);
int sc_densify_apply(const sc_densify_group* groups_host, int n_groups, sc_stream_t stream);

/* ---- the head of a frame: StreetGaussianModel.parse_camera + get_scaling / get_rotation / get_xyz / get_features /
 *      get_opacity (street_gaussian_model.py:202-407), GaussianModelActor.get_features_fourier (gaussian_model_actor.py:
 *      67-76), GaussianModelSky.get_scaling / get_xyz (gaussian_model_sky.py:62-76): the flat arrays that
 *      render_kernel_gsplat hands to the projection (street_gaussian_renderer.py:186-209), in one launch
 * Each segment is one sub-model: rows [start, end) of the frame and its six RAW parameter tensors (end - start rows,
 * contiguous fp32): xyz [n,3], scaling [n,3], rotation [n,4] wxyz, opacity [n,1], features_dc [n,F,3] (F = fourier_dim),
 * features_rest [n,K-1,3].  All segments share K (the reference's cat needs that too); with K == 1 features_rest is not
 * looked at.  Arithmetic is fp32.  Per row i of a segment, by kind:
 *   SC_COMPOSE_STATIC (background): means = xyz; quats = rotation / max(|rotation|, 1e-12) (F.normalize);
 *     scales = exp(scaling); opacities = 1 / (1 + exp(-opacity)); sh[:,0] = features_dc[:,0]; sh[:,1:] = features_rest.
 *   SC_COMPOSE_ACTOR (street_gaussian_model.py:296-386): q_l = normalize(rotation), x_l = xyz; where flip[i] (u8 [n],
 *     nullable: no row flips) x_l.y = -x_l.y and q_l = flip_q (x) q_l, flip_q_host being the quaternion of
 *     diag(-1,1,-1) as the reference builds it (:56-58; HOST memory, 4 floats, required when a segment has a flip mask);
 *     means = R(obj_rot) x_l + obj_trans with R of general_utils.quaternion_to_matrix (2 / |q|^2 scaling: obj_rot is NOT
 *     normalised first); quats = normalize(obj_rot (x) q_l), Hamilton product, real part first; obj_rot / obj_trans =
 *     row pose_row of obj_rots [A,4] / obj_trans [A,3] (device); sh[:,0] = sum_f basis[f] features_dc[:,f] with the
 *     caller's IDFT basis (sh_utils.py:120-130 at the frame's time), F <= SC_COMPOSE_MAX_FOURIER; F == 1 is a copy;
 *     scales, opacities, sh[:,1:] as static.
 *   SC_COMPOSE_SKY: as static, except scales = min(exp(scaling), radius) and, with d = xyz - centre and
 *     ratio = |d| / (2 radius), means = centre + d / ratio where ratio < 1, else xyz.  A sky row exactly AT the centre is
 *     outside the contract (the reference divides by zero there).
 * Outputs, contiguous, every element written: means [N,3], quats [N,4], scales [N,3], opacities [N,1], sh [N,K,3].
 * segments_host is HOST memory and travels by value in the kernel arguments: one launch per sc_compose_max_segments()
 * non-empty segments.  The sh block moves as 16-byte vectors where a chunk's run of the output is 16-byte aligned,
 * element by element otherwise.
 * sc_compose_bwd: upstream gradients of the five outputs, each nullable (zeros).  grads_host[k] are segment k's six
 *   gradient tensors in raw parameter space, each written in full and OVERWRITTEN (zeros where nothing arrives): through
 *   exp, sigmoid, both normalisations (below the 1e-12 floor: g / 1e-12), the flip, the sky projection, the clamp (the
 *   scales gradient passes iff exp(scaling) <= radius, as torch.clamp) and the basis (features_dc of an actor gets
 *   basis[f] times the DC gradient; features_dc[:,1:] of another kind gets zeros).  grad_obj_rots [A,4] and
 *   grad_obj_trans [A,3], each nullable (the reduction is then skipped; the parameter gradients are the same bits
 *   either way): zeroed, then fp32 atomic adds of per-workgroup partial sums over each actor's rows; the sum order is
 *   not fixed.  Rows of poses no segment names stay zero.
 * Nothing waits for the device.  N == 0: SC_OK, nothing launched.  Empty segments are legal.  SC_EINVAL (nothing
 * launched): N, A or n_segments < 0, a null table with n_segments > 0, K < 1, a segment with start > end, segments that
 * do not tile [0,N) in order, an unknown kind, fourier_dim outside [1, SC_COMPOSE_MAX_FOURIER], an actor whose pose_row is
 * outside [0,A), a null pointer in a non-empty segment (features_rest only when K > 1; obj_rots / obj_trans when there
 * is an actor row; flip_q_host when there is a flip mask), a null output with N > 0. */
#define SC_COMPOSE_STATIC 0
#define SC_COMPOSE_ACTOR 1
#define SC_COMPOSE_SKY 2
#define SC_COMPOSE_MAX_FOURIER 8
typedef struct {
    int64_t start, end;
    const float* xyz;
    const float* scaling;
    const float* rotation;
    const float* opacity;
    const float* features_dc;
    const float* features_rest; /* not looked at when K == 1 */
    const uint8_t* flip;        /* actors, nullable */
    int32_t kind;
    int32_t pose_row;           /* actors */
    int32_t fourier_dim;        /* F */
    int32_t reserved;
    float basis[SC_COMPOSE_MAX_FOURIER]; /* actors: the first F entries */
    float centre[3];            /* sky */
    float radius;               /* sky */
} sc_compose_segment;
typedef struct {
    float* xyz;
    float* scaling;
    float* rotation;
    float* opacity;
    float* features_dc;
    float* features_rest;       /* not looked at when K == 1 */
} sc_compose_grads;
int sc_compose_max_segments(void);
int sc_compose_fwd(const sc_compose_segment* segments_host, int n_segments, int64_t N, int K, const float* obj_rots,
                   const float* obj_trans, int A, const float* flip_q_host /* nullable */, float* means, float* quats,
                   float* scales, float* opacities, float* sh, sc_stream_t stream);
int sc_compose_bwd(const sc_compose_segment* segments_host, const sc_compose_grads* grads_host, int n_segments, int64_t N,
                   int K, const float* obj_rots, const float* obj_trans, int A, const float* flip_q_host /* nullable */,
                   const float* g_means, const float* g_quats, const float* g_scales, const float* g_opacities,
                   const float* g_sh, float* grad_obj_rots /* nullable */, float* grad_obj_trans /* nullable */,
                   sc_stream_t stream);

/* ---- the actor poses of a frame: ActorPose.get_tracking_rotation / get_tracking_translation of every visible actor
 *      (street_gaussian/models/actor_pose.py:83-144, general_utils.quaternion_raw_multiply_theta :222-241), the inputs
 *      obj_rots [A,4] / obj_trans [A,3] of sc_compose_fwd, in one launch; backward into the opt_trans / opt_rots tables
 * The tracklet tables are flat: rows = cams * frames * max_obj, a row index is the flat index into the reference's
 * [cams, frames, max_obj, .] tensors.  input_trans [rows,3], input_rots [rows,4] wxyz (not normalised), opt_trans
 * [rows,3], opt_rots [rows,1] (an angle about the local z axis), contiguous fp32.  Item i gives row i of the outputs.
 * Every fp32 product, sum and quotient is rounded on its own (no contraction).  P(row), the plain pose at a row:
 *     t = input_trans[row]                              (+ opt_trans[row] with SC_POSE_DELTA)
 *     q = a = input_rots[row];  with SC_POSE_DELTA, c = cosf(opt_rots[row] / 2), s = sinf(opt_rots[row] / 2):
 *         q = (aw c - az s,  ax c + ay s,  ay c - ax s,  az c + aw s)          NOT normalised: sc_compose_fwd takes it raw
 *   without SC_POSE_INTERP: (t, q) = P(row).
 *   with SC_POSE_INTERP (a validation frame between two valid neighbours): (t_p, p) = P(row_prev), (t_n, n) = P(row_next);
 *     t = alpha * t_n + one_minus_alpha * t_p (two products, one sum);  q = slerp(p, n, alpha), the geometric one:
 *     ph = p / max(|p|, 1e-12), nh likewise; r = conj(ph) (x) nh, negated when r.w < 0 (the shorter arc); with
 *     v = (r.x, r.y, r.z) and phi = atan2f(|v|, r.w):  q = ph (x) (cosf(alpha phi), v sinf(alpha phi) / |v|); where
 *     phi <= 1e-3 the series (1 - (alpha phi)^2 / 2,  v alpha (1 + (1 - alpha^2) phi^2 / 6)), so p == n gives ph and
 *     nothing is NaN.  The sign of q follows ph.  Hamilton products sum their four terms left to right.
 * items_host is HOST memory and travels by value in the kernel arguments: one launch per sc_actor_poses_max_items()
 * items, one thread per item.  No staging buffer, no copy.
 * sc_actor_poses_bwd: g_obj_rots [A,4] / g_obj_trans [A,3], each nullable (zeros).  grad_opt_trans [rows,3] and
 *   grad_opt_rots [rows,1], each nullable (not computed), are OVERWRITTEN in full: one memset per table, then plain
 *   stores at the rows of the SC_POSE_DELTA items: grad_opt_trans[row] = g_obj_trans[i]; grad_opt_rots[row] =
 *   sum_k g_k d q_k / d theta with dc = -s / 2, ds = c / 2 (four terms, summed in the order w, x, y, z).  No atomics: the
 *   same bits from run to run.  An SC_POSE_INTERP item is SC_EUNSUPPORTED (the reference interpolates validation frames
 *   only, and those are rendered under no_grad: train.py:240,313, render.py).
 * Nothing waits for the device.  A == 0: SC_OK, nothing launched.  SC_EINVAL (nothing launched): A or rows < 0, a null
 * table with A > 0, a row an item uses (row; row_prev and row_next with SC_POSE_INTERP) outside [0, rows), unknown flag
 * bits, a null input_trans / input_rots, SC_POSE_DELTA with a null opt_trans / opt_rots (backward: a null input_rots /
 * opt_rots when grad_opt_rots is asked for and an item has SC_POSE_DELTA), a null output with A > 0 (forward), two
 * SC_POSE_DELTA items of a backward call naming the same row. */
#define SC_POSE_DELTA 1   /* add opt_trans / rotate by opt_rots: opt_track and not a novel view */
#define SC_POSE_INTERP 2  /* validation frame between two valid neighbours */
typedef struct {
    int32_t row, row_prev, row_next, flags;
    float alpha, one_minus_alpha;
} sc_actor_pose_item;
int sc_actor_poses_max_items(void);
int sc_actor_poses_fwd(const sc_actor_pose_item* items_host, int A, int64_t rows, const float* input_trans,
                       const float* input_rots, const float* opt_trans /* nullable */, const float* opt_rots /* nullable */,
                       float* obj_rots, float* obj_trans, sc_stream_t stream);
int sc_actor_poses_bwd(const sc_actor_pose_item* items_host, int A, int64_t rows, const float* input_rots,
                       const float* opt_rots, const float* g_obj_rots /* nullable */, const float* g_obj_trans /* nullable */,
                       float* grad_opt_trans /* nullable */, float* grad_opt_rots /* nullable */, sc_stream_t stream);

/* ---- scene initialisation: from the LiDAR sweeps to the first Gaussians (street_gaussian/pointcloud_processor/
 *      base_processor.py:65-131 initailize_ply; models/gaussian_model.py:56-80, gaussian_model_actor.py:79-157) ------------
 * Points and colours of the two open3d calls are float64 [n,3], contiguous; every decision is taken in float64 with each
 * operation rounded on its own.  Both calls are RESTATEMENTS: open3d's source is not vendored, parity with it is unpinned.
 * Each of them reads the cloud's bounds back (the bit widths of the cell key come from the extents): they WAIT for the
 * stream.  Nothing persistent is allocated.  SC_EINVAL before any launch: n <= 0 (n < 0 for the radius filter) or
 * n >= 2^31, a null required pointer, voxel_size / radius not positive and finite, nb_points < 0; after the bounds are known:
 * a coordinate that is NaN or infinite, or a cell key of more than 63 bits.
 *
 * sc_point_bounds_f32 / _f64: bounds_host[6] = min x y z, max x y z of xyz [n,3]; exact in any order.
 *
 * sc_voxel_downsample_plan: vmin = min - 0.5 voxel_size; the voxel index per axis is floor((p - vmin) / voxel_size), one
 *   subtraction and one IEEE division; key = ix << (by + bz) | iy << bz | iz with bx, by, bz the bits the largest index of
 *   each axis needs; a stable radix sort over exactly bx + by + bz bits with the input index as value; segment heads,
 *   scan, compacted segment starts.  *m_host: the number of occupied voxels (the second and last wait).  info_host
 *   (nullable) [4] = bx, by, bz, the number of points in the fullest voxel.
 * sc_voxel_downsample_reduce, with the workspace the plan left for the same xyz and n, and m = *m_host: voxel s in
 *   ascending key order, i.e. lexicographic (ix, iy, iz): points[s] / colors_out[s] = the float64 sum of its points /
 *   colours taken SEQUENTIALLY IN ASCENDING INPUT INDEX (open3d's accumulation order), divided by counts[s].  Same bits
 *   from run to run.  colors nullable (colors_out is then not written).  One lane walks one voxel: a crowded voxel is a
 *   long serial walk by design, nothing is reassociated.
 *
 * sc_radius_outlier_mask: keep[i] = 1 when #{ j : d2(i, j) < radius * radius } > nb_points, else 0; the count includes i
 *   itself, the comparison is strict, d2 = (dx dx + dy dy) + dz dz.  An integer count: exact and order-free.  Cells of
 *   edge radius (1 + 2^-20) (at most 26 key bits per axis: SC_EINVAL beyond), a table of the occupied cells, nine column
 *   searches per point, counting stops once the count exceeds nb_points.  info_host (nullable) [3] = bx, by, bz.
 *
 * sc_gaussian_init: one launch.  rgb [m,3], dist2 [m] (sc_knn3_mean_dist2), fp32.
 *     features_dc [m, fourier_dim, 3]: row 0 = (rgb - 0.5) / 0.28209479177387814 (RGB2SH), the other rows 0
 *     features_rest [m, n_rest, 3] = 0 (nullable when n_rest == 0)      semantic [m, num_classes] = 0 (likewise)
 *     scaling [m,3] = logf(sqrtf(max(dist2, 1e-7f))) three times        rotation [m,4] = (1, 0, 0, 0)
 *     opacity_out [m,1] = opacity (the host's inverse_sigmoid(0.1))     max_radii2d [m] = 0 */
size_t sc_point_bounds_workspace_bytes(void);
int sc_point_bounds_f32(const float* xyz, int64_t n, float* bounds_host, void* workspace, size_t ws_bytes,
                        sc_stream_t stream);
int sc_point_bounds_f64(const double* xyz, int64_t n, double* bounds_host, void* workspace, size_t ws_bytes,
                        sc_stream_t stream);
size_t sc_voxel_downsample_workspace_bytes(int64_t n);
int sc_voxel_downsample_plan(const double* xyz, int64_t n, double voxel_size, void* workspace, size_t ws_bytes,
                             int64_t* m_host, int32_t* info_host /* nullable */, sc_stream_t stream);
int sc_voxel_downsample_reduce(const double* xyz, const double* colors /* nullable */, int64_t n, int64_t m,
                               const void* workspace, size_t ws_bytes, double* points, double* colors_out /* nullable */,
                               int32_t* counts, sc_stream_t stream);
size_t sc_radius_outlier_workspace_bytes(int64_t m);
int sc_radius_outlier_mask(const double* xyz, int64_t m, int nb_points, double radius, uint8_t* keep, void* workspace,
                           size_t ws_bytes, int32_t* info_host /* nullable */, sc_stream_t stream);
int sc_gaussian_init(const float* rgb, const float* dist2, int64_t m, int fourier_dim, int n_rest, int num_classes,
                     float opacity, float* features_dc, float* features_rest /* nullable */, float* scaling, float* rotation,
                     float* opacity_out, float* semantic /* nullable */, float* max_radii2d, sc_stream_t stream);

/* ---- fused forward behind gsplat.rendering.rasterization() (imported at
 *      street_gaussian/models/street_gaussian_renderer.py:204) -------------------------------------
 * sc_camera_centers: out[c] = -R^T t of the rigid world-to-camera matrices viewmats [C,4,4]
 *   (= Camera.camera_center, street_gaussian/utils/camera_utils.py:51; gsplat takes inverse(viewmat)).
 * sc_projection_sh_fwd: renderer.py:219-266 in one pass per (camera, Gaussian): projection, opacity *
 *   compensation (when antialiased), dirs = mean - camera centre, SH colour where radius > 0,
 *   clamp_min(colour + 0.5, 0), depth appended as 4th channel.  opacities [N], sh_coeffs [N,K,3];
 *   outputs radii [C,N], means2d [C,N,2], depths [C,N], conics [C,N,3], opacities_out [C,N],
 *   colors4 [C,N,4].  Bit-identical to the separate operators + torch glue.
 * sc_rasterize_fwd_ed: sc_rasterize_fwd (no last_ids) whose 4th output channel is divided by
 *   max(alpha, 1e-10) (renderer.py:284; gsplat render_mode "RGB+ED").  D must be 4 and tile_size 16,
 *   otherwise SC_EUNSUPPORTED. */
int sc_camera_centers(const float* viewmats, int C, float* out, sc_stream_t stream);
int sc_projection_sh_fwd(const float* means, const float* quats, const float* scales,
                         const float* opacities, const float* sh_coeffs, const float* viewmats,
                         const float* Ks, const float* camera_centers, int C, int N, int K,
                         int sh_degree, int width, int height, float eps2d, float near_plane,
                         float far_plane, float radius_clip, int antialiased, int32_t* radii,
                         float* means2d, float* depths, float* conics, float* opacities_out,
                         float* colors4,
                         float* records /* nullable: [C,N,12], 16-B aligned: everything the rasterizer gathers per
                             splat in one 48-B record (x, y, conic a, b | conic c, opacity, colour 0, 1 | colour 2,
                             3, -, -) for sc_rasterize_fwd_packed.  With records, conics / opacities_out / colors4
                             may each be NULL (sc_records_unpack rebuilds them on demand) */,
                         sc_stream_t stream);
/* The VJP of sc_projection_sh_fwd with respect to the five leaves, in one kernel (the training form of
 * gsplat.rendering.rasterization()): camera tensors carry no gradient, as in sc_projection_bwd.  radii / conics are the
 * forward's.  Upstream: v_means2d [C,N,2], v_depths [C,N] (nullable: the depth then arrives through v_colors4[..., 3]
 * alone), v_conics [C,N,3], v_opacities_out [C,N], v_colors4 [C,N,4] (16-B aligned).  A (camera, Gaussian) with
 * radii <= 0 is skipped WITHOUT its upstream rows being read.  Outputs v_means [N,3], v_quats [N,4], v_scales [N,3],
 * v_opacities [N], v_sh [N,K,3]: each nullable (not computed then), each written in full and overwritten, exact zeros
 * for a Gaussian visible in no camera and for the bases beyond (sh_degree + 1)^2.  No atomics: the result is the same
 * from run to run.  The compensation is recomputed; the clamp passes where the forward's SH colour + 0.5 >= 0. */
int sc_projection_sh_bwd(const float* means, const float* quats, const float* scales,
                         const float* opacities, const float* sh_coeffs, const float* viewmats,
                         const float* Ks, const float* camera_centers, int C, int N, int K,
                         int sh_degree, int width, int height, float eps2d, int antialiased,
                         const int32_t* radii, const float* conics, const float* v_means2d,
                         const float* v_depths, const float* v_conics, const float* v_opacities_out,
                         const float* v_colors4, float* v_means, float* v_quats, float* v_scales,
                         float* v_opacities, float* v_sh, sc_stream_t stream);
/* sc_rasterize_fwd (4 channels, tile 16, no last_ids) reading `records` instead of the four parameter arrays: one
 * gather line per splat instead of four.  depth_normalise != 0: the epilogue of
 * sc_rasterize_fwd_ed.  Bit-identical output.  SC_EUNSUPPORTED when the reference-shaped raster kernel is selected. */
int sc_rasterize_fwd_packed(const float* records, const float* backgrounds, const uint8_t* tile_masks,
                            int C, int N, int width, int height, int tile_width, int tile_height,
                            const int32_t* isect_offsets, const int32_t* flatten_ids, int64_t n_isects,
                            float* render_colors, float* render_alphas, const int32_t* tile_order,
                            int32_t* tile_work, int depth_normalise, sc_stream_t stream);
/* sc_rasterize_fwd with render_colors stored as PLANES, [C][D][H][W] (one plane per channel), for inference (no
 * last_ids).  The reference's caller slices the result channel-wise right behind the operator
 * (street_gaussian_renderer.py:282-300: `render_colors[..., :-1]`, `[..., -1:] / alpha`, clamp, `.permute(2, 0, 1)`):
 * strided kernels over the interleaved buffer, dense ones over planes.  The Python operator hands the buffer out as a
 * permuted [C,H,W,D] view, so the values a caller sees are identical.  Wave kernel only (tile_size 16, D = 3 or 4):
 * SC_EUNSUPPORTED otherwise. */
int sc_rasterize_fwd_planar(const float* means2d, const float* conics, const float* colors,
                            const float* opacities, const float* backgrounds, const uint8_t* tile_masks,
                            int C, int N, int D, int width, int height, int tile_size,
                            int tile_width, int tile_height,
                            const int32_t* isect_offsets, const int32_t* flatten_ids, int64_t n_isects,
                            float* render_colors, float* render_alphas,
                            const int32_t* tile_order, int32_t* tile_work, sc_stream_t stream);
/* conics [CN,3] / opacities [CN] / colors4 [CN,4] (each nullable) out of CN records */
int sc_records_unpack(const float* records, int64_t CN, float* conics, float* opacities, float* colors4,
                      sc_stream_t stream);
int sc_rasterize_fwd_ed(const float* means2d, const float* conics, const float* colors,
                        const float* opacities, const float* backgrounds, const uint8_t* tile_masks,
                        int C, int N, int D, int width, int height, int tile_size, int tile_width,
                        int tile_height, const int32_t* isect_offsets, const int32_t* flatten_ids,
                        int64_t n_isects, float* render_colors, float* render_alphas,
                        const int32_t* tile_order, int32_t* tile_work, sc_stream_t stream);

/* ---- trajectory mode: StreetGaussianRenderer.render_all in one rasterizer pass
 *      (street_gaussian/models/street_gaussian_renderer.py:17-45: three whole operator sequences per frame, over all
 *      non-sky models, over ['background'] and over pc.obj_list, of which rgb, rgb_background / acc_background and
 *      rgb_object / acc_object are kept).  The background and the object Gaussians partition the full set, and a tile's
 *      depth-sorted list of a subset is the subsequence of the full tile list, so one walk of the full list with one
 *      accumulator set for the composite and one per group gives all three images, each bit-identical to its own
 *      render ("render_all in one pass").  Forward only.
 * group_ids: uint8 [N], one group per Gaussian, shared by all C cameras; an id >= n_groups (and a dead list entry)
 *   belongs to no group and is blended into the composite only.  n_groups is 1 or 2.
 * sc_group_extents: group_end int32 [C*tile_width*tile_height, n_groups] = one past the position in flatten_ids of the
 *   last record of group k inside the tile's range (read from isect_offsets as the rasterizer reads it: clamped into
 *   [0, n_isects]), the range's start when the tile holds no record of group k.
 * sc_rasterize_fwd_groups: render_colors [C,H,W,D], render_alphas [C,H,W,1], group_colors [n_groups,C,H,W,D],
 *   group_alphas [n_groups,C,H,W,1]; fp32, interleaved, every pixel written.  No backgrounds, tile masks, last_ids or
 *   dispatch list.  group_end comes from sc_group_extents on the same lists: group k's images are finished in a tile
 *   once the walk has reached group_end[tile][k] (values are clamped into the tile's range).
 * Both: n_isects == 0 is valid (outputs zero, extents = range starts); C == 0 returns 0.  SC_EINVAL (nothing launched):
 *   n_groups outside 1..2, a non-positive size, n_isects outside [0, 2^31), a tile grid that does not cover the image,
 *   C*N >= 2^31, a null required pointer.  SC_EUNSUPPORTED (nothing launched): tile_size != 16, D other than 3 or 4. */
int sc_group_extents(const int32_t* isect_offsets, const int32_t* flatten_ids, int64_t n_isects,
                     const uint8_t* group_ids /* [N] */, int C, int N, int n_groups,
                     int tile_width, int tile_height, int32_t* group_end, sc_stream_t stream);
int sc_rasterize_fwd_groups(const float* means2d, const float* conics, const float* colors,
                            const float* opacities, const uint8_t* group_ids, const int32_t* group_end,
                            int C, int N, int D, int n_groups, int width, int height, int tile_size,
                            int tile_width, int tile_height,
                            const int32_t* isect_offsets, const int32_t* flatten_ids, int64_t n_isects,
                            float* render_colors, float* render_alphas,
                            float* group_colors, float* group_alphas, sc_stream_t stream);

/* ---- training on the composite and the group images from one pass
 *      (train.py:202-208: the object accumulation loss renders pc.obj_list a second time under grad -- projection,
 *      intersection, SH, rasterizer forward and backward -- on four of every five iterations after densification, only to
 *      get acc_obj.  With the objects as a group of the composite's own walk, that second sequence is one more accumulator
 *      set in the forward and in the backward.)
 * sc_rasterize_fwd_groups_ids: sc_rasterize_fwd_groups (same arguments, same checks, bit-identical images) that also
 *   writes last_pos int32 [n_groups + 1, C, H, W]: per pixel and accumulator set (0 = composite, 1 + k = group k) the
 *   position in flatten_ids of the last record that set blended into the pixel; range_start - 1 of the pixel's tile (its
 *   clamped isect_offsets entry minus one, -1 for the first tile) where the set blended nothing.  A null last_pos with
 *   C > 0 is SC_EINVAL.
 * sc_rasterize_bwd_groups: replays every tile list back to front, once, for all sets.  render_alphas, group_alphas and
 *   last_pos are the forward's outputs.  Upstream gradients v_render_colors [C,H,W,D], v_render_alphas [C,H,W,1],
 *   v_group_colors [n_groups,C,H,W,D], v_group_alphas [n_groups,C,H,W,1]: each nullable; null means zero, and a set both
 *   of whose pointers are null is off (all four null: returns 0, nothing launched).  Outputs v_means2d [C,N,2], v_conics
 *   [C,N,3], v_colors [C,N,D], v_opacities [C,N]: accumulated with float atomics, must arrive zero-filled; the gradient
 *   of a Gaussian is the sum over the sets it is in (the composite, and its own group when group_ids[n] < n_groups).
 *   v_means2d_abs [C,N,2] (nullable, zero-filled): sum over pixels of |d L / d mean| of the COMPOSITE set's terms only --
 *   exactly what sc_rasterize_bwd on the full set writes; the group images add nothing to it (the reference's object
 *   render has its own means2d and never reaches viewspace_points.absgrad).
 *   Values read from last_pos are clamped into the tile's [range_start - 1, range_end); ids and ranges as in the forward.
 *   n_isects == 0 and C == 0 return 0 and launch nothing.  Errors as sc_rasterize_fwd_groups (nothing launched); the
 *   four gradient outputs are required whenever C > 0. */
int sc_rasterize_fwd_groups_ids(const float* means2d, const float* conics, const float* colors,
                                const float* opacities, const uint8_t* group_ids, const int32_t* group_end,
                                int C, int N, int D, int n_groups, int width, int height, int tile_size,
                                int tile_width, int tile_height,
                                const int32_t* isect_offsets, const int32_t* flatten_ids, int64_t n_isects,
                                float* render_colors, float* render_alphas,
                                float* group_colors, float* group_alphas, int32_t* last_pos, sc_stream_t stream);
int sc_rasterize_bwd_groups(const float* means2d, const float* conics, const float* colors,
                            const float* opacities, const uint8_t* group_ids, int C, int N, int D, int n_groups,
                            int width, int height, int tile_size, int tile_width, int tile_height,
                            const int32_t* isect_offsets, const int32_t* flatten_ids, int64_t n_isects,
                            const float* render_alphas, const float* group_alphas, const int32_t* last_pos,
                            const float* v_render_colors, const float* v_render_alphas,
                            const float* v_group_colors, const float* v_group_alphas,
                            float* v_means2d_abs, float* v_means2d, float* v_conics, float* v_colors,
                            float* v_opacities, sc_stream_t stream);

/* ---- novel-view mode: the foreground and the sky of StreetGaussianRenderer.render_novel_view in one rasterizer pass
 *      (street_gaussian/models/street_gaussian_renderer.py:136-163: the whole operator sequence over every sub-model but
 *      the sky, the whole sequence again over the sky Gaussians alone, then rgb + rgb_sky * (1 - acc) and a clamp).
 *      Two INDEPENDENT layers: rows [0, n_front) of every camera are the front layer, rows [n_front, N) the back layer.
 *      The lists must come from the intersection stage run on LAYERED depth keys (street_crafter_amd/layers.py: back rows'
 *      depths times a power of two larger than far / near), so that every tile's list is [front records by depth][back records by depth]; each layer's
 *      images are then bit-identical to sc_rasterize_fwd on that layer's own rows and lists.  Per
 *      tile the kernel finds where the back part begins (a search: a dead entry, id outside [0, C*N), counts as front),
 *      blends the front part until it terminates or reaches that position, jumps there and blends the back part.  On lists
 *      that are not layered the images are unspecified; every access stays in bounds.  Forward only; no backgrounds, tile
 *      masks or dispatch list.
 * epilogue 0 (layers): out0 front_colors [C,H,W,D], out1 front_alphas [C,H,W,1], out2 back_colors [C,H,W,3] (the first
 *   three colour channels), out3 back_alphas [C,H,W,1]; raw, as sc_rasterize_fwd writes them.
 * epilogue 1 (frame, float): out0 rgb [C,H,W,3] = clamp(clamp(front,0,1) + clamp(back,0,1) * (1 - acc), 0, 1), every
 *   product and sum rounded separately (= sc_frame_composite_u8 before quantisation); out1 acc [C,H,W,1] = the front
 *   alpha; out2 depth [C,H,W,1] = front[...,3] / max(acc, 1e-10) (D == 4 only; nullable, ignored for D == 3); out3 unused.
 * epilogue 2 (frame, uint8): out_u8 [C,H,W,3], the same composite quantised with `rounding` 0 = (uint8)(x * 255),
 *   1 = (uint8)(x * 255 + 0.5), as sc_frame_composite_u8; out0..out3 unused.
 * layer_begin (nullable): int32 [C*tile_width*tile_height], the list position the kernel took as the back part's start.
 * n_front == 0 and n_front == N are valid (an absent layer's images are zero); n_isects == 0 is valid; C == 0 returns 0.
 * SC_EINVAL (nothing launched, no GPU needed): D other than 3 or 4, tile_size other than 16, n_front outside [0, N],
 *   epilogue outside 0..2, rounding outside 0..1, a non-positive size, n_isects outside [0, 2^31 - 256), C*N >= 2^31, a
 *   tile grid that does not cover the image, a null required pointer. */
int sc_rasterize_fwd_layers(const float* means2d, const float* conics, const float* colors,
                            const float* opacities, int C, int N, int D, int n_front, int width, int height,
                            int tile_size, int tile_width, int tile_height,
                            const int32_t* isect_offsets, const int32_t* flatten_ids, int64_t n_isects,
                            int epilogue, int rounding, float* out0, float* out1, float* out2, float* out3,
                            uint8_t* out_u8, int32_t* layer_begin, sc_stream_t stream);

/* ---- frame export for the multi-GPU gather: the tail of render_novel_view
 *      (street_gaussian/models/street_gaussian_renderer.py:151-163: fg + sky * (1 - acc), clamp) and the
 *      visualizer's uint8 conversion (street_gaussian/visualizers/street_gaussian_visualizer.py:88-101),
 *      which the reference does with torch elementwise ops + .cpu().numpy() per frame.
 * fg / sky: the rasterizer's raw f32 images with `*_stride` floats per pixel (>= 3; 4 for RGB+depth);
 * acc: the foreground pass's alpha [n_pixels]; sky and acc are both given or both NULL (single pass).
 * out u8[n_pixels,3] = q(clamp(clamp(fg,0,1) + clamp(sky,0,1) * (1 - acc), 0, 1)), with
 * rounding 0: q(x) = (uint8)(x * 255)        -- the novel-view video frames, `(rgb * 255).astype(np.uint8)`
 * rounding 1: q(x) = (uint8)(x * 255 + 0.5)  -- torchvision.utils.save_image PNGs.
 * Each product / sum is rounded separately: bit-identical to the reference's torch composition. */
int sc_frame_composite_u8(const float* fg, int fg_stride, const float* acc, const float* sky, int sky_stride,
                          int64_t n_pixels, int rounding, uint8_t* out, sc_stream_t stream);
/* The same for images with a channel stride: channel c of pixel i at fg[i * fg_pix_stride + c * fg_ch_stride] -- the
 * planes sc_rasterize_fwd_planar writes have pixel stride 1 and channel stride H * W. */
int sc_frame_composite_u8_strided(const float* fg, int64_t fg_pix_stride, int64_t fg_ch_stride, const float* acc,
                                  const float* sky, int64_t sky_pix_stride, int64_t sky_ch_stride, int64_t n_pixels,
                                  int rounding, uint8_t* out, sc_stream_t stream);

/* ---- visualizer frames: the depth / squared-error colour maps and the `* 255` casts of the reference's visualizer
 *      (street_gaussian/visualizers/street_gaussian_visualizer.py:49-132 and summarize(); visualize_depth_numpy,
 *      street_gaussian/utils/img_utils.py:239-252), so that every video frame leaves the GPU as uint8.
 * Maps, one value v per pixel i of n_pixels:
 *   depth kind: v = depth[i * depth_stride]  (a dense [1,H,W] image: stride 1; the [..., 3] view of an [H,W,4] render: 4);
 *   diff kind:  d_c = (m ? rgb_c : 0) - (m ? gt_c : 0), v = (d_0 d_0 + d_1 d_1) + d_2 d_2, channel c of pixel i at
 *     rgb[i * rgb_pix_stride + c * rgb_ch_stride] (gt alike); m = mask[i] != 0 (uint8 / bool [n_pixels]; NULL: all
 *     true): visualize_diff's numpy expression.  The map is recomputed where needed, never stored.
 * Range of a map: x = nan_to_num(v) (NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX); mi = the smallest x > 0 (denormals
 *   are positive), ma = the largest x.  A map without a positive value has mi = 0 (np.min raises there).  Exact in any
 *   order: deterministic, no atomics, no memset.
 * q(t) = the low 8 bits of trunc(t) as a two's-complement integer, 0 for NaN / inf: what `.astype(np.uint8)` gives on
 *   the x86 hosts the reference runs on (-30.7 -> 226, 256.5 -> 0, 1e10 -> 0).
 * colour map: out[i] = lut[q(255 * ((x - mi) / ((ma - mi) + 1e-8f)))], lut uint8 [256,3] in device memory, the caller's
 *   (cv2.applyColorMap of 0..255, channels reversed); grey map: out[i] = q(255 * a[i]).  All float32, every operation
 *   rounded separately, true division: what NumPy >= 2 computes (NumPy 1.x forms the denominator in float64: not matched).
 * sc_frame_viz_range: ONE launch, at most 1024 blocks; block b leaves {min positive or +inf, max} of its pixels of the
 *   depth map and / or the diff map (each absent with a NULL source) in `workspace`.
 * sc_frame_viz_range_finish: a one-block launch; range4 = {mi_depth, ma_depth, mi_diff, ma_diff} (device) from the
 *   partials sc_frame_viz_range left for the SAME n_pixels; maps: bit 0 depth, bit 1 diff; an unselected map's pair is
 *   written as 0, 0.  Only for a caller who wants the numbers.
 * sc_frame_viz_u8: ONE launch that writes every output given (each nullable, at least one): depth_u8 [n_pixels,3] (needs
 *   depth and depth_lut), diff_u8 [n_pixels,3] (needs rgb, gt and diff_lut), acc_u8 [n_pixels] = q(255 * acc),
 *   acc_object_u8 [n_pixels] = q(255 * acc_object); acc / acc_object dense.  The colour maps' ranges are range4 (device
 *   float[4] as above; both maps') when given, else the partials in `workspace` left by sc_frame_viz_range for the same
 *   n_pixels and sources, which every block reduces itself.
 * Four pixels per lane; 16-byte loads where a source has pixel stride 1 and a 16-byte aligned address (planes: a channel
 *   stride that is a multiple of 4 as well), 32-bit stores into 4-byte aligned outputs, scalar accesses with the same
 *   results otherwise and for the last n_pixels mod 4 pixels.
 * SC_EINVAL (nothing launched, no GPU needed): n_pixels < 0 or >= 2^31, a negative stride, rgb without gt or the
 *   reverse, a mask without rgb / gt, no map (range) or no output (u8), maps outside 1..3, an output without its source or
 *   its lut, a colour output with neither range4 nor workspace, a null required pointer.  SC_EWORKSPACE: a workspace of
 *   fewer than sc_frame_viz_workspace_bytes() bytes where one is read or written.  n_pixels == 0: SC_OK. */
size_t sc_frame_viz_workspace_bytes(void);
int sc_frame_viz_range(const float* depth /* nullable */, int64_t depth_stride, const float* rgb /* nullable */,
                       int64_t rgb_pix_stride, int64_t rgb_ch_stride, const float* gt, int64_t gt_pix_stride,
                       int64_t gt_ch_stride, const uint8_t* mask /* nullable */, int64_t n_pixels, void* workspace,
                       size_t workspace_bytes, sc_stream_t stream);
int sc_frame_viz_range_finish(const void* workspace, size_t workspace_bytes, int64_t n_pixels, int maps, float* range4,
                              sc_stream_t stream);
int sc_frame_viz_u8(const float* depth, int64_t depth_stride, const float* rgb, int64_t rgb_pix_stride,
                    int64_t rgb_ch_stride, const float* gt, int64_t gt_pix_stride, int64_t gt_ch_stride,
                    const uint8_t* mask, const float* acc, const float* acc_object, int64_t n_pixels,
                    const uint8_t* depth_lut, const uint8_t* diff_lut, const float* range4 /* nullable */,
                    const void* workspace, size_t workspace_bytes, uint8_t* depth_u8, uint8_t* diff_u8, uint8_t* acc_u8,
                    uint8_t* acc_object_u8, sc_stream_t stream);

/* unit-test hook for the backward kernel's transposing reduction (v_permlane32/16_swap + DPP):
 * in [n_waves][16][64] per-lane partial sums, out [n_waves][64]: lane l = 64-lane total of value l >> 2 */
int sc_test_wave_transpose_sum16(const float* in, int n_waves, float* out, sc_stream_t stream);

/* unit-test hook for the rasterizers' exact tile cull and lane-to-pixel map (csrc/raster_common.h, csrc/raster_walk.h):
 * one wave per record, through the helpers the tile walk itself calls.
 * records f32[n,6] = (conic a, b, c, opacity, centre x, y); geometry i32[n,6] = (txi, tyi, sub, NSUB, width, height):
 * tile (txi, tyi) of a width x height image, walked whole (NSUB 1, sub 0) or as its upper / lower half (NSUB 2, sub 0 / 1).
 * verdict i32[n]: 1 = the cull drops the record for this rectangle, 0 = it keeps it, -1 = the geometry is not a rectangle
 * of the image.  valid u32[n,8]: bit 16 * row + column (row, column counted from the rectangle's first pixel; 256 bits
 * for a whole tile, 128 for a half) is set when the walk's pair evaluation reports "this record blends" for that pixel;
 * pixels outside the image are evaluated the way the walk evaluates them (x centre +inf) and must come out 0. */
int sc_test_tile_cull(const float* records, const int32_t* geometry, int n, int32_t* verdict, uint32_t* valid,
                      sc_stream_t stream);

/* ---- HIP streams with a CU mask or a priority (frame loop: street_crafter_amd/dist.py, bench.py) ----------------
 * Frames are independent (render.py:64-70) and several are kept in flight on different streams; the VALU-bound
 * rasterizer (10.7 k one-wave workgroups) otherwise starves the 8..16-wave workgroups of the NEXT frame's latency-bound
 * intersection kernels of CU slots.  sc_stream_create makes a non-blocking stream that is either confined to a set of
 * CUs (n_mask_words > 0: hipExtStreamCreateWithCUMask; bit i of the mask = CU i, the driver deals the bits round-robin
 * over the 8 XCDs, so "the first K bits" is K / 8 CUs of every XCD) or has a priority (n_mask_words == 0:
 * hipStreamCreateWithPriority; the range is returned by sc_stream_priority_range, lower number = higher priority).
 * The handle is a hipStream_t; the caller destroys it with sc_stream_destroy after synchronising it. */
int sc_stream_create(int priority, const uint32_t* cu_mask, int n_mask_words, sc_stream_t* out);
int sc_stream_destroy(sc_stream_t stream);
int sc_stream_priority_range(int* least, int* greatest);

/* ---- tuning / introspection ------------------------------------------------------------ */
/* Select a kernel variant at run time (for A/B measurements in one process).
 *   key "proj_clamp": the clamp of x/z, y/z in fully_fused_projection's EWA Jacobian (forward, fused forward and backward):
 *                     0 = +-1.3 tan(fov/2) (upstream gsplat v1.0-1.3; default), 1 = [-(cx/fx + 0.3 tan), (W - cx)/fx +
 *                     0.3 tan] (v1.4+).  The two agree for a centred principal point.
 *   key "radius_floor": the floor under the discriminant of the 3-sigma radius, sqrt(max(floor, b^2 - det)):
 *                     0 = 0.01 (gsplat v1.x; default), 1 = 0.1 (the original Inria rasterizer and early forks).
 *                     The reference installs an UNPINNED gsplat fork (README.md:35): INTEGRATION.md says how to tell which
 *                     pair a checkout has.  Environment: SC_PROJ_CLAMP=asymmetric / SC_RADIUS_FLOOR=0.1 set them at load.
 *   key "raster_fwd": 0 = reference-shaped (all pixels x all splats; generic fallback / cross-check),
 *                     3 = one wave per tile, 4 pixels per lane, exact tile-level cull (default)
 *   key "raster_map": block -> tile map of the wave rasterizer: 1 = neighbouring tiles round-robin over the
 *                     8 XCDs (default), 0 = one band of tile rows per XCD
 *   key "raster_split": 0..100: the dispatch list sc_isect_bin_count builds lists a tile as two 16 x 8 halves when
 *                     its work hint is at least this percentage of the heaviest tile's (default 50; 0 = never)
 *   key "raster_hint_blend": 0..4: a tile's work hint = max(its own, this many quarters of the largest hint within
 *                     2 tiles of it) (default 3; 0 = own value only: exact for a camera that stands still)
 *   key "point_raster_waves": waves per 16 x 16 tile of sc_point_rasterize_fwd: 4 = four 16 x 4 strips, one pixel
 *                     per lane (default), 1 = the whole tile, 4 pixels per lane.  Same results bit for bit.
 *   key "raster_bwd": 0 = reference-shaped (one lane per pixel), 1 = one wave per tile (default)
 *   key "raster_bwd_split": 1 = the backward follows the forward's dispatch list including its half tiles (default),
 *                     0 = the whole-tile list behind it
 * Returns the previous value, or SC_EINVAL for an unknown key.
 * (The diagnostic skips "debug0".."debug3" of rounds 1-2 are NOT part of this library any more: they exist only in
 *  the separate diagnostic build, lib/libstreet_crafter_hip_diag.so (-DSC_DIAG), which tools/exp_*.py load
 *  explicitly; here they are unknown keys.) */
int sc_set_option(const char* key, int value);

#ifdef __cplusplus
}
#endif
#endif /* STREET_CRAFTER_AMD_H */
