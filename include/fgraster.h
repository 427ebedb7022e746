/*
 * fgraster.h -- C ABI of libfgraster.so, the MI355X (gfx950) Gaussian-raster hot path.
 *
 * This is the drop-in boundary for the ONE call the reference makes into native code:
 *     gsplat.rendering.rasterization(...)
 *         freegaussian/freegaussian_model.py:847-868          (stage 1 training / eval)
 *         freegaussian/freegaussian_control_model.py:158-179  (stage 2)
 *         preprocess/knn_gaussian.py:93-113, preprocess/render_depth.py:99,157,
 *         preprocess/render_color.py:93, preprocess/o3d_color_splat.py:188   (packed / "ED")
 * and for the flow-derivative math of preprocess/epipolar_flow.py:274-309 and
 * docs/index.html:256-300.  The Python binding that calls these symbols is
 * freegaussian_amd/_lib.py (ctypes); INTEGRATION.md shows the stub a maintainer adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the comment says "host";
 *   - the library allocates nothing, keeps no global state, reads no environment variable and never
 *     synchronises (launch policy comes in through fg_raster_config): the
 *     caller owns every buffer (scratch sizes from the *_workspace_bytes queries) and every
 *     call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - re-entrant across streams; return 0 on success, a negative FG_ERR_* code otherwise;
 *     nothing is thrown across the ABI;
 *   - all floating data is fp32, row-major, contiguous; "radii" is int32 with >0 <=> visible;
 *   - one camera per call (the reference asserts camera.shape[0]==1,
 *     freegaussian_model.py:773); views are sharded over processes, not batched.
 */
#ifndef FGRASTER_H
#define FGRASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fg_stream_t;

#define FG_OK 0
#define FG_ERR_INVALID_ARG (-1)
#define FG_ERR_LAUNCH (-2)
#define FG_ERR_WORKSPACE (-3)
#define FG_ERR_UNSUPPORTED (-4)

#define FG_MAX_CHANNELS 8    /* composited feature channels per splat (RGB, depth, flow, ...) */
#define FG_SPLAT_FLOATS 16   /* one 64-byte record per Gaussian, see fg_pack_splats */
#define FG_SH_JAC_FLOATS 10  /* per-Gaussian note of the SH colour for the backward, see fg_preprocess_fwd */
#define FG_ABI_VERSION 14
#define FG_ABI_MINOR 1 /* symbols added since FG_ABI_VERSION was last raised: 1 = fg_abi_minor, fg_mlp_train_bwd* */
/* (fg_mlp_precision_supported, added later still, is discovered BY NAME -- dlsym, or ctypes' hasattr -- not by the minor
 * number, which stays 1: a library without the symbol takes fg_mlp_desc::precision as the reserved word it was and
 * computes in fp32.  Likewise BY NAME: fg_mlp_wgrad_precision_supported, fg_mlp_param_grads_p and fg_mlp_train_bwd_p -- a
 * library without them forms the weight gradients in exact fp32 through fg_mlp_param_grads / fg_mlp_train_bwd.  Likewise BY
 * NAME: fg_bilagrid_supported, fg_bilagrid_bwd_workspace_bytes, fg_bilagrid_slice_fwd and fg_bilagrid_slice_bwd -- a library
 * without them has no fused bilateral-grid slice, and the host keeps its torch statement of it.  Likewise BY NAME:
 * fg_color_correct_workspace_bytes and fg_color_correct -- a library without them has no fused colour correction of the
 * metrics, and the host keeps its torch statement of it.  Likewise BY NAME: fg_se3_apply_fwd and fg_se3_apply_bwd -- a library
 * without them has no fused SE(3) transform of the means, and the host keeps its torch statement of it.  Likewise BY NAME:
 * fg_control_supported, fg_control_workspace_bytes, fg_control_attr_mean, fg_control_value_rows, fg_control_scatter_fwd and
 * fg_control_scatter_bwd -- a library without them has no fused stage-2 control stage, and the host keeps its torch statement
 * of it.  Likewise BY NAME: fg_target_loss_supported, fg_target_loss_workspace_floats, fg_target_loss_fwd and
 * fg_target_loss_bwd -- a library without them has no fused training target, and the host keeps its torch statement of it.
 * Likewise BY NAME: fg_flow_disp_fwd, fg_flow_disp_bwd, fg_flow_l1_workspace_bytes, fg_flow_l1_fwd and fg_flow_l1_bwd -- a
 * library without them has no flow-supervised training: the model's flow term is an error there, not a torch fall-back.
 * Likewise BY NAME: fg_dbscan_workspace_bytes and fg_dbscan -- a library without them cannot cluster the dynamic Gaussians:
 * a stage-2 mask then has to come from annotated label maps.  Likewise BY NAME: fg_optflow_supported,
 * fg_optflow_workspace_bytes, fg_optflow_pyramid and fg_optflow -- a library without them estimates no optical flow: the
 * flow maps then have to come from elsewhere.) */
#define FG_COUNT_OUT_WORDS 16 /* int64 words of a count_out block (fg_stbin_count, fg_step_io): ABI 9 */

int fg_abi_version(void);
const char* fg_error_string(int code);

/* ---- K1: projection (replaces the fully-fused projection stage implied by the kwargs
 * viewmats/Ks/near_plane/far_plane/rasterize_mode at freegaussian_model.py:847-865) --------
 * means[N,3] quats[N,4](wxyz, any norm) scales[N,3]; viewmat[16] world->camera (OpenCV axes,
 * as built by freegaussian/utils.py:162-179); K[9].  Outputs (culled Gaussians: 0):
 * radii[N] means2d[N,2] depths[N] conics[N,3] compensations[N](nullable) and
 * tiles_touched[N] = number of tile_size x tile_size tiles in the splat's bounding rectangle. */
int fg_project_fwd(int N, const float* means, const float* quats, const float* scales,
                   const float* viewmat, const float* K, int width, int height, float eps2d,
                   float near_plane, float far_plane, float radius_clip, int tile_size,
                   int32_t* radii, float* means2d, float* depths, float* conics,
                   float* compensations, int32_t* tiles_touched, fg_stream_t stream);

/* Backward of K1 (autograd of the call at freegaussian_model.py:847; viewmat gradients are
 * not produced: camera_optimizer mode is "off", freegaussian_model.py:120).
 * v_compensations / compensations nullable together.  Writes v_means[N,3] v_quats[N,4]
 * v_scales[N,3] (zeros where radii==0). */
int fg_project_bwd(int N, const float* means, const float* quats, const float* scales,
                   const float* viewmat, const float* K, int width, int height, float eps2d,
                   const int32_t* radii, const float* conics, const float* compensations,
                   const float* v_means2d, const float* v_depths, const float* v_conics,
                   const float* v_compensations, float* v_means, float* v_quats,
                   float* v_scales, fg_stream_t stream);

/* ---- K2: spherical harmonics (sh_degree / colors[N,K,3] kwargs, freegaussian_model.py:801,
 * :826-830).  colour = max(SH(dir) + 0.5, 0), dir = mean - camera position (derived from
 * viewmat).  coeffs[N,k_stored,3]; degree 0..3; only radii>0 rows are shaded (others 0). */
int fg_sh_fwd(int N, int degree, int k_stored, const float* means, const float* viewmat,
              const float* coeffs, const int32_t* radii, float* colors, fg_stream_t stream);
/* v_coeffs[N,k_stored,3] is written densely (sparse_grad=False, freegaussian_model.py:863);
 * v_means[N,3] (nullable) receives the view-direction gradient. */
int fg_sh_bwd(int N, int degree, int k_stored, const float* means, const float* viewmat,
              const float* coeffs, const int32_t* radii, const float* colors,
              const float* v_colors, float* v_coeffs, float* v_means, fg_stream_t stream);

/* ---- K3: tile binning (tile_size=16, freegaussian_model.py:806) --------------------------
 * fg_scan_tiles: inclusive prefix sum, cum_tiles[N] int64; cum_tiles[N-1] = I, the number of
 * (Gaussian, tile) intersections, which the host reads to size the lists. */
size_t fg_scan_workspace_bytes(int N);
int fg_scan_tiles(int N, const int32_t* tiles_touched, int64_t* cum_tiles, void* workspace,
                  size_t workspace_bytes, fg_stream_t stream);
/* isect_ids[I]  = (tile_id << 32) | float32 bits of depth;  flatten_ids[I] = Gaussian id.
 * Emission order: Gaussian-major, row-major over the tile rectangle. */
int fg_tile_bin(int N, const float* means2d, const int32_t* radii, const float* depths,
                const int64_t* cum_tiles, int tile_size, int tile_w, int tile_h,
                int64_t* isect_ids, int32_t* flatten_ids, fg_stream_t stream);

/* ---- K4: stable LSD radix sort of (key, value) pairs on key bits [0, end_bit), in place
 * (workspace holds the ping-pong copies and histograms), then per-tile ranges:
 * tile_offsets[n_tiles+1], tile t owns sorted entries [tile_offsets[t], tile_offsets[t+1]). */
size_t fg_sort_workspace_bytes(int64_t n);
int fg_sort_pairs(int64_t n, int64_t* keys, int32_t* vals, int end_bit, void* workspace,
                  size_t workspace_bytes, fg_stream_t stream);
int fg_tile_ranges(int64_t n, const int64_t* sorted_keys, int n_tiles, int32_t* tile_offsets,
                   fg_stream_t stream);

/* 32-bit-key variant of fg_sort_pairs (same kernels, half the key traffic). */
size_t fg_sort32_workspace_bytes(int64_t n);
int fg_sort_pairs32(int64_t n, uint32_t* keys, int32_t* vals, int end_bit, void* workspace,
                    size_t workspace_bytes, fg_stream_t stream);

/* ---- K3+K4, depth-first form (what rasterization() uses; identical final lists) -------------
 * Instead of sorting I 45-bit (tile|depth) keys, sort the N Gaussians by depth once
 * (fg_bin_prepare: order[N] = ids by ascending depth bits, culled last, stable; cum_tiles[k] =
 * inclusive tile count of order[0..k]), emit (tile, id) pairs in that order, and stably sort
 * them on the ceil(log2 T) tile bits only (fg_bin_emit_sort).  A stable sort by tile of a
 * depth-ordered sequence IS the (tile, depth, id) order of the 64-bit-key sort, so
 * flatten_ids / tile_offsets are bit-identical to fg_tile_bin + fg_sort_pairs + fg_tile_ranges,
 * at ~1/7 of the sort traffic.  The host reads cum_tiles[N-1] (= I) between the two calls.
 * fg_isect_keys rebuilds the reference-style 64-bit keys (tile << 32 | depth bits) on demand. */
size_t fg_bin_prepare_workspace_bytes(int N);
int fg_bin_prepare(int N, const float* depths, const int32_t* radii, const int32_t* tiles_touched,
                   int32_t* order, int64_t* cum_tiles, void* workspace, size_t workspace_bytes,
                   fg_stream_t stream);
/* The same, but the tile counts come from the tile rectangles, computed here from means2d / radii
 * with the arithmetic of the projection pass (width x height == tiles_touched), and
 * rects_sorted[N] receives every Gaussian's rectangle (x0 | y0 << 10 | width << 20) IN DEPTH ORDER:
 * handed to fg_bin_emit_sort[_capacity], the emission reads it coalesced instead of gathering
 * radii / means2d by id (35 -> 20 us at 1M Gaussians).  Needs tile_w, tile_h <= 1023. */
int fg_bin_prepare_rects(int N, const float* depths, const int32_t* radii, const float* means2d,
                         int tile_size, int tile_w, int tile_h, int32_t* order, int64_t* cum_tiles,
                         int32_t* rects_sorted, void* workspace, size_t workspace_bytes,
                         fg_stream_t stream);
/* The same from what fg_preprocess_fwd / fg_preprocess_raw_fwd already wrote: depth_keys[N] (sorted
 * IN PLACE here -- a scratch array from the caller's point of view) and tile_rects[N,2] (read
 * only).  No key / rectangle kernel runs and the first radix pass numbers the values itself.  With
 * the preprocess pass's FOOTPRINT rectangles the lists hold only (splat, tile) pairs in which the
 * splat can reach alpha >= 1/255 -- the reference's lists minus dead entries, same order.
 * count_out (nullable): one more copy of the list length cum_tiles[N-1], stored with system scope --
 * pass the device-visible address of pinned host memory and the host has the count after an event
 * wait, with no copy launch in the stream (the reference reads it with a blocking .item()). */
int fg_bin_prepare_keys(int N, uint32_t* depth_keys, const int32_t* tile_rects, int32_t* order,
                        int64_t* cum_tiles, int32_t* rects_sorted, int64_t* count_out, void* workspace,
                        size_t workspace_bytes, fg_stream_t stream);
/* ---- K3+K4, supertile form (what rasterization() runs when the fused preprocess pass supplied keys and
 * rectangles; identical lists) -------------------------------------------------------------------------
 * Count per tile and per supertile (2 x 2 tiles) -> scans -> one 8-byte element (depth bits << 32 | id << 4 |
 * which of the four tiles) scattered per (Gaussian, supertile) pair into the supertile's segment -> every
 * segment sorted ONCE by (depth bits, Gaussian id) in LDS and the four tile lists read off the sorted run:
 * 6 launches instead of the 26 of fg_bin_prepare_keys + fg_bin_emit_sort, 2.5x fewer scattered and sorted
 * elements than (Gaussian, tile) pairs on the 1M / 1080p scene (csrc/stbin.hip).
 * tile_rects / depth_keys: the optional outputs of fg_preprocess_fwd.  fg_stbin_count writes
 * tile_offsets[T + 1] (exact, independent of any capacity) and, if count_out is not NULL, FIVE words of a block of
 * FG_COUNT_OUT_WORDS = SIXTEEN int64 (ABI 9; a block of four before) with system scope (pinned host memory):
 * count_out[0] the list length, count_out[2] the longest tile list (a host turns fg_raster_config::heavy_tiles on
 * from it), count_out[1] the longest supertile segment, count_out[3] the number of segments of more than 3072
 * elements, and count_out[14] the summed AREA of the footprint rectangles in tiles -- what the list length would be without tile_masks: a host keeps the masks for an
 * image size only while list length / area says they drop enough (ops.RasterContext.masks_on: below 0.8).  (Words 4..13
 * and 15 belong to fg_stbin_fill_jobs' ckpt_need_out and fg_raster_jobs_fwd's walk_out when the host hands them the same
 * block, as ops.py does.)
 * (segments beyond 7936 elements are sorted by one workgroup through global memory -- correct, slow -- unless
 * fg_stbin_fill is called with FG_STBIN_LONG_SEGMENTS, see below).  fg_stbin_fill writes flatten_ids[0 .. tile_offsets[T]) and
 * list_offsets[T + 1] = tile_offsets -- or, when the list is longer than `capacity`, no ids at all and
 * list_offsets = 0 (empty lists: consumers enqueued speculatively behind the call walk nothing; the host then
 * repeats the call with exact buffers, the count workspace stays valid).  Consumers of flatten_ids read
 * list_offsets, not tile_offsets.  N < 2^28; fg_stbin_supported = 0 for tile grids wider than ~2700 tiles
 * (callers then take fg_bin_prepare_keys + fg_bin_emit_sort).
 * Replaces the binning + sort implied by tile_size=16 at freegaussian_model.py:806,857. */
int fg_stbin_supported(int N, int tile_w, int tile_h);
size_t fg_stbin_count_workspace_bytes(int N, int tile_w, int tile_h);
/* tile_masks (ABI 8; nullable, the optional output of fg_preprocess_fwd): per Gaussian which blocks of its footprint
 * rectangle the ELLIPSE alpha >= 1/255 reaches -- the rectangle's w x h tiles in at most 8 x 8 blocks of b x b tiles
 * (b = 1 up to 8 x 8 tiles, then the next power of two with ceil(max(w, h) / b) <= 8), bit 8 by + bx.  Counted and
 * scattered are the set blocks' tiles only: a needle lying diagonally across a 12 x 12-tile rectangle enters 20 lists, not
 * 144 (30 % needles of axis ratio 10 in the 1M / 1080p scene: 57 % fewer list entries, profiles/r05_exact_tiles.md); the
 * lists stay an order-preserving subsequence of the reference's and every dropped entry is one no pixel of the tile would
 * have taken.  The SAME array must be given to fg_stbin_count and fg_stbin_fill (the scatter drops exactly the pairs the
 * count did not count).  NULL: whole rectangles, as before ABI 8. */
int fg_stbin_count(int N, const int32_t* tile_rects, const uint64_t* tile_masks, int tile_w, int tile_h,
                   int32_t* tile_offsets, int64_t* count_out, void* workspace, size_t workspace_bytes, fg_stream_t stream);
size_t fg_stbin_fill_workspace_bytes(int64_t capacity);
/* flags (ABI 7): FG_STBIN_LONG_SEGMENTS -- supertile segments beyond the small-segment launch's LDS capacity (3072
 * elements; a dense cluster: thousands to hundreds of thousands of splats over one 32 x 32-pixel supertile) are cut
 * into buckets of ~1536 elements by a multi-workgroup sample sort (splitters from a sorted sample inside the
 * large-segment launch, then a count, a scatter, a bucket-sort and an overflow launch) instead of being sorted one
 * segment per 1024-thread workgroup in LDS (up to 7936 elements) or by ONE workgroup through global memory (beyond).
 * Same lists bit for bit either way; a host sets the flag for shapes whose earlier calls reported a segment beyond
 * 7936 elements (count_out[1]) or more than a handful beyond 3072 (count_out[3]) -- ops.bin_tiles does -- on scenes
 * without such segments the flag only costs three empty launches (ABI 9: count + scatter of the long elements in one pass
 * into per-bucket slabs of the workspace; four launches before). */
#define FG_STBIN_LONG_SEGMENTS 1
#define FG_STEP_NO_FOOTPRINT_MASKS 2 /* (fg_step_desc::flags only) */
/* (ABI 9, with FG_STBIN_LONG_SEGMENTS; a TEST hook: a bucket of the sample sort counts as having outgrown its slab from 1600
 * elements instead of 3072 -- it is gathered again from its segment and sorted by a larger LDS sort -- and, in even
 * supertiles, a segment with a bucket beyond 1728 elements instead of 7936 goes through global memory whole, so that both
 * paths behind an outgrown slab run in tests on segments of any size; same lists.  Without the hook they are rare only on
 * segments of up to ~147 000 elements -- 96 buckets, 32 samples each: a 1e-6 event per bucket --; the sample has 3072
 * elements at most, so longer segments have fewer samples per bucket, down to ~3 at the 1008-bucket cap (1 548 288
 * elements), where outgrown slabs are common and from ~2.5M elements a segment sorted whole is the normal route) */
#define FG_STBIN_TEST_SMALL_SLABS 4
int fg_stbin_fill(int N, const uint32_t* depth_keys, const int32_t* tile_rects, const uint64_t* tile_masks, int tile_w,
                  int tile_h, int64_t capacity, const int32_t* tile_offsets, const void* count_workspace,
                  int32_t* flatten_ids, int32_t* list_offsets, void* workspace, size_t workspace_bytes,
                  int flags, fg_stream_t stream);
/* (fg_stbin_fill_jobs, with the job lists further down: this call and fg_raster_build_jobs in the same launches) */

/* tile_keys may be NULL in both emit entry points when the caller does not need the keys (up to
 * 65536 tiles): they are then kept as 16-bit values inside the workspace -- 34 instead of 48 bytes
 * of traffic per intersection over emission + the two sort passes. */
size_t fg_bin_emit_workspace_bytes(int64_t n_isects);
/* rects_sorted: from fg_bin_prepare_rects, or NULL (rectangles are then recomputed from means2d /
 * radii, which may be NULL otherwise). */
int fg_bin_emit_sort(int N, int64_t n_isects, const float* means2d, const int32_t* radii,
                     const int32_t* order, const int64_t* cum_tiles, const int32_t* rects_sorted,
                     int tile_size, int tile_w, int tile_h, uint32_t* tile_keys, int32_t* flatten_ids,
                     int32_t* tile_offsets, void* workspace, size_t workspace_bytes, fg_stream_t stream);
/* fg_bin_emit_sort without the host round trip for the count: the buffers hold `capacity`
 * entries (tile_keys[capacity], flatten_ids[capacity], workspace for `capacity`), the number of
 * intersections is read ON THE DEVICE from cum_tiles[N-1].  When that count exceeds the capacity
 * the lists are truncated and invalid: the caller compares its own (asynchronous) readback of
 * cum_tiles[N-1] with the capacity and repeats the call with exact buffers in that case. */
int fg_bin_emit_sort_capacity(int N, int64_t capacity, const float* means2d, const int32_t* radii,
                              const int32_t* order, const int64_t* cum_tiles,
                              const int32_t* rects_sorted, int tile_size, int tile_w, int tile_h,
                              uint32_t* tile_keys, int32_t* flatten_ids, int32_t* tile_offsets,
                              void* workspace, size_t workspace_bytes, fg_stream_t stream);
int fg_isect_keys(int64_t n_isects, const uint32_t* tile_keys, const int32_t* flatten_ids,
                  const float* depths, int64_t* isect_ids, fg_stream_t stream);

/* ---- K5/K6: front-to-back alpha compositing over 16x16 tiles -----------------------------
 * fg_pack_splats builds one 64-byte record per Gaussian:
 *   [x, y, opacity, conic_a, conic_b, conic_c, f0..f(C-1), 0...]      C <= FG_MAX_CHANNELS
 * features[N,C] are the composited channels (RGB | RGB+depth | depth | +flow ...). */
int fg_pack_splats(int N, int channels, const float* means2d, const float* conics,
                   const float* opacities, const float* features, float* splats,
                   fg_stream_t stream);
/* LAUNCH POLICY of the raster kernels (ABI version 3: rounds 1-2 read FG_RASTER_* environment variables
 * inside the library).  Every raster entry point takes a `const fg_raster_config*`; NULL = the defaults
 * measured on MI355X (csrc/raster.hip), and so is every field left at its fg_raster_config_init value.
 * Results do not depend on the policy (same images; gradients up to float summation order) -- it decides
 * how the work is cut into jobs.  The SAME config must go to all calls of one image (job-list words, build,
 * forward, checkpoint size, backward).  The Python host fills it from the FG_RASTER_* variables it reads
 * (freegaussian_amd/ops.py::LaunchPolicy); a non-Python host fills the struct directly. */
typedef struct fg_raster_config {
  int32_t size;            /* sizeof(fg_raster_config) of the caller's build (set by fg_raster_config_init) */
  int32_t ppt_fwd;         /* pixels per lane of the forward: 0 = by tile count; 1 | 2 | 4 = forced (classic launch) */
  int32_t ppt_bwd;         /* the same for the backward */
  int32_t tile_order;      /* classic launches, workgroup -> tile map: -1 = default (2: XCD row bands walked
                              column-major); 0 rows, 1 bands, 2 cols, 3 split, 4 / 5 rectangles */
  int32_t bands_nx;        /* mixed launches: XCD shares as nx x (8 / nx) rectangles; 0 / 1 = row bands (default) */
  int32_t tail4_fwd;       /* forward: the last tail4 tiles of every XCD's sequence as four single-strip jobs ... */
  int32_t tail2_fwd;       /* ... the tail2 tiles before them as two two-strip jobs; -1 = defaults; 0,0 = classic launch */
  int32_t tail4_bwd;
  int32_t tail2_bwd;
  int32_t split4_fwd;      /* content split: a tile longer than total * split4 / 65536 becomes four jobs ... */
  int32_t split2_fwd;      /* ... longer than total * split2 / 65536 two; -1 = defaults, 0 = off */
  int32_t split4_bwd;
  int32_t split2_bwd;
  int32_t use_liveness;    /* 0: the backward ignores the forward's liveness words (A/B); default 1 */
  int32_t seg_parts;       /* list shares per split tile of the backward (0 / 1 = off); -1 = default (5; 6 below 5000 tiles) */
  int32_t seg_tail;        /* tiles per XCD, at the end of its sequence, whose lists are split (0 = every tile); -1 = default */
  int32_t seg_parts2;      /* graded tail: the last seg_tail2 tiles get seg_parts2 shares; -1 = default (off) */
  int32_t seg_tail2;
  int32_t debug_only_xcd;  /* measurement hooks of the classic launches: only this XCD's workgroups work (-1 = off) */
  int32_t debug_k_mod;     /* ... only every m-th tile of each XCD (0 = off) */
  int32_t balance_bands;   /* job lists (ABI 7): the XCDs' shares of the tile grid are SPANS of the row-major tile sequence
                              with equal numbers of tiles (a span may begin and end inside a row; walked column-major) --
                              or, when the heaviest such share would be more than 15% above the mean, bands of whole tile
                              rows holding equal shares of the tiles' expected cost (list lengths, capped): a cluster of
                              splats under one band no longer sets the launch time; 0 = equal numbers of ROWS always
                              (rounds 1-3: 8 or 9 of a 1080p frame's 68); 2 = equal numbers of tiles always, the costs are
                              not looked at and lists and grids are sized for equal shares (for a host that knows the
                              scene is even: fg_stbin_count's count_out[2] against the mean list; 5-10 us less per step);
                              3 (ABI 8, round 6) = INTERLEAVED: the image's 2 x 2-tile blocks dealt to the XCDs round-robin in
                              raster order -- every XCD a uniform sample of the image, balanced on any content without a
                              cost model (what a host picks for uneven scenes; lists and grids sized as for the cost bands);
                              -1 / 1 = default; p >= 100: the threshold in percent of the mean (100 = always by cost) */
  int32_t heavy_tiles;     /* forward, job lists + list segments (ABI 7): a tile whose list is longer than this many entries
                              is walked serially for its first 2048 entries only; if pixels are still open there, the rest
                              of the list is composited by MANY jobs over shares of it -- every 64-entry batch by itself
                              -- and one combining pass per strip (two more launches) instead of four serial walks; the
                              backward gives such a tile up to 64 shares.  For scenes with unsaturated lists of thousands
                              of entries (a host turns it on when fg_stbin_count's count_out[2] says so); not bit-identical
                              to the serial walk (1e-7 relative).  <= 0 = off (default); values below 2560 mean 2560
                              (heavy_wide, below: the one-launch form that replaced this in round 5, from 256 entries) */
  int32_t seg_slots;       /* list segments, job lists (ABI 7): COMPACT checkpoint slots -- the buffer of
                              fg_raster_seg_ckpt_floats holds this many slots (4352 B each; rounded up to a multiple of 8)
                              instead of one per 64 entries of the list's capacity: only the tiles the backward may cut
                              into shares own slots, ceil(list length / 64) each, granted by the list build per XCD band
                              (an eighth of the slots each) from the end of the band's sequence while they last; a tile
                              without slots runs as one job, without checkpoints -- slower, never wrong.  What the bands
                              would take together is reported by fg_stbin_fill_jobs (ckpt_need_out): size the next call's
                              buffer as 8 x the largest word + a margin.  The SAME value must reach the list build, the size
                              query and both raster calls.  <= 0 = off (default): a slot per 64 entries of every tile */
  int32_t prio_fwd;        /* job lists / mixed launches (ABI 7): issue priority of a job's wavefront by its expected length,
                              lo | hi << 16 in percent of the launch's mean single-strip job (list length x the job kind's
                              cost per entry): above lo the wavefront runs at priority 2, above hi at 3 (s_setprio) -- the
                              launch's longest jobs, which start first and set its end, get through sooner; -1 = default
                              (forward 250 | 350 << 16, backward 120 | 160 << 16), 0 = off */
  int32_t prio_bwd;
  int32_t heavy_wide;      /* forward, heavy tiles (ABI 8): 1 / -1 (default) = the four strip jobs of a heavy tile walk its list's
                              first 512 entries; a strip with pixels still open there continues as ONE job of a 16-wavefront
                              workgroup in a launch behind the main one: the list in rounds of 16 64-entry batches, every
                              wavefront its batch by itself, the batches folded in LDS, a batch in which a pixel may stop
                              walked again from the true state; the job ends with the round in which its last pixel stops.
                              heavy_tiles may then be as low as 768.  0 = round 4's form (2048 entries serially, then local
                              jobs and combine jobs in two launches; heavy_tiles >= 2560) */
  int32_t seg_fine;        /* list segments (ABI 8): the checkpoint grid -- the forward leaves a checkpoint in front of every 64th
                              entry of a tile's list for the list's first seg_fine entries and in front of every 128th behind
                              them (a checkpoint slot each; the backward's shares are cut at those entries): a list of the
                              tail needs the fine grid for its five shares, a list of thousands has segments to spare.
                              -1 = default (640), 0 = every 64th throughout (rounds 2-4; also with heavy_wide = 0); rounded up
                              to a multiple of 64.  The SAME value must reach the list build, the size function and both raster
                              calls. */
} fg_raster_config;
void fg_raster_config_init(fg_raster_config* config);

/* render[H,W,C] alphas[H,W] last_ids[H,W] (index into the sorted list of the last splat that
 * contributed; tile start - 1 if none).  No background: the caller composites it
 * (freegaussian_model.py:875-877). */
int fg_raster_fwd(int channels, int width, int height, int tile_size, const float* splats,
                  const int32_t* tile_offsets, const int32_t* flatten_ids, float* render,
                  float* alphas, int32_t* last_ids, const fg_raster_config* config,
                    fg_stream_t stream);
/* v_alphas may be NULL (no gradient on alpha).
 * v_splats[N,16] must be ZEROED by the caller; per-Gaussian gradients are accumulated as
 *   [v_x, v_y, v_opacity, v_conic_a, v_conic_b, v_conic_c, |v_x|, |v_y|, v_f0..v_f(C-1)]
 * (|v_x|,|v_y| = absgrad, freegaussian_model.py:864 / :377). */
int fg_raster_bwd(int channels, int width, int height, int tile_size, const float* splats,
                  const int32_t* tile_offsets, const int32_t* flatten_ids,
                  const float* alphas, const int32_t* last_ids, const float* v_render,
                  const float* v_alphas, float* v_splats, const fg_raster_config* config,
                    fg_stream_t stream);
/* The same kernels with the model's post-composite O1 folded in (SURVEY.md section 8f row 3;
 * freegaussian_model.py:875-877 `rgb = clamp(render[..., :3] + (1 - alpha) * background, 0, 1)`):
 *   image[c] = render[c] + (1 - alpha) * background[c]   (background[C], nullable = none),
 * the first n_clamp channels clamped to [0,1].  clamp_mask[H,W] (uint8, required when
 * n_clamp > 0) receives per pixel bit c = "channel c was strictly outside [0,1]"; the backward
 * takes it back, zeroes those channels of v_image and folds -sum_c v_image[c]*background[c]
 * into the alpha gradient, so that v_image / v_alphas are the gradients of `rgb` / `alpha`. */
int fg_raster_composite_fwd(int channels, int width, int height, int tile_size, const float* splats,
                            const int32_t* tile_offsets, const int32_t* flatten_ids,
                            const float* background, int n_clamp, float* image, float* alphas,
                            int32_t* last_ids, uint8_t* clamp_mask, const fg_raster_config* config,
                    fg_stream_t stream);
int fg_raster_composite_bwd(int channels, int width, int height, int tile_size, const float* splats,
                            const int32_t* tile_offsets, const int32_t* flatten_ids,
                            const float* background, int n_clamp, const uint8_t* clamp_mask,
                            const float* alphas, const int32_t* last_ids, const float* v_image,
                            const float* v_alphas, float* v_splats, const fg_raster_config* config,
                    fg_stream_t stream);
/* ---- Job lists for the raster launches ---------------------------------------------------------
 * At 200 tiles and more the library runs the raster kernels as one wavefront per JOB: a whole tile
 * (4 pixels per lane), half a tile or a quarter.  Without a list the job sizes depend on the tile's
 * position only (the end of every XCD's tile sequence is split); with a list they also depend on
 * the tile's list length (tiles far longer than the mean are split wherever they are), which is
 * what non-uniform scenes need (scripts/clustered_check.py).  Caller-allocated like everything else:
 *   words = fg_raster_jobs_words(...)   int32 words of ONE list; 0 = the library would not use lists
 *                                        for this size / config (call the plain entry points)
 *   fg_raster_build_jobs(...)            one small launch, after tile_offsets exist; either list nullable
 *   fg_raster_jobs_fwd / _bwd            fg_raster_composite_fwd / _bwd with a list (jobs == NULL:
 *                                        identical to those)
 * LIST SEGMENTS of the backward (3 channels): floats = fg_raster_seg_ckpt_floats(...) (0 = off for
 * this size / config); seg_ckpt[floats], uninitialised, goes to BOTH calls and `image` (the
 * forward's output) to the backward: the forward leaves every pixel's compositing state at every
 * 64th entry of a tile's list (only for the tiles the backward's job list splits: hand both calls the
 * lists of ONE fg_raster_build_jobs call), the last list index each (tile, strip) used and every
 * pixel's exact final transmittance; the backward runs several jobs per tile, each over its share of
 * the list, instead of one serial walk.  Same gradients up to float summation order (a share job
 * reproduces the reference's T_final = 1 - alpha rounding per pixel).  The buffer is opaque.  NULL = off.
 * fg_raster_build_jobs(bwd_list_shares = 1) must then have built the backward's list (its entries
 * are (tile, part, parts) instead of (tile, strip)).
 * LIVENESS (any channel count): live_words[n_isects] uint32, uninitialised, to BOTH calls: the
 * forward notes per (list entry, 4-row strip) whether any pixel took the entry (byte s of word i =
 * strip s of entry i), and the backward evaluates exactly those pairs instead of re-testing every
 * strip of every entry -- same gradients, about a third fewer vector issue cycles.  NULL = off.
 * ZERO FILL IN PASSING: zero_buf[zero_floats] (nullable) is zero-filled by the forward call -- meant
 * for the v_splats array of the coming fg_raster_jobs_bwd, which accumulates with atomics: the forward
 * launch leaves the memory pipe mostly idle, a separate fill costs ~10 us and a launch boundary. */
int64_t fg_raster_jobs_words(int width, int height, int tile_size, const fg_raster_config* config);
int fg_raster_build_jobs(int width, int height, int tile_size, const int32_t* tile_offsets,
                         int32_t* jobs_fwd, int32_t* jobs_bwd, int bwd_list_shares, const fg_raster_config* config,
                    fg_stream_t stream);
/* fg_stbin_fill + fg_raster_build_jobs in the same launches: eight extra workgroups at the end of the
 * scatter launch build the forward's job list from tile_offsets beside the scatter, eight at the head of the
 * small-segment sort launch the backward's -- no launch
 * between the sorted lists and fg_raster_jobs_fwd (10 us of a 0.75 ms step on the 1M / 1080p scene).  width, height,
 * tile_size must give tile_w x tile_h; jobs_fwd / jobs_bwd / bwd_list_shares / config as for fg_raster_build_jobs
 * (both lists NULL: identical to fg_stbin_fill).  The lists depend on tile_offsets only: they stay valid when the
 * call is repeated with a larger capacity.
 * ckpt_need_out (nullable; int64[9], pinned host memory or device memory, written by the launch): with
 * bwd_list_shares and a forward list, word x < 8 = the checkpoint slots the tiles of XCD x's band that the backward may
 * split would take together (whether or not they got them; whatever fg_raster_config::seg_slots is): 8 x the largest
 * word, + a margin, is the seg_slots that leaves no tile without.  Word 8 (whenever the forward list is built): what the
 * cost pass over the XCDs' shares decided -- 1 = bands balanced by cost, 0 = the equal spans stood, -1 = it did not run
 * (balance_bands 0 / 2, small or huge grids): a host whose last calls of a shape all read 0 can set balance_bands = 2.  * walk_out (ABI 8; nullable; one int64 in pinned host or device memory, zeroed by the caller): a forward job whose strip
 * evaluated more than 2560 list entries for its strips (the entries its strip mask reaches; until late in round 6: walked) stores that number there (system scope; any such job's, not the largest) -- lists
 * that are long AND stay open, which is what fg_raster_config::heavy_tiles is for: a host turns the policy on by it
 * instead of by the longest LIST alone (a dense opaque cluster has lists of ten thousand entries and closes after a few
 * hundred).
 */
int fg_stbin_fill_jobs(int N, const uint32_t* depth_keys, const int32_t* tile_rects, const uint64_t* tile_masks,
                       int tile_w, int tile_h, int64_t capacity, const int32_t* tile_offsets, const void* count_workspace,
                       int32_t* flatten_ids, int32_t* list_offsets, void* workspace, size_t workspace_bytes,
                       int width, int height, int tile_size, int32_t* jobs_fwd, int32_t* jobs_bwd,
                       int bwd_list_shares, const fg_raster_config* config, int flags, int64_t* ckpt_need_out,
                       fg_stream_t stream);
int fg_raster_jobs_fwd(int channels, int width, int height, int tile_size, const float* splats,
                       const int32_t* tile_offsets, const int32_t* flatten_ids, const int32_t* jobs,
                       const float* background, int n_clamp, float* image, float* alphas,
                       int32_t* last_ids, uint8_t* clamp_mask, float* seg_ckpt, uint32_t* live_words,
                       float* zero_buf, int64_t zero_floats, int64_t* walk_out, const fg_raster_config* config,
                       fg_stream_t stream);
int64_t fg_raster_seg_ckpt_floats(int channels, int width, int height, int tile_size, int64_t n_isects, const fg_raster_config* config);
int fg_raster_jobs_bwd(int channels, int width, int height, int tile_size, const float* splats,
                       const int32_t* tile_offsets, const int32_t* flatten_ids, const int32_t* jobs,
                       const float* background, int n_clamp, const uint8_t* clamp_mask,
                       const float* alphas, const int32_t* last_ids, const float* v_image,
                       const float* v_alphas, float* v_splats, const float* seg_ckpt, const float* image,
                       const uint32_t* live_words, const fg_raster_config* config,
                    fg_stream_t stream);
/* Split v_splats back into per-tensor gradients (any output nullable). */
int fg_unpack_grads(int N, int channels, const float* v_splats, float* v_means2d,
                    float* v_means2d_abs, float* v_conics, float* v_opacities,
                    float* v_features, fg_stream_t stream);

/* ---- Fused per-Gaussian stages (what rasterization() uses) ----------------------------------
 * fg_preprocess_fwd = fg_project_fwd + fg_sh_fwd + fg_pack_splats in one pass; bit-identical
 * outputs.  Composited channels of the record, in order: colour (3 from SH when sh_degree >= 0
 * with colors[N,k_stored,3]; or n_color direct channels colors[N,n_color] when sh_degree = -1;
 * n_color may be 0), camera depth if with_depth, then n_extra channels from extra[N,n_extra];
 * at most FG_MAX_CHANNELS in total.  antialiased != 0 multiplies the record's opacity by the
 * compensation (rasterize_mode="antialiased", freegaussian_model.py:110-119).
 * Optional outputs for the depth-first binning (both nullable; fg_bin_prepare_keys consumes them):
 *   depth_keys[N] u32  = float bits of the camera depth, 0xFFFFFFFF when culled;
 *   tile_rects[N,2] i32 = the FOOTPRINT rectangle {x0 | y0 << 16, w | h << 16}: the reference's
 *   radius-box tile rectangle (floor / ceil of (mean +- radius) / tile) shrunk to the tiles in which
 *   the splat can reach alpha >= 1/255 at a pixel centre (opacity-aware extents of the ellipse
 *   sigma <= ln(255 o), inflated so that rounding only ever keeps more).  Lists binned from it are
 *   the reference's lists minus entries that contribute to no pixel, in the same order; images and
 *   gradients are unchanged.  (0, 0) when culled or when nothing is reached.
 *   tile_masks[N] u64 (ABI 8; nullable, needs tile_rects) = the FOOTPRINT MASK of the rectangle, see fg_stbin_count: which
 *   of its (at most 8 x 8) blocks the ellipse itself reaches with a pixel centre; 0 when the rectangle is empty.
 * Optional output for the backward (nullable; SH colours of degree >= 1 only, ignored otherwise):
 *   sh_jac[N,FG_SH_JAC_FLOATS] f32 = d colour_c / d direction_d before the clamp (9 floats, c-major) and the
 *   clamp mask (bit c of the 10th float's bits: channel c passed max(. + 0.5, 0)).  Handed to
 *   fg_preprocess_bwd it replaces the 192-byte coefficient row the backward would read again per
 *   Gaussian by 40 bytes (same gradients up to the order of fp32 sums).  Rows of culled Gaussians are 0. */
int fg_preprocess_fwd(int N, const float* means, const float* quats, const float* scales,
                      const float* opacities, const float* colors, int sh_degree, int k_stored,
                      int n_color, int with_depth, const float* extra, int n_extra,
                      const float* viewmat, const float* K, int width, int height, float eps2d,
                      float near_plane, float far_plane, float radius_clip, int tile_size,
                      int antialiased, int32_t* radii, float* means2d, float* depths, float* conics,
                      float* compensations, int32_t* tiles_touched, float* splats,
                      uint32_t* depth_keys, int32_t* tile_rects, uint64_t* tile_masks, float* sh_jac, fg_stream_t stream);
/* Camera-pose gradient (ABI 8): dL/d viewmat of the view from the SAME cotangents fg_preprocess_bwd /
 * fg_preprocess_raw_bwd consume -- v_splats (the raster backward's record gradients), v_means2d (+ stride), v_depths,
 * v_conics (nullable) -- for a host whose camera pose requires a gradient (the reference's CameraOptimizer,
 * freegaussian_model.py:120: "off" in every shipped config, applied at :774; gsplat returns v_viewmats from its projection
 * backward and lets autograd carry the SH colour's share through dirs = means - inverse(viewmats)[:3, 3]).  raw != 0: the
 * parameter forms of fg_preprocess_raw_fwd (quats + d_quats, log-scales + d_scales, opacity logits, colors = features_dc,
 * features_rest); raw == 0: those of fg_preprocess_fwd (d_quats, d_scales, features_rest ignored).  sh_jac: the forward's
 * note (nullable: the coefficient rows are read instead).
 * out[19] f32: out[0..15] = dL/d viewmat, row-major 4 x 4 (through the camera-space mean p = W m + t and covariance
 * W C W^T; last row 0), out[16..18] = dL/d campos, the gradient w.r.t. the camera POSITION -W^-1 t that the SH view
 * direction is taken from -- the host adds its pull-back through the matrix inverse (d(A^-1) = -A^-1 dA A^-1) to out[0..15].
 * Deterministic (per-workgroup partial sums in `workspace`, summed in a fixed order).  A pass of its own, ~the cost of the
 * projection backward: the per-Gaussian backward is unchanged when the pose needs no gradient. */
size_t fg_viewmat_bwd_workspace_bytes(int N);
int fg_viewmat_bwd(int N, int raw, const float* means, const float* quats, const float* d_quats, const float* scales,
                   const float* d_scales, const float* opacities, const float* colors, const float* features_rest,
                   int sh_degree, int k_stored, int n_color, int with_depth, int n_extra, const float* viewmat,
                   const float* K, int width, int height, float eps2d, int antialiased, const int32_t* radii,
                   const float* v_splats, const float* v_means2d, int v_means2d_stride, const float* v_depths,
                   const float* v_conics, const float* sh_jac, float* out, void* workspace, size_t workspace_bytes,
                   fg_stream_t stream);
/* The colour + record half of fg_preprocess_fwd on its own: inputs are the projection outputs of
 * fg_project_fwd (radii, means2d, depths, conics; compensations when antialiased).  Splitting the
 * forward this way lets a host run this HBM-bound half on a second stream while the
 * latency-bound binning (fg_bin_prepare / fg_bin_emit_sort) runs on the first; records are
 * bit-identical to fg_preprocess_fwd's. */
int fg_sh_pack_fwd(int N, const float* means, const float* opacities, const float* colors, int sh_degree,
                   int k_stored, int n_color, int with_depth, const float* extra, int n_extra,
                   const float* viewmat, int antialiased, const int32_t* radii, const float* means2d,
                   const float* depths, const float* conics, const float* compensations, float* splats,
                   fg_stream_t stream);
/* fg_preprocess_bwd = fg_unpack_grads + fg_sh_bwd + fg_project_bwd in one pass.  v_splats[N,16]
 * is the record fg_raster_bwd accumulated; its xy slots are IGNORED and v_means2d is used
 * instead (autograd routes that gradient through info["means2d"] so .grad exists there): row i
 * is at v_means2d + i * v_means2d_stride floats (2 = contiguous [N,2]; 16 = the xy slots of a
 * record array, i.e. v_means2d may simply point at v_splats);
 * v_depths[N] / v_conics[N,3] (nullable) are extra gradients on those outputs.  Every output is
 * overwritten densely (zeros for culled Gaussians): v_means[N,3] v_quats[N,4] v_scales[N,3]
 * v_opacities[N] v_colors (same shape as colors) v_extra[N,n_extra].
 * sh_jac (nullable): the note fg_preprocess_fwd wrote for the same inputs; NULL = the coefficient rows
 * are read and the clamp mask / direction gradient recomputed from them. */
int fg_preprocess_bwd(int N, const float* means, const float* quats, const float* scales,
                      const float* opacities, const float* colors, int sh_degree, int k_stored,
                      int n_color, int with_depth, int n_extra, const float* viewmat, const float* K,
                      int width, int height, float eps2d, int antialiased, const int32_t* radii,
                      const float* v_splats, const float* v_means2d, int v_means2d_stride,
                      const float* v_depths, const float* v_conics, float* v_means, float* v_quats,
                      float* v_scales, float* v_opacities, float* v_colors, float* v_extra,
                      const float* sh_jac, fg_stream_t stream);

/* The same two passes on the RAW parameter forms of the reference's gauss_params
 * (freegaussian_model.py:187-196), with the activations its get_outputs applies before the raster
 * call folded in, SH path only (sh_degree >= 0):
 *   quats          -> quats / |quats| + d_quats            (:845;  d_quats[N,4] nullable)
 *   log_scales     -> exp(log_scales) + d_scales           (:844;  d_scales[N,3] nullable)
 *   opacity_logits -> sigmoid(opacity_logits)              (:851;  [N])
 *   colours        -> cat(features_dc[N,1,3], features_rest[N,k_stored-1,3])   (:801)
 * The backward returns gradients of the raw forms (v_quats through the normalisation,
 * v_log_scales through exp, v_opacity_logits through sigmoid, v_features_dc / v_features_rest)
 * and of the deltas (v_d_quats / v_d_scales, required exactly when the delta was given); every
 * output is overwritten densely. */
int fg_preprocess_raw_fwd(int N, const float* means, const float* quats, const float* d_quats,
                          const float* log_scales, const float* d_scales,
                          const float* opacity_logits, const float* features_dc,
                          const float* features_rest, int sh_degree, int k_stored, int with_depth,
                          const float* extra, int n_extra, const float* viewmat, const float* K,
                          int width, int height, float eps2d, float near_plane, float far_plane,
                          float radius_clip, int tile_size, int antialiased, int32_t* radii,
                          float* means2d, float* depths, float* conics, float* compensations,
                          int32_t* tiles_touched, float* splats, uint32_t* depth_keys,
                          int32_t* tile_rects, uint64_t* tile_masks, float* sh_jac, fg_stream_t stream);
int fg_preprocess_raw_bwd(int N, const float* means, const float* quats, const float* d_quats,
                          const float* log_scales, const float* d_scales,
                          const float* opacity_logits, const float* features_dc,
                          const float* features_rest, int sh_degree, int k_stored, int with_depth,
                          int n_extra, const float* viewmat, const float* K, int width, int height,
                          float eps2d, int antialiased, const int32_t* radii, const float* v_splats,
                          const float* v_means2d, int v_means2d_stride, const float* v_depths,
                          const float* v_conics, float* v_means, float* v_quats, float* v_d_quats,
                          float* v_log_scales, float* v_d_scales, float* v_opacity_logits,
                          float* v_features_dc, float* v_features_rest, float* v_extra,
                          const float* sh_jac, fg_stream_t stream);

/* ---- X: factored SH-gradient exchange for view-sharded data parallelism (section 8e) ----------
 * The SH coefficient gradient of one view is rank-1 per Gaussian: v_coeffs[i,k,:] =
 * basis_k(dir_view(i)) * g[i,:] with g the clamp-masked colour gradient.  Instead of all-reducing
 * 192 B per Gaussian, ranks all-gather g (12 B) and rebuild the sum locally.
 * fg_preprocess_bwd_factored = fg_preprocess_bwd (SH colours) that writes v_rgb[N,v_rgb_floats]
 * instead of v_colors: g (3 floats), or g + the unit view direction the basis was evaluated at
 * (6 floats) when every rank renders its own deformed means.  fg_sh_grad_accumulate: payload =
 * n_views blocks of view_stride floats; payload_floats = 3: block v = [g_v (3N floats) | camera
 * position of view v (3 floats) | padding] and the direction is normalize(means - cam_v);
 * payload_floats = 6: block v = N rows [g_v | direction] (means unused, may be NULL).  Writes
 * v_coeffs[N,k_stored,3] = scale * sum_v basis(direction_v) (x) g_v densely. */
int fg_preprocess_bwd_factored(int N, const float* means, const float* quats, const float* scales,
                               const float* opacities, const float* colors, int sh_degree, int k_stored,
                               int with_depth, int n_extra, const float* viewmat, const float* K,
                               int width, int height, float eps2d, int antialiased, const int32_t* radii,
                               const float* v_splats, const float* v_means2d, int v_means2d_stride,
                               const float* v_depths, const float* v_conics, float* v_means,
                               float* v_quats, float* v_scales, float* v_opacities, float* v_rgb,
                               int v_rgb_floats, float* v_extra, const float* sh_jac, fg_stream_t stream);
int fg_sh_grad_accumulate(int N, int n_views, int sh_degree, int k_stored, const float* means,
                          const float* payload, int64_t view_stride, int payload_floats, float scale,
                          float* v_coeffs, fg_stream_t stream);
/* The same exchange for the MODEL's parameter layout (ABI 7; freegaussian_model.py:187-196: features_dc [N,3] and
 * features_rest [N,K-1,3] are two tensors, the other gradients come out of fg_preprocess_raw_bwd):
 * fg_preprocess_raw_bwd_factored = fg_preprocess_raw_bwd that writes v_rgb[N,v_rgb_floats] instead of the two
 * coefficient gradients; fg_sh_grad_accumulate_split rebuilds them from the gathered payloads into the two arrays. */
int fg_preprocess_raw_bwd_factored(
    int N, const float* means, const float* quats, const float* d_quats, const float* log_scales, const float* d_scales,
    const float* opacity_logits, const float* features_dc, const float* features_rest, int sh_degree, int k_stored,
    int with_depth, int n_extra, const float* viewmat, const float* K, int width, int height, float eps2d, int antialiased,
    const int32_t* radii, const float* v_splats, const float* v_means2d, int v_means2d_stride, const float* v_depths,
    const float* v_conics, float* v_means, float* v_quats, float* v_d_quats, float* v_log_scales, float* v_d_scales,
    float* v_opacity_logits, float* v_rgb, int v_rgb_floats, float* v_extra, const float* sh_jac, fg_stream_t stream);
int fg_sh_grad_accumulate_split(int N, int n_views, int sh_degree, int k_stored, const float* means,
                                const float* payload, int64_t view_stride, int payload_floats, float scale,
                                float* v_features_dc, float* v_features_rest, fg_stream_t stream);
/* Sparse payload of the factored view-DP exchange (ABI 8).  Only Gaussians that took part in a pixel of the view have a
 * colour gradient; a rank's all-gathered block can be [count, camera position(3) | capacity rows of (id, g[3] (, unit
 * direction[3]))] instead of N dense rows (the reference is single-GPU, scripts/run.sh:58: new capability).
 * fg_payload_compact: the rows of dense[N, payload_floats] with a non-zero g, in id order -- incl_scan[N] (int32) is the
 * inclusive scan of the caller's row flags, row i goes to slot incl_scan[i] - 1 --, into out[4 + capacity * (1 +
 * payload_floats)]; out[0] = the count as int bits (rows beyond capacity are dropped: count > capacity tells the receiver
 * not to use the block), out[1..3] are left to the caller.
 * fg_payload_expand: n_views such blocks (block_stride floats apart) back into dense blocks of dense_stride floats laid out
 * as fg_sh_grad_accumulate[_split] reads them; the dense blocks must be zero on entry. */
int fg_payload_compact(int N, int payload_floats, const float* dense, const int32_t* incl_scan, int64_t capacity,
                       float* out, fg_stream_t stream);
int fg_payload_expand(int N, int payload_floats, int n_views, const float* compact, int64_t block_stride,
                      int64_t capacity, float* dense, int64_t dense_stride, fg_stream_t stream);

/* ---- One call per direction (ABI 7): the whole eager step of one view ------------------------------------------
 * fg_step_fwd = fg_preprocess_fwd (raw = 0) or fg_preprocess_raw_fwd (raw = 1) -> fg_stbin_count -> fg_stbin_fill_jobs ->
 * fg_raster_jobs_fwd; fg_step_bwd = fg_raster_jobs_bwd -> the matching per-Gaussian backward (the factored one when
 * io->v_rgb is given).  Same kernels, same results as the stage-wise calls: what changes is the host's work per step
 * -- three small structs instead of ~150 marshalled arguments, two workspace allocations instead of ~20 buffers -- which
 * is the whole cost of a launch-bound step (the reference's quarter- and half-resolution phases,
 * freegaussian_model.py:626-633).  Replaces, like those calls, the rasterization(...) of freegaussian_model.py:847-868
 * and its autograd backward.
 *   fg_step_desc    what is rendered (sizes, SH degree, channels, composite epilogue, list capacity, flags)
 *   fg_step_io      device pointers: the inputs (plain or raw parameter forms, as the two preprocess entry points take
 *                   them), count_out (pinned host memory: a block of FG_COUNT_OUT_WORDS int64, the five words of
 *                   fg_stbin_count among them, see there; a smaller block is written past), and for the backward the
 *                   upstream gradients and the output gradients
 *   fg_step_layout  from fg_step_layout_query: offsets / sizes of every buffer inside the two caller-allocated
 *                   workspaces -- `keep` (read by the backward and by the caller: FG_STEP_RADII .. FG_STEP_CLAMP_MASK;
 *                   uninitialised) and `tmp` (FG_STEP_COUNT_WS, FG_STEP_FILL_WS: free again once the call's launches
 *                   have run).  FG_ERR_UNSUPPORTED: shapes the supertile binning or the job-list launches do not take
 *                   (use the stage-wise entry points).
 * A list longer than desc->capacity leaves empty lists (see fg_stbin_fill) and an image of the background: the host
 * sees it in count_out[0] and repeats fg_step_fwd with a larger capacity and fresh workspaces. */
enum {
  FG_STEP_RADII, FG_STEP_MEANS2D, FG_STEP_DEPTHS, FG_STEP_CONICS, FG_STEP_COMP, FG_STEP_TILES, FG_STEP_SPLATS,
  FG_STEP_DEPTH_KEYS, FG_STEP_TILE_RECTS, FG_STEP_TILE_MASKS, FG_STEP_SH_JAC, FG_STEP_TILE_OFFSETS, FG_STEP_LIST_OFFSETS, FG_STEP_FLATTEN_IDS,
  FG_STEP_JOBS, FG_STEP_LIVE, FG_STEP_SEG_CKPT, FG_STEP_V_SPLATS, FG_STEP_RENDER, FG_STEP_ALPHAS, FG_STEP_LAST_IDS,
  FG_STEP_CLAMP_MASK, FG_STEP_COUNT_WS, FG_STEP_FILL_WS, FG_STEP_BUFFERS
};
typedef struct fg_step_desc {
  int32_t size;           /* sizeof(fg_step_desc) */
  int32_t N, width, height, tile_size;
  int32_t raw;            /* 1: the raw parameter forms of fg_preprocess_raw_* (SH colours only) */
  int32_t sh_degree;      /* -1: colors[N,n_color] direct channels */
  int32_t k_stored, n_color, with_depth, n_extra, antialiased;
  int32_t n_clamp;        /* composite epilogue: clamp the first n_clamp channels; io->background nullable */
  int32_t want_backward;  /* 0: no liveness words / checkpoints / record-gradient array / SH note */
  int32_t list_shares;    /* backward over shares of the tiles' lists (three channels; fg_raster_seg_ckpt_floats) */
  int32_t flags;          /* FG_STBIN_LONG_SEGMENTS | FG_STEP_NO_FOOTPRINT_MASKS (ABI 8: the step bins by footprint masks -- see
                             fg_stbin_count -- unless this is set: whole rectangles, as before) */
  float eps2d, near_plane, far_plane, radius_clip;
  int64_t capacity;       /* list entries the workspaces hold */
} fg_step_desc;
typedef struct fg_step_io {
  const float *means, *quats, *d_quats, *scales, *d_scales, *opacities, *colors, *features_rest, *extra, *viewmat, *K,
      *background;        /* raw = 1: scales = log-scales, opacities = logits, colors = features_dc */
  int64_t* count_out;     /* nullable; FG_COUNT_OUT_WORDS int64 */
  /* backward only */
  const float *v_render, *v_alphas, *v_depths, *v_conics;  /* upstream gradients; all but v_render nullable */
  float *v_means, *v_quats, *v_d_quats, *v_scales, *v_d_scales, *v_opacities, *v_colors, *v_features_rest, *v_extra;
  float* v_rgb;           /* non-NULL: the factored form (v_colors / v_features_rest unused) */
  int32_t v_rgb_floats;
  /* optional hipEvent_t pair recorded on `stream` around the call's raster launch (forward call: the raster forward,
     backward call: the raster backward): a host that times the dominant kernel of the step does not have to take the
     stage-wise entry points for it */
  void *ev_raster_begin, *ev_raster_end;
  int64_t* ckpt_need_out; /* nullable, forward only: fg_stbin_fill_jobs' ckpt_need_out (int64[9]); + one more word, [9]:
                             fg_raster_jobs_fwd's walk_out (the caller zeroes it) */
} fg_step_io;
typedef struct fg_step_layout {
  int64_t keep_bytes, tmp_bytes;
  int64_t offset[FG_STEP_BUFFERS], nbytes[FG_STEP_BUFFERS];  /* nbytes 0: the step has no such buffer */
  int64_t jobs_words, seg_ckpt_floats;
  int32_t channels;
} fg_step_layout;
int fg_step_layout_query(const fg_step_desc* desc, const fg_raster_config* config, fg_step_layout* out);
int fg_step_fwd(const fg_step_desc* desc, const fg_raster_config* config, const fg_step_io* io, void* keep, void* tmp,
                const fg_step_layout* layout, fg_stream_t stream);
int fg_step_bwd(const fg_step_desc* desc, const fg_raster_config* config, const fg_step_io* io, void* keep,
                const fg_step_layout* layout, fg_stream_t stream);

/* S1 in one pass: the densification statistics after_train_iter keeps (freegaussian_model.py:369-392), all in place:
 * for radii[i] > 0: xys_grad_norm[i] += |absgrad[i]| (absgrad [N,2]), vis_counts[i] += 1,
 * max_2dsize[i] = max(max_2dsize[i], radii[i] / max_dim); other rows untouched. */
int fg_densify_stats(int N, const float* absgrad, const int32_t* radii, float max_dim, float* xys_grad_norm,
                     float* vis_counts, float* max_2dsize, fg_stream_t stream);
/* ---- D: adaptive density control ---------------------------------
 * The reference's refinement_after / split_gaussians / dup_gaussians / cull_gaussians and the
 * Adam-state surgery around them (freegaussian_model.py:313-367, :404-571), as: one decision
 * pass, prefix sums (the caller's), one map pass, ONE coalesced row copy per tensor into its final
 * place, one fix-up pass over the new rows.
 *
 * fg_densify_flags: flags[N], bit 0 split, bit 1 duplicate, bit 2 old row survives, bit 3 its
 * split children survive the cull, bit 4 its duplicate survives.  Thresholds as in the config
 * (:68-88); pass split_screen_size / cull_scale_thresh / cull_screen_size < 0 to disable the
 * step-dependent tests (:425, :505-511); do_densify = 0 is the cull-only branch (:466-467).
 * max_dim = max(H, W) of the last render (:421).  max_2dsize nullable. */
int fg_densify_flags(int N, int do_densify, float max_dim, float densify_grad_thresh,
                     float densify_size_thresh, float split_screen_size, float cull_alpha_thresh,
                     float cull_scale_thresh, float cull_screen_size, const float* xys_grad_norm,
                     const float* vis_counts, const float* max_2dsize, const float* log_scales,
                     const float* opacity_logits, uint8_t* flags, fg_stream_t stream);
/* pos_old / pos_child / pos_dup [N]: EXCLUSIVE prefix sums of flag bits 2 / 3 / 4; rank_split[N]:
 * of bit 0.  n_old, n_child: totals of bits 2, 3; n_split_total: of bit 0.  Row order of the new set
 * (the reference's): surviving old rows, children sample-major, duplicates.  Outputs for every
 * new-set row j: src_index[j] = the old row it copies; sample_index[j] = row of the
 * randn((n_split_samples * n_split_total, 3)) draw (:530) for a child, -2 for the duplicate of a
 * split parent (it carries the shrunk scales: `dups` is evaluated after the in-place shrink,
 * :428-431), -1 otherwise. */
int fg_densify_map(int N, const uint8_t* flags, const int32_t* pos_old, const int32_t* pos_child,
                   const int32_t* pos_dup, const int32_t* rank_split, int n_old, int n_child,
                   int n_split_total, int n_split_samples, int32_t* src_index, int32_t* sample_index,
                   fg_stream_t stream);
/* dst[j,:] = src[src_index[j],:] for rows of row_floats floats; rows j >= zero_from are zeroed
 * instead (new rows of the Adam moments, :343-356). */
int fg_gather_rows(int64_t n_rows, int row_floats, const float* src, const int32_t* src_index,
                   int64_t zero_from, float* dst, fg_stream_t stream);
/* In place on rows [first_row, first_row + n_rows) of the NEW set: children (sample_index >= 0):
 * mean += R(q/|q|) (exp(s) * z), s = log(exp(s)/1.6) (:530-549); sample_index == -2: only the
 * scales shrink. */
int fg_split_children(int first_row, int n_rows, const int32_t* sample_index, const float* samples,
                      float* means, float* log_scales, const float* quats, fg_stream_t stream);

/* ---- M: attribute-mask back-projection -------------------------
 * One key frame of preprocess/knn_gaussian.py:116-132: every visible Gaussian (radii > 0) whose
 * centre, truncated toward zero, lies in the image and whose depth agrees with the rendered
 * expected depth there (-0.1 d < d - depth_i < d) ORs that pixel's labels into its row:
 *   gaussian_masks[i, j] |= atrb_masks[y, x, j] & mask_valids[j]      j < n_attributes
 * atrb_masks[H,W,n_labels_stored] and mask_valids[n_labels_stored] are bool (1 byte), the last
 * stored label (background) is dropped as the reference's `[..., :-1]` does: pass
 * n_attributes = n_labels_stored - 1.  gaussian_masks[N,n_attributes] bool, caller-zeroed, is
 * accumulated over frames and saved as gaussian_mask_NxM.npy (freegaussian_pipeline.py:45-47). */
int fg_mask_backproject(int N, const float* means2d, const float* depths, const int32_t* radii,
                        const float* depth_map, int width, int height, const uint8_t* atrb_masks,
                        const uint8_t* mask_valids, int n_labels_stored, int n_attributes,
                        uint8_t* gaussian_masks, fg_stream_t stream);

/* ---- F: flow derivative -------------------------------------------------------------------
 * Per-pixel camera flow A v / Z + B w (preprocess/epipolar_flow.py:274-309; pixel centres at
 * integer coordinates, infinite depth -> 0, :315-317).  depth[H,W], veloc[3], omega[3],
 * flow[H,W,2]. */
int fg_camera_flow(int width, int height, const float* depth, const float* K,
                   const float* veloc, const float* omega, float* flow, fg_stream_t stream);
/* Exact-reprojection camera flow (preprocess/epipolar_flow_bp.py:268-295): per pixel, lift with
 * depth0, map by M[3,4] (row-major; the host composes it from the two poses exactly as the
 * reference does, c2w1 . c2w0^-1 after its OpenGL->OpenCV column flip, :265-266, :275-276), project
 * with K, divide by depth1, subtract the pixel (pixel centres at integer coordinates, :268).
 * flow[H,W,2] = sign * (uv - xy); sign = -1 is the "sceneflow" the reference returns (:295).
 * Infinite depth0 -> 0 (:285-287). */
int fg_reprojection_flow(int width, int height, const float* depth0, const float* depth1,
                         const float* K, const float* M, float sign, float* flow, fg_stream_t stream);
/* Per-Gaussian projection-flow Jacobian (Lemma 1, docs/index.html:256-273, code sign
 * convention of epipolar_flow.py:277-298): for visible Gaussian i at means2d mu_i, depth Z_i,
 * camera-frame velocity vel[i]:   u_gs[i] = A(mu_i) vel[i] / Z_i
 *                                 u_cam[i] = A(mu_i) veloc / Z_i + B(mu_i) omega. */
int fg_flow_fwd(int N, const float* means2d, const float* depths, const int32_t* radii,
                const float* vel, const float* K, const float* veloc, const float* omega,
                float* u_gs, float* u_cam, fg_stream_t stream);
int fg_flow_bwd(int N, const float* means2d, const float* depths, const int32_t* radii,
                const float* vel, const float* K, const float* veloc, const float* omega,
                const float* v_u_gs, const float* v_u_cam, float* v_means2d, float* v_depths,
                float* v_vel, fg_stream_t stream);

/* ---- L: the image loss of the training step, fused (csrc/loss.hip) --------------------------------------
 * mean|gt - pred| and mean SSIM(gt, pred) of two [H, W, C] images -- the two terms of the reference's main loss
 * (freegaussian_model.py:965-981; SSIM = pytorch_msssim.SSIM(data_range=1.0, size_average=True, channel=3), :22, :211:
 * 11-tap Gaussian window, sigma 1.5, 'valid' borders) -- in one launch forward and one backward instead of ~200 torch
 * launches each way (10.4 ms per step at 1920 x 1080 on an MI355X, scripts/loss_time.py).  height, width > 10.
 *   fg_l1_ssim_fwd: out[0] = mean |gt - pred|, out[1] = mean SSIM (device floats; reduced in a fixed order: reproducible);
 *                   maps[3 * C * (H-10) * (W-10)]: the SSIM map's partial derivatives, for the backward (opaque);
 *                   workspace[fg_l1_ssim_workspace_floats(H, W, C)] floats.
 *   fg_l1_ssim_bwd: v_out[2] (device) = dL/d out[0], dL/d out[1]  ->  v_pred[H, W, C] (overwritten; gt gets no gradient). */
size_t fg_l1_ssim_workspace_floats(int height, int width, int channels);
int fg_l1_ssim_fwd(int height, int width, int channels, const float* pred, const float* gt, float* maps,
                   float* workspace, size_t workspace_floats, float* out, fg_stream_t stream);
int fg_l1_ssim_bwd(int height, int width, int channels, const float* pred, const float* gt, const float* maps,
                   const float* v_out, float* v_pred, fg_stream_t stream);

/* ---- A: one Adam update of a dense float32 tensor in one launch (csrc/adam.hip) ---------------------------
 * torch.optim.Adam's defaults (no weight decay, no amsgrad), the same fp32 operations in the same order as torch's
 * own step: param, exp_avg, exp_avg_sq updated in place from grad; step = the 1-based count of this update (bias
 * corrections 1 - beta^step computed in double, as torch does; the hyper-parameters are doubles for the same reason).  All four arrays 16-byte aligned, n elements.
 * Replaces optimizer.step() of the reference's six Gaussian parameter groups (freegaussian_config.py optimizers):
 * 1.42 ms -> 0.35 ms per iteration at 1M Gaussians (scripts/train_step_bench.py). */
int fg_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr, double beta1,
                 double beta2, double eps, int64_t step, fg_stream_t stream);
/* The same for several tensors in ONE launch (every 16 tensors one): each tensor with its own hyper-parameters and
 * update count, results identical to fg_adam_step per tensor.  At the reference's low resolutions an iteration is bound
 * by launches: six Gaussian parameter groups, six launches -> one. */
#define FG_ADAM_MAX_TENSORS 16
typedef struct fg_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t n;
  double lr, beta1, beta2, eps;
  int64_t step;
} fg_adam_tensor;
int fg_adam_step_multi(int count, const fg_adam_tensor* tensors, fg_stream_t stream);

/* ---- K9 (ABI 10): exact k nearest neighbours of every row of xyz[n,3] among the OTHER rows (the initial scales of the
 * Gaussians: mean distance to the three nearest neighbours, freegaussian_model.py:158-162, :293-311).
 * dist2_out[n,k]: SQUARED Euclidean distances, ascending per row, d2 = (dx dx + dy dy) + dz dz in fp32 without contraction,
 * dx = x_query - x_neighbour; idx_out[n,k] (nullable): the neighbours' row numbers.  Rows are in the caller's order.
 * Ties: candidates are ordered by (d2, row number), so among equal distances the lower row comes first -- and is the one
 * kept at the k-th place; the query's own row is excluded by number, another row at the same position is a neighbour at
 * distance 0.  1 <= k <= FG_KNN_MAX_K and n > k, n < 2^31 (else FG_ERR_INVALID_ARG, as for a workspace below
 * fg_knn_workspace_bytes(n)); n == 0 does nothing.
 * NOT capturable in a graph: the call reads a few KB of sampled coordinates back (one stream synchronisation) to size
 * its cell grid.  Non-finite coordinates are the caller's responsibility: the call stays in bounds, the rows' results
 * are unspecified. */
#define FG_KNN_MAX_K 8
size_t fg_knn_workspace_bytes(int64_t n);
int fg_knn(int64_t n, const float* xyz, int k, float* dist2_out, int32_t* idx_out, void* workspace,
           size_t workspace_bytes, fg_stream_t stream);

/* ---- K10 (ABI 11): fused fp32 FORWARD of the deformation / control MLP (inference; training keeps the library GEMMs):
 * one call, two launches (the weights re-ordered into the workspace, then the network).
 * Per row: [posenc(x, 10) (63 wide, computed in the kernel with the accurate sin / cos), aux (aux_width wide)] -> 8 linears
 * of 256 with ReLU, the input row re-injected IN FRONT of h after layer 4 (layer 5's weight is [256, in_ch + 256]) -> up
 * to FG_MLP_MAX_HEADS head linears of together <= 16 rows over the final h.  Weights and biases as nn.Linear stores them
 * ([out, in] row-major).  aux[N, aux_width] has a row stride in floats; stride 0 = one row for all.  Products run (under
 * precision = FG_MLP_FP32, the default; FG_MLP_BF16X3 is described at the constants below) on the
 * exact-fp32 matrix instructions: every output element is one fmaf chain over its own row in a fixed order, so a row's
 * result does not depend on the other rows or on its place; no atomics.
 *   FG_MLP_SE3   heads (3, 3, 4, 3) = (w, v, rotation, scaling): theta = |w|, screw = (w / theta + 1e-5, v / theta + 1e-5),
 *                out[0] = exp_se3 [N,4,4] (bottom row 0,0,0,1), out[1] = rotation [N,4], out[2] = scaling [N,3],
 *                out[3] = the transform applied to x [N,3]
 *   FG_MLP_PLAIN out[h] = head h [N, head_rows[h]]
 * Every out[] pointer is nullable (that array is not written).  The workspace receives a re-ordered copy of the weights in
 * the same call (about 2 MB read and written, nothing kept between calls); 16-byte aligned, fg_mlp_workspace_bytes(N)
 * bytes (FG_ERR_WORKSPACE below that).  N == 0 does nothing.  FG_ERR_INVALID_ARG: a null required pointer, aux_width
 * outside 1..64, head rows outside 1..16 (or more than 16 together, or not (3,3,4,3) in SE(3) mode), an unknown mode;
 * FG_ERR_UNSUPPORTED: depth / width / multires other than 8 / 256 / 10.  Asynchronous and capturable in a graph. */
#define FG_MLP_ROW_TILE 64 /* rows per workgroup */
#define FG_MLP_MAX_HEADS 4
#define FG_MLP_SE3 0
#define FG_MLP_PLAIN 1
/* fg_mlp_desc::precision -- how the products of the trunk and of the backward's data chain are formed.  The word was
 * `reserved` (same type, same offset, sizeof unchanged): every earlier caller passes 0.
 *   FG_MLP_FP32    the exact-fp32 matrix instructions, as described above and below.  The default.
 *   FG_MLP_BF16X3  opt-in: the split-bf16 product on the bf16 matrix instructions.  The contract, which a caller can restate:
 *     split(v):  hi = bf16(v), round to nearest even (v_cvt_pk_bf16_f32); lo = bf16(v - float(hi)), the subtraction exact in fp32.
 *     A.B     =  A_hi.B_hi + A_hi.B_lo + A_lo.B_hi, accumulated in fp32 by v_mfma_f32_32x32x16_bf16; A_lo.B_lo is dropped.  The
 *                accumulator starts from the bias where the fp32 chain does (from 0 in the backward).  Order per output
 *                element: K in steps of 16, ascending; inside a step the three terms in the order written, each the
 *                instruction's own sum over k = 16 s + 8 h + j (lane half h, j = 0..7).  Nothing but the element's own row enters.
 *     where   :  forward -- trunk layers 0..7, both halves of layer 5; backward -- g(h_7) = g_heads W_h, g(h_{l-1}) = P_l W_l,
 *                and under fg_mlp_bwd_inputs / a non-null g_enc the two g_enc products.  Values are split once: the weights by
 *                the pack launch of the same call, an activation / gradient tile by the lane that holds its accumulator.
 *     fp32 as before: the positional encoding, biases, ReLU, the SE(3) epilogue, the mask h_l > 0 (read from acts), and the
 *                forward's 16-row head product (v_mfma_f32_16x16x4_f32 over the fp32 h_7: 0.6 % of the FLOP).
 *     stored  :  acts, enc, heads, g_pre, g_enc and the outputs are the fp32 accumulator values, never re-rounded ones, so
 *                fg_mlp_param_grads runs unchanged, in exact fp32, on them: the WEIGHT-GRADIENT products are not split.
 *     Against float64 the results stay within 1e-4 of each array's largest magnitude (measured: about 1e-5, an order above
 *     fp32's 1e-6); a pre-activation moves by about 5e-6 of its layer's scale, so a row within that of a ReLU kink may take the
 *     other branch.  Two runs are bit for bit equal, rows are independent of one another and of their tile, no atomics;
 *     non-finite inputs give non-finite outputs (|v| beyond bf16's largest finite value, 3.39e38, splits to infinity).
 *     Workspace sizes, arguments and error codes are those of FG_MLP_FP32.
 * Honoured by fg_mlp_fwd, fg_mlp_train_fwd, fg_mlp_bwd, fg_mlp_bwd_inputs and fg_mlp_train_bwd (whose chunks run the same
 * chain kernel); IGNORED by fg_mlp_param_grads (always fp32; the weight-gradient products have a word of their own, the
 * wgrad_precision of fg_mlp_param_grads_p / fg_mlp_train_bwd_p further down).  Any other value: FG_ERR_INVALID_ARG from the five calls.
 * fg_mlp_precision_supported(precision) = 1 where this library takes the value, else 0: ask before the call. */
#define FG_MLP_FP32 0
#define FG_MLP_BF16X3 1
int fg_mlp_precision_supported(int32_t precision);
typedef struct fg_mlp_desc {
  int32_t size; /* sizeof(fg_mlp_desc) */
  int32_t mode;
  int32_t depth, width, multires;
  int32_t aux_width;
  int32_t n_heads;
  int32_t head_rows[FG_MLP_MAX_HEADS];
  int32_t precision; /* FG_MLP_FP32 (0) or FG_MLP_BF16X3 */
  int64_t aux_stride;
  const float* x;   /* [N,3] */
  const float* aux; /* [N or 1, aux_width] */
  const float* weight[8];
  const float* bias[8];
  const float* head_weight[FG_MLP_MAX_HEADS];
  const float* head_bias[FG_MLP_MAX_HEADS];
  float* out[FG_MLP_MAX_HEADS];
} fg_mlp_desc;
size_t fg_mlp_workspace_bytes(int64_t N);
int fg_mlp_fwd(int64_t N, const fg_mlp_desc* desc, void* workspace, size_t workspace_bytes, fg_stream_t stream);

/* ---- K10 training (ABI 12): the same network with what a backward needs, and the backward's data chain.  Both take the
 * descriptor of fg_mlp_fwd with mode = FG_MLP_PLAIN (FG_ERR_INVALID_ARG otherwise); desc->out is not read, and
 * fg_mlp_bwd does not read desc->x / desc->aux.  rows_total = the sum of head_rows.  Trunk layers are 0-based:
 * h_0 = relu(W_0 inp + b_0), h_l = relu(W_l in_l + b_l) with in_l = h_{l-1} except in_5 = [inp, h_4].
 *   fg_mlp_train_fwd  the forward of fg_mlp_fwd (the same kernel tile, k order and fmaf chains: heads is bit for bit what
 *                     FG_MLP_PLAIN writes), which also stores per row
 *                       heads [N, rows_total]  the raw head outputs, packed in head order
 *                       enc   [N, FG_MLP_ENC_WIDTH(aux_width)]  the encoded input row [posenc(x, 10), aux, 0 ...]
 *                       acts  [8, N, 256]      the post-ReLU activations h_0 .. h_7
 *   fg_mlp_bwd        from the head cotangents g_heads [N, rows_total] and acts: g(h_7) = g_heads W_h, then for l = 7 .. 0
 *                       P_l = g(h_l) where h_l > 0, else 0 (the rule of the ReLU's backward), stored to g_pre [8, N, 256];
 *                       g(h_{l-1}) = P_l W_l[:, hidden columns]  (l >= 1; layer 5's hidden columns are W_5[:, in_ch:])
 *                     No gradient is formed for the input row (layer 0's input, layer 5's input columns): in training the
 *                     network's inputs want none (fg_mlp_bwd_inputs, below, forms it).  The parameter gradients are products of these arrays
 *                     (gW_l = P_l^T in_l, gb_l = sum of P_l over the rows, gW_head = g_heads^T h_7), left to the caller.
 *                     Every element of g_pre is one fmaf chain over its own row in a fixed order (64-row tiles on the exact
 *                     fp32 matrix instructions, the gradient tile in place in shared memory): rows are independent and two
 *                     runs are bit for bit equal; plain stores, no atomics.  A second re-ordered copy of the weights (the
 *                     transpose of the forward's: the reduction runs over a layer's output index) is written into the
 *                     workspace by a launch of the same call; nothing is kept between calls.
 * Rows >= N of the last tile are neither read nor written.  The workspace: 16-byte aligned, fg_mlp_train_workspace_bytes(N)
 * bytes for either call (FG_ERR_WORKSPACE below that).  N == 0 does nothing; error codes as fg_mlp_fwd.  Asynchronous and
 * capturable in a graph. */
#define FG_MLP_ENC_WIDTH(aux_width) ((63 + (aux_width) + 7) / 8 * 8)
size_t fg_mlp_train_workspace_bytes(int64_t N);
int fg_mlp_train_fwd(int64_t N, const fg_mlp_desc* desc, float* heads, float* enc, float* acts, void* workspace,
                     size_t workspace_bytes, fg_stream_t stream);
int fg_mlp_bwd(int64_t N, const fg_mlp_desc* desc, const float* g_heads, const float* acts, float* g_pre, void* workspace,
               size_t workspace_bytes, fg_stream_t stream);

/* ---- K10 training with input-row gradients (ABI 13): fg_mlp_bwd, which also forms the gradient of the encoded input row
 * that fg_mlp_train_fwd stores as enc -- what a network in front of the trunk (the blender net's timenet), a per-row aux
 * or the points themselves need.  Descriptor, g_heads, acts and error codes as fg_mlp_bwd (FG_MLP_PLAIN only; desc->x /
 * desc->aux / desc->out are not read); a null g_enc is FG_ERR_INVALID_ARG.
 *   g_pre [8, N, 256]   exactly what fg_mlp_bwd writes: the same chains, bit for bit
 *   g_enc [N, FG_MLP_ENC_WIDTH(aux_width)]
 *                       g_enc[row, k] = sum_j P_5[row, j] W_5[j, k] + sum_j P_0[row, j] W_0[j, k] for k < in_ch = 63 +
 *                       aux_width; the pad columns k >= in_ch are written as exact zeros.  One fmaf chain per element over
 *                       its own row in a fixed order: from 0, layer 5's 256 terms in the k order of the other products, then
 *                       layer 0's.  Rows are independent and two runs are bit for bit equal; plain stores, no atomics.
 * The chain from g_enc to the inputs is the caller's: g_aux = g_enc[:, 63:63 + aux_width] (summed over the rows for a
 * one-row aux), g_x = g_enc[:, :3] + sum_k 2^k (g_sin_k cos_k - g_cos_k sin_k) with sin_k = enc[3 + 6 k + c] and
 * cos_k = enc[3 + 6 k + 3 + c].  The kernel is fg_mlp_bwd's tile with two products more (8/7 of its matrix instructions):
 * the layer-5 part is taken while P_5 sits in shared memory and waits in g_enc, written and read back by the same lane, until
 * layer 0; no more shared memory.
 * A third re-ordered block of weights (the input columns of layers 0 and 5, 256 KB) is written behind the other two by a
 * launch of the same call.  Rows >= N of the last tile are neither read nor written.  The workspace: 16-byte aligned,
 * fg_mlp_bwd_inputs_workspace_bytes(N) bytes (FG_ERR_WORKSPACE below that; fg_mlp_train_workspace_bytes is unchanged).
 * N == 0 does nothing.  Asynchronous and capturable in a graph. */
size_t fg_mlp_bwd_inputs_workspace_bytes(int64_t N);
int fg_mlp_bwd_inputs(int64_t N, const fg_mlp_desc* desc, const float* g_heads, const float* acts, float* g_pre, float* g_enc,
                      void* workspace, size_t workspace_bytes, fg_stream_t stream);

/* ---- K10 parameter gradients (ABI 14): the products that fg_mlp_bwd leaves to the caller, in one call of two launches.
 * From enc and acts as fg_mlp_train_fwd stores them, g_pre (P_l) as fg_mlp_bwd / fg_mlp_bwd_inputs store it and the head
 * cotangents g_heads [N, rows_total]:
 *   gW_l    = P_l^T in_l          in_0 = enc[:, :in_ch], in_5 = [enc[:, :in_ch], h_4], in_l = h_{l-1} otherwise (in_ch = 63 + aux_width)
 *   gb_l    = sum over the rows of P_l
 *   gW_head = g_heads^T h_7 (split by head_rows),   gb_head = sum over the rows of g_heads
 * Outputs go to fg_mlp_grads in the layout nn.Linear stores: weight[0] [256, in_ch], weight[5] [256, in_ch + 256] (the input
 * columns in front), the other weights [256, 256], bias[l] [256], head_weight[h] [head_rows[h], 256], head_bias[h]
 * [head_rows[h]].  Every pointer in it is nullable: a null entry is not formed and nothing is written for it; all null is
 * FG_OK and launches nothing.  The descriptor supplies the shape only (size, mode = FG_MLP_PLAIN, depth, width, multires,
 * aux_width, n_heads, head_rows): its parameter and input pointers are not read and may be null.  An input array may be
 * null where no gradient asked for reads it (enc: weight[0], weight[5]; acts: weight[1..7], head weights; g_pre: trunk
 * weights and biases; g_heads: head weights and biases); enc, acts and g_pre are 16-byte aligned.
 *   Matrix instructions: v_mfma_f32_32x32x2_f32 (exact fp32) for the hidden and input products -- the A lane (i, k) takes
 *     P[row k][col i], the B lane (k, j) in[row k][col j], so both operands are read along the rows as stored and nothing is
 *     transposed -- and v_mfma_f32_16x16x4_f32 for the 16-wide head cotangents.  All accumulation is fp32.
 *   Deterministic, no atomics: the rows are cut into slabs; each slab's partial results go to the workspace with plain
 *     stores; a second launch of the same call adds the partials in slab order and writes the outputs.  Two runs on the
 *     same inputs are bit for bit equal.
 *   The cut depends on N alone, never on the device or its load: fg_mlp_param_grads_slab_rows(N) rows per slab -- a multiple
 *     of 64, at most FG_MLP_WGRAD_MAX_SLAB = 4096, the slabs as equal as that allows; max(ceil(N / 4096), min(32, ceil(N / 512)))
 *     slabs at the most, so below 131 072 rows the slabs are shorter and a small N still fills the machine.
 *   Chain length: an output element of a slab is one fmaf chain over the slab's rows in row order: never more than 4096 terms
 *     (half the 8192-row chunk of the library path it replaces).
 *   Bias sums are formed in the pass that reads g_pre / g_heads for the products (from the staged operand tile); a bias
 *     whose weight is null reads its P_l once.
 *   Rows >= N are never read (acts[l] is followed directly by acts[l + 1]); the pad columns k >= in_ch of enc never reach
 *     an output.  The rows of weight[0] / weight[5] have strides in_ch / in_ch + 256, odd for odd aux widths: outputs are
 *     written with scalar stores, no alignment is assumed.
 * The workspace: 16-byte aligned, fg_mlp_param_grads_workspace_bytes(N) bytes = 2 121 792 bytes per slab of the bound above
 * (FG_ERR_WORKSPACE below that; 0 for N <= 0).  N == 0 does nothing.  FG_ERR_INVALID_ARG: negative N, a null desc, a null
 * input whose product is asked for, a null out, wrong size fields, aux_width outside 1..64, head rows outside 1..16 (or more
 * than 16 together), mode other than FG_MLP_PLAIN, a null or misaligned workspace; FG_ERR_UNSUPPORTED: depth / width /
 * multires other than 8 / 256 / 10.  Asynchronous and capturable in a graph. */
#define FG_MLP_WGRAD_MAX_SLAB 4096 /* rows of the longest slab */
#define FG_MLP_WGRAD_MIN_SPLIT 512 /* up to 32 slabs of about N / 32 rows, none cut below this */
typedef struct fg_mlp_grads {
  int32_t size; /* sizeof(fg_mlp_grads) */
  int32_t reserved;
  float* weight[8];
  float* bias[8];
  float* head_weight[FG_MLP_MAX_HEADS];
  float* head_bias[FG_MLP_MAX_HEADS];
} fg_mlp_grads;
size_t fg_mlp_param_grads_workspace_bytes(int64_t N);
int fg_mlp_param_grads_slab_rows(int64_t N);
int fg_mlp_param_grads(int64_t N, const fg_mlp_desc* desc, const float* enc, const float* acts, const float* g_pre,
                       const float* g_heads, const fg_mlp_grads* out, void* workspace, size_t workspace_bytes,
                       fg_stream_t stream);

/* ---- K10 backward in row chunks (ABI 14, minor 1): fg_mlp_bwd / fg_mlp_bwd_inputs and fg_mlp_param_grads as ONE call that
 * never holds g_pre [8, N, 256] whole.  The rows are cut into the slabs of fg_mlp_param_grads (fg_mlp_param_grads_slab_rows(N)
 * rows, a function of N alone, a multiple of 64); a chunk is chunk_slabs consecutive slabs, the last chunk may be shorter.
 * On the caller's stream, in row order:
 *   once       the chain's weight re-ordering launches (Tp; Tin too where g_enc is wanted)
 *   per chunk  the data-chain kernel of fg_mlp_bwd (of fg_mlp_bwd_inputs where g_enc is non-null) over the chunk's rows:
 *              g_heads, acts (layer stride N * 256) and g_enc at the rows themselves, P_l into a workspace array
 *              [8, chunk_rows, 256] at the row less the chunk's first; then the slab kernel of fg_mlp_param_grads over the
 *              chunk's slabs, P_l from that array, each slab's partial block at the slab's own index
 *   once       the reduction of fg_mlp_param_grads over all the slabs
 * so 1 (2 with g_enc) + 2 ceil(slabs / chunk_slabs) + 1 launches: a function of N, chunk_slabs and what is asked for.  Same
 * slabs, same chain inside a slab, same slab-order sum: every output of fg_mlp_grads, and g_enc, is bit for bit what
 * fg_mlp_bwd[_inputs] followed by fg_mlp_param_grads writes from the same inputs, for every chunk_slabs.  No atomics, nothing kept
 * between calls, no host synchronisation; asynchronous and capturable in a graph.
 *   chunk_slabs  0 = FG_MLP_TRAIN_BWD_CHUNK_SLABS; a positive value is taken as given, capped at the number of slabs (all
 *                the slabs = one chunk: what the two calls do); negative: FG_ERR_INVALID_ARG
 *   g_enc        [N, FG_MLP_ENC_WIDTH(aux_width)] or null (not formed)
 *   out          as for fg_mlp_param_grads: every entry nullable.  No trunk gradient asked for: the chunks still run where
 *                g_enc is wanted; nothing asked for and g_enc null: FG_OK, nothing is launched
 *   desc         as for fg_mlp_bwd: the chain reads its weight pointers; x / aux / out are not read
 *   fg_mlp_train_bwd_chunk_rows(N, chunk_slabs) = min(chunk_slabs, slabs) * slab rows: the rows of the workspace array
 * The workspace: 16-byte aligned, fg_mlp_train_bwd_workspace_bytes(N, chunk_slabs, want_g_enc) bytes =
 *   fg_mlp_train_workspace_bytes(N) (want_g_enc: fg_mlp_bwd_inputs_workspace_bytes(N)) rounded up to a multiple of
 *   FG_MLP_TRAIN_BWD_ALIGN = 4096 (the chunk array's rows then start on cache-line boundaries of an allocator's block: at
 *   the 64-byte offset of the bare size the call was 3 % slower) + 8 * chunk_rows * 256 * 4
 *   + fg_mlp_param_grads_workspace_bytes(N);  0 for N <= 0.  Next to acts (8 KB per row) the call needs nothing that grows
 * with N but the partial blocks (0.5 KB per row): at 1M rows 1.07 GB for the default chunk, against the 8.2 GB of g_pre.  (The
 * slab length is not monotone in N, so neither is this size in general: ask per call.)
 * FG_MLP_TRAIN_BWD_CHUNK_SLABS = 16: chosen among 16 / 21 / 32 / 42 by the median backward at 240 000 rows (profiles/mlp_chunked_bwd.md,
 * table (a), MI355X: 6.98 / 7.45 / 7.36 / 7.43 ms, p10 .. p90 of 16 apart from the others; the two calls 6.65 ms, one chunk 6.77 ms).
 * 16 slabs are 1024 tiles of the chain, two full rounds of its 512 workgroup places.  The call is slower than the two calls it
 * combines: 1.05 x at 33 000 and 240 000 rows, 1.03 x at 1 000 000; what it saves is the 8 KB per row of g_pre.
 * Error codes as the two calls: N == 0 does nothing; FG_ERR_INVALID_ARG: negative N or chunk_slabs, a null desc or out, wrong
 * size fields, a null weight pointer, aux_width / head rows out of range, a mode other than FG_MLP_PLAIN, null g_heads / acts
 * (always read) or enc (where weight[0] / weight[5] is asked for), a null or misaligned workspace; FG_ERR_WORKSPACE: a
 * workspace too small; FG_ERR_UNSUPPORTED: depth / width / multires other than 8 / 256 / 10. */
#define FG_MLP_TRAIN_BWD_CHUNK_SLABS 16
#define FG_MLP_TRAIN_BWD_ALIGN 4096 /* bytes: where the chunk array starts in the workspace */
int fg_abi_minor(void);
int64_t fg_mlp_train_bwd_chunk_rows(int64_t N, int32_t chunk_slabs);
size_t fg_mlp_train_bwd_workspace_bytes(int64_t N, int32_t chunk_slabs, int32_t want_g_enc);
int fg_mlp_train_bwd(int64_t N, const fg_mlp_desc* desc, const float* g_heads, const float* enc, const float* acts, float* g_enc,
                     const fg_mlp_grads* out, int32_t chunk_slabs, void* workspace, size_t workspace_bytes, fg_stream_t stream);

/* ---- K10 weight-gradient products in split bf16 (found BY NAME, see FG_ABI_MINOR): fg_mlp_param_grads and fg_mlp_train_bwd with
 * one more word, wgrad_precision, which governs the hidden and input products gW_l = P_l^T in_l and nothing else.
 * fg_mlp_desc::precision keeps its meaning: it governs the chain of fg_mlp_train_bwd_p and is ignored by fg_mlp_param_grads_p.
 * The two words are independent: all four combinations are legal.
 *   FG_MLP_FP32    fg_mlp_param_grads / fg_mlp_train_bwd themselves: the old functions ARE the new ones with this value, bit for
 *                  bit and launch for launch.
 *   FG_MLP_BF16X3  opt-in.  Same slabs (fg_mlp_param_grads_slab_rows(N)), same jobs, same partial blocks, same reduction in slab
 *                  order, same workspace; the 128 x 128 tile jobs run on v_mfma_f32_32x32x16_bf16.  The contract:
 *     split(v):  as for fg_mlp_desc::precision: hi = bf16(v) rounded to nearest even, lo = bf16(v - float(hi)).  Both operands,
 *                P_l and in_l, are split as they are read, once per value and tile job.
 *     chain   :  an output element (i, j) of one slab starts from 0 and walks the slab's rows in steps of 16, ascending.  Per
 *                step s it takes P_hi.in_hi, then P_hi.in_lo, then P_lo.in_hi, each the instruction's own sum over the rows
 *                k = 16 s + 8 h + j (lane half h, j = 0..7) of P[k][i] in[k][j], accumulated in fp32; P_lo.in_lo is dropped.
 *                Rows from the slab's end on are zeros and are never read; the pad columns k >= in_ch of enc are zeros.  At most
 *                4096 rows = 256 steps to a chain; the slabs' partials are added in slab order by the unchanged reduction.
 *     biases  :  gb_l stays an fp32 sum of the unsplit P_l, taken from the fetched values before the split.  Order, per slab
 *                and column: the rows go in blocks of 64; row group r = 0..7 of a block is its rows 8 r .. 8 r + 7; a group's 8
 *                values are added in row order and that sum to the running sum of its r; after the last block the 8 running
 *                sums are added in the order r = 0..7.  (Not the fp32 mode's order: the sums may differ in the last bits.)
 *     heads   :  head weight and bias gradients are the fp32 mode's, bit for bit: the same jobs, the same code
 *                (v_mfma_f32_16x16x4_f32; 1/112 of the FLOP).
 *     No atomics: two runs are bit for bit equal; zero cotangents give exact zeros.  Against float64 the trunk weight gradients
 *     stay within 1e-4 of each array's largest magnitude (emulated and measured: about 5e-6 .. 2e-5; with the third term left
 *     out some 2e-3).  A single 1.0 in P_l at (r, i) makes row i of gW_l exactly hi(in_l[r]) + lo(in_l[r]).
 * Any other wgrad_precision: FG_ERR_INVALID_ARG, before anything else about the call is looked at (N == 0 with a good value
 * stays FG_OK).  Workspace queries, sizes, alignment rules and every other error code are those of the old calls.
 * fg_mlp_train_bwd_p stays bit for bit the chain call followed by fg_mlp_param_grads_p, for every chunk_slabs and both values
 * of either word.  fg_mlp_wgrad_precision_supported(precision) = 1 for FG_MLP_FP32 and FG_MLP_BF16X3, else 0.
 * Measured (profiles/mlp_wgrad_split.md). */
int fg_mlp_wgrad_precision_supported(int32_t precision);
int fg_mlp_param_grads_p(int64_t N, const fg_mlp_desc* desc, const float* enc, const float* acts, const float* g_pre,
                         const float* g_heads, const fg_mlp_grads* out, int32_t wgrad_precision, void* workspace,
                         size_t workspace_bytes, fg_stream_t stream);
int fg_mlp_train_bwd_p(int64_t N, const fg_mlp_desc* desc, const float* g_heads, const float* enc, const float* acts, float* g_enc,
                       const fg_mlp_grads* out, int32_t chunk_slabs, int32_t wgrad_precision, void* workspace,
                       size_t workspace_bytes, fg_stream_t stream);

/* ---- BG bilateral-grid colour correction of a rendered image (found BY NAME, see FG_ABI_MINOR): the slice of ONE camera's
 * grid of 3 x 4 affine colour transforms at (x, y, luma) and its application, forward and backward (csrc/bilagrid.hip;
 * freegaussian_amd/bilagrid.py apply_to_render is the torch statement: grid_sample with mode = "bilinear", align_corners =
 * True, padding_mode = "border").  All fp32.
 *   grid[12, GL, GY, GX]  one camera's block (the host passes the address of grids[cam_idx]);  rgb, out, v_out, v_rgb [H, W, 3].
 *   Pixel (py, px):  fx = px / (W-1) (GX-1),  fy = py / (H-1) (GY-1),  fz = luma (GL-1),  luma = 0.299f r + 0.587f g + 0.114f b,
 *   each clamped to [0, n-1];  i0 = min(floor(f), n-1), i1 = min(i0 + 1, n-1), t = f - i0;  A[12] = the trilinear mix of the
 *   eight corners, read as a 3 x 4 matrix;  out = A[:, :3] rgb + A[:, 3].  (The kernels put a pixel that sits on the last node
 *   into the last cell with t = 1: the same weights on the same nodes.)
 *   fg_bilagrid_slice_bwd recomputes A from grid and rgb (the forward saves nothing) and forms
 *     v_grid[k, z, y, x] = sum over the pixels of  w_z w_y w_x  v_out[k / 4]  (r, g, b, 1)[k % 4]      every element written
 *     v_rgb = A[:, :3]^T v_out + (0.299f, 0.587f, 0.114f) (GL-1) sum_k (dA/dz)[k] v_out[k / 4] (r, g, b, 1)[k % 4]   overwritten
 *   with dA/dz the (x, y)-bilinear mix of grid[z1] - grid[z0]; the term through fz is exactly zero where the unclamped
 *   fz <= 0 or fz >= GL-1 (torch's border rule: an exactly black and an exactly white pixel get none); x and y carry no
 *   gradient.  Either of v_rgb / v_grid may be null: that gradient is not formed (both null: nothing is launched).
 *   v_grid is a gather without atomics: the pixels of a grid cell, in chunks of FG_BILAGRID_CHUNK_PIXELS, are summed per level
 *   and corner into partial blocks in the workspace, and a second launch adds each node's (up to four) cells and their chunks
 *   in a fixed order: two runs are bit for bit equal, and a node whose four cells hold no pixel is exactly 0.
 *   A cell of cw x ch pixels takes ceil(cw ch / FG_BILAGRID_CHUNK_PIXELS) chunks; fg_bilagrid_bwd_workspace_bytes =
 *   (chunks of the largest cell) * GL * 48 * (GX-1) * (GY-1) * 4, with the cell of index c along an axis of n nodes and S
 *   pixels holding the pixels ceil(c (S-1) / (n-1)) .. ceil((c+1) (S-1) / (n-1)) - 1 (the last cell: up to S - 1).
 *   Supported: 2 <= GX, GY <= 64, 2 <= GL <= 16 (fg_bilagrid_supported = 1, else 0), 2 <= H, W <= 16384.
 *   The workspace query is pure and returns 0 for anything unsupported.  workspace: 16-byte aligned, needed for v_grid only.
 *   FG_ERR_INVALID_ARG: H or W < 2, a null grid / rgb / out / v_out, an output that overlaps an input, another output or the
 *   workspace, a null or misaligned workspace with v_grid asked for;  FG_ERR_UNSUPPORTED: a grid shape or image size outside the
 *   range above;  FG_ERR_WORKSPACE: workspace_bytes below the query.  All before any launch.  Asynchronous, capturable in a
 *   graph, no state, no environment.  Measured (profiles/bilagrid_fused.md). */
#define FG_BILAGRID_CHUNK_PIXELS 1024
int fg_bilagrid_supported(int GX, int GY, int GL);
size_t fg_bilagrid_bwd_workspace_bytes(int H, int W, int GX, int GY, int GL);
int fg_bilagrid_slice_fwd(int H, int W, int GX, int GY, int GL, const float* grid, const float* rgb, float* out,
                          fg_stream_t stream);
int fg_bilagrid_slice_bwd(int H, int W, int GX, int GY, int GL, const float* grid, const float* rgb, const float* v_out,
                          float* v_rgb, float* v_grid, void* workspace, size_t workspace_bytes, fg_stream_t stream);

/* ---- CC colour correction of the metrics (found BY NAME, see FG_ABI_MINOR): `img` warped to the colours of `ref` by a
 * per-channel quadratic colour transform, fitted by least squares on the pixels unclipped in both and re-fitted num_iters
 * times (csrc/color_correct.hip; freegaussian_amd/bilagrid.py color_correct is the torch statement), with no host round trip.
 *   img, ref, out [P, 3] float32;  warps [num_iters, 10, 3] float32 and rank [num_iters, 3] int32: either may be null.
 *   lo = (float)eps,  hi = (float)(1.0 - eps),  unclipped(z) = z >= lo && z <= hi  (fp32 comparisons: what torch does with a
 *   float32 tensor and a Python scalar; tests/test_color_correct_host.py decides it against the torch path).
 *   x_0 = img,  mask0[p, c] = unclipped(img[p, c]).  Iteration k = 0 .. num_iters - 1:
 *     a(x) = [x0 x0, x0 x1, x0 x2, x1 x1, x1 x2, x2 x2, x0, x1, x2, 1]: the quadratic terms are fp32 products, widened to
 *            float64 afterwards (torch forms the feature matrix in fp32 before .double());
 *     per channel c, over the pixels with  m = mask0[p, c] && unclipped(x_k[p, c]) && unclipped(ref[p, c]):
 *            G_c = sum a a^T,  r_c = sum a ref[p, c],  products and sums in float64;
 *     w_c  = D^-1/2 pinv(D^-1/2 G_c D^-1/2) D^-1/2 r_c,  D = diag(G_c): the pseudo-inverse through the eigen-decomposition
 *            (cyclic Jacobi, float64) of the unit-diagonal Gram, eigenvalues at or below FG_COLOR_CORRECT_RCOND times the
 *            largest dropped.  A zero diagonal (a zero feature column) gives w_i = 0; G_c = 0 (no unmasked pixel) gives
 *            w_c = 0.  w_c is stored as float32 -> warps[k, :, c];  rank[k, c] = the eigenvalues kept, -1 where a weight is
 *            not finite (the device cannot assert as the torch path does: out then carries the NaN).
 *     x_{k+1} = clamp(a(x_k) . [w_0 w_1 w_2], 0, 1) for EVERY pixel, fp32 accumulation in feature order.
 *   out = x_{num_iters}.
 *   Where G_c has full rank, w_c is the least-squares fit.  Where it has not, w_c is a least-squares fit -- the one of
 *   least norm in the column-scaled variables D^1/2 w -- with the fitted values every least-squares solution has on the
 *   unmasked pixels.  torch.linalg.lstsq's default driver on the device-to-host path of the torch statement (gelsy) returns
 *   something that is NOT a least-squares solution where the feature matrix has exactly zero columns (an image channel that
 *   is 0 everywhere): the two paths differ there, and this one is the fit.
 *   No atomics: a workgroup sums a chunk of pixels on the float64 matrix instruction and writes one partial block; the
 *   solve launch adds the blocks in a fixed order.  Two runs are bit for bit equal.  No intermediate image: pass k
 *   recomputes x_k from img through the k warps already solved, so the call makes num_iters + 1 passes over the image and
 *   reads only img and ref.
 *   A chunk is FG_COLOR_CORRECT_CHUNK_PIXELS pixels while that makes at most FG_COLOR_CORRECT_MAX_CHUNKS chunks; beyond, it is
 *   ceil(P / FG_COLOR_CORRECT_MAX_CHUNKS) rounded up to a multiple of 256.  fg_color_correct_workspace_bytes = 2048 +
 *   min(ceil(P / FG_COLOR_CORRECT_CHUNK_PIXELS), FG_COLOR_CORRECT_MAX_CHUNKS) * 3 * 128 * 8: pure, monotone in P, and 0 for
 *   anything unsupported.  workspace: 16-byte aligned.
 *   Supported: 1 <= P <= 16384 * 16384, 1 <= num_iters <= FG_COLOR_CORRECT_MAX_ITERS, 0 < eps < 0.5.
 *   FG_ERR_INVALID_ARG: a null img / ref / out, an output (out, warps, rank) that overlaps an input, another output or the
 *   workspace, a workspace that overlaps an input, a null or misaligned workspace;  FG_ERR_UNSUPPORTED: P, num_iters or eps
 *   outside the range above;  FG_ERR_WORKSPACE: workspace_bytes below the query.  All before any launch.  Byte offsets
 *   are 64-bit.  Asynchronous (no host read anywhere), capturable in a graph, no state, no environment.
 *   Measured (profiles/color_correct_fused.md). */
#define FG_COLOR_CORRECT_MAX_ITERS 8
#define FG_COLOR_CORRECT_CHUNK_PIXELS 4096
#define FG_COLOR_CORRECT_MAX_CHUNKS 2048
#define FG_COLOR_CORRECT_RCOND 1e-12
size_t fg_color_correct_workspace_bytes(int64_t P, int num_iters);
int fg_color_correct(int64_t P, const float* img, const float* ref, int num_iters, double eps, float* out, float* warps,
                     int32_t* rank, void* workspace, size_t workspace_bytes, fg_stream_t stream);

/* ---- SE the SE(3) exponential of the deformation net's (w, v) heads applied to points (found BY NAME, see FG_ABI_MINOR),
 * forward and backward, one streaming launch each (csrc/se3_apply.hip, csrc/se3_math.h; freegaussian_amd/deform.py _se3 +
 * utils.exp_se3 + utils.transform_points are the torch statement).  All fp32.  Per row r < N:
 *   theta = |w_r|,  ws = w_r / theta + 1e-5,  vs = v_r / theta + 1e-5  (the offsets are constants of the function),
 *   W = hat(ws),  R = I + sin(theta) W + (1 - cos theta) W^2,  G = theta I + (1 - cos theta) W + (theta - sin theta) W^2,
 *   out_r = R pts_r + G vs     in the arithmetic of utils.exp_se3; the homogeneous coordinate is exactly 1: no divide.
 *   w, v    rows of 3 floats, w_stride / v_stride floats apart (>= 3): two contiguous [N,3] arrays (stride 3), or columns 0..2
 *           and 3..5 of the fused MLP's [N,13] head block read in place (stride 13).  They may overlap each other.
 *   pts, out, g_out, g_pts   contiguous [N,3].
 *   g_w, g_v   rows of 3 floats, gw_stride / gv_stride floats apart (>= 3; looked at only where the pointer is not null).
 * fg_se3_apply_fwd writes out and nothing else.  fg_se3_apply_bwd recomputes everything from w, v, pts (the forward saves
 * nothing) and writes the exact derivative of the function above:  g_w, g_v, g_pts = d(sum g_out . out) / d(w, v, pts),
 * evaluated in fp32 in forms that do not cancel at small theta (profiles/se3_apply_parity.md).  Any of g_w / g_v / g_pts may
 * be null: that gradient is neither computed nor written (all null: nothing is launched).
 *   Rows are independent: a row with w = 0 gives non-finite values in its own outputs, as the torch ops do, and touches no
 *   other row.  No atomics, no workspace: two runs are bit for bit equal.
 *   Aliasing: an output must not overlap an input or another output, by the span from its first to its last float -- except
 *   that g_w and g_v may be columns of one row block: equal strides, at least 3 floats and at most stride - 3 floats apart.
 *   FG_ERR_INVALID_ARG: N < 0, a null w / v / pts / out / g_out, a stride below 3, an output that overlaps as above;
 *   FG_ERR_UNSUPPORTED: N > FG_SE3_MAX_ROWS or a stride above FG_SE3_MAX_STRIDE.  N == 0 is FG_OK with no launch (after the
 *   null, sign and stride checks).  All before any launch.  Row and byte offsets are 64-bit.  Asynchronous, capturable in a
 *   graph, no state, no environment.  Measured (profiles/se3_apply_fused.md). */
#define FG_SE3_MAX_ROWS ((int64_t)1 << 38)
#define FG_SE3_MAX_STRIDE ((int64_t)1 << 16)
int fg_se3_apply_fwd(int64_t N, const float* w, int64_t w_stride, const float* v, int64_t v_stride, const float* pts, float* out,
                     fg_stream_t stream);
int fg_se3_apply_bwd(int64_t N, const float* w, int64_t w_stride, const float* v, int64_t v_stride, const float* pts,
                     const float* g_out, float* g_w, int64_t gw_stride, float* g_v, int64_t gv_stride, float* g_pts,
                     fg_stream_t stream);

/* ---- CT the stage-2 control stage around the control MLP (found BY NAME, see FG_ABI_MINOR; csrc/control.hip;
 * freegaussian_amd/model.py FreeGaussianControlModel holds the torch statement: boolean indexing, a loop of masked means, a
 * [n,M] x [M,3] product and three zeros + index_put).  The calls work on a PLAN the host builds once per [N,M] bool mask
 * (1 <= M <= FG_CONTROL_MAX_ATTRS; ops.control_plan), n = the rows with any attribute:
 *   sel_index  int32 [n]   those rows, ascending              rank    int32 [N]  a row's position in sel_index, or -1
 *   bits       uint32 [n]  bit m set: row sel_index[i] has attribute m           counts  int32 [M], HOST: rows per attribute
 * All floating data fp32.  Strides are in floats and at least the row's width; rows of d_xyz / d_rot / d_scale (and of the
 * g_d_* outputs) may be three contiguous arrays or columns 0..2, 3..6, 7..9 of the fused MLP's [n,10] head block, in place.
 *   fg_control_supported(M)           1 where 1 <= M <= FG_CONTROL_MAX_ATTRS, else 0.  Host only.
 *   fg_control_workspace_bytes(n, M)  bytes of fg_control_attr_mean's workspace (float64 partial sums, one set per
 *                                     FG_CONTROL_BLOCK_ROWS rows); 0 for an M or an n (1 .. FG_CONTROL_MAX_ROWS) outside the
 *                                     range.  Host only.
 *   fg_control_attr_mean   d_avg[m] = (sum over the rows i with bit m of (a_i - b_i)) / counts[m],  d_avg [M,3].  The
 *       difference is formed in fp32 (what the torch statement subtracts), the sum in float64, and the quotient is rounded to
 *       fp32 once:  |d_avg - exact mean of the fp32 differences| <= 2^-24 |mean| + n 2^-53 mean|a_i - b_i|.  Two launches:
 *       partial sums per workgroup over a row partition that depends on n alone, then one pass that adds them in block
 *       order.  No atomics: two runs are bit for bit equal.  a, b: rows of 3 floats.  workspace: 8-byte aligned.  The second
 *       pass is one workgroup in which a lane adds one output's partials one after the other: n / FG_CONTROL_BLOCK_ROWS
 *       dependent float64 additions (about 1000 at a million rows, 16 384 at FG_CONTROL_MAX_ROWS, which is set with that
 *       in mind).
 *   fg_control_value_rows  value[i] = (sum of d_avg[m] over the set bits of bits[i], ascending m, in fp32) / popcount(bits[i]),
 *       value [n,3] contiguous.  One launch.  (A row without a bit is 0 / 0, as in the torch statement; a plan has none.)
 *   fg_control_scatter_fwd out_means [N,3] = means + (rank >= 0 ? d_xyz[rank] : 0),  d_rotation [N,4] (16-byte aligned) and
 *       d_scaling [N,3] = the row of d_rot / d_scale, or zeros.  One launch; every element of the three outputs is written.
 *   fg_control_scatter_bwd g_d_xyz[i] = g_means[sel_index[i]], g_d_rot[i] = g_rotation[...], g_d_scale[i] = g_scaling[...]: a
 *       gather, one launch.  A null upstream gradient (g_means [N,3], g_rotation [N,4], g_scaling [N,3]) counts as zeros; a
 *       null output is not wanted and not written (all null: nothing is launched).  The gradient of means is g_means itself.
 *   Bits at or above M are ignored; a rank or a sel_index entry outside its range reads nothing (zeros).
 *   Aliasing: an output must not overlap an input or the workspace, by the span from its first to its last float; the g_d_*
 *   outputs may be columns of one row block (equal strides, column ranges that do not meet).
 *   FG_ERR_INVALID_ARG: a null pointer other than those named nullable, a negative count, n > N, attr_mean with n < 1 or a
 *   counts[m] outside 1 .. n (an attribute without a row has no mean: an error, not a NaN), a stride below the row's width, a
 *   misaligned workspace or d_rotation, an overlap as above;  FG_ERR_UNSUPPORTED: M above FG_CONTROL_MAX_ATTRS, n or N above
 *   FG_CONTROL_MAX_ROWS, a stride above FG_CONTROL_MAX_STRIDE;  FG_ERR_WORKSPACE: workspace_bytes below the query.  All
 *   before any launch.  n == 0 (value_rows, scatter_bwd) and N == 0 (scatter_fwd) are FG_OK with no launch.  Row and byte
 *   offsets are 64-bit.  Asynchronous (no host read anywhere), capturable in a graph, no state, no environment.
 *   Measured (profiles/control_fused.md). */
#define FG_CONTROL_MAX_ATTRS 32
#define FG_CONTROL_BLOCK_ROWS 1024
#define FG_CONTROL_MAX_ROWS ((int64_t)1 << 24)
#define FG_CONTROL_MAX_STRIDE ((int64_t)1 << 16)
int fg_control_supported(int M);
size_t fg_control_workspace_bytes(int64_t n, int M);
int fg_control_attr_mean(int64_t n, int M, const float* a, int64_t a_stride, const float* b, int64_t b_stride, const uint32_t* bits,
                         const int32_t* counts, void* workspace, size_t workspace_bytes, float* d_avg, fg_stream_t stream);
int fg_control_value_rows(int64_t n, int M, const uint32_t* bits, const float* d_avg, float* value, fg_stream_t stream);
int fg_control_scatter_fwd(int64_t N, int64_t n, const int32_t* rank, const float* means, const float* d_xyz, int64_t xyz_stride,
                           const float* d_rot, int64_t rot_stride, const float* d_scale, int64_t scale_stride, float* out_means,
                           float* d_rotation, float* d_scaling, fg_stream_t stream);
int fg_control_scatter_bwd(int64_t n, int64_t N, const int32_t* sel_index, const float* g_means, const float* g_rotation,
                           const float* g_scaling, float* g_d_xyz, int64_t xyz_stride, float* g_d_rot, int64_t rot_stride,
                           float* g_d_scale, int64_t scale_stride, fg_stream_t stream);

/* ---- TL the training loss and the PSNR's squared error straight from the RAW batch image (found BY NAME, see FG_ABI_MINOR;
 * csrc/target_loss.hip): the target of fg_l1_ssim_fwd -- the batch image as floats, box-downscaled, composited over the
 * step's background, masked (freegaussian_amd/model.py get_gt_img, composite_with_background and the mask lines of
 * get_loss_dict are the torch statement) -- is formed per pixel inside the loss kernels.  No target tensor is written.
 *
 *   The source is [height, width, channels] contiguous, uint8 or float32, channels 3 or 4; the output (= pred) is
 *   [H, W, 3] float32 contiguous with H = height / downscale, W = width / downscale (integer division).
 *   Per output pixel (y, x), channel c, d = downscale:
 *     s_k   source channel k as a real number: a uint8 v is v / 255, a float32 is taken as it is
 *     t_k   = mean of s_k over the d x d source block at (y d, x d), for every source channel, alpha included; source rows
 *             and columns at or beyond H d, W d are never read (as a strided pooling ignores them); the sum is exact (uint8: an
 *             integer; float32: in double) and the mean rounded once, so a flat block gives its own value back
 *     gt_c  = t_c with 3 channels;  t_3 t_c + (1 - t_3) background[c] with 4: the composite comes AFTER the downscale, on
 *             values that are not premultiplied.  background: 3 device floats
 *     m     = the same box mean of the mask ([height, width] bytes -- a bool's 0 / 1, a uint8 by its value -- or float32);
 *             1 without a mask
 *   fg_target_loss_fwd:  out[0] = mean |gt m - pred m|, out[1] = mean SSIM(pred m, gt m) with the window, borders and
 *     constants of fg_l1_ssim_fwd, out[2] = mean (pred - gt)^2 of the UNMASKED images (the PSNR's).  maps[3, 3, H-10, W-10]
 *     are fg_l1_ssim_fwd's; a null maps keeps none (a forward whose pred needs no gradient).  The per-workgroup partial sums
 *     (workspace[fg_target_loss_workspace_floats(target)] floats, 16-byte aligned) are reduced in a fixed order by a second
 *     launch: no atomics, two runs are bit for bit equal.
 *   fg_target_loss_bwd:  v_out[2] (device) = dL/d out[0], dL/d out[1]  ->  v_pred[H, W, 3] = m (v_out[0] L1 term + v_out[1]
 *     SSIM term), overwritten; target pixel and mask are recomputed from the source.  Exactly 0 where m = 0.  out[2] carries no
 *     gradient; the source, the mask and the background get none.
 *   Supported (fg_target_loss_supported = 1, else 0; the query gives 0 floats): downscale 1, 2, 4 or 8; channels 3 or 4;
 *     src_dtype and -- with a mask -- mask_dtype FG_TARGET_U8 or FG_TARGET_F32; height, width <= 32768; H, W >= 11.
 *   FG_ERR_INVALID_ARG: a null descriptor or one whose size is not sizeof(fg_target_desc), height or width <= 0, a null src /
 *   pred / workspace / out (fwd) or pred / maps / v_out / v_pred (bwd), a null background with 4 channels, a source that is not
 *   aligned to its pixel (4-channel: 4 bytes uint8, 16 bytes float32; 3-channel float32: 4 bytes), a misaligned float mask,
 *   background or workspace, an output (maps, workspace, out; v_pred) that overlaps an input or another output;
 *   FG_ERR_UNSUPPORTED: anything outside the supported range;  FG_ERR_WORKSPACE: workspace_floats below the query.  All before
 *   any launch.  Asynchronous, capturable in a graph, no state, no environment.  Measured (profiles/target_loss_fused.md). */
#define FG_TARGET_U8 0
#define FG_TARGET_F32 1
typedef struct fg_target_desc {
  int32_t size;       /* sizeof(fg_target_desc) */
  int32_t src_dtype;  /* FG_TARGET_U8 or FG_TARGET_F32 */
  int32_t height, width, channels; /* of the source */
  int32_t downscale;
  int32_t mask_dtype; /* FG_TARGET_U8 (bool too) or FG_TARGET_F32; not looked at with a null mask */
  int32_t reserved;   /* 0 */
  const void* src;
  const void* mask;        /* or null */
  const float* background; /* or null (3 channels only) */
} fg_target_desc;
int fg_target_loss_supported(const fg_target_desc* target);
size_t fg_target_loss_workspace_floats(const fg_target_desc* target);
int fg_target_loss_fwd(const fg_target_desc* target, const float* pred, float* maps, float* workspace, size_t workspace_floats,
                       float* out, fg_stream_t stream);
int fg_target_loss_bwd(const fg_target_desc* target, const float* pred, const float* maps, const float* v_out, float* v_pred,
                       fg_stream_t stream);

/* ---- FD the 2-D displacement of the projected Gaussian centres between frame 0 and the current frame (found BY NAME, see
 * FG_ABI_MINOR; csrc/flow_disp.hip), forward and backward, one streaming launch each: the per-Gaussian term mu_t - mu_0 of the
 * composited Gaussian flow that the raster pass carries as two extra channels.  All fp32.  Per row r < N:
 *   p_t = R_t m_t + tau_t,  p_0 = R_0 m_0 + tau_0   (R, tau: the upper 3 x 4 of a row-major [4,4] world-to-camera matrix)
 *   VALIDITY RULE: the row is valid iff z_t > near and z_0 > near and both projected centres (f_x x / z + c_x, f_y y / z + c_y)
 *     lie in [-margin, width + margin] x [-margin, height + margin]; margin = inf switches the rectangle test off (a centre
 *     that is not a number is outside).  An invalid row writes exact zeros and gets exact zero gradients.
 *   CANCELLATION-FREE FORM: with Delta = p_t - p_0,
 *     disp_x = f_x (Delta_x z_0 - x_0 Delta_z) / (z_t z_0),   disp_y = f_y (Delta_y z_0 - y_0 Delta_z) / (z_t z_0)
 *     -- f (x_t / z_t - x_0 / z_0) without the two quotients, whose difference at small motion keeps only their last bits.
 *     c_x, c_y never enter the value.  viewmat_0 null = one camera for both frames: Delta = R_t (m_t - m_0) and
 *     p_t = p_0 + Delta, so the translation never enters Delta.
 *   means_t, means_0   rows of 3 floats, mt_stride / m0_stride floats apart (>= 3): contiguous [N,3] or columns of a wider
 *     row block, read in place; they may overlap each other.  viewmat_t, viewmat_0 (or null), K [3,3]: device arrays, constants.
 *   disp, g_disp [N,2] contiguous, 8-byte aligned; g_means_t, g_means_0 [N,3] contiguous.
 * fg_flow_disp_bwd recomputes everything from the inputs (the forward saves nothing) and writes the closed form
 *   g_means_t = R_t^T (a, b, -(a x_t + b y_t) / z_t),  a = g_x f_x / z_t, b = g_y f_y / z_t;   g_means_0 likewise with R_0, p_0
 *   and the opposite sign.  Either may be null: that gradient is neither computed nor written (both null: no launch).
 *   DETERMINISM: rows are independent, no atomics, no workspace: two runs are bit for bit equal, a gradient asked for alone
 *   has the bits of the joint call, permuted rows give permuted bits.
 *   Aliasing: an output must not overlap an input or another output (csrc/arg_check.h).
 *   FG_ERR_INVALID_ARG: N < 0, a null means_t / means_0 / viewmat_t / K / disp / g_disp, a stride below 3, width or height
 *   <= 0, near negative, infinite or not a number, margin negative or not a number, a misaligned disp / g_disp, an output that
 *   overlaps;  FG_ERR_UNSUPPORTED: N > FG_FLOW_DISP_MAX_ROWS or a stride above FG_FLOW_DISP_MAX_STRIDE.  N == 0 is FG_OK with no
 *   launch (after the null, sign and stride checks).  All before any launch.  Asynchronous, capturable, no state, no environment.
 *   Measured (profiles/flow_supervision.md). */
#define FG_FLOW_DISP_MAX_ROWS ((int64_t)1 << 38)
#define FG_FLOW_DISP_MAX_STRIDE ((int64_t)1 << 16)
int fg_flow_disp_fwd(int64_t N, const float* means_t, int64_t mt_stride, const float* means_0, int64_t m0_stride,
                     const float* viewmat_t, const float* viewmat_0, const float* K, int width, int height, float near,
                     float margin, float* disp, fg_stream_t stream);
int fg_flow_disp_bwd(int64_t N, const float* means_t, int64_t mt_stride, const float* means_0, int64_t m0_stride,
                     const float* viewmat_t, const float* viewmat_0, const float* K, int width, int height, float near,
                     float margin, const float* g_disp, float* g_means_t, float* g_means_0, fg_stream_t stream);

/* ---- FL the masked L1 between the rendered flow channels and the batch's flow array at FULL resolution (found BY NAME, see
 * FG_ABI_MINOR; csrc/flow_loss.hip).  No target tensor is written.
 *   pred   [H, W, 2] float32 read in place: channel stride 1, pixel_stride floats between two pixels (>= 2), row_stride floats
 *          between two rows (>= (W - 1) pixel_stride + 2) -- the last two channels of a [1,H,W,C] render.
 *   flows  [H0, W0, 2] float32 contiguous, 8-byte aligned, in full-resolution pixels.  H = H0 / d, W = W0 / d (integer division),
 *          d = downscale in 1, 2, 4, 8; the source rows and columns at or beyond H d, W d are never read.
 *   mask   null, or [H0, W0] bytes (FG_TARGET_U8: a bool's 0 / 1, a uint8 by its value) or float32 (FG_TARGET_F32).
 *   TARGET AND WEIGHT, per render pixel:
 *     t = the mean of the d x d source block at (y d, x d) DIVIDED BY d (a flow in full-resolution pixels shrinks with the image);
 *     w = 0 if any of the block's 2 d^2 source values is not finite, else the same box mean of the mask (1 without a mask).
 *     Block sums are exact (double) and rounded once.
 *   fg_flow_l1_fwd:  out[0] = sum w (|pred_x - t_x| + |pred_y - t_y|) / (2 max(sum w, FG_FLOW_L1_TINY)); sum w = 0 gives 0.  A
 *     pixel with w = 0 is not read from pred.
 *   fg_flow_l1_bwd:  g_pred[H, W, 2] (contiguous, 8-byte aligned, overwritten) = v_out[0] w sign(pred - t) / (2 max(sum w, tiny)),
 *     sign(0) = 0; exactly 0 where w = 0, so sum w = 0 gives a zero gradient, never NaN.  flows and mask get none.
 *   DETERMINISM: per-pixel terms, per-workgroup partial sums and their fixed-order total are doubles, rounded once; no atomics;
 *     two runs are bit for bit equal.  The totals stay in the first 16 bytes of the workspace
 *     (fg_flow_l1_workspace_bytes(H0, W0, d) bytes, 16-byte aligned; 0 = unsupported), which the backward reads: hand it the
 *     forward's workspace unchanged.  Nothing is read back by the host.
 *   FG_ERR_INVALID_ARG: H0 or W0 <= 0, H != H0 / d or W != W0 / d, a null or misaligned pred / flows / workspace / out / v_out /
 *   g_pred, a float mask that is misaligned, a pixel or row stride below the above, an output (workspace, out; g_pred) that
 *   overlaps an input or another output;  FG_ERR_UNSUPPORTED: another d, a side above 32768 or below d, a mask dtype that is
 *   neither, a pixel stride above FG_FLOW_L1_MAX_STRIDE;  FG_ERR_WORKSPACE: workspace_bytes below the query.  All before any
 *   launch.  Asynchronous, capturable, no state, no environment.  Measured (profiles/flow_supervision.md). */
#define FG_FLOW_L1_TINY 1e-30
#define FG_FLOW_L1_MAX_STRIDE ((int64_t)1 << 16)
size_t fg_flow_l1_workspace_bytes(int H0, int W0, int downscale);
int fg_flow_l1_fwd(int H, int W, const float* pred, int64_t pixel_stride, int64_t row_stride, int H0, int W0, int downscale,
                   const float* flows, const void* mask, int mask_dtype, void* workspace, size_t workspace_bytes, float* out,
                   fg_stream_t stream);
int fg_flow_l1_bwd(int H, int W, const float* pred, int64_t pixel_stride, int64_t row_stride, int H0, int W0, int downscale,
                   const float* flows, const void* mask, int mask_dtype, const void* workspace, const float* v_out, float* g_pred,
                   fg_stream_t stream);

/* ---- DB exact DBSCAN over xyz[n,3] fp32 points (found BY NAME, see FG_ABI_MINOR; csrc/dbscan.hip): the clustering of the
 * dynamic Gaussians into the columns of a stage-2 mask (project page, "Dynamic Gaussian clustering and tracking"; the reference
 * has the step only as commented-out scikit-learn lines, preprocess/knn_gaussian.py:139-147).
 *   THE DEFINITION (tests/dbscan_restatement.py states it on the CPU; everything else follows it):
 *     pair distance in fp32 without contraction, as fg_knn: dx = x_i - x_j (y, z alike), d2 = (dx dx + dy dy) + dz dz;
 *     eps2 = eps * eps in fp32;  j is a NEIGHBOUR of i iff d2 <= eps2.  The relation is symmetric bit for bit, a finite row
 *     neighbours itself, a row with a non-finite coordinate neighbours nobody (not itself either) and is noise.
 *     core(i): at least min_samples neighbours, the row itself counted.
 *     CLUSTERS: the connected components of the core rows under the neighbour relation, numbered 0..K-1 by ascending lowest
 *     core row.  A non-core row with at least one core neighbour is a BORDER row and takes the lowest-numbered cluster among
 *     its core neighbours.  Every other row is -1.
 *     This is sklearn.cluster.DBSCAN(eps, min_samples).fit(x).labels_ wherever no pair distance sits at the rounding edge of
 *     eps.  The labels depend on the predicate alone: nothing about the cell grid enters them.
 *   labels_out int32[n], core_out uint8[n] (1 = core), counts_out int32[2] = {K, status}, all device memory, written in the
 *     caller's row order.  status 0 = in order; 1 = a root walk of the union pass exceeded its bound of n + 1 steps (a defect:
 *     the labels are then not to be used).  The pass is lock-free and every loop in it is bounded: such a defect ends as this
 *     word, never as a hang.
 *   DETERMINISM: the partition is unique and the numbering is by row, so two runs are equal bit for bit, whatever order the
 *     atomics of the union pass land in.
 *   Limits: 1 <= n <= FG_DBSCAN_MAX_ROWS, eps > 0 and finite, 1 <= min_samples <= FG_DBSCAN_MAX_MIN_SAMPLES, no null pointer:
 *     else FG_ERR_INVALID_ARG, nothing is clamped.  FG_ERR_UNSUPPORTED: eps outside [FG_DBSCAN_MIN_EPS, FG_DBSCAN_MAX_EPS]
 *     (outside it eps2 is no normal fp32 number).  FG_ERR_WORKSPACE: workspace_bytes below fg_dbscan_workspace_bytes(n), which
 *     is 0 for an n outside the limits.  All before any launch.
 *   NOT capturable in a graph: like fg_knn the call reads a few KB of sampled coordinates back (one stream synchronisation)
 *     to size its cell grid.  The caller reads counts_out back to learn K.  Cost: profiles/dbscan.md. */
#define FG_DBSCAN_MAX_ROWS ((int64_t)1 << 24)
#define FG_DBSCAN_MAX_MIN_SAMPLES 65535
#define FG_DBSCAN_MIN_EPS 1e-18f
#define FG_DBSCAN_MAX_EPS 1e18f
size_t fg_dbscan_workspace_bytes(int64_t n);
int fg_dbscan(int64_t n, const float* xyz, float eps, int min_samples, int32_t* labels_out, uint8_t* core_out,
              int32_t* counts_out, void* workspace, size_t workspace_bytes, fg_stream_t stream);

/* ---- OF dense optical flow from two frames (found BY NAME, see FG_ABI_MINOR; csrc/optflow.hip): the flow maps that the flow
 * loss (FL) and the annotation-free stage-2 masks consume.  The reference makes them with a learned network (mmflow's GMA,
 * preprocess/epipolar_flow.py:367-372); this is a CLASSICAL, weight-free, deterministic estimator: pyramidal, patch-based,
 * inverse-compositional Lucas-Kanade with a forward-backward check.  Its quality against a learned estimator on real footage
 * has not been measured.
 *   THE DEFINITION (tests/optical_flow_restatement.py states it on the CPU, in float64 and in fp32, operation by operation):
 *     images    a, b: [H,W] float32, or [H,W,3] float32 or uint8 (dtype FG_TARGET_F32 / FG_TARGET_U8), device memory, dense.
 *               grey = 0.299 R + 0.587 G + 0.114 B, a uint8 value divided by 255 first.
 *     convention flow[y,x] = u with a(x) ~ b(x + u), in pixels of the full-resolution grid of a.
 *     pyramid   level 0 = grey; level l+1 = level l under the separable 5-tap binomial [1 4 6 4 1]/16, coordinates clamped to
 *               the image, sampled at even coordinates: size ((h+1)/2, (w+1)/2).
 *     per level, coarse to fine: u starts at 0 on the coarsest level -- or, with `init` [H,W,2] (level-0 pixels), at
 *               init[y s, x s] / s, s = 2^(levels-1) -- and on every other level at twice the bilinear sample of the coarser
 *               level's u at (x/2, y/2), clamped.  grad A by central differences on the clamp-padded level.  Per pixel p, over
 *               the (2r+1)^2 box window q, window coordinates clamped to the image:
 *                 G = sum grad A grad A^T + lambda I, lambda = 1e-6
 *                 `iters` times: It(q) = B(clamp(p+q) + u(p)) - A(clamp(p+q)), B sampled bilinearly, the sample position
 *                 clamped to the image;  b = sum It grad A;  u(p) -= G^-1 b.
 *               The WHOLE window moves with the centre's u.  (The cheaper form that warps each pixel by its own flow and
 *               box-filters the products diverges with more iterations: it is not this.)
 *     validity  valid[y,x] = 1 iff (i) the smaller eigenvalue of the level-0 G / (2r+1)^2 >= min_eig, (ii) x + u lies inside
 *               the image [0, W-1] x [0, H-1], and (iii), with both_directions, |u_ab(x) + u_ba(x + u_ab(x))|_2 <= consistency,
 *               u_ba the same estimator from b to a (without init), sampled bilinearly.  An invalid pixel KEEPS its u in
 *               `flow`; the caller marks it (the Python wrappers write NaN, which FL and flow_motion_labels honour).
 *   fg_optflow_supported: 1 where the shape arguments are inside the ranges below, else 0.
 *   fg_optflow_workspace_bytes: the workspace of fg_optflow (0 outside the ranges).  Its head is the pyramid of a: level l as
 *     dense float32 [h_l, w_l] at byte offset sum_{k<l} align256(4 h_k w_k) -- all that fg_optflow_pyramid writes and needs.
 *   fg_optflow_pyramid: grey conversion and all levels of one image into the workspace.
 *   fg_optflow: both pyramids, the level loop in one or both directions, validity.  flow float32 [H,W,2], valid uint8 [H,W].
 *     levels = 1, iters = 1, both_directions = 0 with `init` is ONE update step from init.
 *   Ranges, FG_ERR_UNSUPPORTED outside: FG_OPTFLOW_MIN_SIDE <= H, W <= FG_OPTFLOW_MAX_SIDE; 1 <= levels <=
 *     FG_OPTFLOW_MAX_LEVELS with the coarsest level's shorter side >= FG_OPTFLOW_MIN_COARSEST; 1 <= radius <=
 *     FG_OPTFLOW_MAX_RADIUS; 1 <= iters <= FG_OPTFLOW_MAX_ITERS; a uint8 image has 3 channels.  FG_ERR_INVALID_ARG: sizes or
 *     counts <= 0, channels not 1 or 3, an unknown dtype, min_eig or (with both_directions) consistency negative or not
 *     finite, a null or misaligned pointer (floats 4, flow and init 8, workspace 256 bytes), an output or the workspace
 *     overlapping an input or another output.  FG_ERR_WORKSPACE: workspace_bytes too small.  All before any launch.
 *   No atomics, fixed summation order: two runs are equal bit for bit, and the flow does not depend on both_directions.
 *   Asynchronous, capturable: nothing is read back, nothing allocated; 2 levels + levels (x 2) + 1 launches.  Cost:
 *   profiles/optical_flow.md. */
#define FG_OPTFLOW_MIN_SIDE 16
#define FG_OPTFLOW_MAX_SIDE 16384
#define FG_OPTFLOW_MAX_LEVELS 8
#define FG_OPTFLOW_MIN_COARSEST 8
#define FG_OPTFLOW_MAX_RADIUS 7
#define FG_OPTFLOW_MAX_ITERS 16
int fg_optflow_supported(int H, int W, int levels, int radius, int iters);
size_t fg_optflow_workspace_bytes(int H, int W, int levels, int both_directions);
int fg_optflow_pyramid(int H, int W, int channels, int dtype, const void* img, int levels, void* workspace, size_t workspace_bytes,
                       fg_stream_t stream);
int fg_optflow(int H, int W, int channels, int dtype, const void* a, const void* b, int levels, int iters, int radius, float min_eig,
               int both_directions, float consistency, const float* init, float* flow, uint8_t* valid, void* workspace,
               size_t workspace_bytes, fg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FGRASTER_H */
