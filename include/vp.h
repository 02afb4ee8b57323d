/*
 * vp.h — C ABI of libvp.so, the MI355X (gfx950) implementation of the per-frame detection hot
 * path of ayf7/cuauv-vision-pipeline: colour convert -> inRange -> erode/dilate -> connected
 * components.  Everything behind this header is hand-written HIP; there is no CPU fallback:
 * every compute entry point returns VP_ERR_HIP when no gfx950 device is usable.
 *
 * Each entry point names the reference interface it replaces (file:line under the reference
 * checkout).  The reference implements these by calling cv2 from Python (utils/color.py,
 * utils/transform.py, utils/feature.py); the Python mirror in
 * cuauv-vision-pipeline_amd/vision/utils binds this ABI with ctypes.
 *
 * Conventions: plain pointers and sizes only.  `_host` pointers are ordinary process memory
 * (staged through the context's device workspace); pointers inside vp_chain_buffers are device
 * (HBM) pointers.  Images are row-major, interleaved channels, uint8 unless stated.
 * All functions return VP_OK (0) or a negative VP_ERR_*; none throws.  A context is
 * thread-compatible (one caller at a time); use one context per stream / camera direction.
 */
#ifndef VP_H
#define VP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VP_OK 0
#define VP_ERR_INVALID (-1)     /* bad argument (NULL, size <= 0, unknown enum) */
#define VP_ERR_HIP (-2)         /* HIP runtime error / no device; see vp_last_error() */
#define VP_ERR_NOMEM (-3)       /* device or host allocation failed */
#define VP_ERR_UNSUPPORTED (-4) /* valid request outside what the kernels cover */
#define VP_ERR_CAPACITY (-5)    /* the input exceeds a fixed capacity of the device path; nothing was written (vp_fill_polys_dev) */

typedef struct vp_ctx vp_ctx;

/* colour conversion codes (values are libvp's own, not cv2's) */
enum { VP_BGR2LAB = 0, VP_BGR2HSV = 1, VP_BGR2GRAY = 2, VP_GRAY2BGR = 3, VP_HSV2BGR = 4, VP_BGR2YCRCB = 5, VP_BGR2HLS = 6, VP_LAB2BGR = 7,
       /* the rest of cv2.cvtColor's 8-bit table (vision_common.py:208-221, modules/color_balance.py:227-280, capture_sources/zed*.py) */
       VP_BGR2YUV = 8, VP_YUV2BGR = 9, VP_YCRCB2BGR = 10, VP_BGR2XYZ = 11, VP_XYZ2BGR = 12, VP_HLS2BGR = 13,
       /* RGB order: the same arithmetic with the first and third channel of the BGR side exchanged; VP_BGR2RGB is the plain exchange */
       VP_BGR2RGB = 14, VP_RGB2GRAY = 15, VP_RGB2HSV = 16, VP_HSV2RGB = 17, VP_RGB2HLS = 18, VP_HLS2RGB = 19, VP_RGB2LAB = 20,
       VP_LAB2RGB = 21, VP_RGB2YCRCB = 22, VP_YCRCB2RGB = 23, VP_RGB2YUV = 24, VP_YUV2RGB = 25, VP_RGB2XYZ = 26, VP_XYZ2RGB = 27,
       /* alpha and reorders (4-channel images; a new alpha channel is 255) */
       VP_BGRA2BGR = 28, VP_RGBA2BGR = 29, VP_BGR2BGRA = 30, VP_BGR2RGBA = 31, VP_BGRA2RGBA = 32, VP_GRAY2BGRA = 33, VP_BGRA2GRAY = 34,
       VP_RGBA2GRAY = 35, VP_CVT_CODES = 36 };
/* morphology ops — utils/transform.py:80-164 */
enum { VP_MORPH_ERODE = 0, VP_MORPH_DILATE = 1, VP_MORPH_OPEN = 2, VP_MORPH_CLOSE = 3, VP_MORPH_GRADIENT = 4 };
/* structuring element shapes — cv2.MORPH_RECT / MORPH_CROSS / MORPH_ELLIPSE */
enum { VP_SHAPE_RECT = 0, VP_SHAPE_CROSS = 1, VP_SHAPE_ELLIPSE = 2 };
/* label numbering: VP_CCL_BLOCK2X2 = order of cv2.connectedComponents' default 8-way
 * algorithm (raster order of each component's first 2x2 block); VP_CCL_PIXEL = raster order of
 * each component's first pixel (cv2 CCL_WU / SAUF). */
enum { VP_CCL_PIXEL = 1, VP_CCL_BLOCK2X2 = 2 };

/* ---- context ------------------------------------------------------------------------- */
int vp_version(void);
const char* vp_strerror(int code);
/* Creates a context on HIP device `device` with its own non-blocking stream. NULL on failure
 * (vp_last_error(NULL) tells why). */
/* Devices visible to the process, and the PCI address ("0000:05:00.0") of one: /sys/bus/pci/devices/<address>/numa_node names the
 * host NUMA node next to it (vision/dispatch.py binds each device's feeder threads there).  No context needed. */
int vp_device_count(void);
int vp_device_pci_bus_id(int device, char* out, int len);
vp_ctx* vp_create(int device);
int vp_destroy(vp_ctx* ctx);
const char* vp_last_error(const vp_ctx* ctx);
/* Adopt an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL reverts to
 * the context's own stream. */
int vp_set_stream(vp_ctx* ctx, void* hip_stream);
void* vp_get_stream(vp_ctx* ctx);
int vp_synchronize(vp_ctx* ctx);
/* Options.  VP_OPT_CHAIN_STREAMS (1..4, default 1): vp_chain_run splits a batch into that many sub-batches
 * on internal streams (fork/join around the context's stream); results are identical for every value.
 * Measured on MI355X: no gain over 1 (the kernels of the two halves slow each other down), hence the default.
 * VP_OPT_CCL_LEVELS (1 or 2, default 2): 2 = strip-local components merged by one block per frame, frames that do not fit
 * finished by the one-level kernels; 1 = one-level kernels only.  Results are identical.
 * VP_OPT_CCL_MERGE_CAP (-1 = capacity of the merge block, or a smaller count): strip components per frame above which a frame
 * is handed to the one-level kernels (test hook: 0 sends every non-empty frame there).
 * VP_OPT_FLAT_OPS (0 or 1, default 1): the per-operator kernels (vp_cvt_color_*, vp_inrange_u8_*) use their 16-pixels-per-lane forms
 * whenever rows are packed and pointers 16-B aligned; 0 forces the generic one-pixel-per-thread kernels (the tests run both).
 * VP_OPT_HOUGH_LDS (0 or 1, default 1): the Hough vote counts accumulator rows in LDS and flushes them with global atomics where a
 * row fits the block's LDS budget; 0 makes every vote a global atomic.  Results are identical.
 * VP_OPT_HOUGH_CIRCLES_LDS (0 or 1, default 1): the HoughCircles radius histogram of a centre is kept in LDS where its bins fit
 * (160 KiB); 0 keeps it in device memory, as for more bins than that (the tests reach that path at small sizes).  Results are identical.
 * VP_OPT_BLUR_ONEPASS (1, 0 or -1, default -1): which kernels vp_gaussian_blur_dev runs.  1 = the one-pass kernel (rows and halo staged
 * in LDS, the 16-bit intermediate never written to device memory) wherever its tile fits, i.e. kernels up to 31 on both axes; 0 = always
 * the two passes of vp_gaussian_blur_u8; -1 = the measured choice.  Results are identical.
 * VP_OPT_MEDIAN_MASK (1, 0 or -1, default -1; the environment variable of the same name sets 1 or 0 at vp_create): which kernel
 * vp_median_blur_dev runs on a single-channel image the caller calls a 0/255 mask (binary_hint).  1 = the bit-plane majority vote for
 * every window it can serve (3..63); 0 = never, the general kernels; -1 = the measured choice (whenever the source's bit plane is
 * passed, and from window 5 on without one).  Results are identical.
 * VP_OPT_CLAHE_SPLIT (0..64, default 0; the environment variable of the same name sets 1..64 at vp_create): how many blocks share
 * the histogram of one CLAHE tile in vp_clahe_u8 / vp_clahe_dev.  1 = one block per tile does histogram, clip, scan and table in one
 * launch; n > 1 = n blocks (at most one per tile row) add partial histograms with device atomics and a finishing launch makes the
 * tables; 0 = the measured choice.  Results are identical.
 * VP_OPT_CCL_CROWDED (0, 1 or 2, default 0; the environment variable of the same name sets it at vp_create): what the two-level
 * labelling queues behind its merge for frames the merge hands over as crowded.  1 = always the six launches of the crowded-frame
 * kernels, which leave at once when no frame was handed over; 2 = always one launch that finishes such a frame correctly but slowly
 * (with VP_OPT_CHAIN_STREAMS above 1: still the six); 0 = by a hint - the number of frames an earlier call handed over, read without
 * synchronising: the one launch until a call hands a frame over, the six from the next call on, the one again after 32 calls in a
 * row that handed nothing over; a vp_chain_run_contours call whose contour pass runs beside the labelling always takes the six.
 * Results are identical.
 * VP_OPT_LABEL_MOMENTS_LDS (1, 0 or -1, default -1): where vp_label_moments_* keeps its (nlabels, 10) table while it adds.  1 = in
 * each block's LDS, flushed with device atomics - the whole table when nlabels * 80 bytes fit (768 labels), else its first 64 rows,
 * the background's among them, the other rows taking device atomics; 0 = device atomics for every run; -1 = the measured choice
 * (that of 1).  Results are identical. */
enum { VP_OPT_CHAIN_STREAMS = 1, VP_OPT_CCL_LEVELS = 2, VP_OPT_CCL_MERGE_CAP = 3, VP_OPT_FLAT_OPS = 4, VP_OPT_HOUGH_LDS = 5,
       VP_OPT_HOUGH_CIRCLES_LDS = 6, VP_OPT_BLUR_ONEPASS = 7, VP_OPT_MEDIAN_MASK = 8, VP_OPT_CLAHE_SPLIT = 9, VP_OPT_CCL_CROWDED = 10,
       VP_OPT_LABEL_MOMENTS_LDS = 11 };
int vp_set_option(vp_ctx* ctx, int option, int value);
/* Kernels of the labelling sequence that the context's last labelling call queued (vp_ccl_*, vp_chain_run with ccl): tells the tests
 * which form VP_OPT_CCL_CROWDED = 0 chose.  The one-off initialisation of the crowded-frame kernels' accumulators is not counted. */
int vp_ccl_last_launches(vp_ctx* ctx, int32_t* launches);
/* HIP-event stopwatch on the context's stream (bench.py: roofline.achieved). */
int vp_timer_start(vp_ctx* ctx);
int vp_timer_stop(vp_ctx* ctx, float* elapsed_ms); /* records, synchronises, returns ms */
/* Per-kernel attribution: between vp_profile_begin and vp_profile_end every kernel the context
 * launches is bracketed by HIP events on its stream.  vp_profile_end synchronises and fills
 * total_ms[id] / launches[id] for id < VP_PROF_KERNELS (names: vp_profile_kernel_name). */
#define VP_PROF_KERNELS 18
int vp_profile_begin(vp_ctx* ctx, int max_records);
int vp_profile_end(vp_ctx* ctx, double* total_ms, int32_t* launches);
const char* vp_profile_kernel_name(int id);
/* Copies of the integer tables the kernels use (for parity tests against the oracle):
 * gamma[256] u16, cbrt[3072] u16, sdiv[256] i32, hdiv180[256] i32, lab_coeffs[9] i32. */
int vp_get_tables(uint16_t* gamma, uint16_t* cbrt_tab, int32_t* sdiv, int32_t* hdiv180, int32_t* lab_coeffs);
/* Copies of the tables of the 8-bit Lab -> BGR conversion (VP_LAB2BGR and the white balance; OpenCV 4.x Lab2RGBinteger, each may be
 * NULL): yf[512] u16 = (y, f(y)) in Q14 per 8-bit L; ab_xz[VP_LAB_AB_TAB] i32 = x (or z) in Q14 of the Q14 value
 * VP_LAB_MIN_AB + i of f(x) (or f(z)); inv_gamma[4096] u16 = round(255 * sRGB(i / 4096)); coeffs[9] i32 = Q12 coefficients of
 * (x, y, z), white point folded in, rows blue, green, red. */
#define VP_LAB_MIN_AB (-8145)
#define VP_LAB_AB_TAB 36864
int vp_get_lab_inv_tables(uint16_t* yf, int32_t* ab_xz, uint16_t* inv_gamma, int32_t* coeffs);

/* ---- per-operator API, host pointers --------------------------------------------------- */

/* utils/color.py:11-32 `_convert_colorspace` (cv2.cvtColor + cv2.split): bgr_to_lab, bgr_to_hsv,
 * bgr_to_gray, gray_to_bgr, bgr_to_ycrcb, bgr_to_hls (modules/preprocessor.py:66-75), plus HSV2BGR (color_balance.cpp:669).
 * YCrCb is OpenCV's Q14 integer form; HLS is the float32 statement sequence of RGB2HLS_f behind RGB2HLS_b.  src is (h,w,3) (or (h,w) for GRAY2BGR) with `src_stride` bytes per
 * row.  dst_interleaved (tightly packed, may be NULL) receives the converted image; dst_planes[k]
 * (each (h,w) tightly packed, each may be NULL, array may be NULL) receive the split channels.
 * The codes from VP_BGR2YUV on: the channel counts of src and dst_interleaved follow from the code (1, 3 or 4).  All arithmetic is
 * OpenCV's 8-bit form, descale(x, n) = (x + (1 << (n - 1))) >> n, results saturated: YUV and YCrCb are RGB2YCrCb_i / YCrCb2RGB_i in
 * Q14 (YUV stores Y, U, V), XYZ is RGB2XYZ_i / XYZ2RGB_i in Q12, HLS -> BGR the float32 statement sequence of HLS2RGB_f behind
 * HLS2RGB_b (hue 0..180; DESIGN 4.16 holds every constant).  dst_planes of these codes: up to three planes for a 3-channel result;
 * it must be NULL for a 1-channel or 4-channel result (VP_ERR_INVALID otherwise). */
int vp_cvt_color_u8(vp_ctx* ctx, int code, const uint8_t* src_host, size_t src_stride, int w, int h,
                    uint8_t* dst_interleaved_host, uint8_t* const* dst_planes_host);
/* VP_LAB2BGR (utils/color.py:26-32 `lab_to_bgr`, cv2.COLOR_LAB2BGR on 8-bit images) is OpenCV's integer path Lab2RGBinteger:
 * table look-ups, Q14 divisions of a and b by 500 and 200, the XYZ -> sRGB matrix in Q12 fixed point, the 4096-entry inverse gamma. */

/* utils/color.py:370-392 `white_balance_bgr` / `white_balance_bgr_blur` on an 8-bit BGR image (row stride src_stride) into a packed
 * BGR image dst: Lab (as VP_BGR2LAB), a and b each shifted by (mean - 128) in float32 and cast back to uint8 the way numpy's
 * astype does (truncation, low 8 bits), then VP_LAB2BGR.  kernel_size = VP_WB_GLOBAL_MEAN: the mean is np.mean of the plane
 * (float32 sum of exact per-8192-pixel sums, in order); an odd kernel_size k >= 1 (k <= VP_WB_MAX_KERNEL): the k x k box mean of
 * cv2.blur with BORDER_REPLICATE, float32(sum * (1.0 / (k k))).  ab_mean_out (host, may be NULL): the two global means (a, b)
 * (global form only; the call then synchronises).  dst must not overlap src.  The _u8 form synchronises. */
#define VP_WB_GLOBAL_MEAN 0
#define VP_WB_MAX_KERNEL 4095
int vp_white_balance_u8(vp_ctx* ctx, const uint8_t* src_host, size_t src_stride, int w, int h, int kernel_size, uint8_t* dst_host,
                        float* ab_mean_out);

/* Extension (BASELINE north star "LAB floats within 1e-4"; no reference call site converts float images): BGR float32 in
 * [0,1] (h,w,3 tightly packed) -> CIE L*a*b* float32 (L 0..100, a/b about -127..127), analytic sRGB / D65. */
int vp_cvt_bgr2lab_f32(vp_ctx* ctx, const float* src_host, int w, int h, float* dst_host);

/* utils/color_correction/color_balance.hpp:9-14 `process_frame` (modules/color_balance.py:93-110 `balance`,
 * modules/preprocessor.py:87-88): colour-cast equalisation, optional RGB / HSV contrast stretch, 0.2 % extrema clipping.
 * flags = OR of VP_CB_*; the reference's default call is VP_CB_DEFAULT with 1x1 tiles.  Not implemented
 * (VP_ERR_UNSUPPORTED): tilings that do not divide the frame (the reference wraps into the next row and processes
 * pixels twice there).  src and dst are (h,w,3) BGR, tightly packed; dst may equal src. */
enum { VP_CB_EQUALIZE_RGB = 1, VP_CB_RGB_CONTRAST = 2, VP_CB_HSV_CONTRAST = 4, VP_CB_HSI_CONTRAST = 8, VP_CB_EXTREMA_CLIPPING = 16,
       VP_CB_ADAPTIVE_CAST = 32, VP_CB_DEFAULT = 1 | 4 | 16 };
int vp_color_balance_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int flags, int horizontal_blocks, int vertical_blocks,
                        uint8_t* dst_host);
/* Diagnostic: in how many tiles the last colour-balance call on this context had to run the reference's sequential tile mean
 * (cpp:452-467) because its value could have mattered (see csrc/vp_balance.hip); valid until the next call that uses the workspace. */
int vp_color_balance_last_folds(vp_ctx* ctx, int32_t* tiles_folded);
/* Same on device memory for a batch of n frames ((n,h,w,3), packed; dst may equal src); enqueues and returns. */
int vp_color_balance_dev(vp_ctx* ctx, const uint8_t* src_dev, uint8_t* dst_dev, int w, int h, int n_frames, int flags,
                         int horizontal_blocks, int vertical_blocks);

/* utils/color.py:105-121 `range_threshold` / modules/bins.py:16 (cv2.inRange): cn = 1 or 3;
 * lo/hi have cn entries (already rounded to integers); dst is (h,w) 0/255. */
int vp_inrange_u8(vp_ctx* ctx, const uint8_t* src_host, size_t src_stride, int w, int h, int cn,
                  const int32_t* lo, const int32_t* hi, uint8_t* dst_host);
/* cv2.inRange on a CV_32FC1 image (utils/color.py:103 on `dists`). */
int vp_inrange_f32(vp_ctx* ctx, const float* src_host, size_t src_stride_bytes, int w, int h, float lo,
                   float hi, uint8_t* dst_host);

/* utils/color.py:66-103 `thresh_color_distance` arithmetic: d2 = sum_c wts[c]*(f32(p_c)-color[c])^2
 * in float32, channels in order, channel c skipped when bit c of skipmask is set.
 * dist2_out ((h,w) f32) and sqrt_out ((h,w) u8 = uint8(sqrt(d2))) may each be NULL. */
int vp_color_distance_u8(vp_ctx* ctx, const uint8_t* const* planes_host, int w, int h, const float* color,
                         const float* wts, int skipmask, float* dist2_out_host, uint8_t* sqrt_out_host);
/* Order statistics for np.percentile(dists, p) in utils/color.py:98: the k-th and (k+1)-th smallest of n float32 values
 * (exact, by radix selection on the device); v_k1 may be NULL; k+1 is clamped to n-1. */
int vp_order_stats_f32(vp_ctx* ctx, const float* src_host, size_t n, size_t k, float* v_k, float* v_k1);
/* utils/transform.py:27-77 `elliptic_kernel` / `rect_kernel` (cv2.getStructuringElement):
 * out is (kh,kw) 0/1.  Integer geometry on the host, no device needed. */
int vp_structuring_element(int shape, int kw, int kh, uint8_t* out);

/* utils/transform.py:80-164 erode / dilate / morph_remove_noise / morph_close_holes /
 * morph_borders and modules/preprocessor.py:120-129 (cv2.erode / dilate / morphologyEx):
 * src/dst (h,w,cn) tightly packed, cn in 1..4; kernel (kh,kw) non-zero = member, NULL = 3x3 rect;
 * anchor (-1,-1) = centre; border = cv2 default (outside never wins). */
int vp_morph_u8(vp_ctx* ctx, int op, const uint8_t* src_host, int w, int h, int cn, const uint8_t* kernel,
                int kw, int kh, int anchor_x, int anchor_y, int iterations, uint8_t* dst_host);

/* North-star CCL (replaces the cv2.findContours stage of utils/feature.py:5-40 with labels;
 * semantics of cv2.connectedComponentsWithStats(mask, 8, CV_32S)): non-zero = foreground,
 * 8-connectivity.  labels (h,w) i32 may be NULL.  stats (max_labels,5) i32 rows
 * [left, top, width, height, area] and centroids (max_labels,2) f64, row 0 = background; rows
 * beyond max_labels are dropped but *nlabels is always the true count (incl. background). */
int vp_ccl_u8(vp_ctx* ctx, const uint8_t* src_host, size_t src_stride, int w, int h, int numbering,
              int32_t* labels_host, int32_t* stats_host, double* centroids_host, int max_labels,
              int32_t* nlabels);

/* utils/feature.py:5-40 `outer_contours` / `all_contours` (cv2.findContours): mode VP_RETR_EXTERNAL or VP_RETR_LIST,
 * method VP_CHAIN_APPROX_NONE or VP_CHAIN_APPROX_SIMPLE, offset (0,0); non-zero = foreground.  Contours come back in
 * cv2's order (last found first): counts[k] points of contour k, is_hole[k] (may be NULL), points = (x, y) int32 pairs
 * of all contours back to back.  *n_contours / *n_points are always the true totals; when either exceeds its capacity
 * nothing is copied out and the caller retries with larger buffers. */
enum { VP_RETR_EXTERNAL = 0, VP_RETR_LIST = 1, VP_RETR_CCOMP = 2, VP_RETR_TREE = 3 };
enum { VP_CHAIN_APPROX_NONE = 1, VP_CHAIN_APPROX_SIMPLE = 2 };
int vp_find_contours_u8(vp_ctx* ctx, const uint8_t* src_host, size_t src_stride, int w, int h, int mode, int method,
                        int32_t* points_host, int64_t max_points, int32_t* counts_host, uint8_t* is_hole_host, int max_contours,
                        int32_t* n_contours, int64_t* n_points);

/* utils/feature.py:240-265 `contour_centroid` / `contour_area` (cv2.moments / cv2.contourArea of an integer contour): the Green sums
 * out3 = {sum d, sum d (x' + x), sum d (y' + y)}, d = x' y - x y' over consecutive points (x', y') -> (x, y), as exact integers;
 * host code, no context.  The Python mirror applies cv2's factors 1/2 and 1/6 in float64. */
int vp_polygon_sums_i32(const int32_t* pts_xy, int npts, int64_t* out3);
/* Convex hull of integer points by the monotone chain (host code, exact): distinct hull vertices counter-clockwise from the
 * lexicographically smallest point, collinear points dropped; `out` holds up to npts points.  Used by the cv2.minAreaRect stand-in
 * (modules/bins.py:62). */
int vp_convex_hull_i32(const int32_t* pts, int npts, int32_t* out, int* nout);
/* cv2.minAreaRect stand-in for integer points (host code): rotating calipers over that hull; out5 = centre x, y, width, height,
 * angle in degrees in (0, 90] (OpenCV >= 4.5.1 convention), as floats.  modules/bins.py:62 calls it for every contour. */
int vp_min_area_rect_i32(const int32_t* pts, int npts, float* out5);

/* utils/draw.py:283-327 `draw_contours` / `draw_polylines` (modules/red_buoy.py:39): in-place polyline on a HOST image (no device
 * work, no context): Bresenham steps with a square brush of `thickness` pixels - the Python mirror's rasteriser in C.  pts = npts
 * (x, y) int32 pairs; color has cn entries.  Debug overlay only: agreement with cv2's line drawing is not claimed. */
int vp_draw_polyline_u8(uint8_t* img_host, size_t stride, int w, int h, int cn, const int32_t* pts, int npts, int closed,
                        const uint8_t* color, int thickness);
/* several polylines in one call: counts[k] points each, back to back in pts (cv2.drawContours(img, contours, -1, ...)) */
int vp_draw_polylines_u8(uint8_t* img_host, size_t stride, int w, int h, int cn, const int32_t* pts, const int32_t* counts, int npolys,
                         int closed, const uint8_t* color, int thickness);

/* utils/draw.py `draw_contours` / `draw_polylines` with a negative thickness (cv2.drawContours(mask, [contour], -1, 255, thickness=-1)
 * of vision_common.py:282-288 `fill_ratio`): every polygon filled by the even-odd scanline of the Python mirror, then outlined, closed,
 * at thickness 1 - the same pixels, on a HOST image.  Rows max(ymin, 0) .. min(ymax, h - 1); edge (a, b) counts on row y when
 * min(ya, yb) <= y < max(ya, yb) and crosses it at xa + (y - ya)(xb - xa)/(yb - ya); the sorted crossings pair up and pair (p, q) paints
 * [ceil(p), floor(q)], clipped.  The crossings are exact integers here and float64 in Python: the two agree when every coordinate lies
 * within +-VP_FILL_MAX_COORD (distinct crossings then differ by at least 2^-32, the float64 error is below 2^-36), and a polygon with a
 * coordinate beyond that is refused with VP_ERR_UNSUPPORTED.  Any number of crossings per row. */
#define VP_FILL_MAX_COORD 32767
int vp_fill_polys_u8(uint8_t* img_host, size_t stride, int w, int h, int cn, const int32_t* pts, const int32_t* counts, int npolys,
                     const uint8_t* color);

/* ---- device-resident forms of the per-operator entry points ----------------------------- *
 * Same arithmetic and argument meaning as vp_cvt_color_u8 / vp_inrange_u8 / vp_morph_u8 / vp_find_contours_u8; images are
 * device pointers.  Nothing is copied; the first three enqueue on the context's stream and return without synchronising, so a
 * module's process() (modules/red_buoy.py:21-38: bgr_to_lab -> range_threshold -> morph_remove_noise -> morph_close_holes ->
 * outer_contours) uploads its frame once and downloads only what Python reads (the Python mirror hands these images around as
 * lazily materialised arrays, vision/devmat.py).  vp_morph_u8_dev: dst must not overlap src; binary_hint 1 = the image is known
 * to hold only 0 / 255 (a mask this library produced), 0 = unknown (one flag is then read back, synchronising).
 * vp_find_contours_dev returns the lists in host memory and synchronises, like its host form. */
int vp_cvt_color_dev(vp_ctx* ctx, int code, const uint8_t* src_dev, size_t src_stride, int w, int h, uint8_t* dst_interleaved_dev,
                     uint8_t* const* dst_planes_dev);
/* vp_white_balance_u8 on device images, enqueued on the context's stream (synchronises only to fill ab_mean_out). */
int vp_white_balance_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int kernel_size, uint8_t* dst_dev,
                         float* ab_mean_out);
int vp_inrange_u8_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, const int32_t* lo, const int32_t* hi,
                      uint8_t* dst_dev);
/* vp_inrange_u8_dev that can also leave the mask's BIT-PACKED form ((h, ceil(w / 64)) u64, bit i of word j = pixel 64 j + i) in bits_dev
 * (nullable): written when rows are packed, pointers 16-B aligned and w % 64 == 0 - *made_bits says whether (otherwise bits_dev is
 * untouched).  vp_find_contours_bits_dev takes that plane in place of the image and saves the packing launch: the pair serves
 * range_threshold -> outer_contours (modules/red_buoy.py:22, :38) when the mask has not been written to in between. */
int vp_inrange_u8_bits_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, const int32_t* lo, const int32_t* hi,
                           uint8_t* dst_dev, unsigned long long* bits_dev, int* made_bits);
int vp_morph_u8_dev(vp_ctx* ctx, int op, const uint8_t* src_dev, int w, int h, int cn, const uint8_t* kernel, int kw, int kh,
                    int anchor_x, int anchor_y, int iterations, int binary_hint, uint8_t* dst_dev);
/* vp_draw_polylines_u8 into a packed device image (points and counts are host arrays): the same pixels, written by the device, so
 * that an overlay which is only posted (modules/bins.py:20-79) never has to visit the host. */
int vp_draw_polylines_dev(vp_ctx* ctx, uint8_t* img_dev, int w, int h, int cn, const int32_t* pts, const int32_t* counts, int npolys,
                          int closed, const uint8_t* color, int thickness);
/* vp_fill_polys_u8 into a packed device image, enqueued on the context's stream (points and counts are host arrays): the same pixels and
 * the same checks.  The kernel sorts at most 256 crossings per row: when some row of some polygon has more, VP_ERR_CAPACITY comes back
 * and nothing has been painted (the caller fills on the host). */
int vp_fill_polys_dev(vp_ctx* ctx, uint8_t* img_dev, int w, int h, int cn, const int32_t* pts, const int32_t* counts, int npolys,
                      const uint8_t* color);
/* utils/draw.py `draw_rect` / `draw_circle` with a negative thickness on a packed device image, enqueued: columns min(x0, x1) ..
 * max(x0, x1) of rows min(y0, y1) .. max(y0, y1); row cy + dy of the disc spans cx -+ floor(sqrt(r r - dy dy)), the root an exact
 * integer one; both clipped to the image, a negative radius paints nothing.  Coordinates and radius within +-2^20
 * (VP_ERR_UNSUPPORTED beyond). */
int vp_fill_rect_dev(vp_ctx* ctx, uint8_t* img_dev, int w, int h, int cn, int x0, int y0, int x1, int y1, const uint8_t* color);
int vp_fill_circle_dev(vp_ctx* ctx, uint8_t* img_dev, int w, int h, int cn, int cx, int cy, int radius, const uint8_t* color);
/* cv2.addWeighted(a, alpha, b, beta, gamma) on two device images of n bytes (modules/bins.py:20, the mask overlay):
 * saturate(round-half-even(a*alpha + b*beta + gamma)) in correctly rounded doubles; dst may be one of the sources. */
int vp_add_weighted_u8_dev(vp_ctx* ctx, const uint8_t* a_dev, double alpha, const uint8_t* b_dev, double beta, double gamma, size_t n,
                           uint8_t* dst_dev);
int vp_find_contours_bits_dev(vp_ctx* ctx, const unsigned long long* bits_dev, int w, int h, int mode, int method, int32_t* points_host,
                              int64_t max_points, int32_t* counts_host, uint8_t* is_hole_host, int max_contours, int32_t* n_contours,
                              int64_t* n_points);
/* Diagnostic: the largest number of border segments ("heads") a frame of this context's last contour pass held, as far as it has been
 * reported back (single-image calls: exact; batched passes: read from pinned memory without synchronising, so possibly one call
 * late).  It is what the next pass chooses the form of its bookkeeping by (one block per frame / launches over the chip) - a choice
 * the results do not depend on. */
unsigned int vp_contours_last_heads(vp_ctx* ctx);
/* cv2.findContours with its hierarchy: the three entries above with one more argument, hierarchy_host (4 int32 per contour, may be
 * NULL), and all four modes.  VP_RETR_CCOMP / VP_RETR_TREE return the borders of VP_RETR_LIST (same points, start points, hole
 * flags) in the pre-order of the Suzuki-Abe tree - top level first, siblings newest first - and the rows [next, prev, first_child,
 * parent] (indices into the returned list, -1 for none) that cv2 returns as hierarchy[0].  TREE: the parent of an outer border is
 * the hole border of the background region around it (none if that region reaches the frame), the parent of a hole border is the
 * outer border of its component; CCOMP: every outer border is at the top level.  VP_RETR_EXTERNAL / VP_RETR_LIST give what the
 * entries above give, with the flat rows [next, prev, -1, -1].  Totals and retries as above: the rows are filled when the contours
 * are.  The entries above (and vp_chain_run_contours) keep rejecting modes 2 and 3. */
int vp_find_contours_tree_u8(vp_ctx* ctx, const uint8_t* src_host, size_t src_stride, int w, int h, int mode, int method,
                             int32_t* points_host, int64_t max_points, int32_t* counts_host, uint8_t* is_hole_host, int max_contours,
                             int32_t* n_contours, int64_t* n_points, int32_t* hierarchy_host);
int vp_find_contours_tree_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int mode, int method,
                              int32_t* points_host, int64_t max_points, int32_t* counts_host, uint8_t* is_hole_host, int max_contours,
                              int32_t* n_contours, int64_t* n_points, int32_t* hierarchy_host);
int vp_find_contours_tree_bits_dev(vp_ctx* ctx, const unsigned long long* bits_dev, int w, int h, int mode, int method,
                                   int32_t* points_host, int64_t max_points, int32_t* counts_host, uint8_t* is_hole_host, int max_contours,
                                   int32_t* n_contours, int64_t* n_points, int32_t* hierarchy_host);
int vp_find_contours_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int mode, int method,
                         int32_t* points_host, int64_t max_points, int32_t* counts_host, uint8_t* is_hole_host, int max_contours,
                         int32_t* n_contours, int64_t* n_points);

/* ---- fused, batched, device-resident chain -------------------------------------------- */

#define VP_CHAIN_MAX_MORPH 8
typedef struct vp_chain_desc {
    int32_t width, height;
    int32_t color_mode;            /* VP_BGR2LAB, VP_BGR2HSV or VP_BGR2GRAY */
    int32_t lo[3], hi[3];          /* inclusive per-channel bounds on the converted image */
    int32_t n_morph;               /* 0..VP_CHAIN_MAX_MORPH ops applied in order */
    int32_t morph_op[VP_CHAIN_MAX_MORPH];   /* VP_MORPH_ERODE/DILATE/OPEN/CLOSE */
    int32_t morph_kw[VP_CHAIN_MAX_MORPH];   /* all-ones (rect) kernels, anchor = centre */
    int32_t morph_kh[VP_CHAIN_MAX_MORPH];
    int32_t morph_iter[VP_CHAIN_MAX_MORPH];
    int32_t ccl;                   /* 0 = none, 1 = label the cleaned mask, 2 = the threshold mask */
    int32_t numbering;             /* VP_CCL_BLOCK2X2 or VP_CCL_PIXEL */
    int32_t max_labels;            /* stats/centroid rows per frame, incl. background row 0 */
} vp_chain_desc;

typedef struct vp_chain_buffers {  /* device pointers; any output may be NULL */
    const uint8_t* bgr;            /* (n,h,w,3) */
    uint8_t* threshed;             /* (n,h,w) result of inRange — modules/red_buoy.py:23-28 */
    uint8_t* cleaned;              /* (n,h,w) after the morphology ops — red_buoy.py:31-34 */
    int32_t* labels;               /* (n,h,w) */
    int32_t* stats;                /* (n,max_labels,5) */
    double* centroids;             /* (n,max_labels,2) */
    int32_t* nlabels;              /* (n) */
} vp_chain_buffers;

/* Enqueues the whole chain for n frames (n <= 65535, width*height <= 2^30) on the context's stream and returns without
 * synchronising.  This is the hot path bench.py times (one call = one "step"). */
int vp_chain_run(vp_ctx* ctx, const vp_chain_desc* desc, const vp_chain_buffers* dev, int n_frames);
/* Same with host buffers: H2D, chain, D2H, synchronised on return. */
int vp_chain_run_host(vp_ctx* ctx, const vp_chain_desc* desc, const vp_chain_buffers* host, int n_frames);
/* Algorithmic HBM bytes one vp_chain_run call moves (3 B/px read + 1 B/px per mask
 * written + 4 B/px labels), for roofline accounting. */
uint64_t vp_chain_algorithmic_bytes(const vp_chain_desc* desc, const vp_chain_buffers* bufs, int n_frames);

/* ---- chain + contours for the whole batch ------------------------------------------------
 * What modules/red_buoy.py:36-38 (`outer_contours(cleaned)`) and modules/bins.py:27 (`outer_contours`
 * after the morphology) do per frame, for n frames in one launch sequence: the chain above, then
 * cv2.findContours semantics (utils/feature.py:5-40) on the cleaned or the threshold mask. */
typedef struct vp_contour_desc {
    int32_t source;        /* 1 = the cleaned mask, 2 = the threshold mask */
    int32_t mode;          /* VP_RETR_EXTERNAL or VP_RETR_LIST */
    int32_t method;        /* VP_CHAIN_APPROX_NONE or VP_CHAIN_APPROX_SIMPLE */
    int32_t max_contours;  /* capacity per frame */
    int64_t max_points;    /* capacity per frame */
} vp_contour_desc;

typedef struct vp_contour_buffers {  /* device pointers (vp_chain_run_contours) / host pointers (.._host) */
    int32_t* info;         /* (n,2): contours found in the frame; points of all of them (both totals whatever the capacities) */
    int32_t* counts;       /* (n,max_contours) points per contour, in discovery order = raster order of
                              the start pixel; cv2 returns the reverse order */
    int32_t* offsets;      /* (n,max_contours) first point of the contour within the frame's point list */
    uint8_t* is_hole;      /* (n,max_contours) */
    int32_t* points;       /* (n,max_points,2) (x,y) */
    double* features;      /* optional (may be NULL): (n,max_contours,8) per contour {m00, m10, m01 as cv2.moments gives them
                              for the contour (utils/feature.py:240-252), area = cv2.contourArea (:255-265), bounding box x, y,
                              width, height as cv2.boundingRect} - computed on the device, exact (the sums are integers) */
} vp_contour_buffers;

/* Contours beyond max_contours are counted in info[.][0] but not traced; a contour whose points
 * would pass max_points is skipped (info[.][1] counts the points of both kinds), so a caller can
 * repeat with larger capacities.  Enqueues and returns without synchronising. */
int vp_chain_run_contours(vp_ctx* ctx, const vp_chain_desc* desc, const vp_chain_buffers* dev, const vp_contour_desc* cdesc,
                          const vp_contour_buffers* cdev, int n_frames);
/* Host buffers: H2D, chain, contours, D2H, synchronised on return. */
int vp_chain_run_contours_host(vp_ctx* ctx, const vp_chain_desc* desc, const vp_chain_buffers* host, const vp_contour_desc* cdesc,
                               const vp_contour_buffers* chost, int n_frames);

/* ---- contour geometry: perimeter, hull, minimum-area rectangle, enclosing circle ------------------
 * What a module computes per contour after cv2.findContours (modules/bins.py:33,61 cv2.minAreaRect, utils/feature.py:266-325
 * cv2.arcLength / convexHull / minEnclosingCircle), for every contour of a point block in one launch: one row per contour.
 * Points are int32 (x, y) pairs with both coordinates in [-32768, 32767].
 *   perimeter / perimeter_open: cv2.arcLength(c, True) / (c, False) as vp's stand-in computes it - float32 segment roots summed in
 *     float64 - bit for bit (the device adds the roots as integer counts of 2^-23, exact below 2^53).
 *   hull_count, hull_area2: vp_convex_hull_i32's vertex count and twice its area; the vertices on request.
 *   rect: vp_min_area_rect_i32's five floats, bit for bit (the device finds the edge and the extents, one host function finishes).
 *   circle: centre x, y and radius of the smallest circle that contains every point, from an exact support set of 1..3 points
 *     (support_count, support): no safety margin is added (OpenCV adds a small one).  No points: zeros.
 *   status: 0 = finished on the device; VP_GEOM_HULL_CAP = the hull candidates passed the device slot (vp_contour_geometry_plan tells
 *     its size) and VP_GEOM_PERIMETER = the perimeter total reached 2^53 units - vp_contour_geometry_i32 has then finished the row
 *     with the host routines and leaves the bit set, the device forms leave hull, rect and circle (or the two perimeters) zero for
 *     the caller to finish; VP_GEOM_SKIPPED = batch form, the contour was not traced (row zero); VP_GEOM_COORD = device forms, a
 *     coordinate outside the bound (row zero). */
enum { VP_GEOM_OK = 0, VP_GEOM_HULL_CAP = 1, VP_GEOM_PERIMETER = 2, VP_GEOM_SKIPPED = 4, VP_GEOM_COORD = 8 };
typedef struct vp_contour_geom {
    double perimeter;
    double perimeter_open;
    int64_t hull_area2;
    int32_t hull_count;
    uint32_t status;
    float rect[5];         /* centre x, y, width, height, angle */
    float circle[3];       /* centre x, y, radius */
    int32_t support_count;
    int16_t support[6];    /* (x, y) of the support points */
} vp_contour_geom;         /* 80 bytes */
/* Host points: counts_host[k] points of contour k, back to back in pts_host.  hull_pts_out (may be NULL, same size as pts_host)
 * receives the hull of contour k at the place of its points, hull_counts_out (may be NULL) their number.  A coordinate outside the
 * bound is refused with VP_ERR_UNSUPPORTED before anything is launched. */
int vp_contour_geometry_i32(vp_ctx* ctx, const int32_t* pts_host, const int32_t* counts_host, int n_contours, vp_contour_geom* rows_out,
                            int32_t* hull_pts_out, int32_t* hull_counts_out);
/* Points already on the device: first_dev[k] is the index of contour k's first point (int64), pts_dev 8-byte aligned.  hull_pts_dev
 * (may be NULL) as above, on the device.  Rows come back to the host finished; synchronises. */
int vp_contour_geometry_dev(vp_ctx* ctx, const int32_t* pts_dev, const int64_t* first_dev, const int32_t* counts_dev, int n_contours,
                            vp_contour_geom* rows_out_host, int32_t* hull_pts_dev);
/* A batch as vp_chain_run_contours left it on the device: rows_out_host is (n_frames, max_contours); row k of frame f is contour k
 * of cdev->counts / offsets for k < min(info[f][0], max_contours), VP_GEOM_SKIPPED otherwise and for a contour that overflowed
 * max_points.  Nothing but info, counts, offsets and points is read.  Synchronises. */
int vp_contour_geometry_batch_dev(vp_ctx* ctx, const vp_contour_desc* cdesc, const vp_contour_buffers* cdev, int n_frames,
                                  vp_contour_geom* rows_out_host);
/* The plan of a pass over n_contours contours of n_points points, without a context: device workspace of the host-point form,
 * grid3 = blocks x, y and threads per block, *hull_cap = hull candidates a contour may have on the device.  Refuses what the
 * entries refuse: negative counts (VP_ERR_INVALID), more than 2^24 contours or 2^23 points (VP_ERR_UNSUPPORTED). */
int vp_contour_geometry_plan(int64_t n_contours, int64_t n_points, int want_hulls, uint64_t* ws_bytes, int32_t* grid3, int32_t* hull_cap);
/* The smallest enclosing circle of integer points within the coordinate bound (host code, no context): out3 = centre x, y, radius.
 * The single-contour form and the completion of VP_GEOM_HULL_CAP rows.  support7 (may be NULL): count and three (x, y). */
int vp_min_enclosing_circle_i32(const int32_t* pts, int npts, float* out3, int32_t* support7);

/* ---- detector pre / post-processing (BASELINE config 5) ----------------------
 * modules/yolo.py:112 `self.model.track(image)` hides these steps inside ultralytics (not in the reference tree, not
 * installed): LetterBox (scale to fit, centre, pad, BGR->RGB, HWC->CHW, /255) before the network, non-maximum suppression
 * after it.  Checked against plain PyTorch fp32 restatements; parity with the third-party package is unpinned.
 *
 * vp_letterbox_*: src (h,w,3) BGR uint8 -> dst (3,dst_h,dst_w) float32 RGB in [0,1]; the resize is cv2.resize INTER_LINEAR's
 * 8-bit arithmetic; geom_out (3 floats, may be NULL) = {scale r, left pad, top pad} for mapping boxes back.
 * vp_nms_*: boxes (n,4) x1,y1,x2,y2 (rotated: (n,5) x,y,w,h,angle[rad]), scores (n); keep_out receives up to max_keep original
 * indices in descending score order (ties: lower index first).  The order is total for any float32 scores: +inf first, -inf
 * last among the numbers, -0.0 == 0.0 a tie, every number before every NaN, NaNs among themselves by lower index; a NaN-scored
 * box is an ordinary candidate at the end of the order (kept if nothing suppresses it and max_keep allows).  rotated = 0:
 * greedy, suppress IoU > thr.  rotated = 1:
 * probabilistic IoU of the boxes' Gaussian models; a box is dropped when any higher-scored box overlaps it by >= thr.
 * n <= 16384 (VP_ERR_UNSUPPORTED above).  The _dev forms take device pointers (e.g. tensors of a PyTorch-ROCm model via data_ptr()), enqueue on the
 * context's stream and return without synchronising. */
/* cv2.threshold(src, thresh, maxval, type)[1] on 8-bit data of any channel count (utils/color.py:124-199: binary_threshold,
 * binary_threshold_inv, max_threshold, above_threshold, below_threshold): the comparison is against floor(thresh), maxval is
 * rounded and saturated.  n_bytes = h * w * channels of a tightly packed image; dst may equal src. */
enum { VP_THRESH_BINARY = 0, VP_THRESH_BINARY_INV = 1, VP_THRESH_TRUNC = 2, VP_THRESH_TOZERO = 3, VP_THRESH_TOZERO_INV = 4 };
int vp_threshold_u8(vp_ctx* ctx, const uint8_t* src_host, size_t n_bytes, double thresh, double maxval, int type, uint8_t* dst_host);
/* cv2.threshold(src, 0, maxval, type | THRESH_OTSU) on a single-channel 8-bit image (utils/color.py:204-217 otsu_threshold):
 * threshold chosen by getThreshVal_Otsu_8u from the histogram (device) with the reference's double-precision scan (host),
 * returned in *thresh_out, then applied as above. */
int vp_otsu_threshold_u8(vp_ctx* ctx, const uint8_t* src_host, size_t n_bytes, double maxval, int type, double* thresh_out, uint8_t* dst_host);
/* cv2.GaussianBlur(src, (kw, kh), sigma1, sigma2) on 8-bit images, cn = 1..4 (modules/preprocessor.py:110-114,
 * utils/transform.py simple_gaussian_blur): OpenCV's bit-exact fixed-point path (8.8 taps summing to 256, 16.16 vertical sums
 * rounded half up, BORDER_REFLECT_101).  kw, kh odd, 1..511; sigma <= 0 means "from the kernel size", sigma2 <= 0 means sigma1.
 * dst may equal src. */
int vp_gaussian_blur_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, int kw, int kh, double sigma1, double sigma2,
                        uint8_t* dst_host);
/* cv2.resize(src, (dst_w, dst_h)) with the default INTER_LINEAR on 8-bit images, cn = 1..4 interleaved channels
 * (modules/preprocessor.py:136-144): OpenCV's generic fixed-point path (scale = 1. / (dst / src) in double, the column table
 * clamped at the edges, the row weights not), including the 2x2 box average it substitutes at an exact halving.  (IPP-enabled
 * OpenCV builds may round differently.) */
int vp_resize_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, int dst_w, int dst_h, uint8_t* dst_host);
/* the same with cv::resize's inverse scales given, as cv2.resize(src, None, fx=inv_sx, fy=inv_sy) keeps them (the caller passes
 * dst_w = saturate_cast<int>(w * inv_sx), dst_h likewise).  Scale exactly 2 on both axes is OpenCV's area-fast path: supported when
 * w == 2 * dst_w and h == 2 * dst_h, VP_ERR_UNSUPPORTED otherwise (its partial edge cells are not reproduced). */
int vp_resize_u8_scaled(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, int dst_w, int dst_h, double inv_sx, double inv_sy,
                        uint8_t* dst_host);
/* cv2.adaptiveThreshold(src, max_value, ADAPTIVE_THRESH_MEAN_C, type, block_size, c) on a single-channel 8-bit image
 * (utils/color.py:220-254 adaptive_threshold_mean / adaptive_threshold_mean_inv).  type: VP_THRESH_BINARY or VP_THRESH_BINARY_INV;
 * block_size odd, 3..151 (the range in which OpenCV's three roundings of the box mean provably coincide).  dst may equal src. */
int vp_adaptive_threshold_mean_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, double max_value, int type, int block_size, double c,
                                  uint8_t* dst_host);
/* cv2.adaptiveThreshold(src, max_value, ADAPTIVE_THRESH_GAUSSIAN_C, type, block_size, c) on a single-channel 8-bit image
 * (utils/color.py:257-292 adaptive_threshold_gaussian / adaptive_threshold_gaussian_inv): mean = the exact weighted mean of
 * OpenCV's float32 taps getGaussianKernel(block_size, 0, CV_32F), separable, BORDER_REPLICATE, rounded half to even (a side of one
 * pixel takes the single tap 1.0, as BORDER_ISOLATED does); then the compare of the mean method.  block_size odd, 3..511 (larger:
 * VP_ERR_UNSUPPORTED); argument checks and error codes as vp_adaptive_threshold_mean_u8.  dst may equal src. */
int vp_adaptive_threshold_gaussian_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, double max_value, int type, int block_size,
                                      double c, uint8_t* dst_host);
/* the same on a device image (row stride src_stride bytes) into a packed (h, w) device image; enqueued on the context's stream.
 * dst must not overlap src.  Exception: the first call with a block size the context has not cached (8 sizes are kept, counting the
 * single tap of a one-pixel side) waits for the context's stream and uploads the taps synchronously; later calls do not wait. */
int vp_adaptive_threshold_gaussian_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, double max_value, int type,
                                       int block_size, double c, uint8_t* dst_dev);
/* n equal-shape device frames (frame f at src_dev + f * frame_stride) in one launch sequence into packed (n, h, w) dst_dev; waits on
 * a block size's first use as vp_adaptive_threshold_gaussian_dev does. */
int vp_adaptive_threshold_gaussian_batch_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, size_t frame_stride, int n, int w,
                                             int h, double max_value, int type, int block_size, double c, uint8_t* dst_dev);
/* cv2.Canny(image, threshold1, threshold2) with the default 3x3 aperture and L1 gradient on 8-bit images, cn = 1..4
 * (utils/feature.py:43-101 canny / simple_canny): Sobel derivatives, non-maximum suppression with OpenCV's integer direction test,
 * hysteresis as connected components of the surviving pixels that hold a pixel above the high threshold.  dst: (h, w) 0 / 255. */
int vp_canny_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, double threshold1, double threshold2, uint8_t* dst_host);
/* vp_canny_u8 on a device image (row stride src_stride bytes) into a packed device image; enqueued on the context's stream, not
 * synchronised, so that canny -> find_lines (utils/feature.py:43-66, :183-213) never leaves HBM. */
int vp_canny_u8_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, double threshold1, double threshold2,
                    uint8_t* dst_dev);
/* utils/feature.py:183-213 `find_lines` (cv2.HoughLines(image, rho, theta, threshold, srn=0, stn=0, min_theta, max_theta)): the
 * standard Hough transform of OpenCV 4.x HoughLinesStandard on a single-channel 8-bit image, non-zero = edge pixel.  Lines come back
 * as (rho, theta) float pairs in cv2's order (votes descending, then accumulator cell ascending); at most max_lines are written,
 * *n_lines is always the true count (a caller with too small a buffer learns the size it needs).  VP_ERR_INVALID for rho <= 0,
 * theta <= 0 or max_theta < min_theta; VP_ERR_UNSUPPORTED for accumulators above 2^28 cells.  Synchronises. */
int vp_hough_lines_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, double rho, double theta, int threshold, double min_theta,
                      double max_theta, float* lines_host, int max_lines, int* n_lines);
int vp_hough_lines_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, double rho, double theta, int threshold,
                       double min_theta, double max_theta, float* lines_host, int max_lines, int* n_lines);
/* n equal-shape device frames (frame f at src_dev + f * frame_stride) in one launch sequence: frame f's lines at
 * lines_host + 2 * f * max_lines, its true count in n_lines[f]. */
int vp_hough_lines_batch_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, size_t frame_stride, int n, int w, int h, double rho,
                             double theta, int threshold, double min_theta, double max_theta, float* lines_host, int max_lines,
                             int* n_lines);
/* utils/feature.py:128-155 `find_circles` (cv2.HoughCircles(image, cv2.HOUGH_GRADIENT, dp, minDist, None, param1, param2, minRadius,
 * maxRadius)): OpenCV 4.x HoughCirclesGradient on a single-channel 8-bit image.  cvRound(param1) is the upper Canny threshold (the lower
 * one max(1, half of it)), cvRound(param2) the vote and support threshold; minRadius below 0 counts as 0, maxRadius 0 as max(w, h), a
 * maxRadius <= minRadius as minRadius + 2; dp is clamped to >= 1.  Every edge pixel votes along its Sobel gradient in both directions,
 * centres are accumulator cells above the threshold that beat their neighbours, each centre's radius is the best-supported group of ten
 * 1/10-dp bins of the distances to the edge points, and circles are kept strongest first at >= min_dist from every kept one.  Circles
 * come back as (x, y, r) float triplets in cv2's order; at most max_circles are written, *n_circles is always the true count.
 * VP_ERR_INVALID for dp, min_dist, param1 or param2 <= 0 (or a non-finite dp); VP_ERR_UNSUPPORTED for max_radius < 0 (the
 * centres-only mode), images above 2^28 pixels, radii above 2^20 and param1 / param2 above 1e9 (range limits of this path; cv2 itself
 * accepts such values).  Synchronises. */
enum { VP_HOUGH_GRADIENT = 3 };
int vp_hough_circles_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, double dp, double min_dist, double param1, double param2,
                        int min_radius, int max_radius, float* circles_host, int max_circles, int* n_circles);
int vp_hough_circles_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, double dp, double min_dist, double param1,
                         double param2, int min_radius, int max_radius, float* circles_host, int max_circles, int* n_circles);
/* cv2.warpAffine(src, M, (dst_w, dst_h), flags, borderMode, borderValue) with bilinear interpolation on 8-bit images, cn = 1..4
 * (modules/preprocessor.py:130-135 rotate with BORDER_REPLICATE, :145-149 translate; utils/transform.py:180-210).  m23: the 2x3
 * matrix, row-major doubles, mapping source to destination unless VP_WARP_INVERSE_MAP is set.  OpenCV's classical fixed-point path
 * (every release up to 4.10): coordinates in 22.10 fixed point with 5 fractional bits kept, 15-bit weights, round half up.
 * border_value: cn bytes or NULL (0).  src and dst must not overlap. */
enum { VP_BORDER_CONSTANT = 0, VP_BORDER_REPLICATE = 1 };
enum { VP_WARP_INVERSE_MAP = 16 };
int vp_warp_affine_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, const double* m23, int flags, int border_mode,
                      const uint8_t* border_value, uint8_t* dst_host, int dst_w, int dst_h);
int vp_letterbox_u8_f32(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int dst_w, int dst_h, int pad_value, float* dst_host,
                        float* geom_out);
int vp_letterbox_dev(vp_ctx* ctx, const uint8_t* src_dev, int w, int h, int dst_w, int dst_h, int pad_value, float* dst_dev, float* geom_out);
int vp_nms_f32(vp_ctx* ctx, const float* boxes_host, const float* scores_host, int n, float thr, int rotated, int max_keep,
               int32_t* keep_out_host, int32_t* n_keep_out);
int vp_nms_dev(vp_ctx* ctx, const float* boxes_dev, const float* scores_dev, int n, float thr, int rotated, int max_keep,
               int32_t* keep_out_dev, int32_t* n_keep_dev);

/* ---- blur, resize, warp, thresholds, histogram and labelling on device images ------------------------------------------------ *
 * The device-resident forms of vp_gaussian_blur_u8, vp_resize_u8(_scaled), vp_warp_affine_u8, vp_threshold_u8, vp_otsu_threshold_u8,
 * vp_adaptive_threshold_mean_u8 and vp_ccl_u8: the same arithmetic, argument checks, limits and error codes (h <= 65535, odd kernels
 * up to 511, block sizes up to 151, ...), images are device pointers.  A source with a stride is read in place (row stride in bytes,
 * at least w * cn); results are tightly packed; dst must not overlap src (VP_ERR_INVALID).  Nothing is copied and nothing waits:
 * the kernels are enqueued on the context's stream and the call returns - except where a number has to come back, as said below.
 * Small parameters reach the device without a wait as well: the Gaussian taps through the context's pinned staging, the warp matrix
 * as kernel arguments.
 * vp_gaussian_blur_dev: kernels up to 31 x 31 may run as one launch (see VP_OPT_BLUR_ONEPASS); the result is the same either way.
 * vp_resize_dev: inv_sx, inv_sy as vp_resize_u8_scaled; both <= 0 means dst / src, as vp_resize_u8.
 * vp_otsu_threshold_dev: the histogram, getThreshVal_Otsu_8u (one lane of one wave, the doubles of the host form in the same order)
 * and the threshold are three launches with no synchronisation; the threshold chosen is left in *thresh_dev (a double in device
 * memory, may be NULL), for the caller to fetch when it wants the number.
 * vp_hist_u8_dev: the 256-bin histogram of n_bytes device bytes into hist_host (256 uint32); synchronises.
 * vp_ccl_dev / vp_ccl_bits_dev: vp_ccl_u8 on a device mask, or on the bit plane vp_inrange_u8_bits_dev left of it.  labels_dev
 * (nullable) is a packed (h, w) int32 device image and stays there; stats_host / centroids_host / n_labels are host memory as in
 * vp_ccl_u8; synchronises. */
int vp_gaussian_blur_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, int kw, int kh, double sigma1,
                         double sigma2, uint8_t* dst_dev);
int vp_resize_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, int dst_w, int dst_h, double inv_sx,
                  double inv_sy, uint8_t* dst_dev);
int vp_warp_affine_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, const double* m23, int flags,
                       int border_mode, const uint8_t* border_value, uint8_t* dst_dev, int dst_w, int dst_h);
int vp_threshold_u8_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t n_bytes, double thresh, double maxval, int type, uint8_t* dst_dev);
int vp_otsu_threshold_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t n_bytes, double maxval, int type, double* thresh_dev,
                          uint8_t* dst_dev);
int vp_adaptive_threshold_mean_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, double max_value, int type,
                                   int block_size, double c, uint8_t* dst_dev);
int vp_hist_u8_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t n_bytes, uint32_t* hist_host);
int vp_ccl_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int numbering, int32_t* labels_dev,
               int32_t* stats_host, double* centroids_host, int max_labels, int32_t* n_labels);
int vp_ccl_bits_dev(vp_ctx* ctx, const unsigned long long* bits_dev, int w, int h, int numbering, int32_t* labels_dev,
                    int32_t* stats_host, double* centroids_host, int max_labels, int32_t* n_labels);

/* ---- remap, convertMaps and warpPerspective -------------------------------------------------------------------------------------- *
 * cv2.remap(src, map1, map2, interpolation, borderMode, borderValue), cv2.convertMaps and cv2.warpPerspective on 8-bit images of
 * cn = 1..4 channels, OpenCV's classical fixed-point path (every release up to 4.10): every source
 * coordinate becomes an int16 integer part and a 5 + 5 bit fraction index fy * 32 + fx, and a linear sample is the 15-bit bilinear
 * blend of vp_warp_affine_u8.  interp: VP_INTER_NEAREST or VP_INTER_LINEAR; border_mode: VP_BORDER_CONSTANT (border_value: cn bytes,
 * NULL = 0) or VP_BORDER_REPLICATE.  The destination has the maps' size (map_w x map_h), packed; the source is w x h, each at most
 * 32767 as cv2 asserts; map_h <= 65535, map_w <= 2^24 and map_w * map_h < 2^31.  Map planes need only their
 * element's alignment; 16-byte aligned planes and rows of a multiple of four pixels take the wide loads and stores.
 * Maps: float32, as two planes (mapx, mapy) or as one plane of interleaved (x, y) pairs (mapy NULL); or the fixed form: xy, int16
 * (x, y) pairs, plus frac, uint16 fraction indices (only the low 10 bits are read).  Nearest takes xy alone: frac must be NULL then.
 * Float map values must be finite with |v| * 32 < 2^31; what a NaN or a larger value gives is cv2's x86 cvRound behaviour and is
 * not promised.  vp_convert_maps_dev turns float maps into the fixed form (nearest != 0: xy_out holds the rounded coordinates and
 * frac_out must be NULL); remapping from its result gives the bytes vp_remap_f32_dev gives from the float maps.
 * vp_warp_perspective_*: m33 is the 3x3 matrix, row-major doubles, mapping source to destination unless flags has
 * VP_WARP_INVERSE_MAP; flags also carries the interpolation (VP_INTER_NEAREST or VP_INTER_LINEAR).  The matrix and the border value
 * travel as kernel arguments.
 * The _dev entries copy nothing and wait for nothing: one launch on the context's stream.  vp_remap_u8 and vp_warp_perspective_u8
 * stage host operands (float maps) and synchronise.  VP_ERR_INVALID before anything is launched: null pointers, cn outside 1..4,
 * non-positive or oversized dimensions, an unknown interpolation or border, src_stride < w * cn, a destination that overlaps the
 * source or a map, nearest together with a fraction plane, linear without one, a matrix that is not finite. */
enum { VP_INTER_NEAREST = 0, VP_INTER_LINEAR = 1 };
int vp_convert_maps_dev(vp_ctx* ctx, const float* mapx_dev, const float* mapy_dev, int map_w, int map_h, int nearest, int16_t* xy_out_dev,
                        uint16_t* frac_out_dev);
int vp_remap_fixed_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, const int16_t* xy_dev,
                       const uint16_t* frac_dev, int map_w, int map_h, int interp, int border_mode, const uint8_t* border_value,
                       uint8_t* dst_dev);
int vp_remap_f32_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, const float* mapx_dev,
                     const float* mapy_dev, int map_w, int map_h, int interp, int border_mode, const uint8_t* border_value, uint8_t* dst_dev);
int vp_remap_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, const float* mapx_host, const float* mapy_host, int map_w,
                int map_h, int interp, int border_mode, const uint8_t* border_value, uint8_t* dst_host);
int vp_warp_perspective_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, const double* m33, int flags, int border_mode,
                           const uint8_t* border_value, uint8_t* dst_host, int dst_w, int dst_h);
int vp_warp_perspective_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, const double* m33, int flags,
                            int border_mode, const uint8_t* border_value, uint8_t* dst_dev, int dst_w, int dst_h);

/* ---- histogram equalisation and CLAHE ------------------------------------------------------------------------------------------------ *
 * cv2.equalizeHist and cv2.createCLAHE(clip_limit, (tiles_x, tiles_y)).apply on 8-bit single-channel images, byte for byte (DESIGN.md
 * section 4 has the arithmetic: integer histograms, one float32 multiply per table entry, and for CLAHE a float32 bilinear blend of
 * four table entries per pixel in OpenCV's order, no product fused with a sum).
 * vp_equalize_hist_u8 / vp_clahe_u8: packed host images; stage, run the kernels of the device form and synchronise.
 * vp_equalize_hist_dev / vp_clahe_dev: src_dev is read in place (row stride in bytes, at least w), dst_dev is packed and must not
 *   overlap it; enqueued on the context's stream, never synchronise.  equalizeHist is three launches (histogram, table, table-apply).
 * CLAHE cuts tiles_x x tiles_y tiles from the image, extended right by tiles_x - w % tiles_x and down by tiles_y - h % tiles_y with
 *   BORDER_REFLECT_101 whenever EITHER dimension fails to divide (so a dimension that does divide grows by a whole tile count, as in
 *   OpenCV).  clip_limit <= 0 switches clipping off; otherwise the limit per bin is max(int(clip_limit * tile_area / 256), 1).
 * VP_ERR_INVALID, with nothing launched or written: NULL pointers, w or h <= 0, src_stride < w, dst overlapping src in the device
 *   forms, tiles_x or tiles_y < 1, a NaN clip_limit.  VP_ERR_UNSUPPORTED: tiles_x or tiles_y > 64, more than 2^28 pixels, an extension
 *   that is not smaller than the dimension it reflects (only a single reflection is reproduced), clip_limit * tile_area / 256 >= 2^31
 *   (OpenCV's cast is undefined there).  See VP_OPT_CLAHE_SPLIT for the dispatch of the tile histograms. */
int vp_equalize_hist_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, uint8_t* dst_host);
int vp_equalize_hist_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, uint8_t* dst_dev);
int vp_clahe_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, double clip_limit, int tiles_x, int tiles_y, uint8_t* dst_host);
int vp_clahe_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, double clip_limit, int tiles_x, int tiles_y,
                 uint8_t* dst_dev);

/* ---- median filter ------------------------------------------------------------------------------------------------------------------ *
 * cv2.medianBlur on uint8 images of 1..4 interleaved channels: dst[y][x][c] is the median of the ksize x ksize window of channel c
 * centred on (x, y), coordinates outside the image clamped to the nearest edge pixel (BORDER_REPLICATE).  ksize is odd, 1..255
 * (1 copies); h <= 65535.  An order statistic: nothing is rounded, the result equals OpenCV's on every code path of its own.
 * vp_median_blur_u8: packed host images; stages, runs the kernels of the device form and synchronises.
 * vp_median_blur_dev: src_dev is read in place (row stride in bytes, at least w * cn), dst_dev is packed and must not overlap it
 *   (VP_ERR_INVALID, nothing is launched); enqueued on the context's stream, never synchronises.  binary_hint != 0 is the caller's
 *   promise that src holds only 0 and 255, as for vp_morph_u8_dev: a single-channel mask with ksize <= 63 is then filtered as a
 *   majority vote on bits (see VP_OPT_MEDIAN_MASK).  src_bits_dev (nullable): the mask's bit plane in the layout of
 *   vp_inrange_u8_bits_dev / vp_bitwise_u8_dev ((w + 63) / 64 words per row, bit x % 64 of word x / 64 is pixel x), read instead of
 *   the bytes.  dst_bits_dev (nullable): receives the result's bit plane when the mask kernel ran and w % 64 == 0; *made_bits
 *   (nullable) says whether it did, and is left untouched when the call fails.  The planes are 8-byte aligned and overlap neither
 *   image nor each other. */
int vp_median_blur_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, int ksize, uint8_t* dst_host);
int vp_median_blur_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, int ksize, int binary_hint,
                       const unsigned long long* src_bits_dev, uint8_t* dst_dev, unsigned long long* dst_bits_dev, int* made_bits);

/* ---- derivative filters -------------------------------------------------------------------------------------------------------------- *
 * cv2.Sobel / Scharr / Laplacian / spatialGradient on uint8 images of 1..4 interleaved channels with scale = 1 and delta = 0:
 * dst[y][x][c] = saturate_cast<ddepth>(the integer correlation of channel c of the border-extended image with the operator's
 * unnormalised integer kernel).  uint8 clamps to [0, 255], int16 to [-32768, 32767], float and double hold the integer exactly, so the
 * result equals OpenCV's on every code path of its own (tests/deriv_restate.py is the statement).
 * op: VP_DERIV_SOBEL with dx, dy in 0..2, dx + dy > 0, ksize 3, 5 or 7 above both orders (the taps of cv::getDerivKernels), ksize 1
 *   ([-1 0 1] or [1 -2 1] along a differentiated axis, [1] along the other) or ksize -1 = Scharr; VP_DERIV_SCHARR with dx + dy == 1
 *   ([-1 0 1] with [3 10 3]; ksize is ignored); VP_DERIV_LAPLACIAN with ksize 1 ([[0 1 0],[1 -4 1],[0 1 0]]), 3 ([[2 0 2],[0 -8 0],
 *   [2 0 2]]), 5 or 7 (Sobel(2, 0, ksize) + Sobel(0, 2, ksize); dx, dy are ignored).
 * ddepth: -1 or VP_DEPTH_8U, VP_DEPTH_16S, VP_DEPTH_32F, VP_DEPTH_64F (cv2's CV_8U, CV_16S, CV_32F, CV_64F).
 * border: VP_BORDER_REFLECT_101 (cv2's default), VP_BORDER_REPLICATE, VP_BORDER_REFLECT, VP_BORDER_CONSTANT (value 0); the
 *   VP_BORDER_ISOLATED bit is ignored; index maps as cv::borderInterpolate, also for images narrower than the kernel's radius.
 * h <= 65535.  Anything else is VP_ERR_INVALID and nothing is launched or written.
 * vp_deriv_u8 / vp_spatial_gradient_u8: packed host images; stage, run the kernel of the device form and synchronise.
 * vp_deriv_dev / vp_spatial_gradient_dev: src_dev is read in place (row stride in bytes, at least w * cn, no alignment asked of
 *   pointer or stride), dst_dev is packed (w * cn elements of ddepth per row), aligned to its element size, and must not overlap the
 *   source; enqueued on the context's stream, never synchronise.
 * vp_spatial_gradient_*: single channel, ksize 3, VP_BORDER_REFLECT_101 or VP_BORDER_REPLICATE, as cv2; dx = Sobel(1, 0, 3) and
 *   dy = Sobel(0, 1, 3), both int16, from one pass over the source.
 * vp_convert_scale_abs_*: cv2.convertScaleAbs with alpha = 1, beta = 0 on n elements of depth VP_DEPTH_8U / 16S / 32F / 64F:
 *   dst[i] = saturate_cast<uchar>(|src[i]|); a float source is rounded half to even before the clamp (NaN gives 0).  src is aligned
 *   to its element size and does not overlap dst. */
enum { VP_DERIV_SOBEL = 0, VP_DERIV_SCHARR = 1, VP_DERIV_LAPLACIAN = 2 };
enum { VP_DEPTH_8U = 0, VP_DEPTH_16S = 3, VP_DEPTH_32F = 5, VP_DEPTH_64F = 6 };
enum { VP_BORDER_REFLECT = 2, VP_BORDER_REFLECT_101 = 4, VP_BORDER_ISOLATED = 16 };      /* with VP_BORDER_CONSTANT = 0, VP_BORDER_REPLICATE = 1 */
int vp_deriv_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, int op, int dx, int dy, int ksize, int ddepth, int border,
                void* dst_host);
int vp_deriv_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, int op, int dx, int dy, int ksize, int ddepth,
                 int border, void* dst_dev);
int vp_spatial_gradient_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int ksize, int border, int16_t* dx_host, int16_t* dy_host);
int vp_spatial_gradient_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int ksize, int border, int16_t* dx_dev,
                            int16_t* dy_dev);
int vp_convert_scale_abs_u8(vp_ctx* ctx, const void* src_host, int depth, size_t n, uint8_t* dst_host);
int vp_convert_scale_abs_dev(vp_ctx* ctx, const void* src_dev, int depth, size_t n, uint8_t* dst_dev);

/* ---- box filter, pyramid steps, integral image ----------------------------------------------------------------------------------------- *
 * cv2.boxFilter / blur, pyrDown, pyrUp and integral on uint8 images of 1..4 interleaved channels, pure integer arithmetic
 * (tests/box_pyr_restate.py is the statement).  Borders are codes of VP_BORDER_* (the VP_BORDER_ISOLATED bit is ignored), index maps
 * as cv::borderInterpolate, also for windows larger than the image.  Host forms (_u8) take packed host images, stage, run the kernels
 * of the device form and synchronise; device forms (_dev) read src_dev in place (row stride in bytes, at least w * cn, no alignment
 * asked of pointer or stride), write a packed dst_dev aligned to its element size that must not overlap the source, enqueue on the
 * context's stream and never synchronise.  Anything refused is VP_ERR_INVALID with a message, and nothing is launched or written.
 * vp_box_filter_*: the sum over the kh x kw window (1..255 each) anchored at (kw / 2, kh / 2), also for even sizes.  border:
 *   VP_BORDER_REFLECT_101, REPLICATE, REFLECT or CONSTANT (value 0).  normalize == 0: the sum cast to ddepth -1 / VP_DEPTH_8U or
 *   VP_DEPTH_16S (saturated), VP_DEPTH_32S, VP_DEPTH_32F (only while 255 * kw * kh < 2^24) or VP_DEPTH_64F.  normalize != 0: ddepth -1
 *   or VP_DEPTH_8U only, and only areas kw * kh that vp_box_area_exact admits; the result is sum / area rounded half to even.  h <= 65535.
 * vp_box_area_exact: 1 when OpenCV's three roundings of sum / area (the Q23 reciprocal on 16-bit sums for area <= 256, the float32
 *   and the double product otherwise) give one byte for every sum 0 .. 255 * area, 0 when not, negative for area < 1 or above
 *   255 * 255.  Host only, no context, no GPU; enumerates once per area and remembers.
 * vp_pyr_down_*: dst is ((w + 1) / 2) x ((h + 1) / 2); the 5 x 5 kernel [1 4 6 4 1] x [1 4 6 4 1] at every second pixel, (.. + 128) >> 8.
 *   border: VP_BORDER_REFLECT_101, REPLICATE or REFLECT (cv2 refuses CONSTANT).  h <= 32767.
 * vp_pyr_up_*: dst is 2w x 2h; cv2's polyphase form of the same kernel times 4, (.. + 32) >> 6, BORDER_DEFAULT only.  h <= 32767.
 * vp_integral_*: dst is (h + 1) x (w + 1) x cn int32 with a zero first row and column; 255 * w * h must fit int32. */
enum { VP_DEPTH_32S = 4 };
int vp_box_area_exact(int area);
int vp_box_filter_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, int kw, int kh, int normalize, int ddepth, int border,
                     void* dst_host);
int vp_box_filter_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, int kw, int kh, int normalize, int ddepth,
                      int border, void* dst_dev);
int vp_pyr_down_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, int border, uint8_t* dst_host);
int vp_pyr_down_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, int border, uint8_t* dst_dev);
int vp_pyr_up_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, uint8_t* dst_host);
int vp_pyr_up_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, uint8_t* dst_dev);
int vp_integral_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, int32_t* dst_host);
int vp_integral_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t src_stride, int w, int h, int cn, int32_t* dst_dev);

/* ---- element-wise operators on device images ------------------------------------------------------------------------------------ *
 * Packed uint8 device images; every entry enqueues on the context's stream and returns at once, except vp_count_nonzero_u8_dev.
 * Pointers need no alignment (planes of one frame sit at byte offsets inside one allocation): 16-byte accesses are used where the
 * pointers allow them, byte accesses elsewhere.  n_bytes / n_px at most 2^40.
 * vp_bitwise_u8_dev: cv2.bitwise_and / _or / _xor / _not (op: VP_BITWISE_*) on n_bytes bytes.  The second operand is the image b_dev
 *   or, when b_dev is NULL, the byte `scalar` (0..255); VP_BITWISE_NOT reads a_dev alone.  mask_dev (nullable): one byte per pixel of
 *   an image of cn channels (1..4; n_bytes a multiple of cn) - where it is 0 the result is 0, as cv2 leaves a fresh dst.  dst_dev may
 *   be a_dev or b_dev (not a partial overlap).  bits_dev (nullable) with bits_w > 0: the caller states that the result is a 0/255
 *   mask of rows of bits_w pixels (cn == 1) and takes its bit-packed form from the same launch - layout and conditions of
 *   vp_inrange_u8_bits_dev (bits_w % 64 == 0, dst_dev and bits_dev 16-B aligned); *made_bits (nullable) says whether it was written.
 * vp_arith_u8_dev: cv2.add / subtract / absdiff (op: VP_ARITH_*) of two images, saturated to 0..255; dst_dev may be a source.
 * vp_lut_u8_dev: dst[p, c] = lut_host[c * 256 + src[p, c]] for cn (1..4) interleaved channels; lut_host: cn * 256 bytes of host
 *   memory, read before the call returns (the tables travel as kernel arguments).  Image-with-scalar arithmetic is a table.
 * vp_split_u8_dev / vp_merge_u8_dev: n_px pixels of cn (2..4) interleaved channels to / from cn planes (plane c at pc_dev; the planes
 *   beyond cn are ignored).  Source and destination must not overlap.  vp_split_u8_dev skips a plane whose pointer is NULL
 *   (cv2.extractChannel: one plane), at least one must be given.
 * vp_count_nonzero_u8_dev: cv2.countNonZero of n_bytes bytes into *count_host; synchronises. */
enum { VP_BITWISE_AND = 0, VP_BITWISE_OR = 1, VP_BITWISE_XOR = 2, VP_BITWISE_NOT = 3 };
enum { VP_ARITH_ADD = 0, VP_ARITH_SUB = 1, VP_ARITH_ABSDIFF = 2 };
int vp_bitwise_u8_dev(vp_ctx* ctx, int op, const uint8_t* a_dev, const uint8_t* b_dev, int scalar, const uint8_t* mask_dev, int cn,
                      size_t n_bytes, uint8_t* dst_dev, int bits_w, unsigned long long* bits_dev, int* made_bits);
int vp_arith_u8_dev(vp_ctx* ctx, int op, const uint8_t* a_dev, const uint8_t* b_dev, size_t n_bytes, uint8_t* dst_dev);
int vp_lut_u8_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t n_bytes, int cn, const uint8_t* lut_host, uint8_t* dst_dev);
int vp_split_u8_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t n_px, int cn, uint8_t* p0_dev, uint8_t* p1_dev, uint8_t* p2_dev,
                    uint8_t* p3_dev);
int vp_merge_u8_dev(vp_ctx* ctx, const uint8_t* p0_dev, const uint8_t* p1_dev, const uint8_t* p2_dev, const uint8_t* p3_dev, size_t n_px,
                    int cn, uint8_t* dst_dev);
int vp_count_nonzero_u8_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t n_bytes, uint64_t* count_host);

/* ---- moments: cv2.moments and cv2.HuMoments --------------------------------------------------------------------------------------- *
 * Order everywhere, cv::Moments': m00 m10 m01 m20 m11 m02 m30 m21 m12 m03, m_pq = sum x^p y^q v, x the column, y the row.
 * vp_moments_u8 / vp_moments_dev: the ten sums of a uint8 image as exact integers into out10_host, v the pixel value, or 1 for a
 *   non-zero pixel when `binary` is set (cv2's binaryImage).  One pass at one byte per pixel; the source is read in place with any row
 *   stride (bytes, at least w) and any pointer alignment.  bits_dev (nullable, `binary` only): the mask's bit plane in the layout of
 *   vp_inrange_u8_bits_dev ((w + 63) / 64 words per row, bit x % 64 of word x / 64 is pixel x; bits past w are ignored), read instead
 *   of the bytes - src_dev may then be NULL.  The host form stages the image; both synchronise.
 * vp_label_moments_i32 / vp_label_moments_dev: the same ten sums with v = 1 for every label value 0 .. nlabels - 1 of an int32 label
 *   image (row stride in bytes, a multiple of 4, at least 4 w) into out_host, (nlabels, 10) uint64; row 0 is the background, as in
 *   cv2.connectedComponentsWithStats.  A label outside that range counts nowhere.  One pass at four bytes per pixel; see
 *   VP_OPT_LABEL_MOMENTS_LDS.  Both synchronise.
 * Refused with VP_ERR_INVALID before anything is launched (the message names the reason): w or h below 1, h > 65535, a stride below
 *   the row, nlabels < 1, a binary bit plane without `binary`, and sizes whose worst-case m30 or m03 - 255 (1 when binary, and for
 *   labels) * h * sum_{x < w} x^3, and the transpose - reaches 2^63.  Below that bound no sum wraps; cv2's doubles are exact only below
 *   2^53, where the two agree (a binary 1080p mask is far below).
 * vp_polygon_moments: cv2.moments of a contour of n points, int32 or float32 (x, y) pairs - contourMoments' float64 loop in its
 *   operation order, out10 = the ten spatial moments; all zero for n = 0 or |a00| <= FLT_EPSILON.  Host code, no context.
 * vp_moments_complete: completeMomentState - out24 = the ten spatial moments, mu20 mu11 mu02 mu30 mu21 mu12 mu03 and nu20 .. nu03, the
 *   order of cv2's dictionary.  Host code, no context.  Both are compiled without contraction: the doubles are OpenCV's bit for bit. */
int vp_moments_u8(vp_ctx* ctx, const uint8_t* src_host, size_t stride, int w, int h, int binary, uint64_t* out10_host);
int vp_moments_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t stride, int w, int h, int binary, const unsigned long long* bits_dev,
                   uint64_t* out10_host);
int vp_label_moments_i32(vp_ctx* ctx, const int32_t* labels_host, size_t stride, int w, int h, int nlabels, uint64_t* out_host);
int vp_label_moments_dev(vp_ctx* ctx, const int32_t* labels_dev, size_t stride, int w, int h, int nlabels, uint64_t* out_host);
int vp_polygon_moments(const void* pts, int is_float32, int n, double* out10);
int vp_moments_complete(const double* m10, double* out24);

/* ---- corners: cv2.cornerMinEigenVal, cv2.cornerHarris and cv2.goodFeaturesToTrack ------------------------------------------------- *
 * On uint8 single-channel images with the 3x3 Sobel (ksize 3).  OpenCV's float32 code is not restated; what it approximates is
 * (tests/corners_restate.py): Dx, Dy the integer Sobel derivatives under `border`; Sxx, Sxy, Syy the
 * unnormalised block_size x block_size box sums (anchor block_size / 2) of Dx Dx, Dx Dy, Dy Dy, the same border applied to the
 * product image - all exact in int32; then in IEEE double, in this order, s = 1 / (4 block_size 255):
 *   harris 0: a = Sxx 0.5, b = Sxy, c = Syy 0.5, response = (float)(((a + c) - sqrt((a - c)(a - c) + b b)) (s s))
 *   harris 1: a = Sxx, b = Sxy, c = Syy, response = (float)(((a c - b b) - k ((a + c)(a + c))) ((s s)(s s)))
 * vp_corner_response_u8 / vp_corner_response_dev: the float32 map, packed, from a source of any row stride (bytes, at least w) and
 *   pointer alignment.  border: VP_BORDER_REFLECT_101 (cv2's default), REPLICATE, REFLECT or CONSTANT (the ISOLATED bit is ignored).
 *   The host form stages the image and synchronises; the device form enqueues one launch and never synchronises, dst_dev must be
 *   4-byte aligned and must not overlap the source.
 * vp_good_features_u8 / vp_good_features_dev: goodFeaturesToTrack's selection on that map (border REFLECT_101).  The maximum is taken
 *   over the pixels where the mask (nullable; mask_w x mask_h bytes, rows of mask_stride) is non-zero; t = (float)((double)max *
 *   quality_level); a candidate is an interior pixel (1 <= x <= w - 2, 1 <= y <= h - 2) admitted by the mask with response > t, != 0
 *   and >= every one of its eight neighbours that is > t; candidates are ordered by response descending, equal responses by larger
 *   y w + x first, and kept greedily: dropped when a kept corner lies at dx dx + dy dy < min_distance^2, until max_corners > 0 are
 *   kept (max_corners <= 0: all).  corners_host receives the first `capacity` (x, y) float32 pairs, *n_corners the true count: a
 *   caller with too small a buffer learns the size it needs.  mask_bits_dev (nullable): the mask's bit plane in the layout of
 *   vp_inrange_u8_bits_dev, read instead of its bytes.  Images with w < 3 or h < 3 give 0.  Both synchronise.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing pointer, w or h below
 *   1 or above 65535, more than 2^28 pixels, a stride below the row, block_size outside 1..31, ksize != 3, an unsupported border, a
 *   k that is not finite, quality_level <= 0 or not finite, min_distance < 0 or NaN, a negative capacity, a mask whose size differs
 *   from the image's or whose stride is below its row. */
int vp_corner_response_u8(vp_ctx* ctx, const uint8_t* src_host, size_t stride, int w, int h, int block_size, int ksize, int harris, double k, int border,
                          float* dst_host);
int vp_corner_response_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t stride, int w, int h, int block_size, int ksize, int harris, double k, int border,
                           float* dst_dev);
int vp_good_features_u8(vp_ctx* ctx, const uint8_t* src_host, size_t stride, int w, int h, int max_corners, double quality_level, double min_distance,
                        const uint8_t* mask_host, size_t mask_stride, int mask_w, int mask_h, int block_size, int harris, double k, float* corners_host,
                        int capacity, int* n_corners);
int vp_good_features_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t stride, int w, int h, int max_corners, double quality_level, double min_distance,
                         const uint8_t* mask_dev, size_t mask_stride, int mask_w, int mask_h, const unsigned long long* mask_bits_dev, int block_size,
                         int harris, double k, float* corners_host, int capacity, int* n_corners);

/* ---- distances: cv2.distanceTransform (DIST_L2 with DIST_MASK_PRECISE, DIST_L1, DIST_C) and cv2.minMaxLoc ------------------------- *
 * vp_distance_transform_u8 / vp_distance_transform_dev: zero pixels of the uint8 source are the sources; every pixel gets its distance
 *   to the nearest one (tests/dist_restate.py).  metric VP_DIST_L2: sqrtf((float)D2), D2 the minimum of
 *   dx dx + dy dy in integers, the root correctly rounded; VP_DIST_L1: |dx| + |dy|; VP_DIST_C: max(|dx|, |dy|).  dst_depth VP_DEPTH_32F,
 *   or VP_DEPTH_8U with VP_DIST_L1 only: min(d, 255).  An image without a zero pixel gives +inf everywhere (255 for VP_DEPTH_8U).
 *   The host form takes a packed image, gives a packed result and synchronises.  The device form reads rows of `stride` bytes and
 *   writes rows of dst_stride bytes, enqueues two launches and never synchronises; src_bits_dev (nullable) is the source's bit plane
 *   in the layout of vp_inrange_u8_bits_dev, read instead of its bytes - its bits past w are not looked at.
 * vp_min_max_loc_u8 / vp_min_max_loc_dev: cv2.minMaxLoc of a single-channel image of depth VP_DEPTH_8U or VP_DEPTH_32F, rows of
 *   `stride` bytes.  out receives struct { double min_val, max_val; int min_x, min_y, max_x, max_y; } (host memory).  Among equal
 *   values the first pixel in raster order wins at both ends.  Only pixels where the mask (nullable; mask_w x mask_h bytes, rows of
 *   mask_stride) is non-zero take part; mask_bits_dev (nullable) is the mask's bit plane, read instead of its bytes.  NaN pixels take
 *   no part; +inf and -inf order as numbers.  When no pixel takes part: (0, 0, (-1, -1), (-1, -1)).  Both synchronise.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing pointer, a bit plane
 *   without its source, w or h outside 1..4096, a stride below the row, a result or float32 stride that is not a multiple of the
 *   element size, an unknown metric, VP_DEPTH_8U with anything but VP_DIST_L1, a depth other than 8U or 32F, a mask whose size differs
 *   from the image's or whose stride is below its row, a result that overlaps the source. */
enum { VP_DIST_L1 = 1, VP_DIST_L2 = 2, VP_DIST_C = 3 };
int vp_distance_transform_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int metric, int dst_depth, void* dst_host);
int vp_distance_transform_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t stride, int w, int h, const unsigned long long* src_bits_dev, int metric,
                              int dst_depth, void* dst_dev, size_t dst_stride);
int vp_min_max_loc_u8(vp_ctx* ctx, const void* src_host, size_t stride, int w, int h, int depth, const uint8_t* mask_host, size_t mask_stride, int mask_w,
                      int mask_h, void* out_host);
int vp_min_max_loc_dev(vp_ctx* ctx, const void* src_dev, size_t stride, int w, int h, int depth, const uint8_t* mask_dev, size_t mask_stride, int mask_w,
                       int mask_h, const unsigned long long* mask_bits_dev, void* out_host);

/* ---- colour k-means (utils/color.py `kmeans`, cv2.kmeans) and the masks of a label image ------------------------------------------ *
 * vp_kmeans_u8 / vp_kmeans_dev: clusters the pixels of a uint8 image of cn = 1..4 channels (w, h <= 4096, so N = w h <= 2^24) around
 *   k = 1..256 centres (k <= N), as DESIGN.md section 4.26 and tests/kmeans_restate.py state it: a pixel goes to the centre with the
 *   smallest sum over the channels of (double(p) - double(c))^2, the lowest index on ties; n, S1 = sum p and S2 = sum p^2 of every
 *   cluster are exact integers; a centre moves to float32(double(S1) / double(n)), an empty cluster keeps its centre; the loop stops
 *   after max_iter (1..100) assign passes, or with the pass after the largest squared shift of a centre fell to eps^2 or below.
 *   The initial centres are centers_init (k * cn finite floats) or the pixels at the k raster indices seed_index (0..N-1): host
 *   arrays, exactly one of them given.  labels (nullable): int32 (h, w), the index of every pixel's centre among the returned ones.
 *   out_host receives struct { double compactness; int32_t iterations; int32_t k; float centers[k * cn]; uint32_t counts[k]; }
 *   (host memory): the sum of squared distances of the last pass - computed on the host from its exact sums, the same bits on
 *   every run -, the assign passes that ran, k, the centres, and the pixels of every cluster.
 *   The host form takes a packed image and gives packed labels.  The device form reads rows of `stride` bytes and writes label rows
 *   of labels_stride bytes; it enqueues the whole loop without visiting the host and synchronises once, at the end, to hand the
 *   table back.
 * vp_label_select_dev: mask = 255 where select_host[label] != 0, else 0, for int32 labels (rows of labels_stride bytes); select_host
 *   holds k bytes; a label outside 0..k-1 gives 0.  mask_bits_dev (nullable): when w % 64 == 0 the mask's bit plane is written as
 *   well, in the layout of vp_inrange_u8_bits_dev (h * w / 64 words); with any other width it is left alone.  One launch, never
 *   synchronises.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing pointer, w or h
 *   outside 1..4096, cn outside 1..4, k outside 1..256 or above w h, both or neither of the initialisers, an initial centre that is
 *   not finite, a seed index outside 0..N-1, max_iter outside 1..100, eps negative or not finite, a stride below the row, a label
 *   stride below the row or not a multiple of 4, labels that are not 4-byte aligned, a bit plane that is not 8-byte aligned, labels
 *   that overlap the source (a mask that overlaps the labels). */
enum { VP_KMEANS_MAX_K = 256, VP_KMEANS_MAX_ITER = 100 };
int vp_kmeans_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, int k, const float* centers_init, const int32_t* seed_index, int max_iter,
                 double eps, int32_t* labels_host, void* out_host);
int vp_kmeans_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t stride, int w, int h, int cn, int k, const float* centers_init, const int32_t* seed_index,
                  int max_iter, double eps, int32_t* labels_dev, size_t labels_stride, void* out_host);
int vp_label_select_dev(vp_ctx* ctx, const int32_t* labels_dev, size_t labels_stride, int w, int h, const uint8_t* select_host, int k, uint8_t* mask_dev,
                        size_t mask_stride, unsigned long long* mask_bits_dev);

/* ---- template matching: cv2.matchTemplate, the six TM_* methods ------------------------------------------------------------------- *
 * vp_match_template_u8 / vp_match_template_dev: slides a uint8 template of tw x th pixels over a uint8 image of w x h pixels, both of
 *   cn = 1..4 channels, and gives the float32 map of (h - th + 1) x (w - tw + 1) scores as DESIGN.md section 4.27 and
 *   tests/match_template_restate.py state it.  Per result pixel C = sum I T, S2 = sum I^2 and S1_c = sum I per channel, over the window
 *   and all channels, are exact integers; the steps after them are cv2's (templmatch.cpp common_matchTemplate) in double arithmetic,
 *   in one fixed order, rounded to float32 once.  cv2 computes C by a float32 DFT: its values approximate these.
 *   The host form takes packed images, gives a packed result and synchronises.  The device form reads rows of `stride` and
 *   templ_stride bytes (a template may be a window of another device image), writes rows of dst_stride bytes, enqueues two to four
 *   launches and never synchronises.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing pointer, w or h outside
 *   1..4096, cn outside 1..4, a template without pixels or larger than the image, tw * th * cn above 65536, an unknown method, a
 *   stride below its row, a result stride that is not a multiple of 4, a result that is not 4-byte aligned or overlaps an input. */
enum { VP_TM_SQDIFF = 0, VP_TM_SQDIFF_NORMED = 1, VP_TM_CCORR = 2, VP_TM_CCORR_NORMED = 3, VP_TM_CCOEFF = 4, VP_TM_CCOEFF_NORMED = 5 };
int vp_match_template_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, const uint8_t* templ_host, int tw, int th, int method, float* dst_host);
int vp_match_template_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t stride, int w, int h, int cn, const uint8_t* templ_dev, size_t templ_stride, int tw, int th,
                          int method, float* dst_dev, size_t dst_stride);

/* ---- colour-histogram tracking: cv2.calcHist, cv2.calcBackProject, cv2.meanShift -------------------------------------------------- *
 * DESIGN.md section 4.28 and tests/hist_restate.py state all of it.  An image is uint8 of cn = 1..4 interleaved channels, w, h <= 4096.
 * A histogram is described by dims = 1..3, a channel index per dimension, hist_size[d] = 1..256 bins and ranges[2 d], ranges[2 d + 1] =
 * (low, high) per dimension - host arrays.  As in cv2's calcHistLookupTables_8u, a = hist_size / (high - low) and b = -a * low in
 * double, byte value j falls into bin floor(j * a + b), and a pixel with a bin outside [0, hist_size) in any dimension takes no part:
 * the upper end of a range is exclusive.  The first dimension is the slowest, like a C array.
 * vp_calc_hist_u8 / vp_calc_hist_dev: the exact count per bin.  mask (nullable, mask_w x mask_h bytes): only its non-zero pixels are
 *   counted; mask_bits_dev (nullable) is the mask's bit plane in the layout of vp_inrange_u8_bits_dev (rows of ceil(w / 64) words),
 *   read instead of its bytes - its bits past w are not looked at.  The host form takes packed arrays, gives float32 counts (exact: an
 *   image has at most 2^24 pixels) and synchronises.  The device form leaves uint32 counts in counts_dev and / or counts_host (at least
 *   one of them); it synchronises only to fill counts_host.
 * vp_back_project_u8 / vp_back_project_dev / vp_back_project_table_dev: dst (uint8, one channel) = saturate_u8(round_half_even(
 *   double(hist[bin]) * scale)) for a pixel's bin, 0 for a pixel without one (a NaN product gives 0).  The result depends on the bin
 *   alone, so the float32 histogram is first folded into a table of one byte per bin - on the host by the host form, by a small kernel
 *   from hist_dev by the device form - and the image kernel gathers from it.  The _table form takes such a table (device memory, one
 *   byte per bin): one launch per frame.  The host form synchronises; the device forms enqueue and never synchronise.
 * vp_mean_shift_dev: cv2.meanShift of n windows (x, y, w, h; host int32) over a single-channel uint8 device image, one block per
 *   window with the whole loop inside it: W = window cut to the image; up to max(max_iter, 1) times: the sums m00, m10, m01 of the
 *   current window as exact integers, stop when m00 == 0, move by round_half_even(m10 / m00 - W.w / 2) and the same in y, clamped into
 *   the image, stop when the squared step is below round_half_even(max(eps, 0)^2).  The result is n rows (x, y, w, h, iterations) of
 *   int32 in out_dev and / or out_host (at least one of them); the call is enqueued and synchronises only to fill out_host.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing pointer, w or h outside
 *   1..4096, cn outside 1..4, a stride below its row, dims outside 1..3, a channel index outside the image's channels, a hist_size
 *   outside 1..256, a range without finite ends low < high, a mask of another size than the image, a bit plane that is not 8-byte
 *   aligned, a scale that is not finite, counters or a histogram that are not 4-byte aligned, a result that overlaps an input, n outside
 *   1..4096, a window of non-positive size or with nothing of it inside the image.  max_iter above 100000: VP_ERR_UNSUPPORTED. */
int vp_calc_hist_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, int dims, const int32_t* channels, const int32_t* hist_size, const double* ranges,
                    const uint8_t* mask_host, int mask_w, int mask_h, float* hist_host);
int vp_calc_hist_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t stride, int w, int h, int cn, int dims, const int32_t* channels, const int32_t* hist_size,
                     const double* ranges, const uint8_t* mask_dev, size_t mask_stride, int mask_w, int mask_h, const unsigned long long* mask_bits_dev,
                     uint32_t* counts_dev, uint32_t* counts_host);
int vp_back_project_u8(vp_ctx* ctx, const uint8_t* src_host, int w, int h, int cn, int dims, const int32_t* channels, const int32_t* hist_size, const double* ranges,
                       const float* hist_host, double scale, uint8_t* dst_host);
int vp_back_project_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t stride, int w, int h, int cn, int dims, const int32_t* channels, const int32_t* hist_size,
                        const double* ranges, const float* hist_dev, double scale, uint8_t* dst_dev, size_t dst_stride);
int vp_back_project_table_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t stride, int w, int h, int cn, int dims, const int32_t* channels, const int32_t* hist_size,
                              const double* ranges, const uint8_t* table_dev, uint8_t* dst_dev, size_t dst_stride);
int vp_mean_shift_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t stride, int w, int h, const int32_t* windows_host, int n, int max_iter, double eps,
                      int32_t* out_dev, int32_t* out_host);

/* ---- sparse optical flow: cv2.calcOpticalFlowPyrLK ------------------------------------------------------------------------------- *
 * Pyramidal Lucas-Kanade tracking of n points between two uint8 single-channel images of one size (the
 * statement: tests/flow_restate.py).  The window sums are exact integers; OpenCV's remaining steps run in double in one fixed order
 * and are rounded to float32 where OpenCV holds a float: the exact value of what cv2's float32 code approximates.
 * Level 0 is the image, level l + 1 is vp_pyr_down of level l with VP_BORDER_REFLECT_101, (w + 1) / 2 x (h + 1) / 2.  Level l exists
 * while its width is above win_w and its height above win_h; the levels used are the existing ones at or below max_level.
 * vp_lk_flow_levels: how many that is (0: level 0 itself is not larger than the window).  Host only, no context.
 * vp_lk_flow_dev: prev_levels / next_levels are host arrays of n_levels device pointers with their row strides in bytes; levels
 *   min(n_levels, vp_lk_flow_levels(..)) of them are read, so one pyramid serves calls with a smaller max_level.  prev_pts: n (x, y)
 *   float32 pairs on the host; init_pts: n starting positions, read only with VP_LK_USE_INITIAL_FLOW.  max_count is clamped to
 *   0..100 and eps to 0..10 as cv2 clamps its TermCriteria.  The result is n rows of four 32-bit words - x, y, err (float32) and
 *   status (uint32, 0 or 1) - in out_dev and / or out_host (at least one of them); the call is one launch, enqueued, and
 *   synchronises only to fill out_host.  err is sum |diff| / (32 win_w win_h) at the final position, or level 0's minimum eigenvalue
 *   with VP_LK_GET_MIN_EIGENVALS; it is 0 whenever status is 0 and that flag is off.  A point (or initial position) with a
 *   coordinate that is not finite or beyond +-2^24 gets status 0, err 0 and its starting position back.
 * vp_lk_flow_u8: two packed host images; stages them, builds both pyramids with vp_pyr_down_dev, runs and synchronises.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing pointer, w or h outside
 *   1..4096, a stride below its row, a window side outside 3..63, an image not larger than the window, n outside 1..2^20, max_level
 *   outside 0..15, n_levels outside 1..16, unknown flag bits, a min_eig_threshold or eps that is not finite, an out_dev that is not
 *   4-byte aligned or overlaps a level. */
enum { VP_LK_USE_INITIAL_FLOW = 4, VP_LK_GET_MIN_EIGENVALS = 8 };
int vp_lk_flow_levels(int w, int h, int win_w, int win_h, int max_level);
int vp_lk_flow_dev(vp_ctx* ctx, const uint8_t* const* prev_levels, const size_t* prev_strides, const uint8_t* const* next_levels, const size_t* next_strides,
                   int n_levels, int w, int h, const float* prev_pts_host, const float* init_pts_host, int n, int win_w, int win_h, int max_level, int max_count,
                   double eps, int flags, double min_eig_threshold, void* out_dev, void* out_host);
int vp_lk_flow_u8(vp_ctx* ctx, const uint8_t* prev_host, const uint8_t* next_host, int w, int h, const float* prev_pts_host, const float* init_pts_host, int n,
                  int win_w, int win_h, int max_level, int max_count, double eps, int flags, double min_eig_threshold, void* out_host);

/* ---- robust motion estimation from point pairs: cv2.findHomography, estimateAffine2D, estimateAffinePartial2D --------------------- *
 * RANSAC over n pairs src[i] -> dst[i] of float32 (x, y).  The contract is the statement
 * tests/model_restate.py, reproduced bit for bit, not cv2's random sequence: hypothesis j draws its 2 / 3 / 4 distinct indices from a
 * counter-based function of (seed, j); degenerate samples are void; the minimal solvers, the squared reprojection distance and the
 * test err <= threshold^2 run in double in one written order; the score is the integer inlier count, ties go to the lowest j.
 * Hypotheses are taken in rounds of vp_model_round_size(); after round r the search stops once the best count has reached the r-th
 * entry of the stop table (cv2's RANSACUpdateNumIters, computed on the host), at the latest at max_iters.  inliers (n bytes of 0 / 1,
 * nullable) is the inlier set of the best hypothesis; model_out (nine doubles, a row-major 3 x 3 whose last row is 0 0 1 for the
 * similarity and the affine model) is the least-squares refit over that set, made on the host in index order.  *n_inliers is 0, and
 * model_out and inliers are zeros, when there is no model; *n_hypotheses is the number of hypotheses taken.
 * vp_estimate_model_f32 stages host points; vp_estimate_model_dev reads two device arrays (8-byte aligned); both enqueue every round
 * at once and synchronise once.  vp_estimate_model_host is the same statement as a host loop: no device, no context.
 * vp_model_hypothesis: hypothesis j as the kernel forms it - sample (four indices, -1 where unused) and its nine doubles; returns 1,
 *   or 0 for a void hypothesis (zeros).  vp_model_stop_table: the table, `capacity` at least ceil(max_iters / round size) entries.
 * vp_model_refit: the refit alone over the points whose mask byte is not 0 (mask NULL: all); returns 1, or 0 when there is no model.
 * vp_model_stage_points: the points a scoring block stages at once.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing pointer, an unknown
 *   model, n below the model's sample size or above 2^20, a threshold that is not finite and above 0, max_iters outside 1..65536, a
 *   confidence outside (0, 1), device points that are not 8-byte aligned, a hypothesis index outside 0..65535, a table too short. */
enum { VP_MODEL_SIMILARITY = 0, VP_MODEL_AFFINE = 1, VP_MODEL_HOMOGRAPHY = 2 };
int vp_model_round_size(void);
int vp_model_stage_points(void);
int vp_estimate_model_f32(vp_ctx* ctx, const float* src_host, const float* dst_host, int n, int model, double threshold, int max_iters, double confidence,
                          uint32_t seed, double* model_out, uint8_t* inliers_host, int* n_inliers, int* n_hypotheses);
int vp_estimate_model_dev(vp_ctx* ctx, const float* src_dev, const float* dst_dev, int n, int model, double threshold, int max_iters, double confidence,
                          uint32_t seed, double* model_out, uint8_t* inliers_host, int* n_inliers, int* n_hypotheses);
int vp_estimate_model_host(const float* src, const float* dst, int n, int model, double threshold, int max_iters, double confidence, uint32_t seed,
                           double* model_out, uint8_t* inliers, int* n_inliers, int* n_hypotheses);
int vp_model_hypothesis(const float* src, const float* dst, int n, int model, uint32_t seed, int j, int32_t* sample, double* model_out);
int vp_model_stop_table(int n, int model, double confidence, int max_iters, int32_t* need, int capacity, int* rounds);
int vp_model_refit(const float* src, const float* dst, int n, const uint8_t* mask, int model, double* model_out);

/* ---- features: FAST-9 corners, a steered 256-bit binary descriptor, brute-force Hamming matching ------------------------------------
 * What utils/sift.py needs in front of vp_estimate_model_*: detect, describe, match.  All integer arithmetic, byte for byte against
 * tests/features_restate.py; DESIGN.md section 4.31.  Images are uint8, single channel, rows of `stride` bytes.
 * vp_fast_*: cv2.FastFeatureDetector_create(threshold, nonmax, TYPE_9_16).detect on a w x h image, w, h >= 7.  Ring: the 16 pixels of
 *   the radius-3 circle in the order (0,3) (1,3) (2,2) (3,1) (3,0) (3,-1) ... (-1,3) as (dx, dy).  M of a pixel with
 *   3 <= x <= w - 4, 3 <= y <= h - 4: the maximum, over the 16 cyclic arcs of 9 contiguous ring pixels and both signs s, of the arc's
 *   minimum of s (centre - ring).  Corner iff M > threshold (0..255); score M - 1.  nonmax != 0: a corner is kept iff its score is
 *   strictly above the score of each of its eight neighbours (a non-corner scores 0), and reports its score; nonmax == 0: every corner
 *   is kept and reports 0.  *n_found is the number kept; the first min(*n_found, capacity) in raster order (y, then x) are written as
 *   (x, y) pairs to xy_host and scores to score_host, both host arrays; capacity 0 with NULL arrays counts.  Synchronises.
 * vp_describe_*: the library's own descriptor of n points (host float32 (x, y) pairs, both forms) on a w x h image, w, h >= 31.  A point
 *   is rounded to the pixel p = floor((double)v + 0.5); closer than 15 to a border, or not finite: status 0, bin 0, 32 zero bytes.
 *   Otherwise status 1; m10 = sum dx I(p + d), m01 = sum dy I(p + d) over dx dx + dy dy <= 225; bin = the k in 0..31 that maximises
 *   m10 C[k] + m01 S[k] in 64-bit integers (C, S: 16384 cos / sin(2 pi k / 32) rounded half away from zero; ties to the lowest k);
 *   bit i = B(p + a'_i) < B(p + b'_i), B the 7 x 7 GaussianBlur of the image at sigma 2 (BORDER_REFLECT_101) made in the workspace,
 *   (a'_i, b'_i) pair i of the pattern steered to the bin; test 8 j + b is bit b of byte j.  desc (n x 32), bin (n), status (n) are
 *   host arrays.  Synchronises.
 * vp_describe_pattern: the table of 32 x 256 x 4 int8 (bin, pair, ax ay bx by); no device, no context.  Base pairs: coordinates
 *   d1 + d2 - 10 from consecutive draws d = (s >> 16) % 11 of s <- s 1664525 + 1013904223 (mod 2^32, from 0x9E3779B9, advanced before
 *   each draw), four per candidate in the order ax ay bx by; a == b or a pair already taken (either order) is dropped; 256 are kept.
 *   Steering: x' = rdiv(x C[k] - y S[k]), y' = rdiv(x S[k] + y C[k]), rdiv(v) = sign(v) ((|v| + 8192) >> 14).
 * vp_hamming_knn_*: cv2.BFMatcher(NORM_HAMMING).knnMatch of (nq, D) query against (nt, D) train descriptors, D a multiple of 8 in
 *   8..128, strides at least D and multiples of 8, k 1 or 2: for each query the first k train rows by (distance, index) ascending into
 *   idx and dist, both (nq, k) int32; entries beyond nt are -1 / -1.  cross_check (k = 1): idx becomes -1 where the train row's best
 *   query by (distance, query index) is another one (dist stays).  nq or nt of 0 launches nothing.  _u8: host arrays in and out,
 *   synchronises; _dev: device arrays in (8-byte aligned) and out (4-byte aligned), enqueued.
 * vp_hamming_plan: the grid the matcher uses - blocks of 256 queries, and the number of splits of the train set (more than one when
 *   the query blocks alone would not fill the device); no device, no context.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing pointer, a side
 *   below 7 (FAST) or 31 (describe) or above 65535, more than 2^28 pixels, a stride below the row, a threshold outside 0..255, a
 *   negative capacity or count, more than 2^20 points or rows, D not a multiple of 8 or outside 8..128, a matcher stride that is
 *   not a multiple of 8, k outside 1..2, cross_check with k = 2, misaligned device arrays. */
int vp_fast_u8(vp_ctx* ctx, const uint8_t* src, size_t stride, int w, int h, int threshold, int nonmax, int32_t* xy_host, int32_t* score_host, int capacity,
               int* n_found);
int vp_fast_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t stride, int w, int h, int threshold, int nonmax, int32_t* xy_host, int32_t* score_host, int capacity,
                int* n_found);
int vp_describe_pattern(int8_t* out);
int vp_describe_u8(vp_ctx* ctx, const uint8_t* src, size_t stride, int w, int h, const float* pts, int n, uint8_t* desc, uint8_t* bin, uint8_t* status);
int vp_describe_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t stride, int w, int h, const float* pts, int n, uint8_t* desc, uint8_t* bin, uint8_t* status);
int vp_hamming_plan(int nq, int nt, int D, int* query_tiles, int* train_splits);
int vp_hamming_knn_u8(vp_ctx* ctx, const uint8_t* query, size_t query_stride, int nq, const uint8_t* train, size_t train_stride, int nt, int D, int k,
                      int cross_check, int32_t* idx, int32_t* dist);
int vp_hamming_knn_dev(vp_ctx* ctx, const uint8_t* query_dev, size_t query_stride, int nq, const uint8_t* train_dev, size_t train_stride, int nt, int D, int k,
                       int cross_check, int32_t* idx_dev, int32_t* dist_dev);

/* ---- features over a scale pyramid (byte for byte against tests/pyr_features_restate.py) -------------------
 * Levels: w_0, h_0 the image; w_l = (5 w_{l-1} + 3) / 6 in integers, h likewise (a step of 1.2); level l is the INTER_LINEAR resize
 *   (vp_resize_dev's arithmetic) of level l - 1.  `levels` (1..8) are asked for; those with min(w_l, h_l) >= 31 are built, possibly none.
 * On each level: FAST-9 as vp_fast_* states it with nonmax, among the pixels that can be described (15 <= x <= w_l - 16, likewise y;
 *   suppression compares with the level's full score map).  Budget: a_l = w_l h_l, A their sum, q_l = (max_points a_l) / A in 64-bit
 *   integers for l >= 1, q_0 the rest; a level keeps its q_l highest scores, ties to the earlier raster position; unused quota is not
 *   handed on.  Order of the result: level, y, x.  Descriptor: vp_describe_*'s arithmetic on the point's own level (orientation from
 *   the level, bits from its 7 x 7 sigma-2 blur).  xy0 = (float)(((double)x_l + 0.5) * ((double)w_0 / w_l) - 0.5), y likewise.
 * vp_pyr_features_plan: the levels built (*n_levels, then (w, h) pairs into level_wh and q_l into quota, room for 8); no device, no
 *   context.
 * vp_pyr_features_*: xy0_host (max_points x 2 float32), lxy_host (max_points x 3 int32: level, x, y on the level), score_host, bin_host,
 *   desc_host (max_points x 32) are host arrays with room for max_points entries, of which the first *n_found <= max_points are
 *   meaningful; desc_dev (nullable): a device array of max_points x 32 bytes, 8-byte aligned, that receives the descriptors too (for
 *   vp_hamming_knn_dev).  No level or max_points == 0: *n_found = 0, nothing is launched.  The number of launches after the pyramid and
 *   its blurs does not depend on the number of levels; synchronises once, at the end.
 * Refused with VP_ERR_INVALID before anything is launched or written: a missing pointer, a side below 1 or above 65535, more than 2^26
 *   pixels, a stride below the row, levels outside 1..8, a threshold outside 0..255, max_points negative or above 2^20, a misaligned
 *   desc_dev. */
int vp_pyr_features_plan(int w, int h, int levels, int max_points, int* n_levels, int32_t* level_wh, int32_t* quota);
int vp_pyr_features_u8(vp_ctx* ctx, const uint8_t* src, size_t stride, int w, int h, int levels, int threshold, int max_points, float* xy0_host, int32_t* lxy_host,
                       int32_t* score_host, uint8_t* bin_host, uint8_t* desc_host, uint8_t* desc_dev, int* n_found);
int vp_pyr_features_dev(vp_ctx* ctx, const uint8_t* src_dev, size_t stride, int w, int h, int levels, int threshold, int max_points, float* xy0_host, int32_t* lxy_host,
                        int32_t* score_host, uint8_t* bin_host, uint8_t* desc_host, uint8_t* desc_dev, int* n_found);

/* ---- stereo block matching: disparity of a rectified pair and metric depth --------------------------------
 * The design of cv2.StereoBM, byte for byte against tests/stereo_restate.py, which is the contract (it has not met a real OpenCV).
 * left, right: uint8, single channel, w x h, rectified: a point of left (x, y) lies at right (x - D, y).  num_disparities n: a multiple
 * of 16 in 16..256; block_size odd in 5..21, r = block_size / 2; min_disparity m in -128..128; pre_filter_cap c in 1..63;
 * texture_threshold >= 0; uniqueness_ratio in 0..100.
 *   Prefilter of both images, rows reflected without the edge row (one row: itself): p = clamp(I(x+1,y-1) - I(x-1,y-1) +
 *     2 (I(x+1,y) - I(x-1,y)) + I(x+1,y+1) - I(x-1,y+1), -c, c) + c for 1 <= x <= w - 2, and c in columns 0 and w - 1.
 *   C(x, y, D) = sum over |i|, |j| <= r of |pL(x+i, y+j) - pR(x+i-D, y+j)|, D in [m, m + n - 1].
 *   Candidates: r <= y <= h-1-r, r <= x <= w-1-r, x - r - (m+n-1) >= 0, x + r - m <= w - 1; every other pixel is (m - 1) * 16.
 *   So is a candidate whose T = window sum of |pL - c| is below texture_threshold, and, for uniqueness_ratio > 0, one with a D,
 *     |D - D*| > 1, of C(D) <= C* + C* uniqueness_ratio / 100 (integer division).  D* minimises C, ties to the larger D.
 *   Else (D* 256 + off + 15) >> 4 with off = (pm - pp) 256 / (pm + pp - 2 C* + |pm - pp|) truncated (0 for a zero denominator),
 *     pm = C(D* - 1), pp = C(D* + 1), the one missing at an end of the range taken as the other.  16 times the disparity, int16.
 * Depth: float32(double(focal_px * baseline_m) * 16.0 / double(disp16)) where disp16 > 0, else 0.
 * vp_stereo_bm_plan: no device, no context.  rect: x, y, w, h of the candidate pixels (zeros when there is none); *ws_bytes: device
 *   scratch of a call; geometry: the matcher's strip columns, band rows, grid x, grid y and LDS bytes per block.
 * _u8 / _i16: packed host images in and out, synchronise.  _dev: device images with strides in bytes, enqueued.  _host: the same
 *   statement as scalar C++, host images with strides, no device and no context.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing pointer, w or h
 *   outside 1..4096, a stride below the row or, for the int16 / float32 images, no multiple of the element size, a parameter outside
 *   its range, a misaligned int16 / float32 image, a result that overlaps an input.  An image without a candidate pixel is no error. */
int vp_stereo_bm_plan(int w, int h, int num_disparities, int block_size, int min_disparity, int32_t* rect, size_t* ws_bytes, int32_t* geometry);
int vp_stereo_bm_u8(vp_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int num_disparities, int block_size, int min_disparity, int pre_filter_cap,
                    int texture_threshold, int uniqueness_ratio, int16_t* disp);
int vp_stereo_bm_dev(vp_ctx* ctx, const uint8_t* left_dev, size_t left_stride, const uint8_t* right_dev, size_t right_stride, int w, int h, int num_disparities,
                     int block_size, int min_disparity, int pre_filter_cap, int texture_threshold, int uniqueness_ratio, int16_t* disp_dev, size_t disp_stride);
int vp_stereo_bm_host(const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride, int w, int h, int num_disparities, int block_size,
                      int min_disparity, int pre_filter_cap, int texture_threshold, int uniqueness_ratio, int16_t* disp, size_t disp_stride);
int vp_depth_from_disparity_i16(vp_ctx* ctx, const int16_t* disp, int w, int h, double focal_px, double baseline_m, float* depth);
int vp_depth_from_disparity_dev(vp_ctx* ctx, const int16_t* disp_dev, size_t disp_stride, int w, int h, double focal_px, double baseline_m, float* depth_dev,
                                size_t depth_stride);
int vp_depth_from_disparity_host(const int16_t* disp, size_t disp_stride, int w, int h, double focal_px, double baseline_m, float* depth, size_t depth_stride);

/* ---- after the matcher: speckle filter of a disparity image, surface normals of a depth image ---------------
 * filter_speckles: the rule of cv2.filterSpeckles on an int16 image, byte for byte against tests/speckle_restate.py, which is the
 *   contract (it has not met a real OpenCV).  Pixels equal to new_val belong to no region and stay.  Two other pixels are linked when
 *   they are 4-neighbours and |a - b| <= max_diff (in int32); links chain.  Every connected region of at most max_speckle_size pixels
 *   becomes new_val, everything else is copied.  max_speckle_size in 0..w*h (0 copies), max_diff in 0..65535, new_val any int16 value.
 *   dst may be src itself (same pointer, same stride); any other overlap is refused.
 * vp_filter_speckles_plan: no device, no context.  *ws_bytes: device scratch of a call (an int32 label and an int32 count per pixel);
 *   geometry: tile width, tile height, grid x, grid y, LDS bytes per block.
 * normals_from_depth: this library's own definition (the vendor SDK's is closed), bit for bit against tests/normals_restate.py.
 *   depth: float32 metres; a pixel is usable iff finite and > 0.  A normal exists at (x, y) iff the pixel and its four neighbours are
 *   inside the image and usable and, with max_jump_m > 0 and finite, no neighbour's depth differs from the centre's by more than it.
 *   P(x, y) = ((x - cx) Z / f, (y - cy) Z / f, Z); du = P(x+1, y) - P(x-1, y); dv = P(x, y+1) - P(x, y-1); c = dv x du (towards the
 *   camera); len = sqrt((c0 c0 + c1 c1) + c2 c2); n = float32(c / len); all in IEEE double, every operation rounded on its own.  No
 *   normal where len is 0 (or not finite).  normals: float32, 3 per pixel; without a normal NaN (0x7fc00000) thrice.  encode != 0:
 *   float32(float32(n + 1) / 2) instead, and 0 without a normal - the reference's `normal` plane.
 * _i16 / _f32: packed host images in and out, synchronise.  _dev: device images with strides in bytes, enqueued.  _host: the same
 *   statements as scalar C++, host images with strides, no device and no context.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing pointer, w or h
 *   outside 1..4096, a stride below the row or no multiple of the element size, a misaligned image, a parameter outside its range,
 *   focal_px not finite or not positive, cx, cy or max_jump_m not a number, a result that overlaps its input (but for dst == src). */
int vp_filter_speckles_plan(int w, int h, size_t* ws_bytes, int32_t* geometry);
int vp_filter_speckles_i16(vp_ctx* ctx, const int16_t* src, int w, int h, int new_val, int max_speckle_size, int max_diff, int16_t* dst);
int vp_filter_speckles_dev(vp_ctx* ctx, const int16_t* src_dev, size_t src_stride, int w, int h, int new_val, int max_speckle_size, int max_diff, int16_t* dst_dev,
                           size_t dst_stride);
int vp_filter_speckles_host(const int16_t* src, size_t src_stride, int w, int h, int new_val, int max_speckle_size, int max_diff, int16_t* dst, size_t dst_stride);
int vp_normals_from_depth_f32(vp_ctx* ctx, const float* depth, int w, int h, double focal_px, double cx, double cy, double max_jump_m, int encode, float* normals);
int vp_normals_from_depth_dev(vp_ctx* ctx, const float* depth_dev, size_t depth_stride, int w, int h, double focal_px, double cx, double cy, double max_jump_m, int encode,
                              float* normals_dev, size_t normals_stride);
int vp_normals_from_depth_host(const float* depth, size_t depth_stride, int w, int h, double focal_px, double cx, double cy, double max_jump_m, int encode, float* normals,
                               size_t normals_stride);

/* ---- semi-global stereo matching with a left-right check -------------------------------------------------
 * Hirschmueller's semi-global matching in the shape of cv2.StereoSGBM, byte for byte against tests/sgm_restate.py, which is the
 * contract; it does not claim OpenCV's bits.  Images, prefilter, C(x, y, d) (D = m + d, d in [0, n)), the candidate rectangle and the
 * invalid value INV = (m - 1) * 16 are the block matcher's above, at this block size; there is no texture test.  num_disparities n: a
 * multiple of 16 in 16..256; block_size odd in 1..9; min_disparity m in -128..128; pre_filter_cap c in 1..63; 0 <= p1 <= p2;
 * uniqueness_ratio in 0..100; disp12_max_diff in -1..255 (-1: no left-right check); paths 4 or 8;
 * paths * (2 c block_size^2 + p2) <= 65535, which keeps the summed path costs in 16 bits.
 *   Paths: directions of travel (dy, dx) = (0,1) (0,-1) (1,0) (-1,0), with paths = 8 also (1,1) (1,-1) (-1,1) (-1,-1).  For a pixel p
 *     whose predecessor q = p - (dy, dx) lies outside the candidate rectangle L(p, d) = C(p, d); else, with M = min over k of L(q, k),
 *     L(p, d) = C(p, d) + min(L(q, d), L(q, d-1) + p1, L(q, d+1) + p1, M + p2) - M, a term whose d -+ 1 leaves [0, n) being absent.
 *     S = the sum of L over the paths.  d* minimises S, ties to the larger d.
 *   Uniqueness (ratio > 0): a d with |d - d*| > 1 and S(d) <= S* + S* ratio / 100 (integer division) gives INV.
 *   Left-right check (disp12_max_diff >= 0): with xr = x - (m + d*), the right view's answer is the d that minimises S(xr + m + d, y, d)
 *     over the d whose column xr + m + d is a candidate column, ties to the larger d; |d_right - d*| > disp12_max_diff gives INV.
 *   Else the block matcher's subpixel rule on S: (D* 256 + off + 15) >> 4, int16.
 * vp_stereo_sgm_plan: no device, no context.  rect: x, y, w, h of the candidate pixels (zeros when there is none); *ws_bytes: device
 *   scratch of a call - both prefiltered images and the uint16 volumes C and S, 2 * 2 * rect.w * rect.h * n bytes; geometry
 *   [VP_SGM_GEOMETRY]: cost kernel: threads, strip columns, grid x, grid y, LDS bytes; path kernel: threads, lanes that hold a pixel,
 *   disparities per lane, lines per block, blocks of a horizontal, a vertical, a diagonal direction (0 with four paths); selection
 *   kernel: threads, pixels per block, blocks.  A call whose workspace would exceed 4 GiB (4294967296 bytes) is refused, by every entry.
 * _u8: packed host images in and out, synchronises.  _dev: device images with strides in bytes, enqueued.  _host: the same statement
 *   as scalar C++, host images with strides, no device and no context.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing pointer, w or h
 *   outside 1..4096, a stride below the row or, for the result, no multiple of 2, a parameter outside its range, p1 > p2, the 16-bit
 *   bound, the workspace cap, a misaligned result, a result that overlaps an input.  An image without a candidate pixel is no error. */
#define VP_SGM_GEOMETRY 15
int vp_stereo_sgm_plan(int w, int h, int num_disparities, int block_size, int min_disparity, int paths, int32_t* rect, size_t* ws_bytes, int32_t* geometry);
int vp_stereo_sgm_u8(vp_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int num_disparities, int block_size, int min_disparity, int pre_filter_cap, int p1,
                     int p2, int uniqueness_ratio, int disp12_max_diff, int paths, int16_t* disp);
int vp_stereo_sgm_dev(vp_ctx* ctx, const uint8_t* left_dev, size_t left_stride, const uint8_t* right_dev, size_t right_stride, int w, int h, int num_disparities,
                      int block_size, int min_disparity, int pre_filter_cap, int p1, int p2, int uniqueness_ratio, int disp12_max_diff, int paths, int16_t* disp_dev,
                      size_t disp_stride);
int vp_stereo_sgm_host(const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride, int w, int h, int num_disparities, int block_size,
                       int min_disparity, int pre_filter_cap, int p1, int p2, int uniqueness_ratio, int disp12_max_diff, int paths, int16_t* disp, size_t disp_stride);

/* ---- stereo rectification and 3-D reprojection: the head and the tail of the stereo stack ------------------
 * vp_rectify_pair_*: both eyes of a raw frame to what the matchers read, in one launch.  left and right: uint8 images of w x h pixels
 *   and cn channels - 1, 3 (BGR) or 4 (BGRA) - each with its own stride, so the two halves of a side-by-side frame are two pointers
 *   into one buffer and nothing is copied.  The tables are the fixed form of cv2.convertMaps for INTER_LINEAR, out_w x out_h entries,
 *   packed: xy int16 x 2 and frac uint16 (what vp_convert_maps_dev writes).  Byte for byte against tests/rectify_restate.py:
 *     each colour result = vp_remap_fixed_dev(eye, table, VP_INTER_LINEAR, VP_BORDER_CONSTANT, 0): every channel interpolated and
 *       rounded (sum + 2^14) >> 15; a tap outside [0, w) x [0, h) of its own eye is 0, whatever lies beside the eye in memory;
 *     each grey result = vp_cvt_color_dev(VP_BGR2GRAY / VP_BGRA2GRAY) of that rounded colour result, (B 1868 + G 9617 + R 4899 + 8192)
 *       >> 14; with cn = 1 it is the remapped image itself.
 *   A colour result that is NULL is not written and costs no traffic.  No workspace.
 * vp_rectify_pair_plan: no device, no context.  geometry[6]: tile columns, tile rows, pixels per lane, grid x, grid y, grid z (the eyes).
 * vp_reproject_to_3d_*: (X, Y, Z, W) = Q (x, y, d, 1) per pixel of a disparity image in double, each row ((q0 x + q1 y) + q2 d) + q3
 *   with one rounding per product and sum, then X / W, Y / W, Z / W as double quotients rounded once more to float32: an (h, w, 3)
 *   float32 image, bit for bit against tests/rectify_restate.py.  disp_type VP_DISP_I16: int16 sixteenths of a pixel, as the matchers
 *   write them (d = value / 16); VP_DISP_F32: float32 pixels.  q16: the 4 x 4 matrix, row-major doubles in host memory; it travels as a
 *   kernel argument.  Three zeros - the library's "unknown", as in vp_depth_from_disparity_* - where the pixel equals invalid_disp
 *   (int16 images; INT_MIN: no such value), where W == 0 and where a float32 disparity is not finite.
 * _u8 / _i16 / _f32: packed host images (and host tables) in and out, synchronises.  _dev: device images with strides in bytes,
 *   enqueued.  _host: the same statements as scalar C++, host images with strides, no device and no context.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing source, table, grey
 *   result, disparity, Q or result; a width or height outside 1..4096; cn outside {1, 3, 4}; a stride below the row or, for int16 and
 *   float32 images, no multiple of the element size; a misaligned table, int16 or float32 image; any result that overlaps a source,
 *   a table or another result; a Q that is not finite or has an entry above 1e100 in magnitude; an unknown disp_type; an invalid_disp
 *   that is neither INT_MIN nor an int16 value, or that is given with a float32 image. */
enum { VP_DISP_I16 = 0, VP_DISP_F32 = 1 };
int vp_rectify_pair_plan(int w, int h, int cn, int out_w, int out_h, int32_t* geometry);
int vp_rectify_pair_dev(vp_ctx* ctx, const uint8_t* left_dev, size_t left_stride, const uint8_t* right_dev, size_t right_stride, int w, int h, int cn,
                        const int16_t* xy_left_dev, const uint16_t* frac_left_dev, const int16_t* xy_right_dev, const uint16_t* frac_right_dev, int out_w, int out_h,
                        uint8_t* grey_left_dev, size_t grey_left_stride, uint8_t* grey_right_dev, size_t grey_right_stride, uint8_t* colour_left_dev,
                        size_t colour_left_stride, uint8_t* colour_right_dev, size_t colour_right_stride);
int vp_rectify_pair_u8(vp_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int cn, const int16_t* xy_left, const uint16_t* frac_left,
                       const int16_t* xy_right, const uint16_t* frac_right, int out_w, int out_h, uint8_t* grey_left, uint8_t* grey_right, uint8_t* colour_left,
                       uint8_t* colour_right);
int vp_rectify_pair_host(const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride, int w, int h, int cn, const int16_t* xy_left,
                         const uint16_t* frac_left, const int16_t* xy_right, const uint16_t* frac_right, int out_w, int out_h, uint8_t* grey_left, size_t grey_left_stride,
                         uint8_t* grey_right, size_t grey_right_stride, uint8_t* colour_left, size_t colour_left_stride, uint8_t* colour_right, size_t colour_right_stride);
int vp_reproject_to_3d_dev(vp_ctx* ctx, const void* disp_dev, size_t disp_stride, int disp_type, int w, int h, const double* q16, int invalid_disp, float* xyz_dev,
                           size_t xyz_stride);
int vp_reproject_to_3d_i16(vp_ctx* ctx, const int16_t* disp, int w, int h, const double* q16, int invalid_disp, float* xyz);
int vp_reproject_to_3d_f32(vp_ctx* ctx, const float* disp, int w, int h, const double* q16, float* xyz);
int vp_reproject_to_3d_host(const void* disp, size_t disp_stride, int disp_type, int w, int h, const double* q16, int invalid_disp, float* xyz, size_t xyz_stride);

/* ---- robust plane fitting to the 3-D points of an image: where a surface is and which way it faces ----------
 * RANSAC for one plane n.P + d = 0 over the usable points of an XYZ image (float32, three floats a pixel, rows of xyz_stride bytes, as
 * vp_reproject_to_3d_* writes it).  The contract is the statement tests/plane_restate.py, reproduced bit for bit in the best hypothesis,
 * its index, the counts and the inlier image.  A pixel is a candidate inside box (x0, y0, rw, rh; NULL: the image) where the mask byte
 * (mask NULL: none) is not 0; a candidate is usable when its three floats are finite and not all three zero.  The points are the
 * usable candidates in raster order.  Hypothesis j draws three distinct point indices from the counter-based sampler of
 * vp_estimate_model_* (seed, j); the plane through them is formed in double in one written order and oriented towards the camera
 * (d > 0); void: a sample whose angle has a sine below 1e-6, a plane through the origin, a number that is not finite, and with
 * VP_PLANE_ALONG_Z a normal with |n2| <= 1e-6.  e = ((n0 x + n1 y) + n2 z) + d; inlier iff e e <= t t (VP_PLANE_PERP) or
 * e e <= (t t) (n2 n2) (VP_PLANE_ALONG_Z: the residual is taken along the third axis, which is what a disparity image needs).  The
 * score is the integer inlier count, ties go to the lowest j; rounds and the stop rule are those of vp_estimate_model_* for a sample of
 * three; with fewer than three points nothing is searched.
 * result (VP_PLANE_RESULT doubles): the refit plane (4), the best hypothesis (4), the inliers' centroid (3), the rms residual.  The
 *   refit is the smallest eigenvector of the inliers' scatter (PERP) or the regression of z on x and y (ALONG_Z), closed on the host
 *   from ten sums the device adds in a free order: it is not bit-exact by design; a degenerate refit repeats the best hypothesis.
 * counts (VP_PLANE_COUNTS): usable points, inliers, hypotheses taken, index of the best hypothesis.  No model: result is zeros,
 *   counts[1] is 0, counts[3] is -1 and the inlier image is zeros.
 * inliers (nullable): uint8 w x h, 255 at the pixel of every inlier and 0 elsewhere; bytes between rows are left alone.
 * vp_fit_plane_dev reads device images and writes a device image; it enqueues every launch, the number of points never leaves the
 *   device before the end, and it synchronises once to hand back result and counts.  vp_fit_plane_f32 stages host images (rows
 *   packed).  vp_fit_plane_host is the same statement as a host loop: host images with strides, no device, no context.
 * vp_fit_plane_plan: the workspace a call on this image and box reserves at most, and geometry[8]: the compaction's run length, the
 *   points a scoring block stages, the hypotheses a scoring block tests, the block size, the round size, the candidates of the box,
 *   the compaction's blocks, the scoring grid's chunks.
 * vp_plane_hypothesis: hypothesis j over n packed points (x, y, z, one float that is ignored) as the kernel forms it - sample3 and
 *   plane4; returns 1, or 0 for a void hypothesis (zeros).  vp_plane_refit: the refit alone over the packed points whose keep byte is
 *   not 0 (keep NULL: all), its sums taken about the first kept point in index order; returns 1, or 0 (zeros) when it is degenerate.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing xyz, result or counts;
 *   w or h outside 1..4096; a box that is empty or leaves the image; a stride below the row; an xyz stride that is no multiple of 4; a
 *   misaligned xyz; an unknown metric; a threshold that is not finite and above 0; max_iters outside 1..65536; a confidence outside
 *   (0, 1); a hypothesis index outside 0..65535; an inlier image that overlaps xyz or the mask. */
enum { VP_PLANE_PERP = 0, VP_PLANE_ALONG_Z = 1 };
#define VP_PLANE_RESULT 12
#define VP_PLANE_COUNTS 4
int vp_fit_plane_plan(int w, int h, const int32_t* box, size_t* ws_bytes, int32_t* geometry);
int vp_fit_plane_dev(vp_ctx* ctx, const float* xyz_dev, size_t xyz_stride, int w, int h, const int32_t* box, const uint8_t* mask_dev, size_t mask_stride, int metric,
                     double threshold, int max_iters, double confidence, uint32_t seed, uint8_t* inliers_dev, size_t inliers_stride, double* result, int32_t* counts);
int vp_fit_plane_f32(vp_ctx* ctx, const float* xyz, int w, int h, const int32_t* box, const uint8_t* mask, int metric, double threshold, int max_iters, double confidence,
                     uint32_t seed, uint8_t* inliers, double* result, int32_t* counts);
int vp_fit_plane_host(const float* xyz, size_t xyz_stride, int w, int h, const int32_t* box, const uint8_t* mask, size_t mask_stride, int metric, double threshold,
                      int max_iters, double confidence, uint32_t seed, uint8_t* inliers, size_t inliers_stride, double* result, int32_t* counts);
int vp_plane_hypothesis(const float* pts4, int n, int metric, uint32_t seed, int j, int32_t* sample3, double* plane4);
int vp_plane_refit(const float* pts4, int n, const uint8_t* keep, int metric, double* result);

/* ---- robust rigid 3-D motion between paired 3-D points: how the scene moved between two stereo frames --------
 * RANSAC for one motion q = R p + t (R a rotation, never a reflection) over n pairs of float32 3-vectors.  The contract is the
 * statement tests/rigid_restate.py, reproduced bit for bit in the best hypothesis, its index, the counts and the inlier bytes.  A pair
 * is usable when both points pass the plane fit's point test (three finite floats, not all three zero); the search runs over the
 * usable pairs in index order.  Hypothesis j draws three distinct pair indices from the counter-based sampler of vp_estimate_model_*
 * (seed, j); each side's triad gives an orthonormal frame (u1 along e1 = p1 - p0, u3 along e1 x e2, u2 = u3 x u1), R carries the source
 * frame onto the destination frame and t carries the source triad's mean onto the destination's, in double in one written order;
 * void: a triad on either side whose angle has a sine below 1e-6, or a number that is not finite.  With m = R p + t a pair is an
 * inlier iff |m - q|^2 <= T^2 (VP_RIGID_EUCLID, T in the points' unit) or, with VP_RIGID_DISPARITY, iff m_z > 0, q_z > 0 and
 * (du^2 + dv^2) + dd^2 <= T^2 with du = f (m_x / m_z - q_x / q_z), dv likewise with y, dd = f b (1 / m_z - 1 / q_z): the distance in
 * pixels and pixels of disparity a rectified rig of focal length f = focal_px and baseline b sees, T in pixels (focal_px and baseline
 * are ignored under VP_RIGID_EUCLID).  The score is the integer inlier count, ties go to the lowest j; rounds and the stop rule are
 * those of vp_fit_plane_*; with fewer than three usable pairs nothing is searched.
 * result (VP_RIGID_RESULT doubles): the refit R (9, row-major) and t (3), the best hypothesis R (9) and t (3), the inliers' source and
 *   destination centroids (3 + 3), the rms residual of the refit over the inliers (the points' unit, under both metrics).  The refit
 *   is the least-squares rotation by Horn's quaternion, closed on the host from seventeen sums the device adds in a free order: it is
 *   not bit-exact by design; a degenerate refit (the inliers lie on a line) repeats the best hypothesis.
 * counts (VP_RIGID_COUNTS): usable pairs, inliers, hypotheses taken, index of the best hypothesis.  No model: result is zeros,
 *   counts[1] is 0, counts[3] is -1 and the inlier bytes are zeros.
 * inliers (nullable): n bytes by original pair index, 1 for an inlier and 0 otherwise; all n are written and nothing beyond them.
 * vp_fit_rigid_dev reads device arrays (n rows of three float32 each) and writes device bytes; it enqueues every launch, the number of
 *   usable pairs never leaves the device before the end, and it synchronises once to hand back result and counts.  vp_fit_rigid_f32
 *   stages host arrays.  vp_fit_rigid_host is the same statement as a host loop: no device, no context.
 * vp_fit_rigid_tracks_*: the pairs come from two XYZ images (float32, three floats a pixel, rows of a stride in bytes, both w x h, as
 *   vp_reproject_to_3d_* writes them) and n tracks: prev_pts, n (x, y) float32 pairs on the host, and the n four-word rows x, y, err,
 *   status that vp_lk_flow_dev leaves in out_dev (device memory for _dev, host memory otherwise).  Track i gives the pair (point of
 *   the previous image at prev_pts[i], point of the current image at its row's x, y) when its status is not 0, its four coordinates
 *   are finite, both positions round to a pixel inside the image - ix = floor(x + 0.5f), admitted iff x >= -0.5f and x < w - 0.5f,
 *   the same for y: the nearest pixel, never an interpolation across a depth edge - and both points are usable.  The inlier bytes
 *   are per track row.  _f32 takes packed host images.
 * vp_fit_rigid_plan: the workspace a call on n pairs or tracks reserves at most (without the copies _f32 stages), and geometry[8]: the
 *   compaction's run length, the pairs a scoring block stages, the hypotheses a scoring block tests, the block size, the round size,
 *   n, the compaction's blocks, the scoring grid's chunks.
 * vp_rigid_hypothesis: hypothesis j over n pairs (all taken as usable) as the kernel forms it - sample3 and motion12 (R, t); returns
 *   1, or 0 for a void hypothesis (zeros).  vp_rigid_refit: the refit alone over the pairs whose keep byte is not 0 (keep NULL: all),
 *   its sums taken about the first kept pair in index order; returns 1, or 0 (zeros) when it is degenerate.
 * Refused with VP_ERR_INVALID before anything is launched or written (the message names the reason): a missing pointer; n outside
 *   1..2^20; w or h outside 1..4096; a stride below the row or no multiple of 4; a misaligned input; an unknown metric; a threshold
 *   that is not finite and above 0, and under VP_RIGID_DISPARITY a focal_px or baseline that is not; max_iters outside 1..65536; a
 *   confidence outside (0, 1); a hypothesis index outside 0..65535; inlier bytes that overlap an input. */
enum { VP_RIGID_EUCLID = 0, VP_RIGID_DISPARITY = 1 };
#define VP_RIGID_RESULT 31
#define VP_RIGID_COUNTS 4
int vp_fit_rigid_plan(int n, size_t* ws_bytes, int32_t* geometry);
int vp_fit_rigid_dev(vp_ctx* ctx, const float* src_dev, const float* dst_dev, int n, int metric, double threshold, double focal_px, double baseline, int max_iters,
                     double confidence, uint32_t seed, uint8_t* inliers_dev, double* result, int32_t* counts);
int vp_fit_rigid_f32(vp_ctx* ctx, const float* src, const float* dst, int n, int metric, double threshold, double focal_px, double baseline, int max_iters,
                     double confidence, uint32_t seed, uint8_t* inliers, double* result, int32_t* counts);
int vp_fit_rigid_host(const float* src, const float* dst, int n, int metric, double threshold, double focal_px, double baseline, int max_iters, double confidence,
                      uint32_t seed, uint8_t* inliers, double* result, int32_t* counts);
int vp_fit_rigid_tracks_dev(vp_ctx* ctx, const float* xyz_prev_dev, size_t xyz_prev_stride, const float* xyz_cur_dev, size_t xyz_cur_stride, int w, int h,
                            const float* prev_pts_host, const void* tracks_dev, int n, int metric, double threshold, double focal_px, double baseline, int max_iters,
                            double confidence, uint32_t seed, uint8_t* inliers_dev, double* result, int32_t* counts);
int vp_fit_rigid_tracks_f32(vp_ctx* ctx, const float* xyz_prev, const float* xyz_cur, int w, int h, const float* prev_pts, const void* tracks, int n, int metric,
                            double threshold, double focal_px, double baseline, int max_iters, double confidence, uint32_t seed, uint8_t* inliers, double* result,
                            int32_t* counts);
int vp_fit_rigid_tracks_host(const float* xyz_prev, size_t xyz_prev_stride, const float* xyz_cur, size_t xyz_cur_stride, int w, int h, const float* prev_pts,
                             const void* tracks, int n, int metric, double threshold, double focal_px, double baseline, int max_iters, double confidence, uint32_t seed,
                             uint8_t* inliers, double* result, int32_t* counts);
int vp_rigid_hypothesis(const float* src3, const float* dst3, int n, uint32_t seed, int j, int32_t* sample3, double* motion12);
int vp_rigid_refit(const float* src3, const float* dst3, int n, const uint8_t* keep, double* result);

/* ---- device memory helpers (so a host program needs no HIP binding of its own) --------- */
int vp_dev_alloc(vp_ctx* ctx, size_t bytes, void** dev_ptr);
int vp_dev_free(vp_ctx* ctx, void* dev_ptr);    /* ctx may be NULL (memory that outlived its context) */
/* Page-locked host memory: transfers to/from it run at PCIe speed (hipHostMalloc / hipHostFree). */
int vp_host_alloc(vp_ctx* ctx, size_t bytes, void** host_ptr);
int vp_host_free(vp_ctx* ctx, void* host_ptr);   /* ctx may be NULL */
/* Page-locks memory the caller already has (hipHostRegister), so that vp_memcpy_h2d_async from it is a DMA at PCIe speed with no
 * staging copy: the runtime registers the mapping of a camera_message_framework block once (cmf_block_mapping,
 * include/camera_message_framework_c.h) and then uploads frames straight out of the ring slots - the replacement for the two host
 * copies of lib/camera_message_framework.cpp:421-452 + core/base.py:765-768.  VP_ERR_UNSUPPORTED when the runtime refuses the range
 * (the caller keeps its copying path); unregister before the memory is unmapped. */
int vp_host_register(vp_ctx* ctx, void* host_ptr, size_t bytes);
int vp_host_unregister(vp_ctx* ctx, void* host_ptr);   /* ctx may be NULL */
/* ---- frame feeder: the newest frame of a camera_message_framework block kept in HBM by a thread of the library's own ----------
 * Replaces, for a module on the runtime, the per-iteration sequence read_frame (seqlock memcpy, lib/camera_message_framework.cpp:
 * 379-455) -> np.array(copy) (core/base.py:765-768) -> upload: the feeder waits on the block's condition variable, copies every new
 * frame out of its ring slot into one of four device buffers on its own stream (the block's mapping must be page-locked:
 * vp_host_register), checks the slot's sequence number after the copy and publishes the buffer; vp_feeder_take hands the newest one
 * over without waiting for anything.  The block library is not linked: its five entry points (cmf_wait_for_frame, cmf_peek_frame,
 * cmf_peek_validate, create_frame, delete_frame of include/camera_message_framework_c.h) are passed as addresses.
 * take -> 0: meta_out (sizeof(Frame) = 360 bytes) + *dev_out; 1: nothing newer than the last frame taken; 2: block deleted.
 * release: the buffer may be overwritten once the work queued so far on `consumer`'s stream has passed (consumer may be NULL).
 * stop ends the thread (buffers handed out stay valid); destroy frees everything. */
typedef struct vp_feeder vp_feeder;
vp_feeder* vp_feeder_start(int device, void* block, size_t entry_bytes, void* fn_wait_for_frame, void* fn_peek_frame, void* fn_peek_validate,
                           void* fn_create_frame, void* fn_delete_frame);
int vp_feeder_take(vp_feeder* f, void* meta_out, void** dev_out);
int vp_feeder_release(vp_feeder* f, vp_ctx* consumer, void* dev);
int vp_feeder_counts(vp_feeder* f, unsigned long long* fetched, unsigned long long* dropped_as_lapped);
int vp_feeder_stop(vp_feeder* f);
int vp_feeder_destroy(vp_feeder* f);

/* ---- posts by DMA: a device image into the ring slot of a camera_message_framework block, no host pass over the pixels ---------
 * Replaces, for ModuleBase.post() of an image that lives in HBM, the download into a fresh array (core/base.py:846-876 `np.array(copy)`)
 * plus write_frame's memcpy into the slot (lib/camera_message_framework.cpp:306-374) at the flush (core/base.py:832-839).  The caller
 * opens the slot (cmf_write_begin, include/camera_message_framework_c.h), then:
 *   vp_post_d2h(ctx, lane, slot_bytes, image_dev, bytes, &done): the image AS IT IS NOW (everything queued so far on the context's
 *     stream) is copied into `slot_bytes` (inside a mapping page-locked with vp_host_register) on post stream `lane` (taken modulo the
 *     four the context has: copies of one lane run in order - a block keeps its lane - different lanes side by side); *done is an
 *     opaque handle on the end of that copy.  Returns at once.
 *   vp_post_done(ctx, done) -> 1 the bytes are in the slot (commit the write), 0 not yet, negative on a device error.
 *   vp_post_wait(ctx, done): blocks the calling thread until they are.
 *   vp_post_fence(ctx, done): work queued on the context's stream from now on starts after the copy - call before anything OVERWRITES
 *     the image (readers may run beside the copy).
 *   vp_post_free(ctx, done): hands the handle back (ctx may be NULL: the context is gone). */
int vp_post_d2h(vp_ctx* ctx, int lane, void* slot_bytes_host, const void* image_dev, size_t bytes, void** done);
int vp_post_done(vp_ctx* ctx, void* done);
int vp_post_wait(vp_ctx* ctx, void* done);
int vp_post_fence(vp_ctx* ctx, void* done);
int vp_post_free(vp_ctx* ctx, void* done);

/* device -> device on the context's stream (ordered with everything else the context runs); returns at once */
int vp_memcpy_d2d_async(vp_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);
int vp_memcpy_h2d(vp_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes); /* synchronous */
/* The same copy enqueued on the context's stream: src_host must stay unchanged until vp_wait_uploads (or vp_synchronize) returns.
 * vp_wait_uploads waits for the copies only, not for kernels enqueued behind them: an operator enqueues the copy of its input,
 * does its host-side work and launches, and waits just before handing control back to code that may change the input. */
int vp_memcpy_h2d_async(vp_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int vp_wait_uploads(vp_ctx* ctx);
int vp_memcpy_d2h(vp_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes); /* synchronous */

#ifdef __cplusplus
}
#endif
#endif /* VP_H */
