// Internal declarations shared by the libvp translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/vp.h"
#include "vp_options.h"
#include "vp_morph_plan.h"
#include "vp_contours_plan.h"
#include "vp_ws_frame.h"

typedef unsigned long long u64;
typedef unsigned int u32;

struct vp_tables {          // device copies of the OpenCV integer tables
    const uint16_t* gamma;  // [256]  sRGBGammaTab_b
    const uint16_t* cbrt;   // [2048] LabCbrtTab_b (indices 0..2040 are reachable)
    const int32_t* sdiv;    // [256]
    const int32_t* hdiv;    // [256]  hdiv_table180
    const uint16_t* yf;     // [512]  LabToYF_b (Lab -> BGR)
    const int32_t* abxz;    // [VP_LAB_AB_TAB] abToXZ_b
    const uint8_t* invg;    // [4096] sRGBInvGammaTab_b (values <= 255, stored as bytes)
};

enum { VPK_COLOR = 0, VPK_MORPH, VPK_CCL_LOCAL, VPK_CCL_BOUNDARY, VPK_CCL_FLATTEN, VPK_CCL_RANK, VPK_CCL_BG, VPK_CCL_STATS,
       VPK_CCL_FINAL, VPK_CCL_WRITE, VPK_MEMSET, VPK_OTHER, VPK_CCL2_LOCAL, VPK_CCL2_MERGE, VPK_CCL2_WRITE, VPK_SGM_COST, VPK_SGM_PATH, VPK_SGM_SELECT, VPK_COUNT };
static_assert(VPK_COUNT == VP_PROF_KERNELS, "every kernel id has a name and a slot in vp_profile_end's arrays");

struct vp_prof {
    bool on;
    int cap, used;          // records
    hipEvent_t* ev;         // 2 per record
    int* ids;
};

// A context's state, by owner.  Every struct here is plain data with no default member initialisers: vp_create zero-fills the whole
// context (post.lock relies on that), and a unit that keeps lazily allocated state frees it in its own vp_<unit>_teardown.

struct vp_runtime {           // the runtime's own (vp_api.hip); vp_ctx derives from it, so these read as ctx->stream, ctx->ws, ...
    int device;
    hipStream_t stream;
    hipStream_t own_stream;
    hipEvent_t ev0, ev1;
    void* d_tables;
    void* d_labinv;   // Lab -> BGR tables (tab.abxz / yf / invg)
    vp_tables tab;
    uint8_t* ws;      // grow-only device workspace; each call lays its buffers out in a vp_ws_frame (vp_ws_commit)
    size_t ws_cap;
    uint8_t* hstage;  // grow-only pinned host staging for small results (contour lists)
    size_t hstage_cap;
    // small host -> device hand-overs that must not wait (overlay vertices): a ring of pinned chunks, each free again once the work
    // queued behind its copy has run
    uint8_t* ring_buf[4];
    size_t ring_cap[4];
    hipEvent_t ring_ev[4];
    int ring_busy[4];
    int ring_next;
    int num_cu;
    hipEvent_t ev_upload;         // recorded after an enqueued host-to-device copy (vp_memcpy_h2d_async / vp_wait_uploads)
    vp_prof prof;
    char err[256];
};

struct vp_chain_state {       // the chain's side streams (vp_api_morph_chain.hip), made by vp_create
    hipStream_t aux[4];           // sub-batches of a chain run on these (VP_OPT_CHAIN_STREAMS of them)
    hipEvent_t ev_fork, ev_join[4];
    hipStream_t fb_stream;        // side stream of the labelling: the one-level kernels for crowded frames run here, beside the label write
    hipEvent_t ev_fb_fork, ev_fb_join;
};

struct vp_ccl_state {         // labelling (vp_ccl.hip, vp_ccl3.inl)
    size_t c3_lds_set[6];         // dynamic LDS the crowded-frame kernels have been allowed on THIS device (link, label; short and tall strips): the attribute is per device
    void* c3_acc;                 // crowded-frame labelling: accumulators of components that span strips, all empty between calls (vp_ccl.hip)
    size_t c3_acc_bytes;
    int c3_acc_dirty;             // not known to be all empty (a call cut short, another stream): c3_acc_acquire reinitialises it before use
    uint32_t* hint_host;          // pinned: frames the merge of the last two-level labelling call handed over, written by the device, read without synchronising (vp_ccl_hint.h)
    int hint_failed;              // the word could not be allocated: the crowded-frame kernels are always queued
    int hint_mode, hint_quiet;    // ccl_hint_state between calls (zero: a new context starts LEAN)
    int beside;                   // set around a vpk_ccl that has other work of the same call on a side stream beside it (the chain's contour pass): counts as a second stream, i.e. FULL
    int prepared[2];              // that run has been queued on this context (short / tall strips)
    u32* zero_dev;                // a device word that holds 0: the empty list of the crowded-frame kernels' one preparing run (ccl_prepare_crowded, vp_ccl.hip)
    int launches;                 // kernels of the labelling sequence the last vpk_ccl queued (vp_ccl_last_launches)
};

struct vp_contour_state {     // contours (vp_contours.inl)
    int lds_set;                  // k_ct_jump's LDS attribute has been set on this context's device
    uint32_t* hint_host;          // pinned: head counts of the last batched contour pass (vp_contours.inl vp_ct_hint_slots)
    int hint_n;
    uint32_t heads_hint;      // border segments the last single-image contour pass counted (vp_find_contours_*: which form of the bookkeeping to launch)
};

struct vp_hough_circles_state {   // HoughCircles (vp_hough_circles.hip)
    void* hist;                   // HoughCircles radius histograms of the global form: grow-only, sized per call by its centre count
    size_t hist_bytes;
};

struct vp_agauss_state {      // Gaussian adaptive threshold (vp_adaptive.hip)
    u32* taps;                    // Gaussian adaptive threshold: 8 slots of 256 integer taps (half kernels), made on first use
    int n[8];                     // block size held by each slot (0: empty)
    int e[8];                     // its scale: tap i = taps[slot][i] * 2^-e
    u32 host[8][256];             // host copy of each slot
    int next;                     // slot replaced next
};

struct vp_post_state {        // posts by DMA (vp_post.hip)
    hipStream_t stream[4];        // device image -> ring slot copies run on these lanes, beside the context's stream; made on first use
    hipEvent_t fork;              // "the image as it is now" on the context's stream
    int ready;                    // the four lanes and the fork event all exist (post_setup)
    hipEvent_t free_ev[32];       // end-of-copy events handed back by vp_post_free
    int nfree;
    int lock;                     // spin lock of the fields above (a context is zero-filled at creation: no constructors in here)
};

struct vp_balance_state {     // colour balance (vp_balance.hip)
    const u32* folds_dev;         // colour balance: device counter of tiles whose running mean had to be folded (last call); null or folds_own
    u32* folds_own;               // context-owned device word the counter is copied to (the workspace it is made in is carved anew per call); lives behind d_tables
};

struct vp_features_state {    // descriptors (vp_api_features.hip)
    int8_t* pattern;              // the 32 steered patterns followed by the blur's taps, uploaded on the first describe call
};

struct vp_ctx : vp_runtime {
    vp_options opt;               // indexed by VP_OPT_* (vp_options.h); written by vp_create and vp_set_option only
    vp_chain_state chain;
    vp_ccl_state ccl;
    vp_contour_state ct;
    vp_hough_circles_state hc;
    vp_agauss_state agauss;
    vp_post_state post;
    vp_balance_state cb;
    vp_features_state ft;
};

// brackets one kernel launch with events when profiling is on
struct vp_prof_scope {
    vp_ctx* c;
    int rec;
    vp_prof_scope(vp_ctx* ctx, int id) : c(ctx), rec(-1)
    {
        if (c->prof.on && c->prof.used < c->prof.cap) {
            rec = c->prof.used++;
            c->prof.ids[rec] = id;
            (void)hipEventRecord(c->prof.ev[2 * rec], c->stream);
        }
    }
    ~vp_prof_scope()
    {
        if (rec >= 0) (void)hipEventRecord(c->prof.ev[2 * rec + 1], c->stream);
    }
};

// What a unit set up lazily on the context, freed beside the code that allocates it (vp_destroy calls them).  Each is safe on state
// that was never set up and safe to call twice.
void vp_post_teardown(vp_ctx* ctx);                        // vp_post.hip: joins and frees the post lanes
void vp_ccl_teardown(vp_ctx* ctx);                         // vp_ccl.hip (vp_ccl3.inl's state as well)
void vp_contours_teardown(vp_ctx* ctx);                    // vp_contours.inl
void vp_hough_circles_teardown(vp_ctx* ctx);               // vp_hough_circles.hip
void vp_adaptive_teardown(vp_ctx* ctx);                    // vp_adaptive.hip
void vp_features_teardown(vp_ctx* ctx);                    // vp_api_features.hip

// ---- workspace ---------------------------------------------------------------------------
// reserves W.bytes() and assigns every pointer W recorded; may reallocate (synchronises), so nothing of the call may be in flight yet
int vp_ws_commit(vp_ctx* ctx, const vp_ws_frame& W, const char* who);
void* vp_hstage(vp_ctx* ctx, size_t bytes);                 // pinned host staging of at least `bytes` (NULL: out of memory)
static inline size_t vp_align(size_t n, size_t a = 256) { return (n + a - 1) / a * a; }
int vp_fail(vp_ctx* ctx, int code, const char* what, hipError_t e = hipSuccess);
#define VP_HIP(ctx, call)                                                   \
    do {                                                                    \
        hipError_t e__ = (call);                                            \
        if (e__ != hipSuccess) return vp_fail((ctx), VP_ERR_HIP, #call, e__); \
    } while (0)

// ---- host-side table generation (vp_tables.cpp) ------------------------------------------
void vp_host_tables(uint16_t* gamma, uint16_t* cbrt_tab, int32_t* sdiv, int32_t* hdiv180, int32_t* labC);
void vp_host_lab_inv_tables(uint16_t* yf, int32_t* abxz, uint16_t* inv_gamma, int32_t* coeffs);

// ---- colour kernels (vp_color.hip) ---------------------------------------------------------
struct vp_range3 { int lo[3], hi[3]; int lo2, hi2; };   // lo2 / hi2: second interval of the hue test inside the HSV threshold kernels (vpk_color_thresh)
// fused convert + inRange (+ optional u8 mask, + optional bit-packed mask) over n frames
int vpk_color_thresh(vp_ctx* ctx, int mode, const uint8_t* d_bgr, size_t stride, int w, int h, int n,
                     const vp_range3& r, uint8_t* d_mask /*nullable*/, u64* d_bits /*nullable*/);
int vpk_cvt_color(vp_ctx* ctx, int code, const uint8_t* d_src, size_t stride, int w, int h, uint8_t* d_dst,
                  uint8_t* d_p0, uint8_t* d_p1, uint8_t* d_p2);
bool vp_cvt_channels(int code, int* scn, int* dcn);     // channels of the source / result of a conversion code; false: no such code
int vpk_inrange_u8(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int cn, const vp_range3& r,
                   uint8_t* d_dst, u64* d_bits = nullptr, int* made_bits = nullptr);
int vpk_inrange_f32(vp_ctx* ctx, const float* d_src, size_t stride_bytes, int w, int h, float lo, float hi,
                    uint8_t* d_dst);
int vpk_kth_f32(vp_ctx* ctx, const float* d_src, size_t n, size_t k, u32* d_hist, float* out);
// white balance (vp_whitebal.hip): kernel_size VP_WB_GLOBAL_MEAN or an odd k; d_mean (nullable) receives the two global means
struct vp_whitebal_ws { int2* sums; uint2 *P, *Q, *T; };   // the global form's chunk sums / the box form's prefix planes
void vp_white_balance_want(vp_ws_frame& W, int w, int h, int kernel_size, vp_whitebal_ws* bw);
int vpk_white_balance(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int kernel_size, uint8_t* d_dst, float* d_mean, const vp_whitebal_ws& bw);
int vpk_bgr2lab_f32(vp_ctx* ctx, const float* d_src, size_t npx, float* d_dst);
int vpk_color_distance(vp_ctx* ctx, const uint8_t* p0, const uint8_t* p1, const uint8_t* p2, size_t npx,
                       const float* color, const float* wts, int skipmask, float* d2, uint8_t* sq);

// ---- colour balance (vp_balance.hip) ----------------------------------------------------------
int vpk_hsv2bgr(vp_ctx* ctx, const uint8_t* d_src, size_t npx, uint8_t* d_dst);
struct vp_balance_ws { u32 *hist, *svhist; uint8_t *lut, *svlut; void *plans, *hst; double* powtab; };
void vp_balance_want(vp_ws_frame& W, int n, int tiles, int flags, vp_balance_ws* bw);
int vpk_color_balance(vp_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int w, int h, int n, int flags, int hblocks, int vblocks, const vp_balance_ws& bw);

// ---- detector pre / post-processing (vp_yolo.hip) ------------------------------------------------
int vpk_letterbox(vp_ctx* ctx, const uint8_t* d_src, int sw, int sh, int dw, int dh, int pad, float* d_dst, float* geom_out);
// sstride: bytes between source rows (0: packed)
int vpk_resize_u8(vp_ctx* ctx, const uint8_t* d_src, int sw, int sh, int cn, int dw, int dh, double inv_sx, double inv_sy, uint8_t* d_dst, size_t sstride = 0);
int vpk_warp_affine_u8(vp_ctx* ctx, const uint8_t* d_src, int sw, int sh, int cn, const double* M23, int inverse_map, int border,
                       const uint8_t* cval, uint8_t* d_dst, int dw, int dh, size_t sstride = 0);
struct vp_nms_ws { int* order; unsigned long long* mask; unsigned char* alive; };
void vp_nms_want(vp_ws_frame& W, int n, vp_nms_ws* nw);
int vpk_nms(vp_ctx* ctx, const float* d_boxes, const float* d_scores, int n, float thr, int rotated, int max_keep, int* d_keep, int* d_nkeep, const vp_nms_ws& nw);

// ---- gathers (vp_remap.hip; the tile: vp_remap_plan.h) ------------------------------------------------
// cv2.remap from the fixed form (d_xy: int16 x,y pairs; d_frac: fraction indices, NULL for nearest) or from float maps (d_mapy NULL:
// d_mapx holds interleaved pairs), cv2.convertMaps (float -> fixed) and cv2.warpPerspective.  sstride: bytes between source rows
// (0: packed); results packed; cval: cn bytes or NULL (0); linear: 1 bilinear, 0 nearest.  All enqueue one launch.
int vpk_remap_fixed(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int sw, int sh, int cn, const int16_t* d_xy, const uint16_t* d_frac, int mw, int mh,
                    int linear, int border, const uint8_t* cval, uint8_t* d_dst);
int vpk_remap_f32(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int sw, int sh, int cn, const float* d_mapx, const float* d_mapy, int mw, int mh,
                  int linear, int border, const uint8_t* cval, uint8_t* d_dst);
int vpk_convert_maps(vp_ctx* ctx, const float* d_mapx, const float* d_mapy, int mw, int mh, int nearest, int16_t* d_xy, uint16_t* d_frac);
int vpk_warp_perspective(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int sw, int sh, int cn, const double* M33, int inverse_map, int linear, int border,
                         const uint8_t* cval, uint8_t* d_dst, int dw, int dh);
void vp_invert33(const double* m33, double* out33);   // cv::invert's 3x3 closed form (zeros when singular)

// ---- filters (vp_filter.hip) -----------------------------------------------------------------------
// d_ithresh (nullable): the threshold comes from that device word (vpk_otsu_scan) instead of ithresh
int vpk_threshold_u8(vp_ctx* ctx, const uint8_t* d_src, size_t n, int ithresh, int imaxval, int type, uint8_t* d_dst, const int32_t* d_ithresh = nullptr);
// Otsu's threshold of a 256-bin device histogram of n bytes -> *d_ithresh (and *d_thresh, a double, nullable); one wave, enqueued
int vpk_otsu_scan(vp_ctx* ctx, const u32* d_hist, size_t n, double* d_thresh, int32_t* d_ithresh);
int vpk_hist_u8(vp_ctx* ctx, const uint8_t* d_src, size_t n, u32* d_hist);   // d_hist: 256 counters
int vpk_adaptive_threshold_mean(vp_ctx* ctx, const uint8_t* d_src, int w, int h, int imax, int idelta, int inv, int block, uint16_t* d_tmp, uint8_t* d_dst,
                                size_t sstride = 0);   // sstride: bytes between source rows (0: packed)
// Canny's scratch, declared on the caller's frame by vp_canny_want.  grad: the winning channel's Sobel (dx, dy), w * h short2, valid
// until the next call commits a frame (HoughCircles reads it for cn = 1)
struct vp_ccl_ws;
struct vp_canny_ws;
void vp_canny_want(vp_ws_frame& W, int w, int h, vp_canny_ws* cw);
int vpk_canny_u8(vp_ctx* ctx, const uint8_t* d_src, int w, int h, int cn, int low, int high, uint8_t* d_dst, const vp_canny_ws& cw);
// ---- Hough lines (vp_hough.hip) ----------------------------------------------------------------------
// n frames of w x h u8 at d_src (row stride, frame stride; or one packed host image at h_src, staged in the workspace): lines of frame f
// -> lines + f * max_lines * 2 (host), true counts -> n_lines; synchronises.  Checks beyond rho / theta / min_theta / max_theta are the caller's.
int vp_hough_run(vp_ctx* ctx, const uint8_t* d_src, const uint8_t* h_src, size_t stride, size_t fstride, int n, int w, int h, double rho, double theta, int threshold,
                 double min_theta, double max_theta, float* lines, int max_lines, int* n_lines);
// sorts the first nkeys[f] 64-bit keys of each of n segments of kcap keys (d_k0, ping-ponging with d_k1) ascending; maxcnt: the largest
// count; *sorted: the buffer that holds the result (k_hough_sort_seg / k_hough_merge)
int vpk_hough_sort_keys(vp_ctx* ctx, u64* d_k0, u64* d_k1, size_t kcap, const u32* d_nkeys, int n, u32 maxcnt, u64** sorted);
// ---- Hough circles (vp_hough_circles.hip) ------------------------------------------------------------------------------------
// one w x h u8 image at d_src (row stride) or at h_src (packed host, staged): cv2.HoughCircles HOUGH_GRADIENT with maxRadius >= 0 ->
// (x, y, r) triplets at circles (host), true count -> *n_circles; synchronises.  All argument checks are done here.
int vp_hough_circles_run(vp_ctx* ctx, const uint8_t* d_src, const uint8_t* h_src, size_t stride, int w, int h, double dp, double min_dist,
                         double param1, double param2, int min_radius, int max_radius, float* circles, int max_circles, int* n_circles);
void vp_gaussian_taps(int n, double sigma, uint16_t* out);   // n odd, <= 511
void vp_gaussian_kernel_f64(int n, double sigma, double* k);  // the double kernel vp_gaussian_taps rounds: n odd, 3..511
// Gaussian adaptive threshold (vp_adaptive.hip): n frames (src row stride, frame stride) -> packed (n, h, w) dst; d_tmp: n * w * h u64
#define VP_AGAUSS_MAX_BLOCK 511
size_t vp_agauss_tmp_bytes(int w, int h, int n);
int vpk_adaptive_threshold_gaussian(vp_ctx* ctx, const uint8_t* d_src, size_t stride, size_t fstride, int n, int w, int h, int imax, int idelta,
                                    int inv, int block, uint64_t* d_tmp, uint8_t* d_dst);
int vpk_gaussian_blur(vp_ctx* ctx, const uint8_t* d_src, int w, int h, int cn, const uint16_t* d_taps, int kw, int kh, uint16_t* d_tmp, uint8_t* d_dst,
                      size_t sstride = 0);             // sstride: bytes between source rows (0: packed)
// the blur in one launch, the 8.8 intermediate kept in LDS (k_gauss_onepass); kernels for which vp_gaussian_onepass_fits only
bool vp_gaussian_onepass_fits(int kw, int kh);
int vpk_gaussian_blur_onepass(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int cn, const uint16_t* d_taps, int kw, int kh, uint8_t* d_dst);

// ---- median filter (vp_median.hip) -------------------------------------------------------------------
// cv2.medianBlur, ksize odd 1..255, borders replicated; sstride: bytes between source rows.  binary_hint: the source holds only 0 / 255;
// d_src_bits / d_dst_bits (nullable): bit planes of such a single-channel mask, read / written by the mask kernel; *made_bits
// (nullable) says whether the result's plane was written, and is left alone when the launch fails
int vpk_median_blur(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int cn, int ksize, int binary_hint, const u64* d_src_bits, uint8_t* d_dst,
                    u64* d_dst_bits, int* made_bits);

// ---- derivative filters (vp_deriv.hip; the plan: vp_deriv_plan.h) --------------------------------------
// cv2.Sobel / Scharr / Laplacian / spatialGradient as vp_deriv_make_plan accepted them; sstride: bytes between source rows; d_dst packed,
// P.esize bytes per element; d_dst2: spatialGradient's dy plane (d_dst is dx)
struct vp_deriv_plan;
int vpk_deriv(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int cn, const vp_deriv_plan& P, void* d_dst, void* d_dst2);

// ---- box filter, pyramid steps, integral (vp_box.hip, vp_pyr.hip, vp_integral.hip; the plan: vp_box_plan.h) ---------------------------
// Arguments as the plan header's checks accepted them; sstride: bytes between source rows; destinations packed.  d_mid: vp_box_mid_bytes
// of workspace for the two-pass box path (0 for the one-pass path).
struct vp_box_plan;
size_t vp_box_mid_bytes(int w, int h, int cn, const vp_box_plan& P);
int vpk_box_filter(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int cn, const vp_box_plan& P, uint16_t* d_mid, void* d_dst);
int vpk_pyr_down(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int cn, int border, uint8_t* d_dst);
int vpk_pyr_up(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int cn, uint8_t* d_dst);
int vpk_integral(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int cn, int32_t* d_dst);
// cv2.convertScaleAbs, alpha 1, beta 0 (vp_elementwise.hip): n elements of depth VP_DEPTH_* to saturate_cast<uchar>(|v|)
int vpk_convert_scale_abs(vp_ctx* ctx, const void* d_src, int depth, size_t n, uint8_t* d_dst);

// ---- histogram equalisation and CLAHE (vp_clahe.hip; the plan: vp_clahe_plan.h) -------------------------
// cv2.equalizeHist of a w x h plane (sstride: bytes between source rows): histogram, table and table-apply, three launches, enqueued.
// d_hist: 256 counters; d_lut: 256 bytes, 4-byte aligned; d_dst packed
int vpk_equalize_hist(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, u32* d_hist, uint8_t* d_lut, uint8_t* d_dst);
// cv2.createCLAHE(...).apply as vp_clahe_make_plan accepted it; d_part: tiles * 256 counters (needed when P.split > 1); d_luts: tiles * 256
// bytes, 16-byte aligned; d_dst packed; enqueued
struct vp_clahe_plan;
int vpk_clahe(vp_ctx* ctx, const uint8_t* d_src, size_t sstride, int w, int h, int tiles_x, int tiles_y, const vp_clahe_plan& P, u32* d_part, uint8_t* d_luts,
              uint8_t* d_dst);

// ---- moments (vp_moments.hip; the plan: vp_moments_plan.h) ------------------------------------------------
// The ten sums m00 m10 m01 m20 m11 m02 m30 m21 m12 m03 as unsigned 64-bit integers, of sizes vp_moments_refusal accepted; one launch
// behind the zeroing of the result, enqueued.  vpk_moments_u8: d_bits (nullable) is the mask's bit plane, read instead of its bytes
// (binary only).  vpk_label_moments_i32: d_table is (nlabels, 10); stride in bytes, a multiple of 4.
int vpk_moments_u8(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int binary, const u64* d_bits, u64* d_out10);
int vp_label_moments_lds_rows(const vp_ctx* ctx, int nlabels);   // rows of the table each block keeps in LDS
int vpk_label_moments_i32(vp_ctx* ctx, const int32_t* d_labels, size_t stride, int w, int h, int nlabels, u64* d_table);

// ---- corners (vp_corners.hip; the plan: vp_corners_plan.h) -------------------------------------------------
// The float32 response map of cv2.cornerMinEigenVal (harris 0) or cornerHarris, arguments as vp_corner_response_refusal admitted them;
// d_dst packed; one launch, enqueued.  vpk_corner_candidates: the masked maximum and goodFeaturesToTrack's candidates of a response
// map as sortable words (d_cnt: two words, the maximum's key and the true candidate count); two launches, enqueued.
int vpk_corner_response(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int block_size, int harris, double k, int border, float* d_dst);
int vpk_corner_candidates(vp_ctx* ctx, const float* d_resp, int w, int h, const uint8_t* d_mask, size_t mstride, const u64* d_bits, double quality,
                          u32* d_cnt, u64* d_keys, size_t kcap);

// ---- distance transform and min / max search (vp_dist.hip; the plan: vp_dist_plan.h) --------------------------
// cv2.distanceTransform of sizes vp_distance_transform_refusal admitted: zero pixels are the sources; d_bits (nullable) is the source's
// bit plane, read instead of its bytes; d_g: vp_dist_g_bytes(w, h) of workspace; d_dst: rows of dstride bytes, float32 or uint8 by
// depth.  Two launches, enqueued.  vpk_min_max_loc: d_out receives the two keys vp_min_max_loc_decode reads; d_mask (rows of mstride
// bytes) or d_mbits (its bit plane) admit pixels, both nullable; one launch behind the zeroing of d_out, enqueued.
int vpk_distance_transform(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, const unsigned long long* d_bits, int metric, int depth, uint16_t* d_g,
                           void* d_dst, size_t dstride);
int vpk_min_max_loc(vp_ctx* ctx, const void* d_src, size_t stride, int w, int h, int depth, const uint8_t* d_mask, size_t mstride,
                    const unsigned long long* d_mbits, unsigned long long* d_out);

// ---- colour k-means and label masks (vp_kmeans.hip; the plan: vp_kmeans_plan.h) ---------------------------------
// The whole loop of tests/kmeans_restate.py for arguments vp_kmeans_refusal admitted, enqueued: one launch that sets the table up from
// d_cinit (k * cn floats) or d_seeds (k raster indices), one of them NULL, then max_iter assign and update launches that return at
// once after the run has ended, then the label write when d_labels is given.  d_table: vp_kmeans_table_bytes(k, cn) bytes in the
// layout of the plan header; lstride in int32 elements.  vpk_label_select: 255 where select[label] != 0 (select: k host bytes, passed
// by value), the bit plane as well when d_bits is given and w % 64 == 0; one launch, enqueued.
int vpk_kmeans(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int cn, int k, const float* d_cinit, const int32_t* d_seeds, int max_iter,
               double eps, uint8_t* d_table, int32_t* d_labels, size_t lstride);
int vpk_label_select(vp_ctx* ctx, const int32_t* d_labels, size_t lstride, int w, int h, const uint8_t* select, int k, uint8_t* d_mask, size_t mstride, u64* d_bits);

// ---- template matching (vp_match.hip; the plan: vp_match_plan.h) ---------------------------------------------------
// cv2.matchTemplate for arguments vp_match_template_refusal admitted and the plan vp_match_make_plan made of them, enqueued: the
// template's statistics and packed form, the window sums the method reads, the correlation with its epilogue.  d_ws: P.ws_bytes of
// workspace, 256-byte aligned; strides in bytes.
struct vp_match_plan;
int vpk_match_template(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int cn, const uint8_t* d_templ, size_t tstride, int tw, int th, int method,
                       const vp_match_plan& P, uint8_t* d_ws, float* d_dst, size_t dstride);

// ---- colour-histogram tracking (vp_hist.hip; the plan: vp_hist_plan.h) ---------------------------------------------
// cv2.calcHist, cv2.calcBackProject and cv2.meanShift for arguments the plan header's checks admitted and the plan vp_hist_make_plan
// made of them; all enqueued.  vpk_calc_hist: zeroes the P.total counters and counts into them; d_mask (rows of mstride bytes) or
// d_mbits (its bit plane, rows of ceil(w / 64) words) admit pixels, both nullable.  vpk_back_project_fold: float32 histogram ->
// byte table.  vpk_back_project: the gather from a table of P.total bytes (a plan made for back-projection).  vpk_mean_shift: one
// block per window of d_windows (n x 4), the whole loop inside; d_out: n x 5 (x, y, w, h, iterations).
struct vp_hist_plan;
int vpk_calc_hist(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, const vp_hist_plan& P, const uint8_t* d_mask, size_t mstride, const u64* d_mbits,
                  u32* d_hist);
int vpk_back_project_fold(vp_ctx* ctx, const float* d_hist, int total, double scale, uint8_t* d_table);
int vpk_back_project(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, const vp_hist_plan& P, const uint8_t* d_table, uint8_t* d_dst, size_t dstride);
int vpk_mean_shift(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, const int32_t* d_windows, int n, int niters, int eps2, int32_t* d_out);

// ---- sparse optical flow (vp_flow.hip; the plan: vp_flow_plan.h) ----------------------------------------------------
// cv2.calcOpticalFlowPyrLK for arguments the plan header's checks admitted: one launch, one wave per point, all P.levels levels of L
// inside it; enqueued.  d_pts: n (x, y) float32; d_guess (nullable): n starting positions; max_count and eps2 already clamped;
// d_out: n x 4 words (x, y, err as float32 bits, status).
struct vp_lk_levels;
struct vp_lk_plan;
int vpk_lk_flow(vp_ctx* ctx, const vp_lk_levels& L, const vp_lk_plan& P, int win_w, int win_h, int max_count, double eps2, int flags, double min_eig,
                const float* d_pts, const float* d_guess, u32* d_out);

// ---- features (vp_features.hip; the plan: vp_features_plan.h) ---------------------------------------------------------
// FAST-9, the steered binary descriptor and the Hamming matcher for arguments the plan header's checks admitted and the plans made of
// them; all enqueued.  vpk_fast: four launches; the count and the first P.out_cap corners in raster order are left in d_ws at the
// plan's offsets.  vpk_describe: one wave per point; d_blur is the packed 7 x 7 blur of the source.  vpk_hamming_knn: the best k <= 2
// train rows of every query by (distance, index); d_partial: P.partial_bytes.  vpk_hamming_cross: clears the matches that are not mutual.
struct vp_fast_plan;
struct vp_hamming_plan_t;
int vpk_fast(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int threshold, int nonmax, const vp_fast_plan& P, uint8_t* d_ws);
int vpk_describe(vp_ctx* ctx, const uint8_t* d_src, size_t stride, const uint8_t* d_blur, int w, int h, const float* d_pts, int n, const int8_t* d_pattern,
                 unsigned grid, uint8_t* d_desc, uint8_t* d_bin, uint8_t* d_status);
int vpk_hamming_knn(vp_ctx* ctx, const uint8_t* d_q, size_t qstride, int nq, const uint8_t* d_t, size_t tstride, int nt, const vp_hamming_plan_t& P, int k,
                    int32_t* d_idx, int32_t* d_dist, void* d_partial);
int vpk_hamming_cross(vp_ctx* ctx, int32_t* d_idx, const int32_t* d_rev, int nq);
// The scale pyramid: score, suppression, the per-level cut, selection and description of all levels of a plan
// with at least one level and one point of capacity, from the levels and blurs already in d_ws; one memset and seven launches.
struct vp_pyr_plan;
int vpk_pyr_features(vp_ctx* ctx, const vp_pyr_plan& P, int threshold, const int8_t* d_pattern, uint8_t* d_ws, uint8_t* d_desc);

// ---- contour geometry (vp_geometry.hip; the plan: vp_geometry_plan.h) ------------------------------------------------------
// One launch, one wave per contour, enqueued: perimeter, hull, calipers and enclosing circle of every contour into d_rows (64-byte raw
// rows), hull vertices into d_hull (nullable; the layout of the points).  vpk_contour_geometry: contour i is counts[i] points from point
// first[i] of d_pts.  vpk_contour_geometry_batch: the buffers of a batched contour pass; rows are (n, max_contours).
struct vp_geom_raw;
int vpk_contour_geometry(vp_ctx* ctx, const int32_t* d_pts, const long long* d_first, const int32_t* d_counts, int n_contours, vp_geom_raw* d_rows,
                         int32_t* d_hull);
int vpk_contour_geometry_batch(vp_ctx* ctx, const int32_t* d_info, const int32_t* d_counts, const int32_t* d_offsets, const int32_t* d_points, int n,
                               int max_contours, long long max_points, vp_geom_raw* d_rows);
// the calipers' tail (vp_api_shapes.hip): edge (x0, y0) -> (x1, y1) and the extents amax, amin, bmax, bmin -> the five floats
void vp_min_area_rect_finish(int x0, int y0, int x1, int y1, const double* ext4, float* out5);

// ---- morphology (vp_morph.hip; the plan: vp_morph_plan.h, with vp_bitstage, vp_bitplan and vp_ww) --------------
// u8 (non-zero = 1) -> bits; d_flags[0] |= 1 if any byte is neither 0 nor 255
int vpk_pack_bits(vp_ctx* ctx, const uint8_t* d_src, size_t stride, int w, int h, int n, u64* d_bits,
                  int* d_flags /*nullable*/);
int vpk_unpack_bits(vp_ctx* ctx, const u64* d_bits, int w, int h, int n, uint8_t* d_dst);
// runs the stage plan on bit images; outputs (each nullable): bits, u8 mask
int vpk_morph_bits(vp_ctx* ctx, const vp_bitplan& plan, const u64* d_in, int w, int h, int n, u64* d_out_bits,
                   uint8_t* d_out_mask);
// generic u8 morphology, arbitrary structuring element, cn channels, one pass
int vpk_morph_generic(vp_ctx* ctx, int dilate, const uint8_t* d_src, int w, int h, int cn, const int16_t* d_offs,
                      int noffs, uint8_t* d_dst);
// span form (see vp_morph.hip): d_spans = nspans triples (dy, x0, x1); d_tab = 7 planes of w*h*cn bytes; max_len = longest span
int vpk_morph_spans(vp_ctx* ctx, int dilate, const uint8_t* d_src, int w, int h, int cn, const int16_t* d_spans, int nspans, int max_len,
                    uint8_t* d_tab, uint8_t* d_dst);
int vpk_draw_small(vp_ctx* ctx, uint8_t* d_img, int w, int h, int cn, const int32_t* pts, const int32_t* nxt, int npts, int thickness, const uint8_t* color);
int vpk_draw_segments(vp_ctx* ctx, uint8_t* d_img, int w, int h, int cn, const int32_t* d_pts, const int32_t* d_nxt, int npts, int thickness,
                      const uint8_t* color);
int vpk_add_weighted_u8(vp_ctx* ctx, const uint8_t* a, const uint8_t* b, size_t n, double alpha, double beta, double gamma, uint8_t* dst);
int vpk_absdiff_sub_u8(vp_ctx* ctx, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* dst);  // a - b saturating

// ---- filled shapes (vp_fill.hip) ------------------------------------------------------------------
// Even-odd scanline fill of vision/utils/draw.py _fill.  Where edge (a, b) meets row y (min(ya, yb) <= y < max(ya, yb)) the crossing
// xa + (y - ya) (xb - xa) / (yb - ya) is kept as an exact 64-bit key: floor(crossing) + 32768 in the high word, floor(2^32 frac) in the
// low one.  For coordinates within VP_FILL_MAX_COORD two different fractions differ by more than 2^-32, so the keys order exactly as
// the rationals do, equal crossings have equal keys, and floor / ceil are read off the key (tests/fill_restate.py).
#define VP_FILL_MAX_CROSS 256      // crossings per row the device kernel sorts (LDS); the host form has no limit
__host__ __device__ static inline u64 vp_fill_cross_key(int xa, int ya, int xb, int yb, int y)
{
    int den = yb - ya;
    long long num = (long long)(y - ya) * (xb - xa);
    if (den < 0) { den = -den; num = -num; }
    const u32 mag = (u32)(num < 0 ? -num : num), d = (u32)den;
    u32 q = mag / d, r = mag - q * d;
    int fl = (int)q;
    if (num < 0) { fl = r ? -(int)q - 1 : -(int)q; r = r ? d - r : 0; }
    return ((u64)(u32)(xa + fl + 32768) << 32) | (u32)(((u64)r << 32) / d);
}
// the rows edge (a, b) counts on, [*lo, *hi): from its upper end to just above its lower end; false for a horizontal edge.  The kernel's
// edge test, the host form's sweep and the host count of crossings per row (vp_fill_polys_dev) all go through these two.
static inline __host__ __device__ bool vp_fill_edge_rows(int ya, int yb, int* lo, int* hi)
{
    *lo = ya < yb ? ya : yb;
    *hi = ya < yb ? yb : ya;
    return ya != yb;
}
static inline __host__ __device__ bool vp_fill_edge_on_row(int ya, int yb, int y)
{
    int lo, hi;
    return vp_fill_edge_rows(ya, yb, &lo, &hi) && lo <= y && y < hi;
}
static inline __host__ __device__ int vp_fill_key_floor(u64 key) { return (int)(key >> 32) - 32768; }
static inline __host__ __device__ int vp_fill_key_ceil(u64 key) { return (int)(key >> 32) - 32768 + ((u32)key != 0); }
// vertices [first, first + count) of the point list; image rows y0 .. y0 + rows - 1 (the bounding box, clipped, rows > 0); row_base: the
// rows of the polygons before it in the list
struct vp_fill_poly { int32_t first, count, y0, rows, row_base; };
#define VP_FILL_SMALL_POLYS 8
// one wave per (polygon, row).  on_host: pts (npts <= 48 points) and polys (<= VP_FILL_SMALL_POLYS) are host arrays and travel as kernel
// arguments; otherwise both are device arrays.  The caller has made sure that no row has more than VP_FILL_MAX_CROSS crossings.
int vpk_fill_polys(vp_ctx* ctx, uint8_t* d_img, int w, int h, int cn, const int32_t* pts, int npts, const vp_fill_poly* polys, int npolys, int total_rows,
                   const uint8_t* color, bool on_host);
// columns xa .. xb of rows ya .. yb, all inside the image
int vpk_fill_rect(vp_ctx* ctx, uint8_t* d_img, int w, int h, int cn, int xa, int xb, int ya, int yb, const uint8_t* color);
// row cy + dy gets columns cx - dx .. cx + dx, dx = floor(sqrt(r r - dy dy)) as an exact integer root, clipped; r >= 0
int vpk_fill_disc(vp_ctx* ctx, uint8_t* d_img, int w, int h, int cn, int cx, int cy, int r, const uint8_t* color);

// ---- element-wise operators (vp_elementwise.hip) ------------------------------------------------
// packed uint8 images of n bytes; dst may be one of the sources of the first three.  b == nullptr: the second operand is `scalar`;
// mask (nullable): one byte per pixel of cn channels; d_bits (nullable): the result's bit plane as vpk_inrange_u8 leaves it, for a
// single-channel 0/255 result of rows of bits_w pixels - *made_bits says whether it was written
int vpk_bitwise_u8(vp_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, int scalar, const uint8_t* mask, int cn, size_t n, uint8_t* dst, int bits_w = 0,
                   u64* d_bits = nullptr, int* made_bits = nullptr);
int vpk_arith_u8(vp_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* dst);
int vpk_lut_u8(vp_ctx* ctx, const uint8_t* src, size_t n, int cn, const uint8_t* lut_host, uint8_t* dst);   // lut_host: cn tables of 256 bytes
int vpk_split_u8(vp_ctx* ctx, const uint8_t* src, size_t npx, int cn, uint8_t* p0, uint8_t* p1, uint8_t* p2, uint8_t* p3);   // null plane: not written
int vpk_merge_u8(vp_ctx* ctx, const uint8_t* p0, const uint8_t* p1, const uint8_t* p2, const uint8_t* p3, size_t npx, int cn, uint8_t* dst);
int vpk_count_nonzero_u8(vp_ctx* ctx, const uint8_t* src, size_t n, u64* d_total);   // zeroes *d_total and counts into it, enqueued

// ---- CCL (vp_ccl.hip) ----------------------------------------------------------------------------
struct vp_ccl_ws {           // per-batch scratch, all device pointers
    u32* parent;             // [n][nids]
    u32* seglabel;           // [n][nids]
    u32* flags;              // [n][nids/32]   root bitmap
    u32* prefix;             // [n][nids/32]   exclusive popcount prefix
    void* acc;               // [n][max_labels] accumulators
    u32* wordlabel;          // [n][h*ww]      label of the first segment of each word
    void* bgpart;            // [n][8]         background partial records
    // two-level path (vp_ccl2.inl); wordlabel / seglabel double as its per-word / per-segment component indices
    u32* c2_ncomp;           // [n][strips]            components per strip (0xffffffff: strip not resolved in LDS)
    void* c2_recs;           // [n][strips][C2_RC]     component records (statistics + numbering key)
    void* c2_bgbox;          // [n][strips]            bounding box of the strip's zero pixels
    u32* c2_label;           // [n][strips][C2_RC]     (strip, component) -> label
    u32* c2_crowded;         // [n]                    1: frame handed over to the crowded-frame path
    // crowded-frame path (vp_ccl3.inl); parent / flags / prefix / acc are shared with the one-level kernels, seglabel holds its u16 roots
    u32* c3_child;           // [n][nids/32]           roots that absorbed a root of another strip
    u32* c3_lroot;           // [n][nids/32]           the strip-local roots (the root bitmap before the boundary unions)
    u32* c3_clist;           // [n]                    the frames handed over, in no particular order
    u32* c3_ncrowded;        // [1]                    their number
    void* c3_state;          // [n]                    per-frame counters and totals
    unsigned char* c3_items; // [n * strips]: which labelling launch takes the strip (vp_ccl3.inl)
    u32* c3_barr;            // [n][strips + 1]        arrivals at every strip boundary
    void* c3_tot;            // [n][strips]            per strip: foreground sums and the box of its zero pixels (for the background row)
};
size_t vp_ccl_nids(int w, int h);   // multiple of 32
struct vp_canny_ws { uint16_t* mag; short2* grad; u64 *cand, *strong; int32_t* labels; uint8_t* seen; int32_t* nl; vp_ccl_ws ccl; };
void vp_ccl_ws_want(vp_ws_frame& W, int w, int h, int n, int max_labels, vp_ccl_ws* out);   // the labelling scratch of n frames, declared on the caller's frame
// scratch of a contour pass over n frames / of the hierarchy pass of one image: the totals of the workspace table of vp_contours_plan.h.
// The caller wants one region of that size (both sums with the hierarchy pass) and hands it to vpk_find_contours as (d_ws, ws_bytes)
size_t vp_contours_ws_bytes(int w, int h, int n, int max_contours);
size_t vp_contour_tree_ws_bytes(int max_contours);
int vpk_contour_features(vp_ctx* ctx, const int32_t* d_info, const int32_t* d_counts, const int32_t* d_offsets, const int32_t* d_points, int n,
                         int max_contours, long long max_points, double* d_features);
// contours of n bit images (no labelling involved: vp_contours.inl; every host decision: ct_make_plan, vp_contours_plan.h).  many_heads:
// the caller expects a frame with very many border segments (ct_want_many of its last pass's count, d_nheads_out / vp_ct_batch_hint) - a
// choice between two forms of the same steps, not of the result.
// host (n == 1 only): pinned, device-visible buffers the producing kernels write the results into as well - info {n_contours,
// n_points, heads}, counts / offsets / is_hole [max_contours], the first points_cap points - so that the caller only synchronises.
// defer_big (n == 1, not many_heads): a frame with more heads than the one block's LDS tables hold reports n_contours = -1 and nothing
// else; the caller repeats the pass with many_heads.
uint32_t vp_ct_batch_hint(vp_ctx* ctx);      // largest head count the last batched pass reported (a guess; no synchronisation)
// d_hier (n == 1 only, [max_contours][4]): RETR_CCOMP / RETR_TREE, which need it - the hierarchy rows in cv2's order (the contour arrays
// stay in device order, reversed by the caller); the modes 0 / 1 take it as NULL.  host->hier: the same rows in the pinned buffer.
struct vp_contour_mirror { int32_t* info; int32_t* counts; int32_t* offsets; uint8_t* is_hole; int32_t* points; long long points_cap; int32_t* hier; };
int vpk_find_contours(vp_ctx* ctx, uint8_t* d_ws, size_t ws_bytes, const u64* d_bits, int w, int h, int n, int mode, int method, int32_t* d_counts,
                      uint8_t* d_is_hole, int32_t* d_offsets, int32_t* d_points, int max_contours, long long max_points, int32_t* d_info, bool many_heads = false,
                      uint32_t* d_nheads_out = nullptr, const vp_contour_mirror* host = nullptr, bool defer_big = false, int32_t* d_hier = nullptr);
int vpk_ccl(vp_ctx* ctx, const u64* d_bits, int w, int h, int n, int numbering, const vp_ccl_ws& ws, int32_t* d_labels,
            int32_t* d_stats, double* d_centroids, int max_labels, int32_t* d_nlabels);

// Timing switches of the measurement build (-DVP_PROBE, tools/build_probe.sh): kernels skip the named part of their work, so results
// are wrong while one is set.  vp_debug_set (vp_ccl.hip) sets them; the product build compiles every test to `false`.
enum { VP_DBG_C3_NO_BOUND = 1, VP_DBG_C3_WALK_ONLY = 2, VP_DBG_C3_NO_UNIONS = 4, VP_DBG_C3_NO_STATS = 8, VP_DBG_C3_NO_LABELS = 16,   // vp_ccl3.inl
       VP_DBG_MORPH_NO_STAGES = 0x100, VP_DBG_MORPH_NO_LOAD = 0x200, VP_DBG_MORPH_NO_BITS = 0x400, VP_DBG_MORPH_NO_MASK = 0x800 };  // k_morph_bits_sym
#ifdef VP_PROBE
#define VP_DBG(bit) ((vp_dbg_bits & (bit)) != 0)     // vp_dbg_bits: a __device__ int of each unit that tests it (vp_ccl.hip, vp_morph.hip)
int vp_morph_debug_set(int bits);                   // vp_morph.hip's copy
#else
#define VP_DBG(bit) false
#endif

// 16-byte streaming store for write-once outputs (masks, labels).  VP_NT_STORES selects the nontemporal form.
#ifndef VP_NT_STORES
#define VP_NT_STORES 1
#endif
typedef int vp_v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void vp_store16(void* dst, u32 a, u32 b, u32 c, u32 d)
{
    vp_v4i v = {(int)a, (int)b, (int)c, (int)d};
#if VP_NT_STORES
    __builtin_nontemporal_store(v, reinterpret_cast<vp_v4i*>(dst));
#else
    *reinterpret_cast<vp_v4i*>(dst) = v;
#endif
}
