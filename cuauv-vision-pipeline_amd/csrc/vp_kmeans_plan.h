// Host arithmetic of the colour k-means (vp_kmeans.hip, DESIGN.md section 4.26, tests/kmeans_restate.py): the admitted arguments, the
// launch geometry, the bounds that keep every sum an exact integer, the layout of the device table and the compactness the host
// computes from it.  Plain C++ - no HIP types, no kernels - and a pure function of its arguments, like vp_dist_plan.h.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define KM_MAX_SIDE 4096       // rows and columns: N = w h <= 2^24
#define KM_MAX_K 256
#define KM_MAX_CN 4
#define KM_MAX_ITER 100
#define KM_LDS_BYTES 65536     // static LDS a block of this library may use

// assign-and-reduce: 256 threads; a lane takes KM_PX neighbouring pixels of one row at a time (KM_PX * cn bytes, whole 32-bit words
// when the row starts on one), KM_ITERS times; a block therefore never sees more than KM_BLOCK_PX pixels
#define KM_THREADS 256
#define KM_PX 4
#define KM_ITERS 4
#define KM_BLOCK_CHUNKS (KM_THREADS * KM_ITERS)
#define KM_BLOCK_PX (KM_BLOCK_CHUNKS * KM_PX)

// the device-side state word of a run
#define KM_RUNNING 0           // the next assign pass is followed by an update
#define KM_LAST 1              // converged: one more assign pass with the new centres, then done
#define KM_DONE 2              // assign and update launches return after reading this word

static_assert((long long)KM_MAX_SIDE * KM_MAX_SIDE <= (1ll << 24), "k-means: N above 2^24");
static_assert(255ll * KM_MAX_SIDE * KM_MAX_SIDE < (1ll << 32), "k-means: a global S1 above uint32");
static_assert(KM_BLOCK_PX <= 65536 && 65025ll * KM_BLOCK_PX < (1ll << 32), "k-means: a block-local S2 above uint32");
static_assert(65025ll * KM_MAX_SIDE * KM_MAX_SIDE < (1ll << 53), "k-means: a global S2 that double(S2) would round");
static_assert(KM_MAX_K <= KM_THREADS, "k-means: the update gives every cluster a thread of its one block");
// LDS of the assign kernel at k = 256, cn = 4: the centres as doubles and the table of n, S1, S2 (uint32 each)
#define KM_LDS_CENTRES(k, cn) ((k) * (cn) * 8)
#define KM_LDS_TABLE(k, cn) ((k) * (1 + 2 * (cn)) * 4)
static_assert(KM_LDS_CENTRES(KM_MAX_K, KM_MAX_CN) + KM_LDS_TABLE(KM_MAX_K, KM_MAX_CN) < KM_LDS_BYTES, "k-means: the assign kernel above 64 KiB of LDS");

static inline unsigned vp_kmeans_chunks_per_row(int w) { return (unsigned)((w + KM_PX - 1) / KM_PX); }
static inline unsigned vp_kmeans_blocks(int w, int h)
{
    const unsigned total = vp_kmeans_chunks_per_row(w) * (unsigned)h;       // at most 1024 * 4096
    return (total + KM_BLOCK_CHUNKS - 1) / KM_BLOCK_CHUNKS;
}

// The device table of a run, one allocation that comes back in one copy: S2 first (64-bit), then the two state words {state,
// assign passes so far} and two words of padding, the centres, n and S1.
static inline size_t vp_kmeans_off_s2(int, int) { return 0; }
static inline size_t vp_kmeans_off_state(int k, int cn) { return (size_t)k * cn * 8; }
static inline size_t vp_kmeans_off_centres(int k, int cn) { return vp_kmeans_off_state(k, cn) + 16; }
static inline size_t vp_kmeans_off_n(int k, int cn) { return vp_kmeans_off_centres(k, cn) + (size_t)k * cn * 4; }
static inline size_t vp_kmeans_off_s1(int k, int cn) { return vp_kmeans_off_n(k, cn) + (size_t)k * 4; }
static inline size_t vp_kmeans_table_bytes(int k, int cn) { return vp_kmeans_off_s1(k, cn) + (size_t)k * cn * 4; }

// what vp_kmeans_* write at out_host; centers[k * cn] and counts[k] follow the header
struct vp_kmeans_result_head { double compactness; int32_t iterations; int32_t k; };
static inline size_t vp_kmeans_result_bytes(int k, int cn) { return sizeof(vp_kmeans_result_head) + (size_t)k * cn * 4 + (size_t)k * 4; }

// sum over k (outer) and ch (inner) of ((S2 - (2 c) S1) + (n c) c), every operation rounded separately (the units are built with
// -ffp-contract=off): the sum of |p - c|^2 of the last pass up to double rounding, and the same bits on every run
static inline double vp_kmeans_compactness(int k, int cn, const float* centres, const uint32_t* n, const uint32_t* s1, const uint64_t* s2)
{
    double total = 0.0;
    for (int i = 0; i < k; i++)
        for (int ch = 0; ch < cn; ch++) {
            const double c = (double)centres[i * cn + ch], a = (double)s1[i * cn + ch], b = (double)s2[i * cn + ch], m = (double)n[i];
            total = total + ((b - (2.0 * c) * a) + (m * c) * c);
        }
    return total;
}

// NULL: admitted; else the reason (VP_ERR_INVALID).  stride in bytes; centers_init / seed_index are host arrays (one of them NULL).
static inline const char* vp_kmeans_refusal(int w, int h, size_t stride, int cn, int k, const float* centers_init, const int32_t* seed_index, int max_iter,
                                            double eps)
{
    if (w < 1 || h < 1) return "kmeans: width and height must be at least 1";
    if (w > KM_MAX_SIDE || h > KM_MAX_SIDE) return "kmeans: width and height must be at most 4096";
    if (cn < 1 || cn > KM_MAX_CN) return "kmeans: 1 to 4 channels";
    if (stride < (size_t)w * cn) return "kmeans: the stride is below the row";
    if (k < 1 || k > KM_MAX_K) return "kmeans: k must be in 1..256";
    if ((long long)k > (long long)w * h) return "kmeans: k is above the number of samples";
    if ((centers_init != nullptr) == (seed_index != nullptr)) return "kmeans: exactly one of centers_init and seed_index must be given";
    if (max_iter < 1 || max_iter > KM_MAX_ITER) return "kmeans: max_iter must be in 1..100";
    if (!(eps >= 0.0) || !isfinite(eps)) return "kmeans: eps must be finite and not negative";
    if (centers_init)
        for (int i = 0; i < k * cn; i++)
            if (!isfinite(centers_init[i])) return "kmeans: an initial centre is not finite";
    if (seed_index)
        for (int i = 0; i < k; i++)
            if (seed_index[i] < 0 || (long long)seed_index[i] >= (long long)w * h) return "kmeans: a seed index is outside 0..N-1";
    return nullptr;
}

// strides in bytes
static inline const char* vp_kmeans_labels_refusal(int w, size_t labels_stride)
{
    if (labels_stride < (size_t)w * 4) return "kmeans: the label stride is below the row";
    if (labels_stride % 4) return "kmeans: the label stride is not a multiple of 4";
    return nullptr;
}

static inline const char* vp_label_select_refusal(int w, int h, size_t labels_stride, int k, size_t mask_stride)
{
    if (w < 1 || h < 1) return "label select: width and height must be at least 1";
    if (w > KM_MAX_SIDE || h > KM_MAX_SIDE) return "label select: width and height must be at most 4096";
    if (k < 1 || k > KM_MAX_K) return "label select: k must be in 1..256";
    if (labels_stride < (size_t)w * 4) return "label select: the label stride is below the row";
    if (labels_stride % 4) return "label select: the label stride is not a multiple of 4";
    if (mask_stride < (size_t)w) return "label select: the mask's stride is below the row";
    return nullptr;
}
