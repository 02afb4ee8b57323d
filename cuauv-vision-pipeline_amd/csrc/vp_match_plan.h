// Host arithmetic of cv2.matchTemplate (vp_match.hip): the argument checks as this library admits them, the bounds that keep every sum
// an exact unsigned 32-bit integer, the packed template's layout, the tile and chunk geometry of the correlation kernel with its LDS
// budget, and the layout of the workspace.  Plain C++ - no HIP types, no kernels - and a pure function of its arguments, like
// vp_dist_plan.h.  DESIGN.md section 4.27; tests/match_template_restate.py is the statement.
#pragma once
#include <stddef.h>
#include <stdint.h>

// methods (cv2's TM_* values) and the admitted sizes
#define MT_SQDIFF 0
#define MT_SQDIFF_NORMED 1
#define MT_CCORR 2
#define MT_CCORR_NORMED 3
#define MT_CCOEFF 4
#define MT_CCOEFF_NORMED 5
#define MT_MAX_SIDE 4096       // rows and columns of the image
#define MT_MAX_CN 4
#define MT_MAX_ELEMS 65536     // tw * th * cn: the bytes of a template

// The correlation kernel.  A row of an image of cn channels is a row of w * cn bytes and a template row a row of tw * cn bytes, padded
// with zero bytes to whole words: result x reads from byte x * cn.  A block of MT_THREADS = MT_LANES_X x MT_LANES_Y lanes owns
// MT_TILE_W x MT_TILE_H results, a lane MT_RX neighbouring results of MT_RY neighbouring rows; its first byte, lane_x * MT_RX * cn, is
// word aligned.  The template is walked in chunks of at most MT_CHUNK_ROWS rows by MT_CHUNK_WORDS words; a block stages the chunk
// (between MT_RY - 1 rows of zeros on either side) and the image patch under it in LDS.
#define MT_RX 4
#define MT_RY 4
#define MT_LANES_X 32
#define MT_LANES_Y 8
#define MT_THREADS 256
#define MT_TILE_W 128
#define MT_TILE_H 32
#define MT_CHUNK_ROWS 16
#define MT_CHUNK_WORDS 64
#define MT_PATCH_SLACK 4       // words of a patch row past the tile's and the chunk's: the shifted words of the last lane
#define MT_LDS_BYTES 65536     // dynamic LDS a block of this library may use

// the window sums: wrapping uint32 integrals of (h + 1) x (w + 1) entries, the column pass in MT_INT_SEGS row segments per block
#define MT_INT_SEGS 16
#define MT_INT_COLS 64

static_assert(MT_THREADS == MT_LANES_X * MT_LANES_Y && MT_TILE_W == MT_LANES_X * MT_RX && MT_TILE_H == MT_LANES_Y * MT_RY, "match template: lanes times results is the tile");
static_assert(MT_RX == 4, "match template: a lane's first byte, lane_x * MT_RX * cn, must be word aligned for every cn");
static_assert(MT_CHUNK_WORDS % 4 == 0, "match template: template words are read four at a time");
static_assert(((MT_RX - 1) * MT_MAX_CN) / 4 + 2 <= MT_PATCH_SLACK + 1, "match template: the last lane's shifted words leave the patch row");
// every sum is below 2^32 and every product with N below 2^48, so uint32 accumulators and double conversions are exact
static_assert(255ull * 255ull * MT_MAX_ELEMS < (1ull << 32), "match template: a sum of products above uint32");
static_assert(255ull * 255ull * MT_MAX_ELEMS * MT_MAX_ELEMS < (1ull << 48), "match template: N times a sum above 2^48");
// the largest block: a full chunk under a full tile of 4-channel results
static_assert(((MT_TILE_H + MT_CHUNK_ROWS - 1) * (MT_LANES_X * MT_MAX_CN + MT_CHUNK_WORDS + MT_PATCH_SLACK) + 3 + (MT_CHUNK_ROWS + 2 * (MT_RY - 1)) * MT_CHUNK_WORDS) * 4
                  <= MT_LDS_BYTES,
              "match template: patch and chunk above the LDS budget");

struct vp_match_plan {
    int rw, rh;                // the result
    int twb;                   // bytes of a template row, tw * cn
    int tpitch;                // words of a packed template row: ceil(twb / 4) rounded up to a multiple of 4, zero padded
    int chunk_rows;            // template rows a block stages at a time: min(th, MT_CHUNK_ROWS)
    int chunk_words;           // ... and words of each: min(tpitch, MT_CHUNK_WORDS)
    int row_chunks, col_chunks;
    int one_piece;             // the whole template is one chunk
    int patch_rows;            // MT_TILE_H + chunk_rows - 1
    int patch_pitch;           // words: MT_LANES_X * cn + chunk_words + MT_PATCH_SLACK
    int templ_off;             // words from the patch to the chunk in LDS (a multiple of 4)
    size_t lds_bytes;
    unsigned grid_x, grid_y;
    int need_s1, need_s2;      // which window sums the method reads
    int planes;                // integrals: need_s2 + need_s1 * cn, the squares first
    int ipitch;                // entries of an integral row, w + 1
    // workspace, byte offsets (all multiples of 256): template statistics, packed template, integrals
    size_t off_stats, off_templ, off_integral, ws_bytes;
};

// what the statistics kernel leaves at off_stats
struct vp_match_stats {
    unsigned long long t2;             // sum of T^2
    unsigned long long t1[MT_MAX_CN];  // sum of T per channel
    unsigned long long tn_int;         // N * t2 - sum_c t1[c]^2 (CCOEFF_NORMED), else N * t2
    double templ_norm;                 // sqrt(double(tn_int) / double(N))
};

#ifdef __HIPCC__
#define VP_MATCH_HD __host__ __device__
#else
#define VP_MATCH_HD
#endif
VP_MATCH_HD static inline int vp_match_normed(int method) { return method == MT_SQDIFF_NORMED || method == MT_CCORR_NORMED || method == MT_CCOEFF_NORMED; }
static inline size_t vp_match_align(size_t n) { return (n + 255) / 256 * 256; }

// NULL: admitted; else the reason (VP_ERR_INVALID).  Strides in bytes; dst_stride of the float32 result.
static inline const char* vp_match_template_refusal(int w, int h, int cn, size_t stride, int tw, int th, size_t templ_stride, int method, size_t dst_stride)
{
    if (w < 1 || h < 1) return "match template: width and height must be at least 1";
    if (w > MT_MAX_SIDE || h > MT_MAX_SIDE) return "match template: width and height must be at most 4096";
    if (cn < 1 || cn > MT_MAX_CN) return "match template: 1 to 4 channels";
    if (tw < 1 || th < 1) return "match template: the template's width and height must be at least 1";
    if (tw > w || th > h) return "match template: the template is larger than the image";
    if ((long long)tw * th * cn > MT_MAX_ELEMS) return "match template: the template holds more than 65536 bytes";
    if (method < MT_SQDIFF || method > MT_CCOEFF_NORMED) return "match template: the method must be one of the six TM_* values";
    if (stride < (size_t)w * cn) return "match template: the stride is below the row";
    if (templ_stride < (size_t)tw * cn) return "match template: the template's stride is below its row";
    if (dst_stride < (size_t)(w - tw + 1) * 4) return "match template: the result's stride is below the row";
    if (dst_stride % 4) return "match template: the result's stride is not a multiple of the element size";
    return nullptr;
}

// arguments as vp_match_template_refusal admitted them
static inline void vp_match_make_plan(int w, int h, int cn, int tw, int th, int method, vp_match_plan* P)
{
    P->rw = w - tw + 1;
    P->rh = h - th + 1;
    P->twb = tw * cn;
    P->tpitch = ((P->twb + 3) / 4 + 3) / 4 * 4;
    P->chunk_rows = th < MT_CHUNK_ROWS ? th : MT_CHUNK_ROWS;
    P->chunk_words = P->tpitch < MT_CHUNK_WORDS ? P->tpitch : MT_CHUNK_WORDS;
    P->row_chunks = (th + MT_CHUNK_ROWS - 1) / MT_CHUNK_ROWS;
    P->col_chunks = (P->tpitch + MT_CHUNK_WORDS - 1) / MT_CHUNK_WORDS;
    P->one_piece = P->row_chunks == 1 && P->col_chunks == 1;
    P->patch_rows = MT_TILE_H + P->chunk_rows - 1;
    P->patch_pitch = MT_LANES_X * cn + P->chunk_words + MT_PATCH_SLACK;
    P->templ_off = (P->patch_rows * P->patch_pitch + 3) / 4 * 4;
    P->lds_bytes = ((size_t)P->templ_off + (size_t)(P->chunk_rows + 2 * (MT_RY - 1)) * P->chunk_words) * 4;
    P->grid_x = (unsigned)((P->rw + MT_TILE_W - 1) / MT_TILE_W);
    P->grid_y = (unsigned)((P->rh + MT_TILE_H - 1) / MT_TILE_H);
    P->need_s2 = method == MT_SQDIFF || method == MT_SQDIFF_NORMED || method == MT_CCORR_NORMED || method == MT_CCOEFF_NORMED;
    P->need_s1 = method == MT_CCOEFF || method == MT_CCOEFF_NORMED;
    P->planes = P->need_s2 + P->need_s1 * cn;
    P->ipitch = w + 1;
    P->off_stats = 0;
    P->off_templ = vp_match_align(sizeof(vp_match_stats));
    P->off_integral = P->off_templ + vp_match_align((size_t)th * P->tpitch * 4);
    P->ws_bytes = P->off_integral + vp_match_align((size_t)P->planes * (h + 1) * P->ipitch * 4);
}
