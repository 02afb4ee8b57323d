// Host arithmetic of cv2.createCLAHE(...).apply on 8-bit single-channel images (vpk_clahe, vp_clahe.hip): the argument check, the
// padded geometry with OpenCV's both-or-neither padding, the integer clip limit, how many blocks share one tile's histogram, and the
// launch geometry and LDS budget of the interpolation kernel.  Plain C++ - no HIP types, no kernels - and a pure function of its
// arguments, like vp_median_plan.h and vp_deriv_plan.h.
#pragma once

#define CL_MAX_TILES 64            // tiles per axis at most
#define CL_MAX_PIXELS (1 << 28)    // pixels per image at most: every count, and the area of a tile of the extended image, fits an int
#define CL_HIST_BLOCK 256          // threads of the histogram and table kernels: one per bin
#define CL_MAX_SPLIT 64            // blocks that share one tile at most
#define CL_PART_PIXELS 8192        // the default share: the fewest blocks per tile that leave no block more than this many pixels
#define CL_APPLY_BLOCK 256         // threads of the interpolation kernel, four result bytes each
#define CL_APPLY_ROWS 8            // result rows per block
#define CL_LDS_BUDGET 65536        // bytes of tile tables the interpolation kernel stages in LDS; above it they are read from device memory

enum { VP_CLAHE_OK = 0, VP_CLAHE_INVALID = 1, VP_CLAHE_UNSUPPORTED = 2 };

struct vp_clahe_plan {
    int status;                    // VP_CLAHE_*: everything below is meaningful for VP_CLAHE_OK only
    int padded;                    // 1: tiles are cut from the image extended right and down by reflection (BORDER_REFLECT_101)
    int ext_w, ext_h;              // size of the image the tiles are cut from
    int tile_w, tile_h, area;      // one tile
    int clip;                      // integer clip limit per bin; 0: no clipping
    float lut_scale;               // float32(255) / float32(area)
    int split;                     // blocks that share one tile's histogram; 1: one block does histogram, clip, scan and table
    int part_rows;                 // tile rows per block, split * part_rows >= tile_h
    int tables_in_lds;             // interpolation: all tile tables staged in LDS
    unsigned lds_bytes;            // ... dynamic LDS of that launch
    unsigned hist_gx, hist_gy;     // histogram launch: (tiles, split)
    unsigned apply_gx;             // interpolation launch: row bands
};

// opt_split: VP_OPT_CLAHE_SPLIT (0 the measured choice, n >= 1 that many blocks per tile, capped by the tile's rows and CL_MAX_SPLIT).
// The default is reasoned, not yet measured (tools/exp_clahe.py times every share): see CL_PART_PIXELS.
static inline vp_clahe_plan vp_clahe_make_plan(int w, int h, double clip_limit, int tiles_x, int tiles_y, int opt_split)
{
    vp_clahe_plan P = {VP_CLAHE_INVALID, 0, 0, 0, 0, 0, 0, 0, 0.f, 1, 0, 0, 0, 0, 0, 0};
    if (w <= 0 || h <= 0 || tiles_x < 1 || tiles_y < 1 || clip_limit != clip_limit) return P;
    P.status = VP_CLAHE_UNSUPPORTED;
    if (tiles_x > CL_MAX_TILES || tiles_y > CL_MAX_TILES || (long long)w * h > CL_MAX_PIXELS) return P;
    P.ext_w = w;
    P.ext_h = h;
    if (w % tiles_x != 0 || h % tiles_y != 0) {          // both amounts whenever either dimension fails to divide (a whole tile count then)
        const int pad_x = tiles_x - w % tiles_x, pad_y = tiles_y - h % tiles_y;
        if (pad_x >= w || pad_y >= h) return P;          // single reflection only
        P.padded = 1;
        P.ext_w = w + pad_x;
        P.ext_h = h + pad_y;
    }
    P.tile_w = P.ext_w / tiles_x;
    P.tile_h = P.ext_h / tiles_y;
    P.area = P.tile_w * P.tile_h;                        // <= (2 w) (2 h) / tiles, and ext_w * ext_h < 4 * 2^28: no overflow
    if (clip_limit > 0) {
        const double c = clip_limit * P.area / 256;      // OpenCV casts this to int: undefined from 2^31 on
        if (!(c < 2147483648.0)) return P;
        P.clip = (int)c > 1 ? (int)c : 1;
    }
    P.lut_scale = 255.f / (float)P.area;
    int split = opt_split;
    if (split < 1) {
        split = 1;
        while (split < CL_MAX_SPLIT && (P.area + split - 1) / split > CL_PART_PIXELS) split *= 2;
    }
    if (split > CL_MAX_SPLIT) split = CL_MAX_SPLIT;
    if (split > P.tile_h) split = P.tile_h;
    P.part_rows = (P.tile_h + split - 1) / split;
    P.split = (P.tile_h + P.part_rows - 1) / P.part_rows;    // no block without a row
    P.hist_gx = (unsigned)(tiles_x * tiles_y);
    P.hist_gy = (unsigned)P.split;
    const unsigned table_bytes = (unsigned)(tiles_x * tiles_y) * 256u;
    P.tables_in_lds = table_bytes <= CL_LDS_BUDGET ? 1 : 0;
    P.lds_bytes = P.tables_in_lds ? table_bytes : 0;
    P.apply_gx = (unsigned)((h + CL_APPLY_ROWS - 1) / CL_APPLY_ROWS);
    P.status = VP_CLAHE_OK;
    return P;
}
