// Tile constants and argument checks of the moment kernels (vp_moments.hip), shared with the C ABI (vp_api_moments.hip); the tests
// read the numbers from this file.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define MM_TB 256             // threads of a block: 4 waves
#define MM_CHUNK 16           // bytes a lane loads of a byte image (one 16-byte aligned load)
#define MM_SPAN 1024          // bytes a wave covers of one row: 64 lanes x MM_CHUNK
#define MM_BIT_SPAN 4096      // pixels a wave covers of one bit-plane row: 64 lanes x one 64-bit word
#define MM_ROWS 8             // rows of a block, dealt to its waves in turn
#define LM_SPAN 1024          // label pixels a wave walks along one row, 64 at a time (runs are stitched across the steps)
#define LM_ROWS 16            // rows of a block, dealt to its waves in turn
#define LM_LDS_LABELS 768     // most labels whose (nlabels, 10) 64-bit table is kept in a block's LDS: 768 * 80 B = 60 KiB
#define LM_HOT_LABELS 64      // rows of a larger table a block still keeps in LDS: the first ones, the background among them

// Worst-case m30 / m03 of a w x h image of values <= vmax: vmax * h * sum_{x < w} x^3 and the transpose.  The kernels add in unsigned
// 64-bit and every other moment is at most the larger of the two (x^p y^q <= (p x^3 + q y^3) / 3 for p + q = 3), so below 2^63 no
// sum wraps.  The bound itself is computed without wrapping: false as soon as it reaches 2^63.
static inline bool vp_moments_bound_ok(int w, int h, int vmax)
{
    const unsigned __int128 lim = (unsigned __int128)1 << 63;
    const unsigned __int128 tw = (unsigned __int128)((uint64_t)w * (uint64_t)(w - 1) / 2), th = (unsigned __int128)((uint64_t)h * (uint64_t)(h - 1) / 2);
    // (w, h < 2^31: the triangular numbers are below 2^61, their squares below 2^122, times h and vmax below 2^128 only while small:
    // compare step by step)
    const unsigned __int128 cw = tw * tw, ch = th * th;
    if (cw >= lim || ch >= lim) return false;
    const unsigned __int128 bw = cw * (unsigned)h, bh = ch * (unsigned)w;          // < 2^63 * 2^31
    if (bw >= lim || bh >= lim) return false;
    return bw * (unsigned)vmax < lim && bh * (unsigned)vmax < lim;                   // < 2^63 * 2^8
}

// what both raster entries and both label entries refuse before anything is launched; NULL: accepted
static inline const char* vp_moments_refusal(int w, int h, size_t stride, size_t elem, int vmax)
{
    if (w < 1 || h < 1) return "moments: w and h must be at least 1";
    if (h > 65535) return "moments: h must be at most 65535";
    if (stride < (size_t)w * elem) return "moments: the stride is below the row";
    if (!vp_moments_bound_ok(w, h, vmax)) return "moments: the worst-case m30 / m03 of this size reaches 2^63";
    return NULL;
}
