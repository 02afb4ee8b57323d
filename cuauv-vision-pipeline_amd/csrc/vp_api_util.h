// Helpers shared by the C-ABI units (vp_api*.hip) only: the kernel units include vp_internal.h and never this file.
#pragma once
#include "vp_internal.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#define VP_TRY(x) do { int rc__ = (x); if (rc__ != VP_OK) return rc__; } while (0)

static inline int h2d(vp_ctx* ctx, void* d, const void* h, size_t n)
{
    VP_HIP(ctx, hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, ctx->stream));
    return VP_OK;
}
static inline int d2h(vp_ctx* ctx, void* h, const void* d, size_t n)
{
    VP_HIP(ctx, hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, ctx->stream));
    return VP_OK;
}
static inline int h2d_rows(vp_ctx* ctx, void* d, size_t dpitch, const void* h, size_t spitch, size_t rowbytes, size_t rows)
{
    if (spitch == rowbytes && dpitch == rowbytes) return h2d(ctx, d, h, rowbytes * rows);
    VP_HIP(ctx, hipMemcpy2DAsync(d, dpitch, h, spitch, rowbytes, rows, hipMemcpyHostToDevice, ctx->stream));
    return VP_OK;
}

static inline int check_ctx(vp_ctx* ctx)
{
    if (!ctx) return VP_ERR_INVALID;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return vp_fail(ctx, VP_ERR_HIP, "hipSetDevice", e);
    return VP_OK;
}

// [a, a + an) and [b, b + bn) share a byte
static inline bool dev_overlap(const void* a, size_t an, const void* b, size_t bn)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bn && pb < pa + an;
}
static inline size_t strided_bytes(size_t stride, size_t rowbytes, int h) { return (size_t)(h - 1) * stride + rowbytes; }

// cv2.inRange bound normalisation (arithm.cpp): empty when lo > hi, lo > 255 or hi < 0 (the in-range entries and the chain)
static inline void norm_range(int cn, const int32_t* lo, const int32_t* hi, vp_range3* q)
{
    for (int c = 0; c < 3; c++) {
        if (c >= cn) { q->lo[c] = 0; q->hi[c] = 255; continue; }
        int l = lo[c], u = hi[c];
        if (l > u || l > 255 || u < 0) { l = 1; u = 0; }
        else { if (l < 0) l = 0; if (u > 255) u = 255; }
        q->lo[c] = l;
        q->hi[c] = u;
    }
}

// Ring of pinned chunks for small host -> device hand-overs (see vp_ctx; defined in vp_api.hip): the chunk is the caller's until
// vp_ring_done, and is handed out again only after everything queued on the context's stream up to vp_ring_done has run.
uint8_t* vp_ring_take(vp_ctx* ctx, size_t bytes, int* slot);   // NULL: out of pinned memory
void vp_ring_done(vp_ctx* ctx, int slot);
