// The span writer of the fill kernels (vp_fill.hip), in a header of its own so that a host program can run it lane by lane
// (tests/native/fill_span_main.cpp): the includer provides u32, uint4 and, outside hipcc, VP_FILL_DEV.
#pragma once
#ifndef VP_FILL_DEV
#define VP_FILL_DEV __device__ __forceinline__
#endif

// nb bytes from p, the first byte being channel 0 of a pixel: byte o gets channel o % cn of the colour word cw.  Lanes 0-15 write the
// bytes in front of the first 16-byte boundary, lanes 16-31 those behind the last one, all lanes the aligned chunks in between.
VP_FILL_DEV u32 fill_pattern(u32 cw, int cn, u32 r)
{
    u32 v = 0;
    for (int k = 0; k < 4; k++) {
        v |= ((cw >> (8 * r)) & 255u) << (8 * k);
        r = r + 1 == (u32)cn ? 0 : r + 1;
    }
    return v;
}
VP_FILL_DEV void fill_span(uint8_t* __restrict__ p, u32 nb, u32 cw, int cn, int lane)
{
    const u32 to_boundary = (u32)((16 - ((uintptr_t)p & 15)) & 15);
    const u32 head = nb < to_boundary ? nb : to_boundary;
    const u32 nchunk = (nb - head) >> 4;
    const u32 tail0 = head + (nchunk << 4);
    if (lane < 16) {
        if ((u32)lane < head) p[lane] = (uint8_t)(cw >> (8 * ((u32)lane % (u32)cn)));
    } else if (lane < 32) {
        const u32 o = tail0 + (u32)(lane - 16);
        if (o < nb) p[o] = (uint8_t)(cw >> (8 * (o % (u32)cn)));
    }
    for (u32 i = (u32)lane; i < nchunk; i += 64) {
        const u32 o = head + (i << 4);
        u32 r = o % (u32)cn;
        uint4 v;
        v.x = fill_pattern(cw, cn, r); r = (r + 4) % (u32)cn;
        v.y = fill_pattern(cw, cn, r); r = (r + 4) % (u32)cn;
        v.z = fill_pattern(cw, cn, r); r = (r + 4) % (u32)cn;
        v.w = fill_pattern(cw, cn, r);
        *reinterpret_cast<uint4*>(p + o) = v;
    }
}
// columns xa .. xb of row y, clipped to the image
VP_FILL_DEV void fill_columns(uint8_t* __restrict__ img, int w, int cn, int y, long long xa, long long xb, u32 cw, int lane)
{
    if (xa < 0) xa = 0;
    if (xb > w - 1) xb = w - 1;
    if (xa > xb) return;
    fill_span(img + ((size_t)y * (size_t)w + (size_t)xa) * (size_t)cn, (u32)(xb - xa + 1) * (u32)cn, cw, cn, lane);
}
