// The cases of tests/golden/contours_plan.txt, in order: what tests/native/contours_plan_main.cpp runs the plan on, and what the program
// that recorded the file from the dispatcher (before the plan had a header of its own) ran the dispatcher's expressions on.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct ct_case {
    int w, h, n, mode, method, mc;
    bool hier, mirror, many, defer;
    uint32_t hint;
    size_t sort;     // stands for what the radix sort would ask for
};

template <typename F> static void ct_each_case(F emit)
{
    static const int W[] = {1, 63, 64, 65, 1920, 3840}, H[] = {1, 2, 255, 256, 257, 1080, 2160}, N[] = {1, 8, 9, 64, 65, 256, 257};
    static const int MC[] = {1, 2, 3, 4, 64, 255, 256, 257, 4096, 262144};       // 262144: nb = 1025, jb and jtb at their cap of 1024
    static const uint32_t HINT[] = {0, 1, 2730, 2731, 8192, 8193, 600000};
    const ct_case base = {1920, 1080, 1, 1, 2, 64, false, true, false, false, 0, 0};
    for (int many = 0; many <= 1; many++) {
        // every frame size, one image and a batch on the far side of n = 8
        for (int w : W)
            for (int h : H)
                for (int n : {1, 9}) { ct_case c = base; c.w = w; c.h = h; c.n = n; c.many = many; c.mirror = n == 1; emit(c); }
        // every batch size, a large and a small frame
        for (int n : N)
            for (int small = 0; small <= 1; small++) { ct_case c = base; if (small) { c.w = 65; c.h = 257; } c.n = n; c.many = many; c.mirror = false; emit(c); }
        // every capacity: flat, and the two hierarchy modes
        for (int mc : MC)
            for (int mode : {1, 2, 3}) { ct_case c = base; c.mc = mc; c.mode = mode; c.hier = mode >= 2; c.many = many; c.sort = mode >= 2 ? (size_t)mc * 8 + 1 : 0; emit(c); }
        // every head-count hint: one image (where it sizes the grid) and two (where it does not), a large frame and one of 192 heads at most
        for (uint32_t hint : HINT)
            for (int n : {1, 2})
                for (int small = 0; small <= 1; small++) { ct_case c = base; if (small) { c.w = 64; c.h = 2; } c.n = n; c.hint = hint; c.many = many; c.mirror = n == 1; emit(c); }
        // modes and methods, the refused ones included; the hierarchy modes need the buffer and one image
        for (int mode = -1; mode <= 4; mode++)
            for (int hier = 0; hier <= 1; hier++)
                for (int n : {1, 2}) { ct_case c = base; c.mode = mode; c.hier = hier; c.n = n; c.many = many; c.sort = hier ? 777 : 0; emit(c); }
        for (int method = 0; method <= 3; method++) { ct_case c = base; c.method = method; c.many = many; emit(c); }
        // deferring, with and without the mirror
        for (int defer = 0; defer <= 1; defer++)
            for (int mirror = 0; mirror <= 1; mirror++)
                for (int n : {1, 2}) { ct_case c = base; c.defer = defer; c.mirror = mirror; c.n = n; c.many = many; emit(c); }
        // the largest frames admitted (2^29 - 1 pixels and the largest square) and the smallest refused (2^29)
        static const int big[][2] = {{536870911, 1}, {1, 536870911}, {23170, 23170}, {536870912, 1}, {1, 536870912}, {32768, 16384}};
        for (const auto& b : big) { ct_case c = base; c.w = b[0]; c.h = b[1]; c.many = many; emit(c); }
    }
    // the benchmark's own: one 1080p image, RETR_EXTERNAL, 64 contours, with the mirror and deferring (a few thousand heads last time);
    // and the chain's batch of 128
    { ct_case c = base; c.mode = 0; c.defer = true; c.hint = 3000; emit(c); }
    { ct_case c = base; c.mode = 0; c.n = 128; c.mirror = false; emit(c); }
}
