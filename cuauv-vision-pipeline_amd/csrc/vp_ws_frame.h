// A call's view of the context's device workspace: every buffer the call needs is declared once with want(), vp_ws_commit
// (vp_api.hip) reserves their sum and only then assigns the pointers.  Regions start on 256-byte boundaries and never overlap, so a
// call cannot under-reserve.  Plain C++ - no HIP types - so that the host test (tests/native/ws_frame_main.cpp) compiles it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

struct vp_ws_frame {
    // the largest call is the host chain at four sub-batches: 7 device copies of its own and per sub-batch 4 buffers of the chain and
    // 20 of the labelling (7 + 4 * 24 = 103); the host chain with contours, which is not split, has 14 + 24 + the contour scratch
    enum { CAP = 128, ALIGN = 256 };
    void* slot[CAP];        // where each pointer goes (the address of the caller's variable)
    size_t off[CAP];
    int n = 0;              // buffers wanted; above CAP: overflow, nothing past CAP was recorded
    size_t end = 0;         // end of the last region
    bool wrapped = false;   // a region's end did not fit size_t: it and everything after it was dropped

    // *p = base + offset at assign(); 0 bytes: a valid pointer that may equal the next buffer's
    template <typename T> void want(T** p, size_t bytes) { want_at((void*)p, bytes); }
    void want_at(void* p, size_t bytes)
    {
        if (end > SIZE_MAX - (ALIGN - 1)) { wrapped = true; return; }
        const size_t o = (end + (ALIGN - 1)) / ALIGN * ALIGN;
        if (wrapped || bytes > SIZE_MAX - o) { wrapped = true; return; }
        if (n < CAP) { slot[n] = p; off[n] = o; }
        n++;
        end = o + bytes;
    }
    size_t bytes() const { return end; }
    bool overflowed() const { return n > CAP; }
    void assign(uint8_t* base) const
    {
        for (int i = 0; i < n && i < CAP; i++) {
            uint8_t* q = base + off[i];
            memcpy(slot[i], &q, sizeof q);
        }
    }
};
