// The workspace frame (csrc/vp_ws_frame.h) driven on the host under the address and undefined-behaviour sanitizers against a fake base
// pointer: over a sweep of buffer counts and sizes every assigned region is 256-byte aligned, inside [base, base + bytes()) and apart
// from every other non-empty region, bytes() is the end of the last region, too many buffers are reported and assign nothing, and a
// sum that would wrap size_t is refused without wrapping.  Prints one line of totals; exits non-zero at the first broken invariant.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "vp_ws_frame.h"

#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::printf("FAILED %s (count=%d case=%ld line %d)\n", #cond, g_count, g_case, __LINE__); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

static int g_count;
static long g_case;
static uint8_t* const BASE = reinterpret_cast<uint8_t*>((uintptr_t)0x7000000000ull);   // 256-byte aligned like a device allocation, never dereferenced
static uint8_t* const POISON = reinterpret_cast<uint8_t*>((uintptr_t)0x1);

// what vp_ws_commit does with a frame, less the allocation: refuse, or assign against BASE
static bool commit(const vp_ws_frame& W)
{
    if (W.overflowed() || W.wrapped) return false;
    W.assign(BASE);
    return true;
}

static int check_sizes(const std::vector<size_t>& sizes, long* regions)
{
    const int n = (int)sizes.size();
    g_count = n;
    g_case++;
    vp_ws_frame W;
    std::vector<uint8_t*> p((size_t)n, POISON);
    for (int i = 0; i < n; i++) W.want(&p[(size_t)i], sizes[(size_t)i]);
    if (n > vp_ws_frame::CAP) {                               // reported, and nothing assigned
        CHECK(W.overflowed() && !commit(W));
        for (int i = 0; i < n; i++) CHECK(p[(size_t)i] == POISON);
        return 0;
    }
    CHECK(!W.overflowed() && !W.wrapped && W.n == n && commit(W));
    size_t end = 0;
    for (int i = 0; i < n; i++) {
        const size_t off = (size_t)(p[(size_t)i] - BASE);
        CHECK(p[(size_t)i] != POISON && off % 256 == 0 && off >= end && off < end + 256);   // aligned, behind the last one, no more than the padding apart
        CHECK(off + sizes[(size_t)i] <= W.bytes());
        end = off + sizes[(size_t)i];
        for (int j = 0; j < i; j++) {                         // apart from every earlier non-empty region
            const size_t oj = (size_t)(p[(size_t)j] - BASE);
            if (sizes[(size_t)i] && sizes[(size_t)j]) CHECK(oj + sizes[(size_t)j] <= off);
        }
        ++*regions;
    }
    CHECK(W.bytes() == end);
    return 0;
}

int main()
{
    long regions = 0, frames = 0, refused = 0;
    const size_t edge[] = {0, 1, 255, 256, 257, 511, 512, 4096, 65537, (size_t)1 << 20, ((size_t)3 << 30) + 5};
    const int ne = (int)(sizeof edge / sizeof edge[0]);
    // every pair and triple of the edge sizes
    for (int a = 0; a < ne; a++)
        for (int b = 0; b < ne; b++) {
            if (check_sizes({edge[a], edge[b]}, &regions)) return 1;
            frames++;
            for (int c = 0; c < ne; c++) {
                if (check_sizes({edge[a], edge[b], edge[c]}, &regions)) return 1;
                frames++;
            }
        }
    // every count from none to past the capacity, sizes from a fixed generator (with empty buffers among them)
    unsigned long long x = 88172645463325252ull;
    for (int n = 0; n <= vp_ws_frame::CAP + 3; n++)
        for (int rep = 0; rep < 8; rep++) {
            std::vector<size_t> s((size_t)n);
            for (auto& v : s) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                const unsigned k = (unsigned)(x >> 60);
                v = k == 0 ? 0 : k < 4 ? edge[(x >> 8) % (unsigned)ne] : (size_t)((x >> 16) % 100000);
            }
            if (check_sizes(s, &regions)) return 1;
            frames++;
            if (n > vp_ws_frame::CAP) refused++;
        }
    // an empty frame: nothing to reserve, nothing assigned
    {
        vp_ws_frame W;
        g_count = 0;
        CHECK(W.bytes() == 0 && commit(W));
    }
    // sizes near SIZE_MAX / 2: two of them fit size_t or not; a refused frame assigns nothing and bytes() has not wrapped
    const size_t half = SIZE_MAX / 2;
    const size_t big[] = {half - 512, half - 256, half - 255, half - 1, half, half + 1, half + 256, SIZE_MAX - 256, SIZE_MAX - 255, SIZE_MAX};
    for (size_t first : big)
        for (size_t second : big)
            for (size_t lead : {(size_t)0, (size_t)1, (size_t)256}) {
                g_count = 3;
                g_case++;
                vp_ws_frame W;
                uint8_t *p0 = POISON, *p1 = POISON, *p2 = POISON, *p3 = POISON;
                W.want(&p0, lead);
                W.want(&p1, first);
                W.want(&p2, second);
                W.want(&p3, 16);                                // a buffer after the one that wrapped must not make the frame look sound again
                // the same layout in 128-bit arithmetic, which cannot wrap
                const size_t want[4] = {lead, first, second, 16};
                size_t off[4] = {0, 0, 0, 0}, good_end = 0;
                unsigned __int128 end = 0;
                bool fits = true;
                for (int i = 0; i < 4 && fits; i++) {
                    const unsigned __int128 o = (end + 255) / 256 * 256;
                    if (o + want[i] > (unsigned __int128)SIZE_MAX) { fits = false; break; }
                    off[i] = (size_t)o;
                    end = o + want[i];
                    good_end = (size_t)end;
                }
                frames++;
                CHECK(!W.overflowed() && W.bytes() == good_end);       // the sum stops at the last region that fitted: it never wraps
                if (fits) {                                             // (no assign here: BASE + such an offset is no address)
                    CHECK(!W.wrapped && W.n == 4);
                    for (int i = 0; i < 4; i++) CHECK(W.off[i] == off[i]);
                } else {
                    CHECK(W.wrapped && !commit(W));
                    CHECK(p0 == POISON && p1 == POISON && p2 == POISON && p3 == POISON);
                    refused++;
                }
            }
    std::printf("frames %ld regions %ld refused %ld capacity %d\n", frames, regions, refused, (int)vp_ws_frame::CAP);
    return 0;
}
