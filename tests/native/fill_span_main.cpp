// The span writer of the fill kernels (csrc/vp_fill_span.h) run on the host, lane by lane: its lanes do not talk to each other, so 64
// sequential calls write what one wave writes.  Every channel count, start alignment of the image and clipping case is compared with a
// byte loop; the bytes around the image must stay as they were.  Built with -fsanitize=address,undefined by tests/test_fill_span_host.py:
// a 16-byte store at an address that is no multiple of 16, or one past the buffer, stops the program.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
typedef unsigned int u32;
struct alignas(16) uint4 { u32 x, y, z, w; };
#define VP_FILL_DEV static inline
#define __restrict__
#include "vp_fill_span.h"

int main()
{
    long checks = 0, bad = 0;
    const int widths[] = {1, 5, 16, 17, 64, 65, 200};
    for (int cn = 1; cn <= 4; cn++)
        for (int w : widths)
            for (int off = 0; off < 16; off++) {
                const int h = 3;
                std::vector<uint8_t> store((size_t)w * h * cn + 96, 0xAA), ref;
                uint8_t* base = store.data();
                while ((uintptr_t)base & 15) base++;
                uint8_t* img = base + 16 + off;
                const u32 cw = cn == 4 ? 0x04030201u : (0x04030201u & ((1u << (8 * cn)) - 1));
                for (int xa = -2; xa <= w; xa++)
                    for (int xb = xa - 1; xb <= w + 1; xb += (w > 64 ? 7 : 1)) {
                        std::fill(store.begin(), store.end(), (uint8_t)0xAA);
                        ref = store;
                        for (int lane = 0; lane < 64; lane++) fill_columns(img, w, cn, 1, xa, xb, cw, lane);
                        const int a = xa < 0 ? 0 : xa, b = xb > w - 1 ? w - 1 : xb;
                        uint8_t* rimg = ref.data() + (img - store.data());
                        for (int x = a; x <= b; x++)
                            for (int c = 0; c < cn; c++) rimg[((size_t)w + x) * cn + c] = (uint8_t)(c + 1);
                        checks++;
                        if (memcmp(ref.data(), store.data(), store.size())) {
                            if (bad++ < 5) printf("mismatch cn=%d w=%d off=%d xa=%d xb=%d\n", cn, w, off, xa, xb);
                        }
                    }
            }
    printf("checks %ld bad %ld\n", checks, bad);
    return bad != 0;
}
