// Prints what csrc/vp_deriv_plan.h decides, for tests/test_deriv_abi.py (built with the address and undefined-behaviour sanitizers):
//   "plan op dx dy ksize ddepth border cn | ok kernel K depth esize border gx gy block | rowA | colA | rowB | colB | corner edge centre"
// for every argument set of a range wider than what is accepted, and "border code len p index" for the index map.
#include <cstdio>
#include "vp_deriv_plan.h"

static void taps(const int* t)
{
    std::printf(" |");
    for (int i = 0; i < DV_MAXK; i++) std::printf(" %d", t[i]);
}

int main()
{
    std::printf("tile %d %d %d %d %d\n", DV_TB, DV_TH, DV_EPL, DV_MAXK, DV_PAD);
    const int depths[] = {-1, 0, 3, 4, 5, 6};
    const int borders[] = {0, 1, 2, 3, 4, 5, 20};
    for (int op = -1; op <= 4; op++)
        for (int dx = -1; dx <= 3; dx++)
            for (int dy = -1; dy <= 3; dy++)
                for (int ksize = -2; ksize <= 9; ksize++)
                    for (int ddepth : depths)
                        for (int border : borders)
                            for (int cn = 1; cn <= 3; cn += 2) {
                                const vp_deriv_plan P = vp_deriv_make_plan(67, 35, cn, op, dx, dy, ksize, ddepth, border);
                                std::printf("plan %d %d %d %d %d %d %d | %d %d %d %d %d %d %u %u %u", op, dx, dy, ksize, ddepth, border, cn, P.ok, P.kernel, P.K, P.depth,
                                            P.esize, P.border, P.gx, P.gy, P.block);
                                taps(P.taps.rowA); taps(P.taps.colA); taps(P.taps.rowB); taps(P.taps.colB);
                                std::printf(" | %d %d %d\n", P.lap_corner, P.lap_edge, P.lap_centre);
                            }
    const int sizes[][3] = {{0, 35, 1}, {67, 0, 1}, {67, 65536, 1}, {67, 35, 0}, {67, 35, 5}, {1 << 29, 4, 4}, {1 << 28, 4, 4}, {1, 1, 1}, {513, 17, 1}};
    for (const auto& s : sizes) {
        const vp_deriv_plan P = vp_deriv_make_plan(s[0], s[1], s[2], VP_DV_OP_SOBEL, 1, 0, 3, VP_DV_16S, VP_DV_REFLECT_101);
        std::printf("size %d %d %d | %d %u %u\n", s[0], s[1], s[2], P.ok, P.gx, P.gy);
    }
    const int codes[] = {VP_DV_CONSTANT, VP_DV_REPLICATE, VP_DV_REFLECT, VP_DV_REFLECT_101};
    for (int code : codes)
        for (int len = 1; len <= 9; len++)
            for (int p = -20; p < len + 20; p++) std::printf("border %d %d %d %d\n", code, len, p, vp_deriv_border_index(p, len, code));
    return 0;
}
