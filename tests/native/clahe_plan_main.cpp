// Prints what csrc/vp_clahe_plan.h decides, for tests/test_clahe_abi.py (built with the address and undefined-behaviour sanitizers):
//   "plan w h clip tiles_x tiles_y opt | status padded ext_w ext_h tile_w tile_h area clip split part_rows in_lds lds_bytes hist_gx hist_gy apply_gx"
// over image sizes, grids, clip limits and forced shares, the rejections among them; "tile ..." are the header's constants.
#include <cmath>
#include <cstdio>
#include "vp_clahe_plan.h"

static void show(int w, int h, double clip, int tx, int ty, int opt)
{
    const vp_clahe_plan P = vp_clahe_make_plan(w, h, clip, tx, ty, opt);
    std::printf("plan %d %d %.17g %d %d %d | %d %d %d %d %d %d %d %d %d %d %d %u %u %u %u\n", w, h, clip, tx, ty, opt, P.status, P.padded, P.ext_w, P.ext_h, P.tile_w,
                P.tile_h, P.area, P.clip, P.split, P.part_rows, P.tables_in_lds, P.lds_bytes, P.hist_gx, P.hist_gy, P.apply_gx);
}

int main()
{
    std::printf("tile %d %d %d %d %d %d %d %d\n", CL_MAX_TILES, CL_MAX_PIXELS, CL_HIST_BLOCK, CL_MAX_SPLIT, CL_PART_PIXELS, CL_APPLY_BLOCK, CL_APPLY_ROWS, CL_LDS_BUDGET);
    const int sizes[][2] = {{1, 1}, {2, 3}, {9, 9}, {16, 16}, {37, 29}, {40, 29}, {64, 64}, {256, 192}, {641, 479}, {1920, 1080}, {4096, 4096}, {16384, 16384},
                            {1 << 28, 1}, {1, 1 << 28}, {0, 5}, {5, 0}, {-1, 5}, {16385, 16384}, {1 << 30, 4}};
    const int grids[][2] = {{1, 1}, {1, 8}, {8, 1}, {2, 2}, {4, 3}, {8, 8}, {16, 16}, {17, 15}, {64, 64}, {65, 8}, {8, 65}, {0, 8}, {8, 0}, {-2, -2}};
    const double clips[] = {-1.0, 0.0, 1e-3, 2.0, 40.0, 1e4, 1e12, 1e300, INFINITY, NAN};
    const int opts[] = {0, 1, 2, 3, 7, 64, 1000};
    for (const auto& s : sizes)
        for (const auto& g : grids)
            for (double c : clips)
                for (int o : opts) show(s[0], s[1], c, g[0], g[1], o);
    return 0;
}
