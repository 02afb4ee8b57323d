// Host arithmetic of the median filter's dispatch (vpk_median_blur, vp_median.hip): which kernel serves a call, whether bit planes are
// read and written, and the launch geometry.  Plain C++ - no HIP types, no kernels - and a pure function of its arguments, like the
// labelling's plan in vp_ccl_plan.h.
#pragma once

// tiles of the three kernels (the kernels assert their LDS budgets from the same numbers)
#define MD_TB 256              // network kernel: result bytes per tile row
#define MD_TH 32               // ... and result rows per tile
#define MD_NET_MAXK 5          // largest window the exchange networks serve
#define MH_LANES 64            // histogram kernel: result byte columns per block, one lane each
#define MH_MIN_STRIP 32        // ... rows per strip at least (a strip starts with ksize rows of window set-up)
#define MM_TW 256              // mask kernel: result pixels per tile row
#define MM_TH 32               // ... and result rows per tile
#define MM_MAXK 63             // largest window whose row fits one 64-bit word

enum { VP_MEDIAN_COPY = 0, VP_MEDIAN_NETWORK = 1, VP_MEDIAN_HIST = 2, VP_MEDIAN_MASK = 3 };

struct vp_median_plan {
    int kernel;                // VP_MEDIAN_*
    int from_bits;             // mask kernel: the source's bit plane is read instead of its bytes
    int write_bits;            // mask kernel: the result's bit plane is written (whole words per row only)
    int strip_h;               // histogram kernel: rows per strip
    unsigned gx, gy, block;    // launch geometry (0 for the copy)
};

// opt_mask: VP_OPT_MEDIAN_MASK (1 the mask kernel for every mask it can serve, 0 never, -1 the measured choice).
// The choices between two kernels that can serve one case follow the measurement on an MI355X (tools/exp_median.py, DESIGN.md
// section 5.10, 1080p): the networks beat the histograms at 3 and 5 by 2.6 to 14 times, so the histograms start at 7; on a mask the
// mask kernel reading the source's bit plane beats the general kernels at every window (1.5 times at 3, 13 times at 15); packing its
// tile from the bytes it loses to the network at 3 (0.024 against 0.013 ms) and wins from 5 on.
static inline vp_median_plan vp_median_make_plan(int w, int h, int cn, int ksize, int binary_hint, bool src_plane, bool dst_plane, int opt_mask)
{
    vp_median_plan P = {VP_MEDIAN_COPY, 0, 0, 0, 0, 0, 0};
    if (ksize == 1) return P;
    const int rowbytes = w * cn;
    const bool mask_can = binary_hint && cn == 1 && ksize <= MM_MAXK;
    if (mask_can && (opt_mask == 1 || (opt_mask < 0 && (src_plane || ksize >= 5)))) {
        P.kernel = VP_MEDIAN_MASK;
        P.from_bits = src_plane ? 1 : 0;
        P.write_bits = (dst_plane && w % 64 == 0) ? 1 : 0;
        P.gx = (unsigned)((w + MM_TW - 1) / MM_TW);
        P.gy = (unsigned)((h + MM_TH - 1) / MM_TH);
        P.block = 256;
        return P;
    }
    if (ksize <= MD_NET_MAXK) {
        P.kernel = VP_MEDIAN_NETWORK;
        P.gx = (unsigned)((rowbytes + MD_TB - 1) / MD_TB);
        P.gy = (unsigned)((h + MD_TH - 1) / MD_TH);
        P.block = 256;
        return P;
    }
    P.kernel = VP_MEDIAN_HIST;
    P.strip_h = ksize > MH_MIN_STRIP ? ksize : MH_MIN_STRIP;
    if (P.strip_h > h) P.strip_h = h;
    P.gx = (unsigned)((rowbytes + MH_LANES - 1) / MH_LANES);
    P.gy = (unsigned)((h + P.strip_h - 1) / P.strip_h);
    P.block = MH_LANES;
    return P;
}
