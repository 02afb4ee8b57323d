// C ABI of libvp.so, morphology and the batched device-resident chain: both plan their erode / dilate stages with the same
// stage planner (kernels: vp_morph, and through the chain vp_color / vp_ccl + contours).
#include "vp_api_util.h"

// ---- morphology planning ---------------------------------------------------------------------------

// the stage planner (splits at extent 31, merges neighbours of one kind) and the grouping into launches: vp_morph_plan.h
typedef mb_rect rect_se;
static_assert(MB_OP_ERODE == VP_MORPH_ERODE && MB_OP_DILATE == VP_MORPH_DILATE && MB_OP_OPEN == VP_MORPH_OPEN && MB_OP_CLOSE == VP_MORPH_CLOSE,
              "vp_morph_plan.h: operation codes");
static void push_rect_stage(std::vector<vp_bitstage>& v, int dilate, const rect_se& k) { mb_push_rect_stage(v, dilate, k); }
static int stages_for_op(std::vector<vp_bitstage>& v, int op, const rect_se& k) { return mb_stages_for_op(v, op, k) ? VP_OK : VP_ERR_INVALID; }

// Runs a stage list over bit images, in the launches mb_group_stages makes of it (each one's halo fits LDS).  bits_in holds the
// input and is only read: no launch writes it, however many there are.  bits_scratch and bits_out are planes of equal size that the
// launches before the last alternate between (the last one reads bits_scratch); it writes bits_out when write_bits is set, and
// out_mask when that is not NULL.  With an empty list the input is forwarded.
static int run_bit_stages(vp_ctx* ctx, const std::vector<vp_bitstage>& st, const u64* bits_in, u64* bits_scratch, u64* bits_out, bool write_bits,
                          int w, int h, int n, uint8_t* out_mask)
{
    const size_t words = (size_t)n * h * vp_ww(w);
    if (st.empty()) {
        if (write_bits) VP_HIP(ctx, hipMemcpyAsync(bits_out, bits_in, words * 8, hipMemcpyDeviceToDevice, ctx->stream));
        if (out_mask) VP_TRY(vpk_unpack_bits(ctx, bits_in, w, h, n, out_mask));
        return VP_OK;
    }
    std::vector<mb_launch> launches;
    if (!mb_group_stages(st, vp_ww(w), launches)) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "image too wide for the LDS bit-morphology strip");
    u64* const plane[4] = {nullptr /* MB_BUF_IN: never a destination */, bits_scratch, bits_out /* MB_BUF_SCRATCH2 */, write_bits ? bits_out : nullptr};
    for (size_t k = 0; k < launches.size(); k++) {
        const mb_launch& L = launches[k];
        const bool last = k + 1 == launches.size();
        vp_bitplan plan;
        plan.n = L.count;
        for (int i = 0; i < L.count; i++) plan.s[i] = st[(size_t)L.first + i];
        const u64* src = L.src == MB_BUF_IN ? bits_in : plane[L.src];
        u64* dst = plane[L.dst];
        if (L.dst == MB_BUF_IN || L.src == L.dst || src == dst || (!last && !dst)) return vp_fail(ctx, VP_ERR_INVALID, "bit morphology: launch planes");
        VP_TRY(vpk_morph_bits(ctx, plan, src, w, h, n, dst, last ? out_mask : nullptr));
    }
    return VP_OK;
}

// cv2 morphOp() normalisation of (kernel, anchor, iterations).  Returns 1 when the op degenerates to a copy.
struct norm_se { std::vector<uint8_t> k; int kw, kh, ax, ay, iterations; bool allones; };
static int normalise_se(const uint8_t* kernel, int kw, int kh, int ax, int ay, int iterations, norm_se* o)
{
    if (iterations < 0) return VP_ERR_INVALID;
    if (!kernel || kw * kh == 0) {
        kw = kh = 1 + iterations * 2;
        ax = ay = iterations;
        iterations = 1;
        o->k.assign((size_t)kw * kh, 1);
    } else {
        if (kw <= 0 || kh <= 0) return VP_ERR_INVALID;
        o->k.assign(kernel, kernel + (size_t)kw * kh);
    }
    if (ax < 0) ax = kw / 2;
    if (ay < 0) ay = kh / 2;
    if (ax >= kw || ay >= kh) return VP_ERR_INVALID;
    bool allones = true;
    for (uint8_t b : o->k) allones = allones && b != 0;
    if (iterations > 1 && allones) {
        ax *= iterations;
        ay *= iterations;
        kw = kw + (iterations - 1) * (kw - 1);
        kh = kh + (iterations - 1) * (kh - 1);
        iterations = 1;
        o->k.assign((size_t)kw * kh, 1);
    }
    o->kw = kw; o->kh = kh; o->ax = ax; o->ay = ay; o->iterations = iterations; o->allones = allones;
    return VP_OK;
}

extern "C" {

int vp_structuring_element(int shape, int kw, int kh, uint8_t* out)
{
    // imgproc getStructuringElement(): integer geometry, anchor at the centre
    if (!out || kw <= 0 || kh <= 0 || shape < 0 || shape > 2) return VP_ERR_INVALID;
    if (kw == 1 && kh == 1) shape = VP_SHAPE_RECT;
    const int r = kh / 2, c = kw / 2;
    const double inv_r2 = (shape == VP_SHAPE_ELLIPSE && r) ? 1.0 / ((double)r * r) : 0.0;
    for (int i = 0; i < kh; i++) {
        int j1 = 0, j2 = 0;
        if (shape == VP_SHAPE_RECT || (shape == VP_SHAPE_CROSS && i == r)) j2 = kw;
        else if (shape == VP_SHAPE_CROSS) { j1 = c; j2 = c + 1; }
        else {
            const int dy = i - r;
            if (abs(dy) <= r) {
                const int dx = (int)__builtin_nearbyint(c * __builtin_sqrt((r * r - dy * dy) * inv_r2));
                j1 = c - dx > 0 ? c - dx : 0;
                j2 = c + dx + 1 < kw ? c + dx + 1 : kw;
            }
        }
        for (int j = 0; j < kw; j++) out[i * kw + j] = (j >= j1 && j < j2) ? 1 : 0;
    }
    return VP_OK;
}

// one erode or dilate (after cv2 normalisation) on a device image; result in d_out
static int morph_basic_dev(vp_ctx* ctx, int dilate, const norm_se& se, const uint8_t* d_in, int w, int h, int cn, bool binary,
                           uint8_t* d_out, uint8_t* d_tmp, u64* bits_a, u64* bits_b, u64* bits_c, int16_t* d_offs, uint8_t* d_tab = nullptr)
{
    const size_t nbytes = (size_t)w * h * cn;
    if (se.iterations == 0 || se.kw * se.kh == 1) {
        VP_HIP(ctx, hipMemcpyAsync(d_out, d_in, nbytes, hipMemcpyDeviceToDevice, ctx->stream));
        return VP_OK;
    }
    if (se.allones && cn == 1 && binary) {
        std::vector<vp_bitstage> st;
        rect_se k = {se.kw, se.kh, se.ax, se.ay};
        push_rect_stage(st, dilate, k);
        VP_TRY(vpk_pack_bits(ctx, d_in, (size_t)w, w, h, 1, bits_a, nullptr));
        return run_bit_stages(ctx, st, bits_a, bits_b, bits_c, false, w, h, 1, d_out);
    }
    // generic: offsets of the structuring element (all-ones kernels are applied separably)
    std::vector<int16_t> offs;
    int passes_first = 0;
    if (se.allones) {
        for (int j = 0; j < se.kw; j++) { offs.push_back((int16_t)(j - se.ax)); offs.push_back(0); }
        passes_first = se.kw;
        for (int i = 0; i < se.kh; i++) { offs.push_back(0); offs.push_back((int16_t)(i - se.ay)); }
    } else {
        for (int i = 0; i < se.kh; i++)
            for (int j = 0; j < se.kw; j++)
                if (se.k[(size_t)i * se.kw + j]) { offs.push_back((int16_t)(j - se.ax)); offs.push_back((int16_t)(i - se.ay)); }
    }
    VP_HIP(ctx, hipMemcpyAsync(d_offs, offs.data(), offs.size() * 2, hipMemcpyHostToDevice, ctx->stream));
    VP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // offs is a local vector
    if (se.allones) {
        VP_TRY(vpk_morph_generic(ctx, dilate, d_in, w, h, cn, d_offs, passes_first, d_tmp));
        VP_TRY(vpk_morph_generic(ctx, dilate, d_tmp, w, h, cn, d_offs + 2 * passes_first, se.kh, d_out));
        return VP_OK;
    }
    const int noffs = (int)(offs.size() / 2);
    // span form when it saves reads: one (dy, x0, x1) triple per run of members in a row of the element
    std::vector<int16_t> spans;
    int max_len = 1;
    for (int i = 0; i < se.kh; i++)
        for (int j = 0; j < se.kw;) {
            if (!se.k[(size_t)i * se.kw + j]) { j++; continue; }
            int e = j;
            while (e + 1 < se.kw && se.k[(size_t)i * se.kw + e + 1]) e++;
            spans.push_back((int16_t)(i - se.ay)); spans.push_back((int16_t)(j - se.ax)); spans.push_back((int16_t)(e - se.ax));
            max_len = std::max(max_len, e - j + 1);
            j = e + 1;
        }
    const int nspans = (int)(spans.size() / 3);
    const bool use_spans = d_tab && 2 * nspans < noffs && max_len <= 255 && nspans <= 2048 && (size_t)w * cn <= 16384;
    if (use_spans) {
        VP_HIP(ctx, hipMemcpyAsync(d_offs, spans.data(), spans.size() * 2, hipMemcpyHostToDevice, ctx->stream));
        VP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // spans is a local vector
    }
    const uint8_t* cur = d_in;
    uint8_t* bufs[2] = {d_out, d_tmp};
    // arrange so that the last pass lands in d_out
    int which = (se.iterations % 2 == 1) ? 0 : 1;
    for (int it = 0; it < se.iterations; it++) {
        if (use_spans) VP_TRY(vpk_morph_spans(ctx, dilate, cur, w, h, cn, d_offs, nspans, max_len, d_tab, bufs[which]));
        else VP_TRY(vpk_morph_generic(ctx, dilate, cur, w, h, cn, d_offs, noffs, bufs[which]));
        cur = bufs[which];
        which ^= 1;
    }
    return VP_OK;
}

// temporaries a morphology call needs besides its source / result images
struct morph_bufs { uint8_t *tab, *b, *c, *tmp; u64 *bits_a, *bits_b, *bits_c; int16_t* offs; int* flag; };
static void morph_want(vp_ws_frame& W, const norm_se& se, int w, int h, int cn, morph_bufs* m)
{
    const size_t nbytes = (size_t)w * h * cn;
    const size_t bitbytes = (size_t)h * vp_ww(w) * 8;
    m->tab = nullptr;
    if (!se.allones) W.want(&m->tab, 7 * nbytes);   // running min/max tables of the span form
    W.want(&m->b, nbytes);
    W.want(&m->c, nbytes);
    W.want(&m->tmp, nbytes);
    W.want(&m->bits_a, bitbytes);
    W.want(&m->bits_b, bitbytes);
    W.want(&m->bits_c, bitbytes);   // a plan of three or more launches alternates between bits_b and bits_c: bits_a is only read
    W.want(&m->offs, ((size_t)se.kw * se.kh + se.kw + se.kh) * 4 + 64);
    W.want(&m->flag, 4);
}

// One morphology operation between device images (d_dst may equal neither d_src nor overlap it); temporaries: m, in the caller's frame
// (morph_want).  binary_hint: 1 = the image is known to hold only 0 / 255 (a mask this
// library produced), 0 = unknown: one flag comes back from the device to decide between the bit-plane and the grey-level path.
static int morph_core(vp_ctx* ctx, int op, const norm_se& se, const uint8_t* d_src, int w, int h, int cn, int binary_hint, uint8_t* d_dst, const morph_bufs& m)
{
    const size_t nbytes = (size_t)w * h * cn;
    uint8_t *d_tab = m.tab, *d_b = m.b, *d_c = m.c, *d_tmp = m.tmp;
    u64 *bits_a = m.bits_a, *bits_b = m.bits_b, *bits_c = m.bits_c;
    int16_t* d_offs = m.offs;
    int* d_flag = m.flag;
    bool binary = false;
    if (cn == 1 && se.allones) {
        // a 0/255 mask can take the bit-plane path; anything else is grey-level
        if (binary_hint == 1) {
            VP_TRY(vpk_pack_bits(ctx, d_src, (size_t)w, w, h, 1, bits_a, nullptr));
            binary = true;
        } else {
            VP_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
            VP_TRY(vpk_pack_bits(ctx, d_src, (size_t)w, w, h, 1, bits_a, d_flag));
            int flag = 1;
            VP_TRY(d2h(ctx, &flag, d_flag, 4));
            VP_HIP(ctx, hipStreamSynchronize(ctx->stream));
            binary = flag == 0;
        }
    }
    if (binary && op != VP_MORPH_GRADIENT) {
        // whole op (incl. OPEN/CLOSE) as one fused bit-plane launch
        std::vector<vp_bitstage> st;
        rect_se k = {se.kw, se.kh, se.ax, se.ay};
        if (!(se.iterations == 0 || se.kw * se.kh == 1)) stages_for_op(st, op, k);
        VP_TRY(run_bit_stages(ctx, st, bits_a, bits_b, bits_c, false, w, h, 1, d_dst));
    } else if (op == VP_MORPH_ERODE || op == VP_MORPH_DILATE) {
        VP_TRY(morph_basic_dev(ctx, op == VP_MORPH_DILATE, se, d_src, w, h, cn, binary, d_dst, d_tmp, bits_a, bits_b, bits_c, d_offs, d_tab));
    } else if (op == VP_MORPH_OPEN || op == VP_MORPH_CLOSE) {
        const int first = op == VP_MORPH_CLOSE;
        VP_TRY(morph_basic_dev(ctx, first, se, d_src, w, h, cn, binary, d_b, d_tmp, bits_a, bits_b, bits_c, d_offs, d_tab));
        VP_TRY(morph_basic_dev(ctx, !first, se, d_b, w, h, cn, binary, d_dst, d_tmp, bits_a, bits_b, bits_c, d_offs, d_tab));
    } else {  // GRADIENT = dilate - erode
        VP_TRY(morph_basic_dev(ctx, 1, se, d_src, w, h, cn, binary, d_b, d_tmp, bits_a, bits_b, bits_c, d_offs, d_tab));
        VP_TRY(morph_basic_dev(ctx, 0, se, d_src, w, h, cn, binary, d_c, d_tmp, bits_a, bits_b, bits_c, d_offs, d_tab));
        VP_TRY(vpk_absdiff_sub_u8(ctx, d_b, d_c, nbytes, d_dst));
    }
    return VP_OK;
}

int vp_morph_u8(vp_ctx* ctx, int op, const uint8_t* src, int w, int h, int cn, const uint8_t* kernel, int kw, int kh, int ax, int ay,
                int iterations, uint8_t* dst)
{
    VP_TRY(check_ctx(ctx));
    if (!src || !dst || w <= 0 || h <= 0 || h > 65535 || cn < 1 || cn > 4 || op < VP_MORPH_ERODE || op > VP_MORPH_GRADIENT)
        return vp_fail(ctx, VP_ERR_INVALID, "vp_morph_u8 arguments");
    norm_se se;
    if (normalise_se(kernel, kw, kh, ax, ay, iterations, &se) != VP_OK) return vp_fail(ctx, VP_ERR_INVALID, "structuring element");
    const size_t nbytes = (size_t)w * h * cn;
    vp_ws_frame W;
    uint8_t* d_src; W.want(&d_src, nbytes);
    uint8_t* d_a; W.want(&d_a, nbytes);
    morph_bufs m;
    morph_want(W, se, w, h, cn, &m);
    VP_TRY(vp_ws_commit(ctx, W, "vp_morph_u8"));
    VP_TRY(h2d(ctx, d_src, src, nbytes));
    VP_TRY(morph_core(ctx, op, se, d_src, w, h, cn, 0, d_a, m));
    VP_TRY(d2h(ctx, dst, d_a, nbytes));
    return vp_synchronize(ctx);
}

int vp_morph_u8_dev(vp_ctx* ctx, int op, const uint8_t* d_src, int w, int h, int cn, const uint8_t* kernel, int kw, int kh, int ax, int ay,
                    int iterations, int binary_hint, uint8_t* d_dst)
{
    VP_TRY(check_ctx(ctx));
    if (!d_src || !d_dst || d_src == d_dst || w <= 0 || h <= 0 || h > 65535 || cn < 1 || cn > 4 || op < VP_MORPH_ERODE || op > VP_MORPH_GRADIENT)
        return vp_fail(ctx, VP_ERR_INVALID, "vp_morph_u8_dev arguments");
    norm_se se;
    if (normalise_se(kernel, kw, kh, ax, ay, iterations, &se) != VP_OK) return vp_fail(ctx, VP_ERR_INVALID, "structuring element");
    vp_ws_frame W;
    morph_bufs m;
    morph_want(W, se, w, h, cn, &m);
    VP_TRY(vp_ws_commit(ctx, W, "vp_morph_u8_dev"));
    return morph_core(ctx, op, se, d_src, w, h, cn, binary_hint, d_dst, m);
}

// ---- chain -------------------------------------------------------------------------------------------

static int check_desc(vp_ctx* ctx, const vp_chain_desc* d, int n)
{
    if (!d || n <= 0 || d->width <= 0 || d->height <= 0) return vp_fail(ctx, VP_ERR_INVALID, "chain: size");
    // frames ride on gridDim.y; segment ids and pixel indices are 32-bit
    if (n > 65535 || (unsigned long long)d->width * (unsigned long long)d->height > (1ull << 30)) return vp_fail(ctx, VP_ERR_UNSUPPORTED, "chain: batch or frame too large");
    if (d->color_mode != VP_BGR2LAB && d->color_mode != VP_BGR2HSV && d->color_mode != VP_BGR2GRAY)
        return vp_fail(ctx, VP_ERR_INVALID, "chain: color_mode");
    if (d->n_morph < 0 || d->n_morph > VP_CHAIN_MAX_MORPH) return vp_fail(ctx, VP_ERR_INVALID, "chain: n_morph");
    for (int i = 0; i < d->n_morph; i++)
        if (d->morph_op[i] < VP_MORPH_ERODE || d->morph_op[i] > VP_MORPH_CLOSE || d->morph_kw[i] <= 0 || d->morph_kh[i] <= 0 ||
            d->morph_iter[i] < 0)
            return vp_fail(ctx, VP_ERR_INVALID, "chain: morph op");
    if (d->ccl < 0 || d->ccl > 2) return vp_fail(ctx, VP_ERR_INVALID, "chain: ccl");
    if (d->ccl && d->numbering != VP_CCL_BLOCK2X2 && d->numbering != VP_CCL_PIXEL) return vp_fail(ctx, VP_ERR_INVALID, "chain: numbering");
    if (d->ccl && d->max_labels < 1) return vp_fail(ctx, VP_ERR_INVALID, "chain: max_labels");
    return VP_OK;
}

// frames per contour pass: the contour scratch is about 41 B/px per frame (85 MB at 1080p: sized for the worst case of 1.25 heads per
// pixel); a pass takes as many frames as fit a budget of 16 GiB (VP_CT_SCRATCH_MB overrides) - measured at 1080p, batch 128 (round 3): 16
// frames per pass 2.26 ms, 64 1.57 ms, 128 1.40 ms
static int ct_group_for(int w, int h, int max_contours)
{
    const char* e = getenv("VP_CT_SCRATCH_MB");
    long long budget = (e ? atoll(e) : 16384ll) << 20;
    if (budget < (1ll << 20)) budget = 1ll << 20;
    const long long per = (long long)vp_contours_ws_bytes(w, h, 1, max_contours);
    return (int)std::max<long long>(1, std::min<long long>(budget / per, 1 << 20));
}
// temporaries of a chain over n frames; with cd, the scratch of its contour passes: one region for min(n, ct_group_for) frames, which
// every group of frames uses again (stream order keeps them apart)
struct chain_bufs { u64 *bits_t, *bits_a, *bits_b; int32_t* nl; vp_ccl_ws ccl; uint8_t* ct; size_t ct_bytes; };
static void chain_want(vp_ws_frame& W, const vp_chain_desc* d, int n, chain_bufs* t, const vp_contour_desc* cd = nullptr)
{
    const int w = d->width, h = d->height;
    const size_t bitbytes = (size_t)n * h * vp_ww(w) * 8;
    W.want(&t->bits_t, bitbytes);   // threshold bits
    W.want(&t->bits_a, bitbytes);
    W.want(&t->bits_b, bitbytes);
    W.want(&t->nl, (size_t)n * 4);
    memset(&t->ccl, 0, sizeof t->ccl);
    if (d->ccl) vp_ccl_ws_want(W, w, h, n, d->max_labels, &t->ccl);
    t->ct = nullptr;
    t->ct_bytes = cd ? vp_contours_ws_bytes(w, h, std::min(n, ct_group_for(w, h, cd->max_contours)), cd->max_contours) : 0;
    if (cd) W.want(&t->ct, t->ct_bytes);
}

// core: all pointers device; t: its temporaries, in the frame of the caller (chain_want with the same d, n and cd)
static int chain_core(vp_ctx* ctx, const vp_chain_desc* d, const vp_chain_buffers* b, int n, const chain_bufs& t, const vp_contour_desc* cd = nullptr,
                      const vp_contour_buffers* cb = nullptr)
{
    const int w = d->width, h = d->height;
    u64 *bits_t = t.bits_t, *bits_a = t.bits_a, *bits_b = t.bits_b;
    int32_t* d_nl = t.nl;
    vp_range3 q;
    norm_range(d->color_mode == VP_BGR2GRAY ? 1 : 3, d->lo, d->hi, &q);
    VP_TRY(vpk_color_thresh(ctx, d->color_mode, b->bgr, (size_t)w * 3, w, h, n, q, b->threshed, bits_t));

    std::vector<vp_bitstage> st;
    for (int i = 0; i < d->n_morph; i++) {
        norm_se se;
        // rect kernel kw x kh, centre anchor, cv2 iteration collapse for all-ones kernels
        std::vector<uint8_t> ones((size_t)d->morph_kw[i] * d->morph_kh[i], 1);
        if (normalise_se(ones.data(), d->morph_kw[i], d->morph_kh[i], -1, -1, d->morph_iter[i], &se) != VP_OK)
            return vp_fail(ctx, VP_ERR_INVALID, "chain: kernel");
        if (se.iterations == 0 || se.kw * se.kh == 1) continue;
        rect_se k = {se.kw, se.kh, se.ax, se.ay};
        if (stages_for_op(st, d->morph_op[i], k) != VP_OK) return vp_fail(ctx, VP_ERR_INVALID, "chain: op");
    }
    const bool need_clean_bits = d->ccl == 1 || (cd && cd->source == 1);
    const u64* ccl_bits = bits_t;
    const u64* clean_bits = bits_t;   // no morphology: the cleaned mask is the threshold mask
    const vp_ccl_ws& ws = t.ccl;
    if ((!st.empty() && (need_clean_bits || b->cleaned)) || (st.empty() && b->cleaned)) {
        if (st.empty()) {
            VP_TRY(vpk_unpack_bits(ctx, bits_t, w, h, n, b->cleaned));
        } else {
            // bits_t must survive: CCL (ccl = 2) and contours (source = threshed) read it afterwards.  run_bit_stages never writes its
            // input, whatever the number of launches (mb_group_stages: they alternate between bits_b and bits_a)
            VP_TRY(run_bit_stages(ctx, st, bits_t, bits_b, bits_a, need_clean_bits, w, h, n, b->cleaned));
            if (need_clean_bits) clean_bits = bits_a;
            if (d->ccl == 1) ccl_bits = bits_a;
        }
    }
    auto contours_of_batch = [&]() -> int {
        const u64* src = cd->source == 1 ? clean_bits : bits_t;
        const size_t fw = (size_t)h * vp_ww(w);
        const size_t mc = (size_t)cd->max_contours;
        const int group = ct_group_for(w, h, cd->max_contours);
        // speckled frames in the last batch (its prefix kernel left the head counts in pinned memory): the bookkeeping as launches over
        // the chip instead of one block per frame (VP_CT_MANY=0 / 1: never / always)
        const bool many = ct_want_many(vp_ct_batch_hint(ctx));
        for (int f0 = 0; f0 < n; f0 += group) {
            const int g = std::min(group, n - f0);
            VP_TRY(vpk_find_contours(ctx, t.ct, t.ct_bytes, src + (size_t)f0 * fw, w, h, g, cd->mode, cd->method, cb->counts + f0 * mc, cb->is_hole + f0 * mc,
                                     cb->offsets + f0 * mc, cb->points + 2 * (size_t)f0 * (size_t)cd->max_points, cd->max_contours,
                                     cd->max_points, cb->info + 2 * (size_t)f0, many));
        }
        if (cb->features) VP_TRY(vpk_contour_features(ctx, cb->info, cb->counts, cb->offsets, cb->points, n, cd->max_contours, cd->max_points, cb->features));
        return VP_OK;
    };
    // The contour pass needs the mask only, not the labelling: when the chain does both it is queued on the context's side stream as
    // soon as the mask exists and runs beside the labelling and its label write (latency-bound launches beside a bandwidth-bound one);
    // the caller's stream joins it at the end.  One pass for the whole batch only (there is one scratch region).  VP_CT_SIDE=0: in a row.
    static const bool ct_side_off = getenv("VP_CT_SIDE") && atoi(getenv("VP_CT_SIDE")) == 0;
    const bool ct_side = cd && d->ccl && !ct_side_off && ctx->opt.v[VP_OPT_CHAIN_STREAMS] == 1 && ct_group_for(w, h, cd->max_contours) >= n;
    int rc_ct = VP_OK;
    bool joined = true;
    hipStream_t s_main = ctx->stream;
    if (ct_side) {
        VP_HIP(ctx, hipEventRecord(ctx->chain.ev_fb_fork, s_main));
        VP_HIP(ctx, hipStreamWaitEvent(ctx->chain.fb_stream, ctx->chain.ev_fb_fork, 0));
        ctx->stream = ctx->chain.fb_stream;
        rc_ct = contours_of_batch();
        const hipError_t ej = hipEventRecord(ctx->chain.ev_fb_join, ctx->chain.fb_stream);
        ctx->stream = s_main;
        joined = false;
        if (ej != hipSuccess) { (void)hipStreamSynchronize(ctx->chain.fb_stream); joined = true; if (rc_ct == VP_OK) rc_ct = vp_fail(ctx, VP_ERR_HIP, "hipEventRecord", ej); }
    }
    int rc_ccl = VP_OK;
    // (with the contour pass beside it the labelling keeps its six crowded-frame launches, vp_ccl_hint.h: without them the label write
    // starts ~15 us earlier and saturates memory under the latency-bound contour kernels, the longer of the two branches, for longer -
    // chain + contours 0.648 -> 0.658 ms per step of 128 frames, EXPERIMENTS.md)
    ctx->ccl.beside = joined ? 0 : 1;
    if (d->ccl) rc_ccl = vpk_ccl(ctx, ccl_bits, w, h, n, d->numbering, ws, b->labels, b->stats, b->centroids, d->max_labels, b->nlabels ? b->nlabels : d_nl);
    ctx->ccl.beside = 0;
    if (!joined && hipStreamWaitEvent(s_main, ctx->chain.ev_fb_join, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(ctx->chain.fb_stream); }
    if (rc_ccl != VP_OK) return rc_ccl;
    if (rc_ct != VP_OK) return rc_ct;
    if (cd && !ct_side) VP_TRY(contours_of_batch());
    return VP_OK;
}

static int check_cdesc(vp_ctx* ctx, const vp_contour_desc* cd, const vp_contour_buffers* cb)
{
    if (!cd || !cb) return vp_fail(ctx, VP_ERR_INVALID, "contours: descriptor");
    if (cd->source != 1 && cd->source != 2) return vp_fail(ctx, VP_ERR_INVALID, "contours: source");
    if (cd->mode != VP_RETR_EXTERNAL && cd->mode != VP_RETR_LIST) return vp_fail(ctx, VP_ERR_INVALID, "contour mode");
    if (cd->method != VP_CHAIN_APPROX_NONE && cd->method != VP_CHAIN_APPROX_SIMPLE) return vp_fail(ctx, VP_ERR_INVALID, "contour approximation");
    if (cd->max_contours <= 0 || cd->max_points <= 0) return vp_fail(ctx, VP_ERR_INVALID, "contours: capacity");
    if (!cb->info || !cb->counts || !cb->offsets || !cb->is_hole || !cb->points) return vp_fail(ctx, VP_ERR_INVALID, "contours: buffers");
    return VP_OK;
}

// Runs the chain for n frames, split into sub-batches on the context's internal streams (fork/join around the
// caller-visible stream).  Frames are independent, so the split changes scheduling only.  Each sub-batch has temporaries of its own.
struct chain_parts { int S; int cnt[4]; chain_bufs t[4]; };
static void chain_split_want(vp_ws_frame& W, vp_ctx* ctx, const vp_chain_desc* d, int n, chain_parts* p)
{
    int S = ctx->opt.v[VP_OPT_CHAIN_STREAMS];   // 1..4 (vp_options.h)
    if (S > n / 4) S = n / 4;      // keep sub-batches worth a launch
    if (S < 1) S = 1;
    p->S = S;
    for (int s = 0; s < S; s++) {
        p->cnt[s] = n / S + (s < n % S ? 1 : 0);
        chain_want(W, d, p->cnt[s], &p->t[s]);
    }
}
static int chain_split(vp_ctx* ctx, const vp_chain_desc* d, const vp_chain_buffers* b, int n, const chain_parts& p)
{
    const int S = p.S;
    if (S <= 1) return chain_core(ctx, d, b, n, p.t[0]);
    const size_t npx = (size_t)d->width * d->height;
    const size_t ml = (size_t)(d->ccl ? d->max_labels : 0);
    hipStream_t user = ctx->stream;
    VP_HIP(ctx, hipEventRecord(ctx->chain.ev_fork, user));
    int rc = VP_OK;
    int f0 = 0;
    for (int s = 0; s < S && rc == VP_OK; s++) {
        const int cnt = p.cnt[s];
        vp_chain_buffers sb = *b;
        sb.bgr = b->bgr + (size_t)f0 * npx * 3;
        if (b->threshed) sb.threshed = b->threshed + (size_t)f0 * npx;
        if (b->cleaned) sb.cleaned = b->cleaned + (size_t)f0 * npx;
        if (b->labels) sb.labels = b->labels + (size_t)f0 * npx;
        if (b->stats) sb.stats = b->stats + (size_t)f0 * ml * 5;
        if (b->centroids) sb.centroids = b->centroids + (size_t)f0 * ml * 2;
        if (b->nlabels) sb.nlabels = b->nlabels + f0;
        hipError_t e = hipStreamWaitEvent(ctx->chain.aux[s], ctx->chain.ev_fork, 0);
        if (e != hipSuccess) { rc = vp_fail(ctx, VP_ERR_HIP, "hipStreamWaitEvent", e); break; }
        ctx->stream = ctx->chain.aux[s];
        rc = chain_core(ctx, d, &sb, cnt, p.t[s]);
        ctx->stream = user;
        // join whatever was queued on the side stream, also after an error: it must not still run when the next call reuses the workspace
        const hipError_t e1 = hipEventRecord(ctx->chain.ev_join[s], ctx->chain.aux[s]);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(user, ctx->chain.ev_join[s], 0) : e1;
        if (rc != VP_OK) break;
        if (e1 != hipSuccess) { rc = vp_fail(ctx, VP_ERR_HIP, "hipEventRecord", e1); break; }
        if (e2 != hipSuccess) { rc = vp_fail(ctx, VP_ERR_HIP, "hipStreamWaitEvent", e2); break; }
        f0 += cnt;
    }
    ctx->stream = user;
    return rc;
}

// device copies of the outputs the host form was asked for (both host entries): d->x is wanted where host->x is given
static void chain_host_want(vp_ws_frame& W, const vp_chain_desc* desc, const vp_chain_buffers* host, int n, vp_chain_buffers* d)
{
    const size_t npx = (size_t)n * desc->width * desc->height;
    const size_t ml = (size_t)(desc->ccl ? desc->max_labels : 1);
    memset(d, 0, sizeof *d);
    W.want(&d->bgr, npx * 3);
    if (host->threshed) W.want(&d->threshed, npx);
    if (host->cleaned) W.want(&d->cleaned, npx);
    if (!desc->ccl) return;
    if (host->labels) W.want(&d->labels, npx * 4);
    if (host->stats) W.want(&d->stats, n * ml * 20);
    if (host->centroids) W.want(&d->centroids, n * ml * 16);
    W.want(&d->nlabels, (size_t)n * 4);
}

int vp_chain_run(vp_ctx* ctx, const vp_chain_desc* desc, const vp_chain_buffers* dev, int n_frames)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(check_desc(ctx, desc, n_frames));
    if (!dev || !dev->bgr) return vp_fail(ctx, VP_ERR_INVALID, "chain: bgr");
    vp_ws_frame W;
    chain_parts p;
    chain_split_want(W, ctx, desc, n_frames, &p);
    VP_TRY(vp_ws_commit(ctx, W, "vp_chain_run"));
    return chain_split(ctx, desc, dev, n_frames, p);
}

int vp_chain_run_host(vp_ctx* ctx, const vp_chain_desc* desc, const vp_chain_buffers* host, int n)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(check_desc(ctx, desc, n));
    if (!host || !host->bgr) return vp_fail(ctx, VP_ERR_INVALID, "chain: bgr");
    const size_t npx = (size_t)n * desc->width * desc->height;
    const size_t ml = (size_t)(desc->ccl ? desc->max_labels : 1);
    vp_ws_frame W;
    vp_chain_buffers d;
    chain_host_want(W, desc, host, n, &d);
    chain_parts p;
    chain_split_want(W, ctx, desc, n, &p);
    VP_TRY(vp_ws_commit(ctx, W, "vp_chain_run_host"));
    VP_TRY(h2d(ctx, const_cast<uint8_t*>(d.bgr), host->bgr, npx * 3));
    VP_TRY(chain_split(ctx, desc, &d, n, p));
    if (host->threshed) VP_TRY(d2h(ctx, host->threshed, d.threshed, npx));
    if (host->cleaned) VP_TRY(d2h(ctx, host->cleaned, d.cleaned, npx));
    if (desc->ccl) {
        if (host->labels) VP_TRY(d2h(ctx, host->labels, d.labels, npx * 4));
        if (host->stats) VP_TRY(d2h(ctx, host->stats, d.stats, n * ml * 20));
        if (host->centroids) VP_TRY(d2h(ctx, host->centroids, d.centroids, n * ml * 16));
        if (host->nlabels) VP_TRY(d2h(ctx, host->nlabels, d.nlabels, (size_t)n * 4));
    }
    return vp_synchronize(ctx);
}

int vp_chain_run_contours(vp_ctx* ctx, const vp_chain_desc* desc, const vp_chain_buffers* dev, const vp_contour_desc* cdesc,
                          const vp_contour_buffers* cdev, int n_frames)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(check_desc(ctx, desc, n_frames));
    VP_TRY(check_cdesc(ctx, cdesc, cdev));
    if (!dev || !dev->bgr) return vp_fail(ctx, VP_ERR_INVALID, "chain: bgr");
    vp_ws_frame W;
    chain_bufs t;
    chain_want(W, desc, n_frames, &t, cdesc);
    VP_TRY(vp_ws_commit(ctx, W, "vp_chain_run_contours"));
    return chain_core(ctx, desc, dev, n_frames, t, cdesc, cdev);
}

int vp_chain_run_contours_host(vp_ctx* ctx, const vp_chain_desc* desc, const vp_chain_buffers* host, const vp_contour_desc* cdesc,
                               const vp_contour_buffers* chost, int n)
{
    VP_TRY(check_ctx(ctx));
    VP_TRY(check_desc(ctx, desc, n));
    VP_TRY(check_cdesc(ctx, cdesc, chost));
    if (!host || !host->bgr) return vp_fail(ctx, VP_ERR_INVALID, "chain: bgr");
    const size_t npx = (size_t)n * desc->width * desc->height;
    const size_t ml = (size_t)(desc->ccl ? desc->max_labels : 1);
    const size_t mc = (size_t)cdesc->max_contours, mp = (size_t)cdesc->max_points;
    vp_ws_frame W;
    vp_chain_buffers d;
    chain_host_want(W, desc, host, n, &d);
    vp_contour_buffers c;
    W.want(&c.info, (size_t)n * 8);
    W.want(&c.counts, n * mc * 4);
    W.want(&c.offsets, n * mc * 4);
    W.want(&c.is_hole, n * mc);
    W.want(&c.points, n * mp * 8);
    c.features = nullptr;
    if (chost->features) W.want(&c.features, n * mc * 64);
    chain_bufs t;
    chain_want(W, desc, n, &t, cdesc);
    VP_TRY(vp_ws_commit(ctx, W, "vp_chain_run_contours_host"));
    VP_TRY(h2d(ctx, const_cast<uint8_t*>(d.bgr), host->bgr, npx * 3));
    VP_TRY(chain_core(ctx, desc, &d, n, t, cdesc, &c));
    if (host->threshed) VP_TRY(d2h(ctx, host->threshed, d.threshed, npx));
    if (host->cleaned) VP_TRY(d2h(ctx, host->cleaned, d.cleaned, npx));
    if (desc->ccl) {
        if (host->labels) VP_TRY(d2h(ctx, host->labels, d.labels, npx * 4));
        if (host->stats) VP_TRY(d2h(ctx, host->stats, d.stats, n * ml * 20));
        if (host->centroids) VP_TRY(d2h(ctx, host->centroids, d.centroids, n * ml * 16));
        if (host->nlabels) VP_TRY(d2h(ctx, host->nlabels, d.nlabels, (size_t)n * 4));
    }
    VP_TRY(d2h(ctx, chost->info, c.info, (size_t)n * 8));
    VP_TRY(d2h(ctx, chost->counts, c.counts, n * mc * 4));
    VP_TRY(d2h(ctx, chost->offsets, c.offsets, n * mc * 4));
    VP_TRY(d2h(ctx, chost->is_hole, c.is_hole, n * mc));
    VP_TRY(d2h(ctx, chost->points, c.points, n * mp * 8));
    if (chost->features) VP_TRY(d2h(ctx, chost->features, c.features, n * mc * 64));
    return vp_synchronize(ctx);
}

uint64_t vp_chain_algorithmic_bytes(const vp_chain_desc* desc, const vp_chain_buffers* bufs, int n)
{
    if (!desc || !bufs || n <= 0) return 0;
    const uint64_t npx = (uint64_t)n * desc->width * desc->height;
    uint64_t per = 3;
    if (bufs->threshed) per += 1;
    if (bufs->cleaned) per += 1;
    if (desc->ccl && bufs->labels) per += 4;
    return npx * per;
}

}  // extern "C"
