// C ABI of libvp.so (see include/vp.h), the context unit: version and tables, device queries, context, stream, options, timer and
// profile, device / pinned memory and copies, the workspace and the pinned ring.  The operator entries are in vp_api_color /
// vp_api_morph_chain / vp_api_shapes / vp_api_label / vp_api_filter.  No CPU arithmetic path exists in any of
// them: every operator stages its operands into HBM and launches HIP kernels.
#include "vp_api_util.h"
#include <cctype>
#include <cstdio>
#include <new>

static char g_err[256] = "";

int vp_fail(vp_ctx* ctx, int code, const char* what, hipError_t e)
{
    char* dst = ctx ? ctx->err : g_err;
    if (e != hipSuccess) snprintf(dst, 256, "%s: %s", what, hipGetErrorString(e));
    else snprintf(dst, 256, "%s", what);
    if (ctx) snprintf(g_err, 256, "%s", dst);
    return code;
}

// the profile's records: the events that exist among its 2 * cap, and the two arrays (vp_profile_begin, vp_destroy)
static void prof_release(vp_prof& P)
{
    for (int i = 0; P.ev && i < 2 * P.cap; i++)
        if (P.ev[i]) (void)hipEventDestroy(P.ev[i]);
    free(P.ev);
    free(P.ids);
    P = vp_prof{};
}

// Every failure after the allocation leaves through create_failed: the error text set at the failure stays (vp_destroy sets none)
// and vp_destroy frees exactly what exists by then.
static vp_ctx* create_failed(vp_ctx* ctx, int code, const char* what, hipError_t e = hipSuccess)
{
    vp_fail(nullptr, code, what, e);
    vp_destroy(ctx);
    return nullptr;
}

extern "C" {

int vp_version(void) { return 100; }

const char* vp_strerror(int code)
{
    switch (code) {
        case VP_OK: return "ok";
        case VP_ERR_INVALID: return "invalid argument";
        case VP_ERR_HIP: return "HIP runtime error";
        case VP_ERR_NOMEM: return "out of memory";
        case VP_ERR_UNSUPPORTED: return "unsupported";
        case VP_ERR_CAPACITY: return "capacity exceeded";
        default: return "unknown error";
    }
}

const char* vp_last_error(const vp_ctx* ctx) { return ctx ? ctx->err : g_err; }

int vp_get_tables(uint16_t* gamma, uint16_t* cbrt_tab, int32_t* sdiv, int32_t* hdiv180, int32_t* lab_coeffs)
{
    vp_host_tables(gamma, cbrt_tab, sdiv, hdiv180, lab_coeffs);
    return VP_OK;
}

int vp_get_lab_inv_tables(uint16_t* yf, int32_t* ab_xz, uint16_t* inv_gamma, int32_t* coeffs)
{
    vp_host_lab_inv_tables(yf, ab_xz, inv_gamma, coeffs);
    return VP_OK;
}

int vp_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// "0000:05:00.0"-style PCI address of a device: /sys/bus/pci/devices/<address>/numa_node tells which host memory and cores sit next
// to it (the multi-device dispatcher binds each feeder thread there)
int vp_device_pci_bus_id(int device, char* out, int len)
{
    if (!out || len < 16) return VP_ERR_INVALID;
    out[0] = 0;
    hipError_t e = hipDeviceGetPCIBusId(out, len, device);
    if (e != hipSuccess) return vp_fail(nullptr, VP_ERR_HIP, "hipDeviceGetPCIBusId", e);
    for (char* c = out; *c; c++) *c = (char)tolower(*c);
    return VP_OK;
}

vp_ctx* vp_create(int device)
{
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { vp_fail(nullptr, VP_ERR_HIP, "no HIP device (libvp has no CPU path)", e); return nullptr; }
    if (device < 0 || device >= ndev) { vp_fail(nullptr, VP_ERR_INVALID, "device index out of range"); return nullptr; }
    if ((e = hipSetDevice(device)) != hipSuccess) { vp_fail(nullptr, VP_ERR_HIP, "hipSetDevice", e); return nullptr; }
    vp_ctx* ctx = new (std::nothrow) vp_ctx();
    if (!ctx) return nullptr;
    memset(ctx, 0, sizeof *ctx);
    ctx->device = device;
    vp_options_defaults(&ctx->opt, getenv);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return create_failed(ctx, VP_ERR_HIP, "hipGetDeviceProperties", e);
    ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if ((e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking)) != hipSuccess) return create_failed(ctx, VP_ERR_HIP, "hipStreamCreate", e);
    ctx->stream = ctx->own_stream;
    if ((e = hipEventCreate(&ctx->ev0)) != hipSuccess || (e = hipEventCreate(&ctx->ev1)) != hipSuccess) return create_failed(ctx, VP_ERR_HIP, "timer events", e);
    for (int i = 0; i < 4; i++) {
        if ((e = hipStreamCreateWithFlags(&ctx->chain.aux[i], hipStreamNonBlocking)) != hipSuccess) return create_failed(ctx, VP_ERR_HIP, "aux stream", e);
        if ((e = hipEventCreateWithFlags(&ctx->chain.ev_join[i], hipEventDisableTiming)) != hipSuccess) return create_failed(ctx, VP_ERR_HIP, "aux event", e);
    }
    if ((e = hipEventCreateWithFlags(&ctx->chain.ev_fork, hipEventDisableTiming)) != hipSuccess) return create_failed(ctx, VP_ERR_HIP, "aux event", e);
    if ((e = hipStreamCreateWithFlags(&ctx->chain.fb_stream, hipStreamNonBlocking)) != hipSuccess) return create_failed(ctx, VP_ERR_HIP, "side stream", e);
    if ((e = hipEventCreateWithFlags(&ctx->chain.ev_fb_fork, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->chain.ev_fb_join, hipEventDisableTiming)) != hipSuccess)
        return create_failed(ctx, VP_ERR_HIP, "side stream event", e);
    if ((e = hipEventCreateWithFlags(&ctx->ev_upload, hipEventDisableTiming)) != hipSuccess) return create_failed(ctx, VP_ERR_HIP, "upload event", e);
    // tables: gamma u16[256] | cbrt u16[2048] | sdiv i32[256] | hdiv i32[256]
    std::vector<uint16_t> gamma(256), cbrt(3072);
    std::vector<int32_t> sdiv(256), hdiv(256);
    int32_t labC[9];
    vp_host_tables(gamma.data(), cbrt.data(), sdiv.data(), hdiv.data(), labC);
    static const int32_t expectC[9] = {1777, 1541, 778, 871, 2929, 296, 73, 448, 3575};
    if (memcmp(labC, expectC, sizeof labC) != 0) return create_failed(ctx, VP_ERR_INVALID, "Lab coefficient table mismatch");
    const size_t bytes = 512 + 4096 + 1024 + 1024;
    if ((e = hipMalloc(&ctx->d_tables, bytes + 256)) != hipSuccess) return create_failed(ctx, VP_ERR_NOMEM, "hipMalloc tables", e);
    uint8_t* base = (uint8_t*)ctx->d_tables;
    hipMemcpy(base, gamma.data(), 512, hipMemcpyHostToDevice);
    hipMemcpy(base + 512, cbrt.data(), 4096, hipMemcpyHostToDevice);
    hipMemcpy(base + 512 + 4096, sdiv.data(), 1024, hipMemcpyHostToDevice);
    e = hipMemcpy(base + 512 + 4096 + 1024, hdiv.data(), 1024, hipMemcpyHostToDevice);
    if (e != hipSuccess) return create_failed(ctx, VP_ERR_HIP, "table upload", e);
    ctx->tab.gamma = (const uint16_t*)base;
    ctx->tab.cbrt = (const uint16_t*)(base + 512);
    ctx->tab.sdiv = (const int32_t*)(base + 512 + 4096);
    ctx->tab.hdiv = (const int32_t*)(base + 512 + 4096 + 1024);
    ctx->cb.folds_own = (u32*)(base + bytes);       // a word of the context's own: workspace pointers do not survive a later call
    hipMemset(ctx->cb.folds_own, 0, 4);
    // Lab -> BGR tables: abToXZ_b i32[VP_LAB_AB_TAB] | LabToYF_b u16[512] | inverse gamma as bytes [4096]
    {
        std::vector<int32_t> abxz(VP_LAB_AB_TAB);
        std::vector<uint16_t> yf(512), invg16(4096);
        std::vector<uint8_t> invg(4096);
        vp_host_lab_inv_tables(yf.data(), abxz.data(), invg16.data(), nullptr);
        for (int i = 0; i < 4096; i++) invg[i] = (uint8_t)invg16[i];
        const size_t nab = (size_t)VP_LAB_AB_TAB * 4;
        if ((e = hipMalloc(&ctx->d_labinv, nab + 1024 + 4096)) != hipSuccess) return create_failed(ctx, VP_ERR_NOMEM, "hipMalloc Lab -> BGR tables", e);
        uint8_t* lb = (uint8_t*)ctx->d_labinv;
        hipMemcpy(lb, abxz.data(), nab, hipMemcpyHostToDevice);
        hipMemcpy(lb + nab, yf.data(), 1024, hipMemcpyHostToDevice);
        if ((e = hipMemcpy(lb + nab + 1024, invg.data(), 4096, hipMemcpyHostToDevice)) != hipSuccess) return create_failed(ctx, VP_ERR_HIP, "Lab -> BGR table upload", e);
        ctx->tab.abxz = (const int32_t*)lb;
        ctx->tab.yf = (const uint16_t*)(lb + nab);
        ctx->tab.invg = lb + nab + 1024;
    }
    return ctx;
}

// Frees whatever exists, so that it also serves a context vp_create could not finish: no HIP call on a null handle, and no error text
// of its own (the one set at a failure stays for vp_last_error(NULL)).
int vp_destroy(vp_ctx* ctx)
{
    if (!ctx) return VP_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    vp_post_teardown(ctx);
    vp_ccl_teardown(ctx);
    vp_contours_teardown(ctx);
    vp_hough_circles_teardown(ctx);
    vp_adaptive_teardown(ctx);
    vp_features_teardown(ctx);
    if (ctx->ws) (void)hipFree(ctx->ws);
    for (int i = 0; i < 4; i++) {
        if (ctx->ring_buf[i]) (void)hipHostFree(ctx->ring_buf[i]);
        if (ctx->ring_ev[i]) (void)hipEventDestroy(ctx->ring_ev[i]);
    }
    if (ctx->hstage) (void)hipHostFree(ctx->hstage);
    if (ctx->d_tables) (void)hipFree(ctx->d_tables);
    if (ctx->d_labinv) (void)hipFree(ctx->d_labinv);
    prof_release(ctx->prof);
    auto drop_event = [](hipEvent_t ev) { if (ev) (void)hipEventDestroy(ev); };
    auto drop_stream = [](hipStream_t s) { if (s) (void)hipStreamDestroy(s); };
    drop_event(ctx->ev0);
    drop_event(ctx->ev1);
    for (int i = 0; i < 4; i++) { drop_stream(ctx->chain.aux[i]); drop_event(ctx->chain.ev_join[i]); }
    drop_event(ctx->chain.ev_fork);
    drop_stream(ctx->chain.fb_stream);
    drop_event(ctx->chain.ev_fb_fork);
    drop_event(ctx->chain.ev_fb_join);
    drop_event(ctx->ev_upload);
    drop_stream(ctx->own_stream);
    delete ctx;
    return VP_OK;
}

int vp_set_stream(vp_ctx* ctx, void* hip_stream)
{
    if (!ctx) return VP_ERR_INVALID;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    // The labelling's accumulator set is kept clean in the order of one stream: another stream starts it anew.  (As for every buffer of
    // the context, the caller has let the old stream's work finish, or ordered the new stream behind it, before using the new one.)
    if (s != ctx->stream) ctx->ccl.c3_acc_dirty = 1;
    ctx->stream = s;
    return VP_OK;
}
void* vp_get_stream(vp_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int vp_set_option(vp_ctx* ctx, int option, int value)
{
    if (!ctx) return VP_ERR_INVALID;
    return vp_options_set(&ctx->opt, option, value) ? VP_OK : vp_fail(ctx, VP_ERR_INVALID, "vp_set_option");
}

int vp_ccl_last_launches(vp_ctx* ctx, int32_t* launches)
{
    if (!ctx || !launches) return VP_ERR_INVALID;
    *launches = ctx->ccl.launches;
    return VP_OK;
}

int vp_synchronize(vp_ctx* ctx)
{
    if (!ctx) return VP_ERR_INVALID;
    VP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VP_OK;
}

int vp_timer_start(vp_ctx* ctx)
{
    if (!ctx) return VP_ERR_INVALID;
    VP_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    return VP_OK;
}
int vp_timer_stop(vp_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return VP_ERR_INVALID;
    VP_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    VP_HIP(ctx, hipEventSynchronize(ctx->ev1));
    VP_HIP(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return VP_OK;
}

int vp_profile_begin(vp_ctx* ctx, int max_records)
{
    if (!ctx || max_records <= 0) return VP_ERR_INVALID;
    vp_prof& P = ctx->prof;
    if (P.cap < max_records) {
        prof_release(P);
        P.ev = (hipEvent_t*)calloc(2 * (size_t)max_records, sizeof(hipEvent_t));
        P.ids = (int*)malloc(sizeof(int) * max_records);
        if (!P.ev || !P.ids) { prof_release(P); return vp_fail(ctx, VP_ERR_NOMEM, "profile records"); }
        P.cap = max_records;                       // from here on prof_release knows the events: the ones not made yet are null
        for (int i = 0; i < 2 * max_records; i++) {
            const hipError_t e = hipEventCreate(&P.ev[i]);
            if (e != hipSuccess) { prof_release(P); return vp_fail(ctx, VP_ERR_HIP, "hipEventCreate(&P.ev[i])", e); }
        }
    }
    P.used = 0;
    P.on = true;
    return VP_OK;
}

int vp_profile_end(vp_ctx* ctx, double* total_ms, int32_t* launches)
{
    if (!ctx || !total_ms || !launches) return VP_ERR_INVALID;
    vp_prof& P = ctx->prof;
    P.on = false;
    VP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < VP_PROF_KERNELS; k++) { total_ms[k] = 0; launches[k] = 0; }
    for (int r = 0; r < P.used; r++) {
        float ms = 0;
        VP_HIP(ctx, hipEventElapsedTime(&ms, P.ev[2 * r], P.ev[2 * r + 1]));
        total_ms[P.ids[r]] += ms;
        launches[P.ids[r]]++;
    }
    return VP_OK;
}

const char* vp_profile_kernel_name(int id)
{
    static const char* names[VP_PROF_KERNELS] = {"k_color_thresh", "k_morph_bits", "k_ccl_local", "k_ccl_boundary", "k_ccl_flatten", "k_ccl_rank",
                                                  "k_ccl_bg", "k_ccl_stats", "k_ccl_final", "k_ccl_write", "memset", "other",
                                                  "k_ccl2_local", "k_ccl2_merge", "k_ccl2_write", "k_sgm_cost", "k_sgm_path", "k_sgm_select"};
    return (id >= 0 && id < VP_PROF_KERNELS) ? names[id] : "?";
}

int vp_dev_alloc(vp_ctx* ctx, size_t bytes, void** p)
{
    if (!ctx || !p) return VP_ERR_INVALID;
    hipSetDevice(ctx->device);
    hipError_t e = hipMalloc(p, bytes ? bytes : 1);
    if (e != hipSuccess) return vp_fail(ctx, VP_ERR_NOMEM, "hipMalloc", e);
    return VP_OK;
}
int vp_dev_free(vp_ctx* ctx, void* p)
{
    if (!ctx) return hipFree(p) == hipSuccess ? VP_OK : VP_ERR_HIP;   // device memory outlives the context it was allocated through
    VP_HIP(ctx, hipFree(p));
    return VP_OK;
}
int vp_host_alloc(vp_ctx* ctx, size_t bytes, void** p)
{
    if (!ctx || !p) return VP_ERR_INVALID;
    hipSetDevice(ctx->device);
    hipError_t e = hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return vp_fail(ctx, VP_ERR_NOMEM, "hipHostMalloc", e);
    return VP_OK;
}
int vp_host_free(vp_ctx* ctx, void* p)
{
    if (!ctx) return hipHostFree(p) == hipSuccess ? VP_OK : VP_ERR_HIP;   // page-locked memory is not tied to a context
    VP_HIP(ctx, hipHostFree(p));
    return VP_OK;
}
int vp_host_register(vp_ctx* ctx, void* p, size_t bytes)
{
    if (!ctx || !p || !bytes) return VP_ERR_INVALID;
    hipSetDevice(ctx->device);
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();                       // a refusal is an answer, not a fault of the context
        snprintf(ctx->err, sizeof ctx->err, "hipHostRegister refused %zu bytes: %s", bytes, hipGetErrorString(e));
        return VP_ERR_UNSUPPORTED;
    }
    return VP_OK;
}
int vp_host_unregister(vp_ctx* ctx, void* p)
{
    const hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) { (void)hipGetLastError(); return ctx ? vp_fail(ctx, VP_ERR_HIP, "hipHostUnregister", e) : VP_ERR_HIP; }
    return VP_OK;
}
int vp_memcpy_d2d_async(vp_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx || !dst || !src) return VP_ERR_INVALID;
    if (bytes) VP_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return VP_OK;
}
int vp_memcpy_h2d(vp_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx) return VP_ERR_INVALID;
    VP_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    VP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VP_OK;
}
// Enqueues the copy and marks its end on the stream; vp_wait_uploads returns once every copy enqueued so far has read its source
// (kernels enqueued behind the copies are not waited for).
int vp_memcpy_h2d_async(vp_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx) return VP_ERR_INVALID;
    VP_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    VP_HIP(ctx, hipEventRecord(ctx->ev_upload, ctx->stream));
    return VP_OK;
}
int vp_wait_uploads(vp_ctx* ctx)
{
    if (!ctx) return VP_ERR_INVALID;
    VP_HIP(ctx, hipEventSynchronize(ctx->ev_upload));
    return VP_OK;
}
int vp_memcpy_d2h(vp_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx) return VP_ERR_INVALID;
    VP_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    VP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VP_OK;
}

}  // extern "C"

// ---- workspace ------------------------------------------------------------------------------------

static int vp_ws_reserve(vp_ctx* ctx, size_t bytes)
{
    if (bytes <= ctx->ws_cap) return VP_OK;
    VP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->ws) { hipFree(ctx->ws); ctx->ws = nullptr; ctx->ws_cap = 0; }
    const size_t want = vp_align(bytes + bytes / 8, 1 << 20);
    hipError_t e = hipMalloc((void**)&ctx->ws, want);
    if (e != hipSuccess) return vp_fail(ctx, VP_ERR_NOMEM, "workspace hipMalloc", e);
    ctx->ws_cap = want;
    return VP_OK;
}

int vp_ws_commit(vp_ctx* ctx, const vp_ws_frame& W, const char* who)
{
    if (W.overflowed()) return vp_fail(ctx, VP_ERR_INVALID, "too many workspace buffers");
    if (W.wrapped) return vp_fail(ctx, VP_ERR_NOMEM, who);
    const int rc = vp_ws_reserve(ctx, W.bytes() ? W.bytes() : 1);   // at least a byte: a frame of empty buffers still gets valid pointers
    if (rc != VP_OK) return rc;
    W.assign(ctx->ws);
    return VP_OK;
}

void* vp_hstage(vp_ctx* ctx, size_t bytes)
{
    if (bytes <= ctx->hstage_cap) return ctx->hstage;
    if (ctx->hstage) { (void)hipStreamSynchronize(ctx->stream); (void)hipHostFree(ctx->hstage); ctx->hstage = nullptr; ctx->hstage_cap = 0; }
    const size_t cap = (bytes + (1u << 20) - 1) >> 20 << 20;
    void* p = nullptr;
    if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess) return nullptr;
    ctx->hstage = (uint8_t*)p;
    ctx->hstage_cap = cap;
    return p;
}

// ---- pinned ring ---------------------------------------------------------------------------------
// small host -> device hand-overs that must not wait (vp_api_util.h has the contract)
uint8_t* vp_ring_take(vp_ctx* ctx, size_t bytes, int* slot)
{
    const int s = ctx->ring_next;
    ctx->ring_next = (s + 1) & 3;
    if (ctx->ring_busy[s]) { (void)hipEventSynchronize(ctx->ring_ev[s]); ctx->ring_busy[s] = 0; }
    if (bytes > ctx->ring_cap[s]) {
        if (ctx->ring_buf[s]) { (void)hipHostFree(ctx->ring_buf[s]); ctx->ring_buf[s] = nullptr; ctx->ring_cap[s] = 0; }
        const size_t cap = (bytes + (1u << 16) - 1) >> 16 << 16;
        void* p = nullptr;
        if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        ctx->ring_buf[s] = (uint8_t*)p;
        ctx->ring_cap[s] = cap;
    }
    if (!ctx->ring_ev[s] && hipEventCreateWithFlags(&ctx->ring_ev[s], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    *slot = s;
    return ctx->ring_buf[s];
}
void vp_ring_done(vp_ctx* ctx, int slot)
{
    if (slot < 0) return;
    if (hipEventRecord(ctx->ring_ev[slot], ctx->stream) == hipSuccess) ctx->ring_busy[slot] = 1;
    else { (void)hipGetLastError(); (void)hipStreamSynchronize(ctx->stream); }
}
