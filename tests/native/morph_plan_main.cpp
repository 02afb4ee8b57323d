// The bit-plane morphology plan (csrc/vp_morph_plan.h) on the host: every stage list below at widths 1..8320 (every multiple of 64
// and its neighbours) and heights 1, 32, 33, 64, 65, 129 is planned the way vp_api_morph_chain.hip and vp_morph.hip plan it, and the
// properties the kernels rely on are asserted per case; then the widths at which the dispatch switches are printed in the format of
// tests/golden/morph_plan.txt.  Built with -fsanitize=address,undefined by tests/test_morph_plan_host.py.
#include "vp_morph_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

struct op_t { int op, kw, kh, ax, ay; };
struct named_plan { std::string name; std::vector<op_t> ops; std::vector<vp_bitstage> st; };

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static op_t rect_op(int op, int kw, int kh, int iterations = 1)
{
    // cv2's collapse of iterations of an all-ones kernel, centre anchor (normalise_se in vp_api_morph_chain.hip)
    int ax = kw / 2, ay = kh / 2;
    ax *= iterations; ay *= iterations;
    kw += (iterations - 1) * (kw - 1); kh += (iterations - 1) * (kh - 1);
    return op_t{op, kw, kh, ax, ay};
}

static named_plan make(const std::string& name, const std::vector<op_t>& ops)
{
    named_plan P;
    P.name = name; P.ops = ops;
    for (const op_t& o : ops) {
        const mb_rect k = {o.kw, o.kh, o.ax, o.ay};
        if (!mb_stages_for_op(P.st, o.op, k)) { fprintf(stderr, "bad op in %s\n", name.c_str()); exit(2); }
    }
    return P;
}

// the elementary erodes / dilates of the operations, neighbours of one kind summed: what the stages must add up to, run by run
static std::vector<vp_bitstage> runs_of(const std::vector<vp_bitstage>& v)
{
    std::vector<vp_bitstage> r;
    for (const vp_bitstage& s : v) {
        if (!r.empty() && r.back().dilate == s.dilate) { r.back().l += s.l; r.back().r += s.r; r.back().u += s.u; r.back().d += s.d; }
        else r.push_back(s);
    }
    return r;
}
static void check_stages(const named_plan& P)
{
    std::vector<vp_bitstage> elem;
    for (const op_t& o : P.ops) {
        const vp_bitstage e = {0, o.ax, o.kw - 1 - o.ax, o.ay, o.kh - 1 - o.ay};
        vp_bitstage d = e; d.dilate = 1;
        if (o.op == MB_OP_ERODE) elem.push_back(e);
        else if (o.op == MB_OP_DILATE) elem.push_back(d);
        else if (o.op == MB_OP_OPEN) { elem.push_back(e); elem.push_back(d); }
        else { elem.push_back(d); elem.push_back(e); }
    }
    const std::vector<vp_bitstage> want = runs_of(elem), got = runs_of(P.st);
    CHECK(want.size() == got.size(), "%s: %zu runs, want %zu", P.name.c_str(), got.size(), want.size());
    for (size_t i = 0; i < want.size() && i < got.size(); i++)
        CHECK(want[i].dilate == got[i].dilate && want[i].l == got[i].l && want[i].r == got[i].r && want[i].u == got[i].u && want[i].d == got[i].d,
              "%s: run %zu sums to %d %d %d %d", P.name.c_str(), i, got[i].l, got[i].r, got[i].u, got[i].d);
    for (const vp_bitstage& s : P.st) {
        CHECK(s.l >= 0 && s.l <= 31 && s.r >= 0 && s.r <= 31 && s.u >= 0 && s.u <= 31 && s.d >= 0 && s.d <= 31, "%s: extent outside 0..31", P.name.c_str());
        CHECK(mb_stage_ok(s), "%s: mb_stage_ok", P.name.c_str());
        CHECK((s.l | s.r | s.u | s.d) != 0, "%s: an empty stage", P.name.c_str());
    }
}

// the planes of a run of launches: no launch writes the input or what it reads, the last and only the last writes the output, every
// launch reads what the one before it wrote, and the last does not read the second scratch plane (a caller may back it with the
// output plane).  Returns a description of the first violation, or an empty string.
static std::string planes_fault(const std::vector<mb_launch>& L)
{
    for (size_t k = 0; k < L.size(); k++) {
        const bool last = k + 1 == L.size();
        if (L[k].dst == MB_BUF_IN) return "launch " + std::to_string(k) + " writes the input";
        if (L[k].src == L[k].dst) return "launch " + std::to_string(k) + " writes what it reads";
        if ((L[k].dst == MB_BUF_OUT) != last) return "launch " + std::to_string(k) + (last ? " is the last and does not write the output" : " writes the output early");
        if (L[k].src != (k == 0 ? (int)MB_BUF_IN : L[k - 1].dst)) return "launch " + std::to_string(k) + " does not read its predecessor's result";
        if (L[k].src < MB_BUF_IN || L[k].src > MB_BUF_SCRATCH2 || L[k].dst < MB_BUF_SCRATCH || L[k].dst > MB_BUF_OUT) return "launch " + std::to_string(k) + ": no such plane";
        if (last && L[k].src == MB_BUF_SCRATCH2) return "the last launch reads the plane that may back the output";
    }
    return "";
}

// the ping-pong as run_bit_stages did it before the plan had a header: input and scratch swap after every launch but the last
static void planes_before(std::vector<mb_launch>& L)
{
    int cur = MB_BUF_IN, other = MB_BUF_SCRATCH;
    for (size_t k = 0; k < L.size(); k++) {
        const bool last = k + 1 == L.size();
        L[k].src = cur;
        L[k].dst = last ? (int)MB_BUF_OUT : other;
        if (!last) { const int t = cur; cur = other; other = t; }
    }
}

static std::string planes_text(const std::vector<mb_launch>& L)
{
    std::string s;
    for (size_t k = 0; k < L.size(); k++) s += (k ? "," : "") + std::to_string(L[k].src) + ">" + std::to_string(L[k].dst);
    return s;
}

static vp_bitplan plan_of(const std::vector<vp_bitstage>& st, const mb_launch& L)
{
    vp_bitplan p;
    p.n = L.count;
    for (int i = 0; i < L.count; i++) p.s[i] = st[(size_t)L.first + i];
    return p;
}

static void check_case(const named_plan& P, int w, int h)
{
    const int ww = vp_ww(w);
    std::vector<mb_launch> L;
    const bool ok = mb_group_stages(P.st, ww, L);
    // a refusal happens exactly when a stage alone - the first one of some launch - exceeds the budget
    size_t stage_lds = 0;
    for (const vp_bitstage& s : P.st) stage_lds = std::max(stage_lds, (size_t)2 * (32 + s.u + s.d) * ww * 8);
    CHECK(ok == (stage_lds <= 150 * 1024), "%s w=%d: refusal %d, the tallest stage takes %zu bytes", P.name.c_str(), w, (int)!ok, stage_lds);
    if (!ok) { CHECK(L.empty(), "%s w=%d: launches left behind a refusal", P.name.c_str(), w); return; }
    CHECK(!L.empty(), "%s w=%d: no launch", P.name.c_str(), w);
    const std::string fault = planes_fault(L);
    CHECK(fault.empty(), "%s w=%d h=%d planes %s: %s", P.name.c_str(), w, h, planes_text(L).c_str(), fault.c_str());
    int next = 0;
    for (const mb_launch& l : L) {
        CHECK(l.first == next && l.count >= 1 && l.count <= VP_MAX_STAGES, "%s w=%d: launches do not partition the stages", P.name.c_str(), w);
        next = l.first + l.count;
        const vp_bitplan p = plan_of(P.st, l);
        for (int sym_ok = 0; sym_ok < 2; sym_ok++)
            for (int tall_ok = 0; tall_ok < 2; tall_ok++) {
                const mb_kernel K = mb_choose_kernel(p, w, h, sym_ok != 0, tall_ok != 0);
                CHECK(K.ok, "%s w=%d h=%d: a grouped launch that no kernel takes (%zu bytes)", P.name.c_str(), w, h, K.lds);
                int rows = 0;   // the rows the kernel stages: recomputed here from the stages, not from the header's helpers
                for (int i = 0; i < p.n; i++) rows += p.s[i].u + p.s[i].d;
                rows += K.strip;
                CHECK(K.lds == (size_t)2 * rows * ww * 8, "%s w=%d h=%d: %zu bytes of LDS for %d rows", P.name.c_str(), w, h, K.lds, rows);
                if (K.sym >= 0) {
                    CHECK(sym_ok && K.sym < MB_SYM_COUNT && mb_sym_lookup(p) == K.sym, "%s w=%d: specialised shape %d", P.name.c_str(), w, K.sym);
                    CHECK(K.strip == 32 || (K.strip == 64 && tall_ok && h > 64), "%s w=%d h=%d: strip %d", P.name.c_str(), w, h, K.strip);
                    CHECK(K.lds <= (K.strip == 64 ? (size_t)40 * 1024 : (size_t)64 * 1024), "%s w=%d h=%d: specialised kernel with %zu bytes", P.name.c_str(), w, h, K.lds);
                } else {
                    CHECK(K.strip == 32 && K.lds <= (size_t)160 * 1024, "%s w=%d h=%d: runtime-plan kernel with %zu bytes", P.name.c_str(), w, h, K.lds);
                }
            }
    }
    CHECK(next == (int)P.st.size(), "%s w=%d: %d of %zu stages launched", P.name.c_str(), w, next, P.st.size());
    // where one or two launches do, the planes are the ones they always were
    if (L.size() <= 2) {
        std::vector<mb_launch> B = L;
        planes_before(B);
        CHECK(planes_text(B) == planes_text(L), "%s w=%d: planes %s, were %s", P.name.c_str(), w, planes_text(L).c_str(), planes_text(B).c_str());
    }
}

// the last width (a multiple of 64, up to 65536) at which `holds` is true, as text: "-" never, ">65536" at every width searched
template <class F> static std::string last_width(F holds)
{
    int last = 0;
    for (int ww = 1; ww <= 1024; ww++)
        if (holds(ww * 64)) last = ww * 64;
        else break;
    return last == 0 ? "-" : last == 65536 ? ">65536" : std::to_string(last);
}

int main()
{
    std::vector<named_plan> plans;
    // the 12 specialised shapes, in the order of MB_SYM_SHAPES
    plans.push_back(make("open5+close5", {rect_op(MB_OP_OPEN, 5, 5), rect_op(MB_OP_CLOSE, 5, 5)}));
    plans.push_back(make("close5+open5", {rect_op(MB_OP_CLOSE, 5, 5), rect_op(MB_OP_OPEN, 5, 5)}));
    plans.push_back(make("open5", {rect_op(MB_OP_OPEN, 5, 5)}));
    plans.push_back(make("close5", {rect_op(MB_OP_CLOSE, 5, 5)}));
    plans.push_back(make("open3+close3", {rect_op(MB_OP_OPEN, 3, 3), rect_op(MB_OP_CLOSE, 3, 3)}));
    plans.push_back(make("close3+open3", {rect_op(MB_OP_CLOSE, 3, 3), rect_op(MB_OP_OPEN, 3, 3)}));
    plans.push_back(make("open3", {rect_op(MB_OP_OPEN, 3, 3)}));
    plans.push_back(make("close3", {rect_op(MB_OP_CLOSE, 3, 3)}));
    plans.push_back(make("erode3", {rect_op(MB_OP_ERODE, 3, 3)}));
    plans.push_back(make("dilate3", {rect_op(MB_OP_DILATE, 3, 3)}));
    plans.push_back(make("erode5", {rect_op(MB_OP_ERODE, 5, 5)}));
    plans.push_back(make("dilate5", {rect_op(MB_OP_DILATE, 5, 5)}));
    const size_t nsym = plans.size();
    for (size_t i = 0; i < nsym; i++) {
        vp_bitplan p;
        p.n = (int)plans[i].st.size();
        CHECK(p.n <= 3, "%s: %d stages", plans[i].name.c_str(), p.n);
        for (int k = 0; k < p.n && k < 3; k++) p.s[k] = plans[i].st[k];
        CHECK(mb_sym_lookup(p) == (int)i, "%s is shape %d, want %zu", plans[i].name.c_str(), mb_sym_lookup(p), i);
    }
    CHECK(nsym == (size_t)MB_SYM_COUNT, "%d specialised shapes", MB_SYM_COUNT);
    static const int rects[][2] = {{7, 7}, {4, 2}, {9, 3}, {71, 5}, {5, 71}, {71, 71}};
    static const char* opname[] = {"erode", "dilate", "open", "close"};
    for (int op : {MB_OP_ERODE, MB_OP_OPEN, MB_OP_CLOSE})
        for (const auto& r : rects)
            plans.push_back(make(std::string(opname[op]) + std::to_string(r[0]) + "x" + std::to_string(r[1]), {rect_op(op, r[0], r[1])}));
    plans.push_back(make("erode3x3i3", {rect_op(MB_OP_ERODE, 3, 3, 3)}));
    plans.push_back(make("erode5x5i20", {rect_op(MB_OP_ERODE, 5, 5, 20)}));
    plans.push_back(make("erode5x45", {rect_op(MB_OP_ERODE, 5, 45)}));
    for (int k : {5, 21, 61})
        for (int len = 1; len <= 8; len++) {
            std::vector<op_t> ops;
            for (int i = 0; i < len; i++) ops.push_back(rect_op(i % 2 ? MB_OP_CLOSE : MB_OP_OPEN, k, k));
            plans.push_back(make("chain" + std::to_string(len) + "x" + std::to_string(k), ops));
        }
    for (size_t i = nsym; i < plans.size(); i++) {
        vp_bitplan p;
        p.n = (int)std::min<size_t>(plans[i].st.size(), VP_MAX_STAGES);
        for (int k = 0; k < p.n; k++) p.s[k] = plans[i].st[k];
        if (plans[i].st.size() <= 3 && plans[i].name != "chain1x5" && plans[i].name != "chain2x5") CHECK(mb_sym_lookup(p) < 0, "%s counts as a specialised shape", plans[i].name.c_str());
    }

    std::vector<int> widths = {1, 2};
    for (int k = 1; k <= 130; k++) for (int d = -1; d <= 1; d++) widths.push_back(64 * k + d);
    static const int heights[] = {1, 32, 33, 64, 65, 129};
    for (const named_plan& P : plans) {
        check_stages(P);
        for (int w : widths)
            for (int h : heights) check_case(P, w, h);
    }

    // the ping-pong as it was fails this program's checks as soon as a plan needs three launches: its second launch writes the input
    for (const named_plan& P : plans) {
        if (P.name != "chain8x21") continue;
        std::vector<mb_launch> L;
        CHECK(mb_group_stages(P.st, vp_ww(3840), L) && L.size() >= 3, "chain8x21 at 3840: %zu launches", L.size());
        planes_before(L);
        CHECK(planes_fault(L) == "launch 1 writes the input", "the former planes %s pass: %s", planes_text(L).c_str(), planes_fault(L).c_str());
        printf("# planes: 0 input, 1 scratch, 2 second scratch, 3 output.  chain8x21 at w=3840 as planned before this table existed: %s (%s)\n", planes_text(L).c_str(),
               planes_fault(L).c_str());
    }

    // the switch widths: the last width, a multiple of 64, on the near side of every switch ("-": never on that side; h = 129, so
    // that 64-row strips are allowed)
    printf("# plan stages halo(sum of u+d) shape : last width with 64-row strips | with a specialised kernel | with one launch | accepted\n");
    for (const named_plan& P : plans) {
        int halo = 0;
        for (const vp_bitstage& s : P.st) halo += s.u + s.d;
        auto launches = [&](int w) { std::vector<mb_launch> L; return mb_group_stages(P.st, vp_ww(w), L) ? (int)L.size() : 0; };
        auto kernel = [&](int w) {
            std::vector<mb_launch> L;
            mb_kernel K = {0, -1, 0, 0};
            if (mb_group_stages(P.st, vp_ww(w), L) && L.size() == 1) K = mb_choose_kernel(plan_of(P.st, L[0]), w, 129, true, true);
            return K;
        };
        const mb_kernel K0 = kernel(64);
        printf("plan=%s stages=%zu halo=%d shape=%s strip64_last=%s sym_last=%s one_launch_last=%s accepted_last=%s\n", P.name.c_str(), P.st.size(), halo,
               K0.sym >= 0 ? std::to_string(K0.sym).c_str() : "-",
               last_width([&](int w) { const mb_kernel K = kernel(w); return K.ok && K.sym >= 0 && K.strip == 64; }).c_str(),
               last_width([&](int w) { const mb_kernel K = kernel(w); return K.ok && K.sym >= 0; }).c_str(),
               last_width([&](int w) { return launches(w) == 1; }).c_str(), last_width([&](int w) { return launches(w) >= 1; }).c_str());
    }
    // single cases the GPU tests and DESIGN.md quote
    struct { const char* plan; int h, w; } cases[] = {{"open5+close5", 1080, 1920}, {"open5+close5", 2160, 3840}, {"close71x71", 70, 3840}, {"open71x71", 70, 3840},
                                                     {"chain8x21", 40, 3840}, {"erode5x45", 40, 8192}, {"open5", 70, 8192}};
    for (const auto& c : cases)
        for (const named_plan& P : plans) {
            if (P.name != c.plan) continue;
            std::vector<mb_launch> L;
            if (!mb_group_stages(P.st, vp_ww(c.w), L)) { printf("case plan=%s h=%d w=%d refused\n", c.plan, c.h, c.w); continue; }
            printf("case plan=%s h=%d w=%d launches=%zu planes=%s kernels=", c.plan, c.h, c.w, L.size(), planes_text(L).c_str());
            for (size_t k = 0; k < L.size(); k++) {
                const mb_kernel K = mb_choose_kernel(plan_of(P.st, L[k]), c.w, c.h, true, true);
                if (K.sym >= 0) {
                    const mb_sym_shape& q = mb_sym_shapes[K.sym];
                    printf("%ssym<%d,%d,%d,%d,%d>/strip%d/lds%zu", k ? "," : "", q.ns, q.r[0], q.r[1], q.r[2], q.kind, K.strip, K.lds);
                } else printf("%splan/stages%d/strip%d/lds%zu", k ? "," : "", L[k].count, K.strip, K.lds);
            }
            printf("\n");
        }
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    return 0;
}
