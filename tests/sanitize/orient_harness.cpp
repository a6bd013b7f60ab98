// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the orientation support (csrc/ig_host_orient.inc): a
// stand-alone program on the fake HIP runtime (fake_hip_runtime.cpp: device memory is the heap, so every copy, fill and model write is
// checked against the real allocation sizes).  The models below script what steers the host -- the error word of a malformed list,
// the number of segments listed for the workgroup form, the largest model value -- with protocol-conforming values and touch the first
// and the last word of what the kernels write; the sums mean nothing here, memory safety, the sizes of the buffers, their growth, their
// life and every error path are the subject.  Built and run by tests/test_orientation_support_sanitize.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "harness_common.h"
enum { N_OBS = 7, CTL_ERR = 0, CTL_LARGE = 1 }; // ig_kernels_orient.cuh: device code, not included here

static int g_n_seg = 0;          // what the last k_orient_segments saw: the other kernels size their writes by it, as the real ones do by seg[] and the lists
static int g_T = 0;
static int g_large_every = 0;    // every n-th segment is listed for the workgroup form (0: none)
static int g_bogus_large = 0;    // the count the device reports on top: a device error the host must catch
static u64 g_maxq = 1;           // what the model pass reports as the largest |q|
static long g_wave = 0, g_group = 0, g_observed[2] = {0, 0}; // what ran

static void model_segments(void** a, dim3, dim3)
{
    const int *first = *(const int**)a[0], *last = *(const int**)a[1];
    const int n_seg = *(int*)a[2], T = *(int*)a[4], window = *(int*)a[5];
    int4 *geo = *(int4**)a[7], *bnd = *(int4**)a[8];
    int *large = *(int**)a[9], *ctl = *(int**)a[10];
    g_n_seg = n_seg;
    for (int k = 0; k < n_seg; k++) {
        int err = 0;
        if (first[k] < 0 || last[k] < first[k] || last[k] >= T) err |= 1;
        if (k > 0 && first[k] <= last[k - 1]) err |= 2;
        if (!err && first[k] / 10 != last[k] / 10) err |= 4; // (as if the contigs held ten positions)
        const int arm = std::min((last[k] - first[k] + 1) / 2, window);
        geo[k] = make_int4(err || arm == 0 ? 1 : 0, arm, 1, 1);
        bnd[k] = make_int4(first[k], last[k], err ? 0 : arm, 0);
        if (!err && arm > 0 && g_large_every && k % g_large_every == 0) large[ctl[CTL_LARGE]++] = k;
        ctl[CTL_ERR] |= err;
    }
    ctl[CTL_LARGE] += g_bogus_large;
}
static void model_paint(void** a, dim3, dim3)
{
    const int n_seg = *(int*)a[2], T = *(int*)a[3];
    int* seg = *(int**)a[4];
    g_T = T;
    for (int r = 0; r < T; r++) seg[r] = n_seg ? r % n_seg : -1;
}
template <int COMBINE>
static void model_observed(void** a, dim3, dim3)
{
    const int* seg = *(const int**)a[4];
    const int4* bnd = *(const int4**)a[5];
    u64 *obs = *(u64**)a[7], *sc = *(u64**)a[8];
    volatile int s = g_T ? seg[g_T - 1] : 0;
    (void)s;
    if (g_n_seg) {
        volatile int b = bnd[g_n_seg - 1].x;
        (void)b;
        obs[0] += 1;
        obs[4 * (size_t)g_n_seg - 1] += 1;
    }
    for (int k = 0; k < N_OBS; k++) sc[k] += (u64)(k + 1);
    g_observed[COMBINE]++;
}
template <int G>
static void model_model(void** a, dim3 grid, dim3)
{
    const int* list = *(const int**)a[3];
    const int n_items = *(int*)a[4];
    u64 *expq = *(u64**)a[7], *maxq = *(u64**)a[8];
    if (G == 256 && (int)grid.x != n_items) std::abort(); // (a workgroup per listed segment)
    for (int i = 0; i < n_items; i++) {
        const int s = list ? list[i] : i;
        expq[2 * (size_t)s] = 7;
        expq[2 * (size_t)s + 1] = 5;
    }
    *maxq = std::max(*maxq, g_maxq);
    (G == 64 ? g_wave : g_group)++;
}

struct Out {
    std::vector<int32_t> geo;
    std::vector<int64_t> obs, exq;
    int64_t sc[8];
    int32_t n_placed;
    void reset(int n_seg)
    {
        geo.assign(4 * (size_t)std::max(n_seg, 1), -7);
        obs.assign(4 * (size_t)std::max(n_seg, 1), -7);
        exq.assign(2 * (size_t)std::max(n_seg, 1), -7);
        for (auto& v : sc) v = -7;
        n_placed = -7;
    }
    bool untouched() const
    {
        for (auto v : geo) if (v != -7) return false;
        for (auto v : obs) if (v != -7) return false;
        for (auto v : exq) if (v != -7) return false;
        for (auto v : sc) if (v != -7) return false;
        return n_placed == -7;
    }
};
static int run(ig_ctx* c, int window, int model, const std::vector<int32_t>& first, const std::vector<int32_t>& last, Out& o)
{
    const int n_seg = (int)first.size();
    o.reset(n_seg);
    return ig_orientation_support(c, window, model, n_seg, first.data(), last.data(), o.geo.data(), o.obs.data(), o.exq.data(), o.sc, &o.n_placed);
}
static void pairs_of(int n_seg, std::vector<int32_t>& first, std::vector<int32_t>& last)
{
    first.clear(), last.clear();
    for (int k = 0; k < n_seg; k++) first.push_back(2 * k), last.push_back(2 * k + 1);
}

int main()
{
    fake_hip::set_model("k_orient_segments", model_segments);
    fake_hip::set_model("k_orient_paint", model_paint);
    fake_hip::set_model("k_orient_observedILb0E", model_observed<0>);
    fake_hip::set_model("k_orient_observedILb1E", model_observed<1>);
    fake_hip::set_model("k_orient_modelILi64E", model_model<64>);
    fake_hip::set_model("k_orient_modelILi256E", model_model<256>);

    const Fixture fx;

    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    Out o;
    std::vector<int32_t> first, last;
    pairs_of(3, first, last);
    const auto untouched = [&] { return o.untouched(); };
    if (bring_up_ladder(fx, c, [&](bool model) { return run(c, 8, model, first, last, o); }, untouched, true, PARAMS_WITH_MODEL)) return 1;
    CHECK(run(c, 8, 0, first, last, o) == 0 && o.n_placed == 80 && o.exq[0] == -7); // (without the model no parameters are needed)
    CHECK(fx.params(c) == 0);

    // a window out of range
    for (int bad : {0, 1025, -3}) CHECK(run(c, bad, 1, first, last, o) != 0 && std::strstr(ig_last_error(), "window") && o.untouched());
    // NULL outputs, NULL lists
    o.reset(3);
    CHECK(ig_orientation_support(c, 8, 1, 3, first.data(), last.data(), nullptr, o.obs.data(), o.exq.data(), o.sc, &o.n_placed) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_orientation_support(c, 8, 1, 3, first.data(), last.data(), o.geo.data(), nullptr, o.exq.data(), o.sc, &o.n_placed) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_orientation_support(c, 8, 1, 3, first.data(), last.data(), o.geo.data(), o.obs.data(), nullptr, o.sc, &o.n_placed) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_orientation_support(c, 8, 1, 3, first.data(), last.data(), o.geo.data(), o.obs.data(), o.exq.data(), nullptr, &o.n_placed) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_orientation_support(c, 8, 1, 3, first.data(), last.data(), o.geo.data(), o.obs.data(), o.exq.data(), o.sc, nullptr) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_orientation_support(c, 8, 1, 3, nullptr, last.data(), o.geo.data(), o.obs.data(), o.exq.data(), o.sc, &o.n_placed) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_orientation_support(c, 8, 1, 3, first.data(), nullptr, o.geo.data(), o.obs.data(), o.exq.data(), o.sc, &o.n_placed) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_orientation_support(c, 8, 1, -1, first.data(), last.data(), o.geo.data(), o.obs.data(), o.exq.data(), o.sc, &o.n_placed) != 0 && o.untouched());
    // model = 0 with a NULL expected_q
    CHECK(ig_orientation_support(c, 8, 0, 3, first.data(), last.data(), o.geo.data(), o.obs.data(), nullptr, o.sc, &o.n_placed) == 0);
    CHECK(o.n_placed == 80 && o.sc[7] == 3 && o.sc[0] == 1 && o.sc[6] == 7 && o.obs[0] == 1 && o.obs[11] == 1 && o.geo[1] == 1 && o.exq[0] == -7);
    // n_seg = 0: every pointer of the arrays may be NULL
    o.reset(0);
    CHECK(ig_orientation_support(c, 8, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, o.sc, &o.n_placed) == 0 && o.n_placed == 80 && o.sc[7] == 0);
    CHECK(run(c, 8, 1, {}, {}, o) == 0 && o.geo[0] == -7 && o.obs[0] == -7 && o.exq[0] == -7);
    // the malformed lists: the error word -> a loud failure, nothing written, the handle usable
    const std::vector<std::vector<int32_t>> bad_lists[] = {{{0, 2}, {2, 3}}, {{4, 0}, {5, 1}}, {{9}, {12}}, {{0}, {80}}, {{-1}, {1}}, {{3}, {2}}};
    for (const auto& b : bad_lists) {
        CHECK(run(c, 8, 1, b[0], b[1], o) != 0 && std::strstr(ig_last_error(), "ig_orientation_support: segment list") && o.untouched());
        CHECK(run(c, 8, 1, first, last, o) == 0 && o.sc[7] == 3);
    }
    pairs_of(41, first, last); // 82 > T positions named: out of range; and more segments than positions
    CHECK(run(c, 8, 1, first, last, o) != 0 && std::strstr(ig_last_error(), "segment list") && o.untouched());
    first.assign(81, 0), last.assign(81, 0);
    CHECK(run(c, 8, 1, first, last, o) != 0 && std::strstr(ig_last_error(), "segment list longer") && o.untouched());
    // buffer growth across two sizes, and back: the arrays of the longest list are kept
    for (int n_seg : {3, 40, 1, 40, 17}) {
        pairs_of(n_seg, first, last);
        for (int model = 0; model < 2; model++) {
            g_wave = g_group = 0;
            CHECK(run(c, 8, model, first, last, o) == 0 && o.n_placed == 80 && o.sc[7] == n_seg);
            CHECK(o.obs[0] == 1 && o.obs[4 * (size_t)n_seg - 1] == 1 && o.geo[4 * (size_t)n_seg - 3] == 1);
            CHECK(model ? (o.exq[0] == 7 && o.exq[2 * (size_t)n_seg - 1] == 5 && g_wave == 1 && g_group == 0) : (o.exq[0] == -7 && g_wave == 0));
        }
    }
    {
        pairs_of(17, first, last);
        const long before = fake_hip::allocations();
        CHECK(run(c, 8, 1, first, last, o) == 0);
        const long kept = fake_hip::allocations() - before;
        pairs_of(40, first, last);
        const long before2 = fake_hip::allocations();
        CHECK(run(c, 8, 1, first, last, o) == 0 && fake_hip::allocations() - before2 == kept); // (40 was seen: nothing of the feature's is allocated again)
    }
    // segments listed for the workgroup form; a count beyond the list is a device error
    g_large_every = 3;
    g_wave = g_group = 0;
    CHECK(run(c, 8, 1, first, last, o) == 0 && g_wave == 1 && g_group == 1 && o.exq[0] == 7);
    g_bogus_large = 100;
    CHECK(run(c, 8, 1, first, last, o) != 0 && std::strstr(ig_last_error(), "device error") && o.untouched());
    g_bogus_large = 0;
    g_large_every = 0;
    // the overflow guard: 2 w^2 max_q >= 2^62
    g_maxq = 1ull << 42; // times 2 * 1024^2 = 2^21: beyond 2^62
    CHECK(run(c, 1024, 1, first, last, o) != 0 && std::strstr(ig_last_error(), "model value too large for this window") && o.untouched());
    CHECK(run(c, 1, 1, first, last, o) == 0);    // (two pairs per class at most: nothing to overflow)
    CHECK(run(c, 1024, 0, first, last, o) == 0); // (without the model pass there is nothing to guard)
    g_maxq = (1ull << 41) - 1;
    CHECK(run(c, 1024, 1, first, last, o) == 0);
    g_maxq = 1;
    // every allocation of a call fails once: an error, nothing written, nothing leaked, and the next call works
    pairs_of(12, first, last);
    const auto model_call = [&] { return run(c, 8, 1, first, last, o); };
    if (allocation_failure_sweep(fx, c, 32, 24, 4, 4, model_call, untouched, [&] { return run(c, 8, 1, first, last, o) == 0 && o.sc[7] == (int64_t)first.size(); })) return 1;
    // the time entry point: both passes, every form
    std::vector<float> ms(3);
    int64_t ck = 0;
    pairs_of(40, first, last);
    g_observed[0] = g_observed[1] = g_wave = g_group = 0;
    for (int form = 0; form < 2; form++) CHECK(ig_debug_orientation_support_time(c, 8, 40, first.data(), last.data(), 0, form, 3, ms.data(), &ck) == 0 && ck != 0);
    CHECK(g_observed[0] == 3 && g_observed[1] == 3);
    for (int form = 0; form < 3; form++) CHECK(ig_debug_orientation_support_time(c, 8, 40, first.data(), last.data(), 1, form, 2, ms.data(), &ck) == 0 && ck != 0);
    CHECK(g_wave == 6 && g_group == 0);
    CHECK(ig_debug_orientation_support_time(c, 8, 40, first.data(), last.data(), 0, 0, 1, ms.data(), nullptr) == 0);
    CHECK(ig_debug_orientation_support_time(c, 8, 0, nullptr, nullptr, 1, 0, 1, ms.data(), &ck) == 0 && ck == 0);
    CHECK(ig_debug_orientation_support_time(c, 8, 40, first.data(), last.data(), 0, 0, 0, ms.data(), &ck) != 0);
    CHECK(ig_debug_orientation_support_time(c, 8, 40, first.data(), last.data(), 0, 0, 1, nullptr, &ck) != 0);
    CHECK(ig_debug_orientation_support_time(c, 8, 40, first.data(), last.data(), 2, 0, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "pass"));
    CHECK(ig_debug_orientation_support_time(c, 8, 40, first.data(), last.data(), 0, 2, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "form"));
    CHECK(ig_debug_orientation_support_time(c, 8, 40, first.data(), last.data(), 1, 3, 1, ms.data(), &ck) != 0);
    CHECK(ig_debug_orientation_support_time(c, 0, 40, first.data(), last.data(), 0, 0, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "window"));
    first[5] = 0;
    CHECK(ig_debug_orientation_support_time(c, 8, 40, first.data(), last.data(), 0, 0, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "segment list"));
    g_maxq = 1ull << 42;
    pairs_of(40, first, last);
    CHECK(ig_debug_orientation_support_time(c, 1024, 40, first.data(), last.data(), 1, 0, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "too large"));
    g_maxq = 1;
    // a failed call right in front of ig_destroy: whatever it left is freed there (LeakSanitizer looks at the exit)
    if (fx.fresh(c)) return 1;
    (void)failed_call_before_destroy(c, 12, model_call);
    std::printf("orient harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
