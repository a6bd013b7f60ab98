// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the gap support (csrc/ig_host_gap.inc): a stand-alone program
// on the fake HIP runtime (fake_hip_runtime.cpp: device memory is the heap, so every copy, fill and model write is checked against the
// real allocation sizes).  The models below script what steers the host -- the error word of a malformed list, the number of junctions
// listed for the workgroup form, the two largest values of the guards, the largest observed -- with protocol-conforming values and
// touch the first and the last word of what the kernels write; the sums mean nothing here, memory safety, the sizes of the buffers,
// their growth, their life and every error path are the subject.  Built and run by tests/test_gap_support_sanitize.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "harness_common.h"
enum { N_OBS = 6, DEV_MAXE = 6, DEV_MAXL = 7, CTL_ERR = 0, CTL_LARGE = 1 }; // ig_kernels_gap.cuh: device code, not included here

static int g_n_junc = 0, g_n_gaps = 0, g_T = 0; // what the last k_gap_junctions / k_gap_paint saw: the other kernels size their writes by them
static int g_large_every = 0;                   // every n-th junction is listed for the workgroup form (0: none)
static int g_bogus_large = 0;                   // the count the device reports on top: a device error the host must catch
static int g_bogus_bin = 0;                     // the bin the device reports for junction 0 on top of the real one
static u64 g_maxe = 1, g_maxl = 1, g_obs = 1;   // what the passes report: the largest |e_q|, the largest |l_q|, observed[0]
static long g_wave = 0, g_group = 0, g_observed = 0; // what ran

static void model_junctions(void** a, dim3, dim3)
{
    const int* junc = *(const int**)a[0];
    const int n_junc = *(int*)a[1], T = *(int*)a[6], window = *(int*)a[7], n_gaps = *(int*)a[8];
    int* status = *(int**)a[10];
    int4* geo = *(int4**)a[11];
    u64* pairs = *(u64**)a[12];
    int *large = *(int**)a[13], *ctl = *(int**)a[14];
    g_n_junc = n_junc, g_n_gaps = n_gaps;
    for (int k = 0; k < n_junc; k++) {
        int err = 0;
        if (junc[k] < 1 || junc[k] >= T) err |= 1;
        if (k > 0 && junc[k] <= junc[k - 1]) err |= 2;
        if (!err && junc[k] % 10 == 0) err |= 4; // (as if the contigs held ten positions)
        const int left = err ? 0 : std::min(window, junc[k] % 10), right = err ? 0 : std::min(window, 10 - junc[k] % 10);
        status[k] = 0;
        geo[k] = make_int4(err ? -1 : junc[k] / 2 + (k == 0 ? g_bogus_bin : 0), left, right, 0);
        pairs[k] = (u64)left * (u64)right;
        if (!err && g_large_every && k % g_large_every == 0) large[ctl[CTL_LARGE]++] = k;
        ctl[CTL_ERR] |= err;
    }
    ctl[CTL_LARGE] += g_bogus_large;
}
static void model_paint(void** a, dim3, dim3)
{
    const int n_junc = *(int*)a[1], T = *(int*)a[2];
    int* nj = *(int**)a[3];
    g_T = T;
    for (int r = 0; r < T; r++) nj[r] = std::min(r, n_junc);
}
static void model_observed(void** a, dim3, dim3)
{
    const int* nj = *(const int**)a[4];
    const float* gaps = *(const float**)a[5];
    const int n_gaps = *(int*)a[6];
    u64 *obs = *(u64**)a[9], *logq = *(u64**)a[10], *sc = *(u64**)a[11];
    volatile int n = g_T ? nj[g_T - 1] : 0;
    volatile float g = gaps[n_gaps - 1];
    (void)n, (void)g;
    if (n_gaps != g_n_gaps) std::abort();
    obs[0] += g_obs;
    obs[(size_t)g_n_junc - 1] += 1;
    logq[0] += 3;
    logq[(size_t)g_n_junc * n_gaps - 1] += 5;
    for (int k = 0; k < N_OBS; k++) sc[k] += (u64)(k + 1);
    sc[DEV_MAXL] = std::max(sc[DEV_MAXL], g_maxl);
    g_observed++;
}
template <int G>
static void model_model(void** a, dim3 grid, dim3)
{
    const int* list = *(const int**)a[5];
    const int n_items = *(int*)a[6], n_gaps = *(int*)a[8];
    u64 *expq = *(u64**)a[12], *maxq = *(u64**)a[13];
    if (G == 256 && (int)grid.x != n_items) std::abort(); // (a workgroup per listed junction)
    if (G == 64 && (int)grid.x != (n_items + 3) / 4) std::abort(); // (four waves, four junctions per workgroup)
    for (int i = 0; i < n_items; i++) {
        const int s = list ? list[i] : i;
        expq[(size_t)s * n_gaps] = 7;
        expq[(size_t)s * n_gaps + n_gaps - 1] = 5;
    }
    *maxq = std::max(*maxq, g_maxe);
    (G == 64 ? g_wave : g_group)++;
}

struct Out {
    std::vector<int32_t> st, geo;
    std::vector<int64_t> obs, prs, lgq, exq;
    int64_t sc[8];
    void reset(int n_junc, int n_gaps)
    {
        const size_t n = (size_t)std::max(n_junc, 1), w = n * (size_t)std::max(n_gaps, 1);
        st.assign(n, -7), geo.assign(4 * n, -7), obs.assign(n, -7), prs.assign(n, -7), lgq.assign(w, -7), exq.assign(w, -7);
        for (auto& v : sc) v = -7;
    }
    bool untouched() const
    {
        for (auto v : st) if (v != -7) return false;
        for (auto v : geo) if (v != -7) return false;
        for (auto v : obs) if (v != -7) return false;
        for (auto v : prs) if (v != -7) return false;
        for (auto v : lgq) if (v != -7) return false;
        for (auto v : exq) if (v != -7) return false;
        for (auto v : sc) if (v != -7) return false;
        return true;
    }
};
static int run(ig_ctx* c, int window, int model, const std::vector<int32_t>& junc, const std::vector<float>& gaps, Out& o)
{
    o.reset((int)junc.size(), (int)gaps.size());
    return ig_gap_support(c, window, model, (int)junc.size(), junc.data(), (int)gaps.size(), gaps.data(), o.st.data(), o.geo.data(), o.obs.data(), o.prs.data(),
                          o.lgq.data(), o.exq.data(), o.sc);
}
// n junctions, none on a multiple of ten: 1, 2, .., 9, 11, ..
static std::vector<int32_t> list_of(int n)
{
    std::vector<int32_t> j;
    for (int r = 1; (int)j.size() < n; r++)
        if (r % 10) j.push_back(r);
    return j;
}
static std::vector<float> grid_of(int n)
{
    std::vector<float> g;
    for (int k = 0; k < n; k++) g.push_back(1.5f * (float)k);
    return g;
}

int main()
{
    fake_hip::set_model("k_gap_junctions", model_junctions);
    fake_hip::set_model("k_gap_paint", model_paint);
    fake_hip::set_model("k_gap_observed", model_observed);
    fake_hip::set_model("k_gap_modelILi64E", model_model<64>);
    fake_hip::set_model("k_gap_modelILi256E", model_model<256>);

    const Fixture fx;
    const int N = Fixture::N;

    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    Out o;
    std::vector<int32_t> junc = list_of(3);
    std::vector<float> gaps = grid_of(4);
    const auto untouched = [&] { return o.untouched(); };
    // (log_q needs the model whatever `model` says)
    if (bring_up_ladder(fx, c, [&](bool model) { return run(c, 8, model, junc, gaps, o); }, untouched, true, PARAMS_ALWAYS)) return 1;
    CHECK(fx.params(c) == 0);
    CHECK(run(c, 8, 1, junc, gaps, o) == 0 && o.sc[7] == 80 && o.sc[6] == 3 && o.sc[0] == 1 && o.sc[5] == 6);
    CHECK(o.obs[0] == 1 && o.obs[2] == 1 && o.lgq[0] == 3 && o.lgq[11] == 5 && o.exq[0] == 7 && o.exq[11] == 5 && o.st[2] == 0 && o.prs[0] == 8);
    // (the canonical id of the bin's contig: junction 1 lies in bin 0, junctions 2 and 3 in bin 1, and every bin is a contig)
    CHECK(o.geo[0] >= 0 && o.geo[0] < N && o.geo[4] >= 0 && o.geo[4] < N && o.geo[4] != o.geo[0] && o.geo[8] == o.geo[4] && o.geo[1] == 1 && o.geo[2] == 8 && o.geo[3] == 0);

    // a window out of range; a grid out of range, not from 0, not ascending, not finite
    for (int bad : {0, 257, -3}) CHECK(run(c, bad, 1, junc, gaps, o) != 0 && std::strstr(ig_last_error(), "window") && o.untouched());
    for (int bad : {0, 1, 65}) CHECK(run(c, 8, 1, junc, grid_of(bad), o) != 0 && std::strstr(ig_last_error(), "n_gaps") && o.untouched());
    const std::vector<float> bad_grids[] = {{1.0f, 2.0f}, {0.0f, 2.0f, 2.0f}, {0.0f, 3.0f, 1.0f}, {0.0f, INFINITY}, {0.0f, NAN, 4.0f}, {0.0f, 1.0f, -INFINITY}};
    for (const auto& g : bad_grids) {
        CHECK(run(c, 8, 1, junc, g, o) != 0 && std::strstr(ig_last_error(), "ig_gap_support: gaps") && o.untouched());
        CHECK(run(c, 8, 1, junc, gaps, o) == 0 && o.sc[6] == 3);
    }
    // NULL outputs, NULL inputs, no junction
    o.reset(3, 4);
    int32_t *st = o.st.data(), *geo = o.geo.data();
    int64_t *obs = o.obs.data(), *prs = o.prs.data(), *lgq = o.lgq.data(), *exq = o.exq.data(), *sc = o.sc;
    CHECK(ig_gap_support(c, 8, 1, 3, junc.data(), 4, gaps.data(), nullptr, geo, obs, prs, lgq, exq, sc) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_gap_support(c, 8, 1, 3, junc.data(), 4, gaps.data(), st, nullptr, obs, prs, lgq, exq, sc) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_gap_support(c, 8, 1, 3, junc.data(), 4, gaps.data(), st, geo, nullptr, prs, lgq, exq, sc) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_gap_support(c, 8, 1, 3, junc.data(), 4, gaps.data(), st, geo, obs, nullptr, lgq, exq, sc) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_gap_support(c, 8, 1, 3, junc.data(), 4, gaps.data(), st, geo, obs, prs, nullptr, exq, sc) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_gap_support(c, 8, 1, 3, junc.data(), 4, gaps.data(), st, geo, obs, prs, lgq, nullptr, sc) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_gap_support(c, 8, 1, 3, junc.data(), 4, gaps.data(), st, geo, obs, prs, lgq, exq, nullptr) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_gap_support(c, 8, 1, 3, nullptr, 4, gaps.data(), st, geo, obs, prs, lgq, exq, sc) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_gap_support(c, 8, 1, 3, junc.data(), 4, nullptr, st, geo, obs, prs, lgq, exq, sc) != 0 && std::strstr(ig_last_error(), "NULL"));
    for (int bad : {0, -1}) CHECK(ig_gap_support(c, 8, 1, bad, junc.data(), 4, gaps.data(), st, geo, obs, prs, lgq, exq, sc) != 0 && std::strstr(ig_last_error(), "junction list"));
    CHECK(o.untouched());
    // model = 0 with a NULL expected_q
    g_wave = g_group = 0;
    CHECK(ig_gap_support(c, 8, 0, 3, junc.data(), 4, gaps.data(), st, geo, obs, prs, lgq, nullptr, sc) == 0);
    CHECK(o.sc[7] == 80 && o.sc[6] == 3 && o.obs[0] == 1 && o.lgq[11] == 5 && o.exq[0] == -7 && g_wave == 0 && g_group == 0);
    // the malformed lists: the error word -> a loud failure, nothing written, the handle usable
    const std::vector<int32_t> bad_lists[] = {{3, 3}, {5, 2}, {10}, {4, 20, 21}, {0}, {80}, {-1}, {1, 2, 99}};
    for (const auto& b : bad_lists) {
        CHECK(run(c, 8, 1, b, gaps, o) != 0 && std::strstr(ig_last_error(), "ig_gap_support: junction list malformed") && o.untouched());
        CHECK(run(c, 8, 1, junc, gaps, o) == 0 && o.sc[6] == 3);
    }
    CHECK(run(c, 8, 1, std::vector<int32_t>(81, 1), gaps, o) != 0 && std::strstr(ig_last_error(), "junction list longer") && o.untouched());
    // buffer growth over three calls of rising size -- in junctions, then in words --, and back: the arrays of the largest call are kept
    const int sizes[][2] = {{3, 4}, {20, 4}, {70, 2}, {70, 64}, {1, 64}, {40, 17}, {70, 64}};
    for (const auto& sz : sizes) {
        junc = list_of(sz[0]), gaps = grid_of(sz[1]);
        for (int model = 0; model < 2; model++) {
            g_wave = g_group = 0;
            CHECK(run(c, 8, model, junc, gaps, o) == 0 && o.sc[7] == 80 && o.sc[6] == sz[0]);
            const size_t words = (size_t)sz[0] * sz[1];
            CHECK(o.obs[0] == (sz[0] == 1 ? 2 : 1) && o.obs[(size_t)sz[0] - 1] >= 1 && o.lgq[words - 1] == (words == 1 ? 8 : 5) && o.geo[4 * (size_t)sz[0] - 1] == 0);
            CHECK(model ? (o.exq[0] == 7 && o.exq[words - 1] == 5 && g_wave == 1 && g_group == 0) : (o.exq[0] == -7 && g_wave == 0));
        }
    }
    {
        junc = list_of(17), gaps = grid_of(5);
        const long before = fake_hip::allocations();
        CHECK(run(c, 8, 1, junc, gaps, o) == 0);
        const long kept = fake_hip::allocations() - before;
        junc = list_of(70), gaps = grid_of(64);
        const long before2 = fake_hip::allocations();
        CHECK(run(c, 8, 1, junc, gaps, o) == 0 && fake_hip::allocations() - before2 == kept); // (70 x 64 was seen: nothing of the feature's is allocated again)
    }
    // junctions listed for the workgroup form; a count beyond the list, and a bin beyond the state, are device errors
    g_large_every = 3;
    g_wave = g_group = 0;
    CHECK(run(c, 8, 1, junc, gaps, o) == 0 && g_wave == 1 && g_group == 1 && o.exq[0] == 7);
    g_bogus_large = 100;
    CHECK(run(c, 8, 1, junc, gaps, o) != 0 && std::strstr(ig_last_error(), "device error") && o.untouched());
    g_bogus_large = 0;
    g_large_every = 0;
    g_bogus_bin = 1000;
    CHECK(run(c, 8, 1, junc, gaps, o) != 0 && std::strstr(ig_last_error(), "device error") && o.untouched());
    g_bogus_bin = 0;
    // the first guard: max |e_q| * w (w + 1) / 2 >= 2^62
    g_maxe = 1ull << 47; // times 256 * 257 / 2 = 32896 > 2^15: beyond 2^62
    CHECK(run(c, 256, 1, junc, gaps, o) != 0 && std::strstr(ig_last_error(), "model value too large for this window") && o.untouched());
    CHECK(run(c, 1, 1, junc, gaps, o) == 0);   // (one pair: nothing to overflow)
    CHECK(run(c, 256, 0, junc, gaps, o) == 0); // (without the model pass there is nothing to guard)
    g_maxe = ((1ull << 62) - 1) / 32896;
    CHECK(run(c, 256, 1, junc, gaps, o) == 0);
    g_maxe += 1;
    CHECK(run(c, 256, 1, junc, gaps, o) != 0 && std::strstr(ig_last_error(), "too large"));
    g_maxe = 1;
    // the second guard: max |l_q| * max observed >= 2^62
    g_maxl = 1ull << 52, g_obs = 1ull << 10;
    CHECK(run(c, 8, 1, junc, gaps, o) != 0 && std::strstr(ig_last_error(), "too many contacts across one junction for this model") && o.untouched());
    CHECK(run(c, 8, 0, junc, gaps, o) != 0 && std::strstr(ig_last_error(), "too many contacts") && o.untouched()); // (the observed pass runs whatever `model` says)
    g_obs = (1ull << 10) - 1;
    CHECK(run(c, 8, 1, junc, gaps, o) == 0 && o.obs[0] == (1 << 10) - 1);
    g_maxl = 1, g_obs = 1;
    CHECK(run(c, 8, 1, junc, gaps, o) == 0);
    // every allocation of a call fails once: an error, nothing written, nothing leaked, and the next call works
    junc = list_of(12), gaps = grid_of(6);
    const auto model_call = [&] { return run(c, 8, 1, junc, gaps, o); };
    if (allocation_failure_sweep(fx, c, 40, 24, 4, 4, model_call, untouched, [&] { return run(c, 8, 1, junc, gaps, o) == 0 && o.sc[6] == (int64_t)junc.size(); })) return 1;
    // the time entry point: every pass
    std::vector<float> ms(3);
    int64_t ck = 0;
    junc = list_of(40), gaps = grid_of(8);
    g_observed = g_wave = g_group = 0;
    CHECK(ig_debug_gap_support_time(c, 8, 40, junc.data(), 8, gaps.data(), 0, 3, ms.data(), &ck) == 0 && ck != 0 && g_observed == 3);
    for (int pass = 1; pass < 4; pass++) CHECK(ig_debug_gap_support_time(c, 8, 40, junc.data(), 8, gaps.data(), pass, 2, ms.data(), &ck) == 0 && ck != 0);
    CHECK(g_wave == 6 && g_group == 0 && g_observed == 3);
    CHECK(ig_debug_gap_support_time(c, 8, 40, junc.data(), 8, gaps.data(), 0, 1, ms.data(), nullptr) == 0);
    CHECK(ig_debug_gap_support_time(c, 8, 40, junc.data(), 8, gaps.data(), 0, 0, ms.data(), &ck) != 0);
    CHECK(ig_debug_gap_support_time(c, 8, 40, junc.data(), 8, gaps.data(), 0, 1, nullptr, &ck) != 0);
    CHECK(ig_debug_gap_support_time(c, 8, 40, junc.data(), 8, gaps.data(), 4, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "pass"));
    CHECK(ig_debug_gap_support_time(c, 8, 40, junc.data(), 8, gaps.data(), -1, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "pass"));
    CHECK(ig_debug_gap_support_time(c, 0, 40, junc.data(), 8, gaps.data(), 0, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "window"));
    CHECK(ig_debug_gap_support_time(c, 8, 40, junc.data(), 1, gaps.data(), 0, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "n_gaps"));
    CHECK(ig_debug_gap_support_time(c, 8, 0, junc.data(), 8, gaps.data(), 0, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "junction list"));
    junc[5] = 1;
    CHECK(ig_debug_gap_support_time(c, 8, 40, junc.data(), 8, gaps.data(), 0, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "junction list malformed"));
    junc = list_of(40);
    g_maxe = 1ull << 47;
    CHECK(ig_debug_gap_support_time(c, 256, 40, junc.data(), 8, gaps.data(), 1, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "too large"));
    g_maxe = 1;
    g_maxl = 1ull << 52, g_obs = 1ull << 10;
    CHECK(ig_debug_gap_support_time(c, 8, 40, junc.data(), 8, gaps.data(), 0, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "too many contacts"));
    g_maxl = 1, g_obs = 1;
    // the host-only model values: no context
    {
        const float s[5] = {0.0f, 1.0f, 100.0f, 250.0f, INFINITY};
        int64_t e[5], l[5];
        CHECK(ig_model_values_host(fx.p8, s, 5, e, l) == 0 && e[0] == e[3] && e[3] == e[4] && e[1] > e[2] && e[2] > e[3] && l[1] > l[2] && l[3] < 0);
        CHECK(ig_model_values_host(fx.p8, nullptr, 0, nullptr, nullptr) == 0);
        CHECK(ig_model_values_host(nullptr, s, 5, e, l) != 0 && ig_model_values_host(fx.p8, s, 5, nullptr, l) != 0 && ig_model_values_host(fx.p8, s, -1, e, l) != 0);
    }
    // a failed call right in front of ig_destroy: whatever it left is freed there (LeakSanitizer looks at the exit)
    if (fx.fresh(c)) return 1;
    (void)failed_call_before_destroy(c, 12, model_call);
    std::printf("gap harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
