// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the cut and join scores (csrc/ig_host_cutjoin.inc): a stand-alone
// program on the fake HIP runtime (fake_hip_runtime.cpp: device memory is the heap, so every copy, fill and model write is checked
// against the real allocation sizes).  The models below script what steers the host -- the entries of the pairs' rows, the work lists of
// the three sort forms, the heads -- with protocol-conforming values and touch the first and the last word of what the kernels write;
// the sums mean nothing here, memory safety, the sizes of the buffers on genomes of other shapes, the result's life, the host-only
// entries and every error path are the subject.  Built and run by tests/test_cut_join_sanitize.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "harness_common.h"
// mirrors of the device structs (ig_kernels_rows.cuh, ig_kernels_cutjoin.cuh: device code, not included here)
struct Item {
    long long off;
    int len, pad;
};
struct Long {
    long long off, scratch, len;
};
struct ZeroTab {
    const long long *hi, *lo;
    int pstar;
};
enum { PASSES = 12, LDS_PAIRS = 256 };

static long long g_entries = 0;  // entries the emit model makes
static bool g_contrib = false;   // the span model adds a contribution that closes between the first two slots (a first contig of two bins at least)
static bool g_open = false;      // the span model leaves a sum that does not close: a device error the host must catch
static bool g_bad_col = false;   // a pair names a contig out of range: caught too
static long g_spans = 0, g_joins_lds = 0, g_joins_atomic = 0, g_vk = 0;

static size_t g_free_bytes = (size_t)1 << 34;
extern "C" hipError_t hipMemGetInfo(size_t* free_bytes, size_t* total_bytes)
{
    *free_bytes = g_free_bytes;
    *total_bytes = (size_t)1 << 34;
    return hipSuccess;
}

static void model_span(void** a, dim3, dim3)
{
    u64* diff = *(u64**)a[8];
    const long long stride = *(long long*)a[9];
    for (int k = 0; k < 3; k++) { // every array's first and last words
        if (g_contrib) diff[k * stride + 1] += 5, diff[k * stride + 2] -= 5;
        diff[k * stride + stride - 1] += 0;
    }
    if (g_open) diff[stride - 1] += 1;
    g_spans++;
}
static void model_scan_apply(void** a, dim3 grid, dim3)
{
    const u64* in = *(const u64**)a[0];
    u64* out = *(u64**)a[1];
    const long long stride = *(long long*)a[2];
    const int n = *(int*)a[3];
    for (unsigned y = 0; y < grid.y; y++) {
        u64 run = 0;
        for (int i = 0; i < n; i++) out[y * stride + i] = run += in[y * stride + i];
    }
}
static void model_vk(void** a, dim3, dim3)
{
    const int n = *(int*)a[1];
    u64 *hi = *(u64**)a[2], *lo = *(u64**)a[3];
    for (int k = 0; k < n; k++) hi[k] = (u64)-1, lo[k] = (u64)k;
    g_vk++;
}
static void model_cut_zero(void** a, dim3, dim3)
{
    const int N = *(int*)a[2];
    const ZeroTab& zt = *(const ZeroTab*)a[8];
    long long* out = *(long long**)a[9];
    for (int f = 0; f < 2 * N; f++) out[f] = 3;
    if (zt.pstar < 2) {
        volatile long long x = zt.hi[0] + zt.lo[0];
        (void)x;
    }
}
static u64 row_of_entry(long long e, int K) { return (u64)(e % std::max(K - 1, 1)); }
static void model_count(void** a, dim3, dim3)
{
    u64 *counter = *(u64**)a[5], *sc = *(u64**)a[8];
    const int* kof = *(const int**)a[4];
    int K = 0;
    for (int f = 0; f < Fixture::N; f++) K = std::max(K, kof[f] + 1);
    if (K < 2) return;
    for (long long e = 0; e < g_entries; e++) counter[row_of_entry(e, K)]++;
    sc[0] += (u64)g_entries;
}
static void model_scatter(void** a, dim3, dim3)
{
    u64 *cursor = *(u64**)a[5], *ent = *(u64**)a[6];
    const u64 n_ent = *(u64*)a[7];
    const int* kof = *(const int**)a[4];
    int K = 0;
    for (int f = 0; f < Fixture::N; f++) K = std::max(K, kof[f] + 1);
    if (K < 2) return;
    for (long long e = 0; e < g_entries; e++) {
        const u64 lo = row_of_entry(e, K), slot = cursor[lo]++;
        const u64 hi = g_bad_col ? (u64)K : std::min<u64>(lo + 1 + (u64)(e % 3), (u64)K - 1);
        if (slot < n_ent) ent[slot] = (hi << 32) | 1ull;
    }
}
template <bool FILL>
static void model_classify(void** a, dim3, dim3)
{
    const u64* rowstart = *(const u64**)a[0];
    const int U = *(int*)a[1], short_max = *(int*)a[2], lds_max = *(int*)a[3];
    u64 *cls = *(u64**)a[4], *cur = *(u64**)a[5];
    int* short_rows = *(int**)a[6];
    Item *lds_items = *(Item**)a[7], *run_items = *(Item**)a[8];
    Long* long_rows = *(Long**)a[9];
    for (int r = 0; r < U; r++) {
        const u64 b = rowstart[r], len = rowstart[r + 1] - b;
        if (len < 2) continue;
        if (len <= (u64)short_max) {
            if (!FILL) cls[0]++, cls[1] += len;
            else short_rows[cur[0]++] = r;
        } else if (len <= (u64)lds_max) {
            if (!FILL) cls[2]++, cls[3] += len;
            else lds_items[cur[1]++] = Item{(long long)b, (int)len, 0};
        } else {
            const u64 run = (u64)lds_max, n_runs = run > 1 ? (len + run - 1) / run : 0;
            if (!FILL) {
                cls[4]++, cls[5] += len, cls[6] += n_runs;
                cls[7] = std::max(cls[7], len);
            } else {
                long_rows[cur[2]++] = Long{(long long)b, (long long)cur[3], (long long)len};
                cur[3] += len;
                for (u64 q = 0; q < n_runs; q++) run_items[cur[4]++] = Item{(long long)(b + q * run), (int)std::min(run, len - q * run), 0};
            }
        }
    }
}
static void model_sort_items(void** a, dim3 grid, dim3)
{
    const Item* items = *(const Item**)a[0];
    u64* ent = *(u64**)a[1];
    for (unsigned i = 0; i < grid.x; i++) std::sort(ent + items[i].off, ent + items[i].off + items[i].len);
}
static void model_sort_wave(void** a, dim3, dim3)
{
    const int* rows = *(const int**)a[0];
    const int n_rows = *(int*)a[1];
    const u64* rowstart = *(const u64**)a[2];
    u64* ent = *(u64**)a[3];
    for (int i = 0; i < n_rows; i++) std::sort(ent + rowstart[rows[i]], ent + rowstart[rows[i] + 1]);
}
static void model_merge(void** a, dim3 grid, dim3)
{
    const Long* rows = *(const Long**)a[0];
    u64 *ent = *(u64**)a[1], *scratch = *(u64**)a[2];
    const int to_scratch = *(int*)a[4];
    for (unsigned i = 0; i < grid.x; i++)
        for (long long e = 0; e < rows[i].len; e++)
            (to_scratch ? scratch[rows[i].scratch + e] : ent[rows[i].off + e]) = to_scratch ? ent[rows[i].off + e] : scratch[rows[i].scratch + e];
}
static void model_head_totals(void** a, dim3 grid, dim3)
{
    const long long n = *(long long*)a[2];
    u64 *totals = *(u64**)a[3], *n_heads = *(u64**)a[4];
    for (unsigned b = 0; b < grid.x; b++) totals[b] = (u64)std::min<long long>(2048, n - 2048ll * b); // every entry is a head
    *n_heads += (u64)n;
}
static void model_reduce(void** a, dim3, dim3)
{
    const u64* ent = *(const u64**)a[0];
    const long long n = *(long long*)a[2];
    const u64* rowstart = *(const u64**)a[4];
    const int U = *(int*)a[5];
    const u64 n_out = *(u64*)a[6];
    int* out_col = *(int**)a[7];
    u64 *out_cnt = *(u64**)a[8], *row_heads = *(u64**)a[9];
    int row = 0;
    for (long long e = 0; e < n && (u64)e < n_out; e++) {
        while (row + 1 < U && rowstart[row + 1] <= (u64)e) row++;
        out_col[e] = (int)(ent[e] >> 32);
        out_cnt[e] += ent[e] & 0xffffffffull;
        row_heads[row]++;
    }
}
template <bool LDS>
static void model_join(void** a, dim3, dim3)
{
    const u64* rowptr = *(const u64**)a[5];
    const int* col = *(const int**)a[6];
    const long long n_pairs = *(int*)a[7], p0 = *(int*)a[8];
    long long* acc = *(long long**)a[13];
    volatile u64 r = rowptr[0];
    volatile int c = col[n_pairs - 1];
    (void)r, (void)c;
    if (LDS) {
        for (long long p = p0; p < std::min<long long>(p0 + LDS_PAIRS, n_pairs); p++) acc[8 * p] += 1, acc[8 * p + 7] += 2;
        g_joins_lds++;
    } else {
        for (long long p = 0; p < n_pairs; p++) acc[8 * p] += 1, acc[8 * p + 7] += 2;
        g_joins_atomic++;
    }
}
static void model_contig_zero(void** a, dim3, dim3)
{
    const int* csl = *(const int**)a[0];
    const int K = *(int*)a[1];
    long long* gc = *(long long**)a[6];
    volatile int x = csl[0] + csl[K - 1];
    (void)x;
    gc[0] = gc[2 * K - 1] = 1;
}
static void model_join_zero(void** a, dim3, dim3)
{
    const long long n_pairs = *(long long*)a[2];
    const int K = *(int*)a[4];
    const long long* gc = *(const long long**)a[5];
    long long* zacc = *(long long**)a[10];
    volatile long long x = gc[2 * K - 1];
    (void)x;
    for (long long p = 0; p < n_pairs; p++) zacc[2 * p] = 4, zacc[2 * p + 1] = 6;
}

// a state of N bins in contigs of `per` bins (the last one shorter), two sub-fragments and 2 000 bp per bin; ring: the first contig is one
static std::vector<int32_t> state_of(int per, bool ring)
{
    const int N = Fixture::N;
    std::vector<int32_t> soa((size_t)17 * N, 0);
    for (int f = 0; f < N; f++) {
        const int c = f / per, p = f % per, L = std::min(per, N - c * per);
        const int v[17] = {p, 2 * p, 100 - c, 2000 * p, 2000, 2, ring && c == 0, f, p ? f - 1 : -1, p < L - 1 ? f + 1 : -1, L, 2 * L, 2000 * L, 1, 0, 1, f};
        for (int k = 0; k < 17; k++) soa[(size_t)k * N + f] = v[k];
    }
    return soa;
}

struct Cuts {
    std::vector<int32_t> valid;
    std::vector<int64_t> contacts, limbs;
    std::vector<double> delta;
    Cuts() { reset(); }
    void reset()
    {
        valid.assign(Fixture::N, -7);
        contacts.assign(Fixture::N, -7);
        limbs.assign(5 * Fixture::N, -7);
        delta.assign(Fixture::N, -7.0);
    }
    bool untouched() const
    {
        for (auto v : valid) if (v != -7) return false;
        for (auto v : limbs) if (v != -7) return false;
        return true;
    }
    int run(ig_ctx* c) { return reset(), ig_cut_scores(c, valid.data(), contacts.data(), limbs.data(), delta.data()); }
};

static int build_and_fetch(ig_ctx* c, long long want_contigs, long long want_pairs)
{
    int64_t K = -7, P = -7;
    CHECK(ig_join_scores_build(c, &K, &P) == 0 && K == want_contigs && P == want_pairs);
    std::vector<int32_t> head((size_t)K + 1, -7), tail((size_t)K + 1, -7), nsub((size_t)K + 1, -7), lbp((size_t)K + 1, -7), col((size_t)P + 1, -7);
    std::vector<int64_t> rowptr((size_t)K + 2, -7), contacts((size_t)P + 1, -7), nz(8 * (size_t)P + 1, -7), z(2 * (size_t)P + 1, -7), dni((size_t)P + 1, -7);
    std::vector<double> delta(4 * (size_t)P + 1, -7.0);
    CHECK(ig_join_scores_fetch(c, head.data(), tail.data(), nsub.data(), lbp.data(), nullptr, col.data(), contacts.data(), nz.data(), z.data(), dni.data(), delta.data()) != 0);
    CHECK(ig_join_scores_fetch(c, head.data(), tail.data(), nsub.data(), lbp.data(), rowptr.data(), col.data(), contacts.data(), nz.data(), z.data(), dni.data(), delta.data()) == 0);
    CHECK(rowptr[0] == 0 && rowptr[(size_t)K] == P && rowptr[(size_t)K + 1] == -7 && head[(size_t)K] == -7 && nz[8 * (size_t)P] == -7 && delta[4 * (size_t)P] == -7.0);
    for (int64_t k = 0; k < K; k++) CHECK(head[(size_t)k] >= 0 && tail[(size_t)k] >= 0 && nsub[(size_t)k] > 0 && lbp[(size_t)k] == 1000 * nsub[(size_t)k]);
    for (int64_t p = 0; p < P; p++) CHECK(nz[8 * (size_t)p] == 1 && nz[8 * (size_t)p + 7] == 2 && z[2 * (size_t)p] == 4 && dni[(size_t)p] > 0 && col[(size_t)p] < K);
    int64_t forms[8];
    CHECK(ig_debug_join_scores_forms(c, forms) == 0);
    return 0;
}

int main()
{
    fake_hip::set_model("k_cut_span", model_span);
    fake_hip::set_model("k_scan64_apply", model_scan_apply);
    fake_hip::set_model("k_cj_vk", model_vk);
    fake_hip::set_model("k_cut_zero", model_cut_zero);
    fake_hip::set_model("k_cj_pairs_emitILb0E", model_count);
    fake_hip::set_model("k_cj_pairs_emitILb1E", model_scatter);
    fake_hip::set_model("k_lift_classifyILb0E", model_classify<false>);
    fake_hip::set_model("k_lift_classifyILb1E", model_classify<true>);
    fake_hip::set_model("k_lift_sort_lds", model_sort_items);
    fake_hip::set_model("k_lift_sort_wave", model_sort_wave);
    fake_hip::set_model("k_lift_merge", model_merge);
    fake_hip::set_model("k_lift_head_totals", model_head_totals);
    fake_hip::set_model("k_lift_reduce", model_reduce);
    fake_hip::set_model("k_cj_joinILb1E", model_join<true>);
    fake_hip::set_model("k_cj_joinILb0E", model_join<false>);
    fake_hip::set_model("k_cj_contig_zero", model_contig_zero);
    fake_hip::set_model("k_cj_join_zero", model_join_zero);

    const Fixture fx;
    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    Cuts cuts;
    int64_t K = -7, P = -7;
    int32_t i32[4];
    int64_t i64[16];
    double f64[4];
    CHECK(ig_join_scores_fetch(c, i32, i32, i32, i32, i64, i32, i64, i64, i64, i64, f64) != 0 && std::strstr(ig_last_error(), "nothing is built"));
    CHECK(ig_join_scores_release(c) == 0 && ig_debug_join_scores_forms(c, i64) != 0);
    if (bring_up_ladder(fx, c, [&](bool) { return cuts.run(c); }, [&] { return cuts.untouched(); }, true, PARAMS_ALWAYS)) return 1;
    if (fx.fresh(c)) return 1;
    ig_destroy(c);
    c = nullptr;
    CHECK(ig_create(0, &c) == 0);
    if (bring_up_ladder(fx, c, [&](bool) { return K = P = -7, ig_join_scores_build(c, &K, &P); }, [&] { return K == -7 && P == -7; }, true, PARAMS_ALWAYS)) return 1;
    CHECK(fx.params(c) == 0);

    // the arguments
    CHECK(ig_cut_scores(c, nullptr, cuts.contacts.data(), cuts.limbs.data(), cuts.delta.data()) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_cut_scores(c, cuts.valid.data(), cuts.contacts.data(), cuts.limbs.data(), nullptr) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_join_scores_build(c, nullptr, &P) != 0 && ig_join_scores_build(c, &K, nullptr) != 0);
    for (int bad : {-2, 2}) CHECK(ig_debug_cut_join_form(c, bad) != 0 && std::strstr(ig_last_error(), "form"));

    // the fixture's own state: one bin per contig -- no cut, 40 linear contigs
    g_entries = 0;
    CHECK(cuts.run(c) == 0 && g_spans == 1);
    for (int f = 0; f < Fixture::N; f++) CHECK(cuts.valid[f] == 0 && cuts.contacts[f] == 0 && cuts.limbs[5 * f] == 0 && cuts.delta[f] == 0.0);
    if (build_and_fetch(c, 40, 0)) return 1;

    // genomes of other shapes on the same handle: contigs of 2, 7 (the last one shorter), 40 bins; with and without a ring; entries none,
    // a few, thousands (rows of every sort form under lowered limits, pairs on both sides of the LDS window); both forms of the pass
    g_contrib = true; // (the first contig by id is the LAST one of these states: two bins at least)
    for (int per : {2, 7, 40}) {
        for (int ring = 0; ring < 2; ring++) {
            const std::vector<int32_t> soa = state_of(per, ring != 0);
            CHECK(ig_upload_state(c, soa.data(), Fixture::N) == 0);
            const int contigs = (Fixture::N + per - 1) / per, K_lin = contigs - ring;
            CHECK(cuts.run(c) == 0);
            for (int f = 0; f < Fixture::N; f++) {
                const bool ok = f % per != 0 && !(ring && f < per);
                CHECK(cuts.valid[f] == ok && cuts.limbs[5 * f + 2] == (ok ? 3 : 0) && cuts.limbs[5 * f + 4] == (ok ? -(long long)(2 * (f % per)) * (2 * (std::min(per, Fixture::N - f / per * per) - f % per)) : 0));
            }
            for (long long entries : {0ll, 50ll, 3000ll}) {
                g_entries = K_lin >= 2 ? std::min<long long>(entries, fx.Z) : 0;
                for (int limits = 0; limits < 2; limits++) {
                    CHECK(ig_debug_assembly_contacts_limits(c, limits ? 2 : 0, limits ? 4 : 0) == 0);
                    for (int form = -1; form < 2; form++) {
                        CHECK(ig_debug_cut_join_form(c, form) == 0);
                        const long lds = g_joins_lds, atomic = g_joins_atomic;
                        if (build_and_fetch(c, K_lin, g_entries)) return 1;
                        if (g_entries) {
                            const bool want_lds = form < 0 ? g_entries <= LDS_PAIRS : form == 0;
                            CHECK(g_joins_lds - lds == (want_lds ? (g_entries + LDS_PAIRS - 1) / LDS_PAIRS : 0) && g_joins_atomic - atomic == (want_lds ? 0 : 1));
                        }
                    }
                }
            }
        }
    }
    CHECK(ig_debug_assembly_contacts_limits(c, 0, 0) == 0 && ig_debug_cut_join_form(c, -1) == 0);
    // a d_max below the contigs' lengths: the prefix table of the zero-pixel terms is built
    {
        float p8[8];
        std::memcpy(p8, fx.p8, sizeof p8);
        p8[5] = 1.0f;
        const long before = g_vk;
        const std::vector<int32_t> one = state_of(40, false);
        CHECK(ig_upload_state(c, one.data(), Fixture::N) == 0);
        CHECK(ig_set_params(c, p8, 1.8f, 0) == 0 && cuts.run(c) == 0 && g_vk == before + 1);
        g_entries = 50;
        if (build_and_fetch(c, 1, 0)) return 1;
        const std::vector<int32_t> soa = state_of(7, false);
        CHECK(ig_upload_state(c, soa.data(), Fixture::N) == 0);
        if (build_and_fetch(c, 6, 50)) return 1;
        CHECK(g_vk == before + 2 && fx.params(c) == 0);
    }
    // device errors the host must catch: a sum that does not close, more entries than contacts, a pair that names no contig
    g_open = true;
    CHECK(cuts.run(c) != 0 && std::strstr(ig_last_error(), "do not close"));
    g_open = false;
    g_entries = fx.Z + 1;
    CHECK(ig_join_scores_build(c, &K, &P) != 0 && std::strstr(ig_last_error(), "device error"));
    CHECK(ig_join_scores_fetch(c, i32, i32, i32, i32, i64, i32, i64, i64, i64, i64, f64) != 0 && std::strstr(ig_last_error(), "nothing is built"));
    g_entries = 50;
    g_bad_col = true;
    CHECK(ig_join_scores_build(c, &K, &P) != 0 && std::strstr(ig_last_error(), "names contig"));
    g_bad_col = false;
    g_free_bytes = 4096; // the entries do not fit what is free: refused with the bytes named
    CHECK(ig_join_scores_build(c, &K, &P) != 0 && std::strstr(ig_last_error(), "bytes of device memory"));
    g_free_bytes = (size_t)1 << 34;
    if (build_and_fetch(c, 6, 50)) return 1;
    // an inconsistent state is refused before anything is launched
    {
        std::vector<int32_t> soa = state_of(7, false);
        soa[(size_t)0 * Fixture::N + 3] = 2; // two bins at one place
        CHECK(ig_upload_state(c, soa.data(), Fixture::N) == 0);
        const long before = fake_hip::launches();
        CHECK(cuts.run(c) != 0 && std::strstr(ig_last_error(), "inconsistent state"));
        CHECK(ig_join_scores_build(c, &K, &P) != 0 && std::strstr(ig_last_error(), "inconsistent state"));
        (void)before;
        soa = state_of(7, false);
        CHECK(ig_upload_state(c, soa.data(), Fixture::N) == 0);
    }
    // the refusals of a handle that cannot answer: a step or a chain in flight, a shard
    c->nuis_in_flight = true;
    CHECK(cuts.run(c) != 0 && std::strstr(ig_last_error(), "nuisance step") && cuts.untouched());
    CHECK(ig_join_scores_build(c, &K, &P) != 0 && std::strstr(ig_last_error(), "nuisance step"));
    c->nuis_in_flight = false;
    c->chain_busy = true;
    CHECK(cuts.run(c) != 0 && std::strstr(ig_last_error(), "chain") && cuts.untouched());
    c->chain_busy = false;
    CHECK(ig_upload_contacts(c, fx.row.data(), fx.col.data(), fx.cnt.data(), fx.Z, Fixture::M, 1, 2) == 0);
    CHECK(cuts.run(c) != 0 && std::strstr(ig_last_error(), "shard 1 of 2") && cuts.untouched());
    CHECK(ig_join_scores_build(c, &K, &P) != 0 && std::strstr(ig_last_error(), "shard"));
    CHECK(fx.contacts(c) == 0 && cuts.run(c) == 0);

    // every allocation of a call fails once: an error, nothing leaked, no stale result, and the next call works
    g_entries = 300;
    for (int n = 0; n < 48; n++) {
        if (n % 6 == 0) {
            if (fx.fresh(c)) return 1;
            const std::vector<int32_t> soa = state_of(7, false);
            CHECK(ig_upload_state(c, soa.data(), Fixture::N) == 0);
        }
        fake_hip::fail_allocation_in(n % 24);
        const int rc = n & 1 ? cuts.run(c) : ig_join_scores_build(c, &K, &P);
        fake_hip::fail_allocation_in(-1);
        if (rc) CHECK(std::strstr(ig_last_error(), "hipMalloc"));
        if (rc && !(n & 1)) CHECK(ig_join_scores_fetch(c, i32, i32, i32, i32, i64, i32, i64, i64, i64, i64, f64) != 0);
        CHECK(cuts.run(c) == 0 && cuts.valid[1] == 1);
        if (build_and_fetch(c, 6, 300)) return 1;
    }
    // the time entry point
    std::vector<float> ms(2 * PASSES);
    int64_t ck = 0, ck2 = 0;
    CHECK(ig_debug_cut_join_time(c, 0, 2, ms.data(), &ck) == 0 && ck != 0);
    CHECK(ig_debug_cut_join_time(c, 1, 2, ms.data(), &ck) == 0 && ck != 0);
    CHECK(ig_debug_cut_join_form(c, 1) == 0 && ig_debug_cut_join_time(c, 1, 1, ms.data(), &ck2) == 0 && ck2 == ck);
    CHECK(ig_debug_cut_join_time(c, 2, 1, ms.data(), &ck) != 0 && ig_debug_cut_join_time(c, 0, 0, ms.data(), &ck) != 0 && ig_debug_cut_join_time(c, 0, 1, nullptr, &ck) != 0);
    // the host-only entries: no handle
    {
        const float s[4] = {0.0f, 1.5f, 300.0f, 2.0f};
        const int32_t d[4] = {0, 1, 170, 5000}, tr[4] = {0, 0, 0, 1}, cnt[4] = {1, 3, 0, 2000}, pos[3] = {1, 5, 400}, len[3] = {2, 9, 500};
        int64_t q[4] = {0, 0, 0, 0}, q2[4] = {0, 0, 0, 0};
        CHECK(ig_contact_terms_host(fx.p8, 1.8f, s, d, tr, cnt, 4, q) == 0 && q[1] != 0 && q[3] != 0 && q[1] != q[3]);
        CHECK(ig_contact_terms_host(fx.p8, 1.8f, s + 3, d, tr + 3, cnt + 3, 1, q2) == 0 && q2[0] == q[3]); // a trans pair: s and d play no part
        CHECK(ig_contact_terms_host(fx.p8, 1.8f, s, d, tr, cnt, 0, nullptr) == 0 && ig_contact_terms_host(nullptr, 1.8f, s, d, tr, cnt, 4, q) != 0);
        CHECK(ig_contact_terms_host(fx.p8, 1.8f, s, d, tr, cnt, 4, nullptr) != 0 && ig_contact_terms_host(fx.p8, 1.8f, s, d, tr, cnt, -1, q) != 0);
        CHECK(ig_zero_terms_host(fx.p8, 1.8f, pos, len, 3, q) == 0 && q[0] < 0 && q[1] < 0 && q[2] < 0);
        CHECK(ig_zero_terms_host(fx.p8, 1.8f, pos, len, 0, nullptr) == 0 && ig_zero_terms_host(fx.p8, 1.8f, nullptr, len, 3, q) != 0);
    }
    // a live result and a failed call right in front of ig_destroy: whatever they left is freed there (LeakSanitizer looks at the exit)
    if (build_and_fetch(c, 6, 300)) return 1;
    (void)failed_call_before_destroy(c, 9, [&] { return ig_join_scores_build(c, &K, &P); });
    std::printf("cutjoin harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
