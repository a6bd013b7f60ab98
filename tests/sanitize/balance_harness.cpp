// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the balancing (csrc/ig_host_bal.inc) with the sort and reduction
// it shares with the contacts in genome coordinates (csrc/ig_host_rows.inc): a stand-alone program on the fake HIP runtime
// (fake_hip_runtime.cpp: device memory is the heap, so every copy, fill and model write is checked against the real allocation sizes).
// The models below script what steers the host -- the units, the entries per row, the totals, the work lists of the three sort forms, the
// heads, and in the loop the marginals, the done flag and the variance of every iteration -- with protocol-conforming values; the sums mean
// nothing here, memory safety, the sizes of the buffers, the lifetimes of build / run / release, the grouped loop against the done flag
// and every error path are the subject.  Built and run by tests/test_balance_sanitize.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "harness_common.h"
// mirrors of the device structs (ig_kernels_rows.cuh, ig_kernels_bal.cuh: device code, not included here)
struct Item {
    long long off;
    int len, pad;
};
struct Long {
    long long off, scratch, len;
};
struct Ctl {
    double mean, k;
    int done, converged, n_iters, pad;
};
struct Rows {
    const u64* rowptr;
    const int* col;
    const u64* cnt;
    const double* b;
    const double* values;
};
enum { NS_KEPT = 3, NS_ENTRIES = 4 };

static int g_per_unit = 3;        // positions per modelled bin (level 1)
static long long g_entries = 0;   // entries the emit model makes
static u64 g_total0 = 0;          // added to the total of unit 0 (the 2^53 refusal)
static bool g_no_heads = false;   // the reduction finds no head: a device error the host must catch
static bool g_many_heads = false; // more units than positions: inconsistent tables
static bool g_zero_marg = false;  // every marginal is zero: k == 0, the rule stops without an iteration
static long g_marg_live = 0;      // launches of the marginals' model that found the done flag down (or were given none)
static long g_marg_idle = 0;      // ... that found it up

static size_t g_free_bytes = (size_t)1 << 34; // what the device reports free
// the fake runtime has no hipMemGetInfo (the library refers to it weakly): this program brings its own, so the check runs here
extern "C" hipError_t hipMemGetInfo(size_t* free_bytes, size_t* total_bytes)
{
    *free_bytes = g_free_bytes;
    *total_bytes = (size_t)1 << 34;
    return hipSuccess;
}

static u64 row_of_entry(long long e, int U) { return (u64)((e * 2654435761ll) % (long long)std::max(U - 2, 1)); }
// the variance the model reports for iteration `it`: halves every time, below 1e-5 from the 17th on
static double var_of(int it) { return std::ldexp(1.0, -(it + 1)); }

static void model_heads(void** a, dim3, dim3)
{
    const int T = *(int*)a[2];
    u64* head = *(u64**)a[3];
    for (int r = 0; r < T; r++) head[r] = g_many_heads ? 2 : r % g_per_unit == 0;
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
static void model_keys(void** a, dim3, dim3) // k_lift_keys: reads the pixel of every sub-fragment (and incl where given), writes every key
{
    const int* pix = *(const int**)a[0];
    const int M = *(int*)a[1], T = *(int*)a[2];
    const u64* incl = *(const u64**)a[3];
    int* key = *(int**)a[4];
    for (int s = 0; s < M; s++) key[s] = pix[s] + (incl && T > 0 ? (int)(incl[T - 1] & 0) : 0);
}
static void model_count(void** a, dim3, dim3)
{
    const int* key = *(const int**)a[3];
    const int U = *(int*)a[4];
    u64 *counter = *(u64**)a[6], *total = *(u64**)a[7], *sc = *(u64**)a[10];
    (void)key[0];
    for (long long e = 0; e < g_entries; e++) counter[row_of_entry(e, U)]++, total[row_of_entry(e, U)] += 1;
    if (U > 0) total[0] += g_total0;
    sc[NS_ENTRIES] += (u64)g_entries;
    sc[NS_KEPT] += (u64)g_entries / 2;
}
static void model_scatter(void** a, dim3, dim3)
{
    const int U = *(int*)a[4];
    u64 *cursor = *(u64**)a[6], *ent = *(u64**)a[8];
    const u64 n_ent = *(u64*)a[9];
    for (long long e = 0; e < g_entries; e++) {
        const u64 row = row_of_entry(e, U), slot = cursor[row]++;
        if (slot < n_ent) ent[slot] = ((u64)(e % std::max(U, 1)) << 32) | 1ull;
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
    if (g_no_heads) return;
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
// k_bal_marginals: honours the done flag; reads every row, every entry (or every value) and b at every column and row; writes every row
static void model_marginals(void** a, dim3, dim3)
{
    const Rows r = *(const Rows*)a[0];
    const long long n_rows = *(long long*)a[1], n_ent = *(long long*)a[2];
    const int* done = *(const int**)a[3];
    double* out = *(double**)a[4];
    if (done && *done) {
        g_marg_idle++;
        return;
    }
    g_marg_live++;
    for (long long row = 0; row < n_rows; row++) {
        double s = 0.0;
        for (u64 e = r.rowptr[row]; e < r.rowptr[row + 1] && e < (u64)n_ent; e++) s += r.values ? r.values[e] : (double)r.cnt[e] * r.b[r.col[e]];
        out[row] = r.values ? s : (g_zero_marg ? 0.0 : 1.0 + s * r.b[row]);
    }
}
static void model_mean(void** a, dim3, dim3)
{
    const double* marg = *(const double**)a[0];
    const long long n = *(long long*)a[1];
    Ctl* ctl = *(Ctl**)a[2];
    if (ctl->done) return;
    long long k = 0;
    for (long long i = 0; i < n; i++) k += marg[i] != 0.0;
    if (!k) {
        ctl->done = 1;
        return;
    }
    ctl->k = (double)k, ctl->mean = 1.0;
}
static void model_update(void** a, dim3, dim3)
{
    const double* marg = *(const double**)a[0];
    const long long n = *(long long*)a[1];
    const Ctl* ctl = *(const Ctl**)a[2];
    double *b = *(double**)a[3], *dd = *(double**)a[4];
    if (ctl->done) return;
    for (long long i = 0; i < n; i++) b[i] = b[i] * 0.5 + 0.25, dd[i] = marg[i] * 0.0;
}
static void model_var(void** a, dim3, dim3)
{
    const double* dd = *(const double**)a[0];
    const long long n = *(long long*)a[1];
    Ctl* ctl = *(Ctl**)a[2];
    const double tol = *(double*)a[3];
    const int max_iters = *(int*)a[4];
    double* variance = *(double**)a[5];
    if (ctl->done) return;
    double s = 0.0;
    for (long long i = 0; i < n; i++) s += dd[i];
    const int it = ctl->n_iters;
    const double var = var_of(it) + s;
    variance[it] = var; // (beyond max_iters: a heap overflow the sanitizer reports)
    ctl->n_iters = it + 1;
    if (var < tol) ctl->converged = ctl->done = 1;
    else if (it + 1 >= max_iters) ctl->done = 1;
}

struct Built {
    int64_t U = 0, E = 0, sc[8];
    std::vector<int64_t> rowptr, nnz, total;
};

static int build(ig_ctx* c, int level, int max_side, int d, Built& b)
{
    for (int k = 0; k < 8; k++) b.sc[k] = -7;
    if (ig_balance_build(c, level, max_side, d, &b.U, &b.E, b.sc)) return -1;
    b.rowptr.assign((size_t)b.U + 1, -7), b.nnz.assign((size_t)b.U, -7), b.total.assign((size_t)b.U, -7);
    return ig_balance_rows(c, b.rowptr.data(), b.nnz.data(), b.total.data(), b.U + 1);
}

// the run under (tol, max_iters): n_iters and converged as the scripted variances say, whatever the group; the marginals ran live once
// per iteration and once more, and idle for the rest of the last group
static int run_and_check(ig_ctx* c, const Built& b, double tol, int max_iters, int group)
{
    int want = max_iters, conv = 0;
    for (int it = 0; it < max_iters; it++)
        if (var_of(it) < tol) {
            want = it + 1, conv = 1;
            break;
        }
    const bool empty = b.sc[7] == 0;
    if (empty || g_zero_marg) want = 0, conv = 0;
    const size_t U = (size_t)b.U;
    std::vector<double> b0(U, 1.0), bb(U, -7.0), marg(U, -7.0), var((size_t)max_iters, -7.0);
    int32_t n = -7, cv = -7;
    const long live = g_marg_live, idle = g_marg_idle;
    CHECK(ig_debug_balance_group(c, group) == 0);
    CHECK(ig_balance_run(c, b0.data(), tol, max_iters, bb.data(), marg.data(), var.data(), &n, &cv) == 0);
    CHECK(n == want && cv == conv);
    for (int it = 0; it < max_iters; it++) CHECK(var[(size_t)it] == (it < want ? var_of(it) : 0.0));
    for (size_t u = 0; u < U; u++) CHECK(bb[u] != -7.0 && marg[u] != -7.0);
    if (empty) CHECK(g_marg_live == live && g_marg_idle == idle); // no launch over empty rows
    else if (g_zero_marg) CHECK(g_marg_live - live == 2);         // the first iteration's, which stops the rule, and the final one
    else {
        const int g = group > 0 ? group : 8;
        const int queued = std::min(max_iters, (want + g - 1) / g * g);
        CHECK(g_marg_live - live == want + 1 && g_marg_idle - idle == queued - want);
    }
    return 0;
}

int main()
{
    fake_hip::set_model("k_lift_heads", model_heads);
    fake_hip::set_model("k_scan64_apply", model_scan_apply);
    fake_hip::set_model("k_lift_keys", model_keys);
    fake_hip::set_model("k_bal_emitILb0E", model_count);
    fake_hip::set_model("k_bal_emitILb1E", model_scatter);
    fake_hip::set_model("k_lift_classifyILb0E", model_classify<false>);
    fake_hip::set_model("k_lift_classifyILb1E", model_classify<true>);
    fake_hip::set_model("k_lift_sort_lds", model_sort_items);
    fake_hip::set_model("k_lift_sort_wave", model_sort_wave);
    fake_hip::set_model("k_lift_merge", model_merge);
    fake_hip::set_model("k_lift_head_totals", model_head_totals);
    fake_hip::set_model("k_lift_reduce", model_reduce);
    fake_hip::set_model("k_bal_marginals", model_marginals);
    fake_hip::set_model("k_bal_mean", model_mean);
    fake_hip::set_model("k_bal_update", model_update);
    fake_hip::set_model("k_bal_var", model_var);

    const Fixture fx;
    const int M = Fixture::M;
    const int64_t Z = fx.Z;

    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    Built b;
    double one = 1.0, out1 = 0.0;
    int32_t n_it = -7, conv = -7;
    {
        if (bring_up_ladder(fx, c, [&](bool) { return build(c, 1, 2048, 2, b); }, [&] { return b.sc[0] == -7; }, true, PARAMS_NEVER)) return 1;
        for (int bad : {0, -1}) CHECK(build(c, 1, 2048, bad, b) != 0 && std::strstr(ig_last_error(), "ignore_diags") && b.sc[0] == -7);
        for (int bad : {-1, 3}) CHECK(build(c, bad, 2048, 2, b) != 0 && std::strstr(ig_last_error(), "level"));
        CHECK(build(c, 2, 0, 2, b) != 0 && std::strstr(ig_last_error(), "max_side"));
        CHECK(ig_balance_build(c, 1, 2048, 2, nullptr, &b.E, b.sc) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(ig_balance_run(c, &one, 1e-5, 10, &out1, &out1, &out1, &n_it, &conv) != 0 && std::strstr(ig_last_error(), "nothing is built") && n_it == -7);
        CHECK(ig_balance_fetch(c, 0, 0, nullptr, nullptr) != 0 && ig_balance_rows(c, b.sc, b.sc, b.sc, 8) != 0);
        CHECK(ig_debug_balance_form(c, 3) != 0 && ig_debug_balance_form(c, -1) != 0 && ig_debug_balance_group(c, -1) != 0);
        CHECK(ig_set_shard(c, 1, 2) == 0); // a sharded handle: refused before anything is allocated
        const long before = fake_hip::allocations();
        CHECK(build(c, 1, 2048, 2, b) != 0 && std::strstr(ig_last_error(), "all contacts on one handle") && fake_hip::allocations() == before);
        CHECK(ig_set_shard(c, 0, 1) == 0);
    }

    // every level; no entry, a few (rows of the short form), many (lds and long rows under lowered limits); both forms; the loop in groups
    for (int level = 0; level < 3; level++) {
        for (long long entries : {0ll, 50ll, (long long)(2 * Z)}) {
            g_entries = entries;
            for (int limits = 0; limits < 3; limits++) {
                CHECK(ig_debug_assembly_contacts_limits(c, limits == 0 ? 0 : limits == 1 ? 2 : 1, limits == 0 ? 0 : limits == 1 ? 4 : 1) == 0);
                CHECK(build(c, level, 16, 1 + limits, b) == 0);
                CHECK(b.U == (level == 0 ? M : level == 1 ? (M + g_per_unit - 1) / g_per_unit : 16) && b.sc[6] == b.U && b.sc[5] == M);
                CHECK(b.sc[NS_ENTRIES] == entries && b.sc[7] == b.E && b.E == entries && b.rowptr[(size_t)b.U] == b.E);
                int64_t nnz = 0, tot = 0;
                for (int64_t u = 0; u < b.U; u++) nnz += b.nnz[(size_t)u], tot += b.total[(size_t)u];
                CHECK(nnz == b.E && tot == entries);
                std::vector<int32_t> cols((size_t)b.E + 1, -7);
                std::vector<int64_t> counts((size_t)b.E + 1, -7);
                CHECK(ig_balance_fetch(c, 0, b.E, cols.data(), counts.data()) == 0 && cols[(size_t)b.E] == -7 && (b.E == 0 || counts[(size_t)b.E - 1] == 1));
                CHECK(ig_balance_fetch(c, 1, b.E, cols.data(), counts.data()) != 0 && ig_balance_rows(c, b.rowptr.data(), b.nnz.data(), b.total.data(), b.U) != 0);
                for (int form = 1; form <= 2; form++) {
                    CHECK(ig_debug_balance_form(c, form) == 0);
                    for (int group : {1, 7, 0}) {
                        if (run_and_check(c, b, 1e-5, 200, group)) return 1; // 17 iterations, converged
                        if (run_and_check(c, b, 0.0, 5, group)) return 1;    // five exactly
                        if (run_and_check(c, b, 1e-5, 9, group)) return 1;   // max_iters first
                    }
                }
            }
        }
    }
    CHECK(ig_debug_assembly_contacts_limits(c, 0, 0) == 0 && ig_debug_balance_form(c, 0) == 0 && ig_debug_balance_group(c, 0) == 0);
    g_entries = 300;
    CHECK(build(c, 1, 2048, 2, b) == 0);
    // every marginal zero: the rule stops in its first iteration; b0 zero everywhere: nothing is launched at all
    g_zero_marg = true;
    if (run_and_check(c, b, 1e-5, 200, 3)) return 1;
    g_zero_marg = false;
    {
        const size_t U = (size_t)b.U;
        std::vector<double> zero(U, 0.0), bb(U, -7.0), marg(U, -7.0), var(4, -7.0);
        const long launches = fake_hip::launches(), allocs = fake_hip::allocations();
        CHECK(ig_balance_run(c, zero.data(), 1e-5, 4, bb.data(), marg.data(), var.data(), &n_it, &conv) == 0 && n_it == 0 && conv == 0);
        CHECK(fake_hip::launches() == launches && fake_hip::allocations() == allocs && bb[0] == 0.0 && marg[U - 1] == 0.0 && var[3] == 0.0);
        // the run's refusals leave the outputs alone
        n_it = conv = -7;
        CHECK(ig_balance_run(c, zero.data(), -1.0, 4, bb.data(), marg.data(), var.data(), &n_it, &conv) != 0 && std::strstr(ig_last_error(), "tol"));
        CHECK(ig_balance_run(c, zero.data(), std::nan(""), 4, bb.data(), marg.data(), var.data(), &n_it, &conv) != 0 && std::strstr(ig_last_error(), "tol"));
        CHECK(ig_balance_run(c, zero.data(), 1e-5, 0, bb.data(), marg.data(), var.data(), &n_it, &conv) != 0 && std::strstr(ig_last_error(), "max_iters"));
        CHECK(ig_balance_run(c, zero.data(), 1e-5, 4, nullptr, marg.data(), var.data(), &n_it, &conv) != 0 && std::strstr(ig_last_error(), "NULL") && n_it == -7);
    }
    // the plausibility checks, before anything is sized by what the device reported
    g_entries = 2 * Z + 2; // more entries than two per contact
    CHECK(build(c, 1, 2048, 2, b) != 0 && std::strstr(ig_last_error(), "device error"));
    CHECK(ig_balance_run(c, &one, 1e-5, 10, &out1, &out1, &out1, &n_it, &conv) != 0 && std::strstr(ig_last_error(), "nothing is built")); // a failed build leaves no rows
    g_entries = 51; // an odd number of entries
    CHECK(build(c, 1, 2048, 2, b) != 0 && std::strstr(ig_last_error(), "device error"));
    g_entries = 300;
    g_many_heads = true; // more units than positions
    CHECK(build(c, 1, 2048, 2, b) != 0 && std::strstr(ig_last_error(), "inconsistent tables"));
    g_many_heads = false;
    g_no_heads = true; // no head among the entries: caught too
    CHECK(build(c, 1, 2048, 2, b) != 0 && std::strstr(ig_last_error(), "distinct"));
    g_no_heads = false;
    g_total0 = 1ull << 53; // a unit whose counts do not convert exactly
    CHECK(build(c, 1, 2048, 2, b) != 0 && std::strstr(ig_last_error(), "2^53"));
    g_total0 = (1ull << 53) - 400; // (just below, with the 300 entries' own)
    CHECK(build(c, 1, 2048, 2, b) == 0 && b.total[0] < (1ll << 53) && b.total[0] >= (1ll << 53) - 400);
    g_total0 = 0;
    g_free_bytes = 4096; // the entries do not fit what is free: refused with the bytes named, before anything is allocated by their number
    {
        const long before = fake_hip::allocations();
        CHECK(build(c, 1, 2048, 2, b) != 0 && std::strstr(ig_last_error(), "bytes of device memory"));
        CHECK(fake_hip::allocations() - before < 16);
    }
    g_free_bytes = (size_t)1 << 34;
    // every allocation of a build and of a run fails once: an error, nothing leaked, and the next call works
    {
        int turn = 0;
        const auto build_and_run = [&] {
            int rc = build(c, turn++ % 3, 16, 2, b);
            if (!rc) {
                std::vector<double> b0((size_t)b.U, 1.0), bb((size_t)b.U), marg((size_t)b.U), var(20);
                rc = ig_balance_run(c, b0.data(), 1e-5, 20, bb.data(), marg.data(), var.data(), &n_it, &conv);
            }
            return rc;
        };
        const auto nothing_to_keep = [] { return true; }; // (a run that fails comes behind a build that wrote its outputs)
        if (allocation_failure_sweep(fx, c, 56, 56, 0, 20, build_and_run, nothing_to_keep, [&] { return build(c, 1, 2048, 2, b) == 0 && run_and_check(c, b, 1e-5, 200, 7) == 0; }))
            return 1;
    }
    // the timed entry points and the ordered sum on caller data
    std::vector<float> ms(3 * 8);
    CHECK(ig_debug_balance_time(c, 0, 3, ms.data()) == 0 && ig_debug_balance_time(c, 1, 3, ms.data()) == 0);
    CHECK(ig_debug_balance_time(c, 2, 1, ms.data()) != 0 && ig_debug_balance_time(c, 0, 0, ms.data()) != 0);
    if (run_and_check(c, b, 1e-5, 200, 0)) return 1; // (the built rows are still there)
    CHECK(ig_debug_balance_build_time(c, 1, 2048, 2, 3, ms.data()) == 0 && ig_debug_balance_build_time(c, 1, 2048, 0, 1, ms.data()) != 0);
    {
        const double values[5] = {1.0, 2.0, 3.0, 4.0, 5.0};
        const int64_t good[4] = {0, 2, 2, 5}, down[4] = {0, 3, 2, 5}, late[2] = {1, 5};
        double sums[3] = {-7.0, -7.0, -7.0};
        CHECK(ig_debug_lane_sums(c, values, good, 3, sums) == 0 && sums[0] == 3.0 && sums[1] == 0.0 && sums[2] == 12.0);
        CHECK(ig_debug_lane_sums(c, values, down, 3, sums) != 0 && std::strstr(ig_last_error(), "decreases"));
        CHECK(ig_debug_lane_sums(c, values, late, 1, sums) != 0 && ig_debug_lane_sums(c, values, good, 0, sums) != 0 && ig_debug_lane_sums(c, nullptr, good, 3, sums) != 0);
    }
    // release: nothing stays; then ig_destroy behind a failed build and with rows still built
    CHECK(build(c, 1, 2048, 2, b) == 0 && ig_balance_release(c) == 0 && ig_balance_fetch(c, 0, 1, nullptr, nullptr) != 0);
    CHECK(ig_debug_balance_time(c, 0, 1, ms.data()) != 0 && std::strstr(ig_last_error(), "nothing is built"));
    fake_hip::fail_allocation_in(5);
    CHECK(build(c, 1, 2048, 2, b) != 0);
    fake_hip::fail_allocation_in(-1);
    CHECK(build(c, 0, 2048, 2, b) == 0);
    ig_destroy(c);
    std::printf("balance harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
