// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the balancing's rows from a built map
// (csrc/ig_host_balsnap.inc) with the counting sort and the sorts it takes from the row builder (csrc/ig_host_rows.inc) and the balancer
// it builds for (csrc/ig_host_bal.inc): a stand-alone program on the fake HIP runtime (fake_hip_runtime.cpp: device memory is the heap,
// so every copy, fill and model write is checked against the real allocation sizes).  The two kernels of the build have word-for-word
// models below -- what they read, what they write and where, a thread at a time -- so the rows that come out are the rule's and are
// held to it here; the sorts' models order whole words as the device does; the loop's models are scripted as in balance_harness.cpp
// (its sums mean nothing here).  The subject: memory safety, the sizes of the buffers, the lifetimes of the snapshot and the rows
// through build / rows / run / release / coarsen, every refusal and every failed allocation.  Built and run by
// tests/test_balance_snapshot_sanitize.py.
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
enum { NS_WITHIN = 0, NS_BAND = 1, NS_OTHER = 2, NS_KEPT = 3, NS_ENTRIES = 4 };

static long long g_lift_entries = 40; // entries the lift's emit models make (the level 0 snapshot of the refusal)
static u64 g_extra_entries = 0;       // added to the count pass's entries: a device error the host must catch
static size_t g_free_bytes = (size_t)1 << 34; // what the device reports free
// the fake runtime has no hipMemGetInfo (the library refers to it weakly): this program brings its own, so the check runs here
extern "C" hipError_t hipMemGetInfo(size_t* free_bytes, size_t* total_bytes)
{
    *free_bytes = g_free_bytes;
    *total_bytes = (size_t)1 << 34;
    return hipSuccess;
}

// ---- k_balsnap_emit, word for word: thread e of the padded range; zoom_row_of's search; the three tests; the two emissions
static int row_of(const u64* start, int n_rows, long long e)
{
    int lo = 0, hi = n_rows;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= (u64)e) lo = mid;
        else hi = mid;
    }
    return lo;
}
template <bool SCATTER>
static void model_emit(void** a, dim3, dim3)
{
    const u64* rowptr = *(const u64**)a[0];
    const int* col = *(const int**)a[1];
    const u64* cnt = *(const u64**)a[2];
    const int U = *(int*)a[3];
    const long long K = *(long long*)a[4];
    const int ignore_diags = *(int*)a[5], mode = *(int*)a[6];
    const int* group = *(const int**)a[7];
    u64 *counter = *(u64**)a[8], *total = *(u64**)a[9], *ent = *(u64**)a[10];
    const u64 n_ent = *(u64*)a[11];
    u64* sc = *(u64**)a[12];
    for (long long e = 0; e < K; e++) {
        const int row = row_of(rowptr, U, e), v = col[e];
        if (v < row || v >= U) continue;
        const u64 cv = SCATTER ? 0 : cnt[e];
        if (v == row) {
            if (!SCATTER) sc[NS_WITHIN] += cv;
        } else if (v - row < ignore_diags) {
            if (!SCATTER) sc[NS_BAND] += cv;
        } else if (mode != 0 && (group[row] == group[v]) != (mode == 1)) {
            if (!SCATTER) sc[NS_OTHER] += cv;
        } else if (!SCATTER) {
            sc[NS_KEPT] += cv, sc[NS_ENTRIES] += 2;
            counter[row]++, counter[v]++;
            total[row] += cv, total[v] += cv;
        } else {
            const u64 su = counter[row]++, sv = counter[v]++, idx = (u64)e & 0xffffffffull;
            if (su < n_ent) ent[su] = ((u64)(unsigned)v << 32) | idx;
            if (sv < n_ent) ent[sv] = ((u64)(unsigned)row << 32) | idx;
        }
    }
    if (!SCATTER) sc[NS_ENTRIES] += g_extra_entries;
}
// ---- k_balsnap_gather, word for word
static void model_gather(void** a, dim3, dim3)
{
    const u64* ent = *(const u64**)a[0];
    const long long E = *(long long*)a[1];
    const u64* snap_cnt = *(const u64**)a[2];
    const long long K = *(long long*)a[3];
    int* out_col = *(int**)a[4];
    u64* out_cnt = *(u64**)a[5];
    for (long long e = 0; e < E; e++) {
        const long long src = (long long)(ent[e] & 0xffffffffull);
        out_col[e] = (int)(ent[e] >> 32);
        out_cnt[e] = src < K ? snap_cnt[src] : 0;
    }
}

// ---- the row builder's kernels (as in zoom_harness.cpp)
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
// k_lift_merge as the device runs it: the runs of `width` entries merged in pairs, from the entries to the scratch buffer or back
static void model_merge(void** a, dim3 grid, dim3)
{
    const Long* rows = *(const Long**)a[0];
    u64 *ent = *(u64**)a[1], *scratch = *(u64**)a[2];
    const long long width = *(long long*)a[3];
    const int to_scratch = *(int*)a[4];
    for (unsigned i = 0; i < grid.x; i++) {
        const u64* src = to_scratch ? ent + rows[i].off : scratch + rows[i].scratch;
        u64* dst = to_scratch ? scratch + rows[i].scratch : ent + rows[i].off;
        for (long long a0 = 0; a0 < rows[i].len; a0 += 2 * width) {
            const long long a1 = std::min(a0 + width, rows[i].len), b1 = std::min(a0 + 2 * width, rows[i].len);
            std::merge(src + a0, src + a1, src + a1, src + b1, dst + a0);
        }
    }
}
// ---- the coarsening behind a balancing (as in zoom_harness.cpp; under the identity map every word is a head and the sums are the counts)
static void model_head_totals(void** a, dim3 grid, dim3)
{
    const long long n = *(long long*)a[2];
    u64 *totals = *(u64**)a[3], *n_heads = *(u64**)a[4];
    for (unsigned b = 0; b < grid.x; b++) totals[b] = (u64)std::min<long long>(2048, n - 2048ll * b);
    *n_heads += (u64)n;
}
static void model_zoom_rowstart(void** a, dim3, dim3)
{
    const u64* rowptr = *(const u64**)a[0];
    const int* map = *(const int**)a[1];
    const int U = *(int*)a[2], C = *(int*)a[3];
    u64* segstart = *(u64**)a[4];
    for (int u = 0; u <= U; u++) {
        const int prev = u == 0 ? -1 : map[u - 1], cur = u == U ? C : map[u];
        for (int R = prev + 1; R <= cur; R++) segstart[R] = rowptr[u];
    }
}
static void model_zoom_words(void** a, dim3, dim3)
{
    const u64* rowptr = *(const u64**)a[0];
    const int* col = *(const int**)a[1];
    const int* map = *(const int**)a[2];
    const int U = *(int*)a[3];
    const long long K = *(long long*)a[4];
    const u64* segstart = *(const u64**)a[5];
    u64* word = *(u64**)a[6];
    int u = 0;
    for (long long e = 0; e < K; e++) {
        while (u + 1 < U && rowptr[u + 1] <= (u64)e) u++;
        word[e] = ((u64)(unsigned)map[col[e]] << 32) | ((u64)e - segstart[map[u]]);
    }
}
static void model_zoom_reduce(void** a, dim3, dim3)
{
    const u64* word = *(const u64**)a[0];
    const long long n = *(long long*)a[2];
    const u64* segstart = *(const u64**)a[4];
    const int C = *(int*)a[5];
    const u64* fine_cnt = *(const u64**)a[6];
    const u64 n_out = *(u64*)a[7];
    int* out_col = *(int**)a[8];
    u64 *out_cnt = *(u64**)a[9], *row_heads = *(u64**)a[10];
    int R = 0;
    for (long long e = 0; e < n && (u64)e < n_out; e++) {
        while (R + 1 < C && segstart[R + 1] <= (u64)e) R++;
        out_col[e] = (int)(word[e] >> 32);
        out_cnt[e] += fine_cnt[segstart[R] + (word[e] & 0xffffffffull)];
        row_heads[R]++;
    }
}
// ---- the lift at level 0 (the snapshot the build refuses): scripted as in zoom_harness.cpp
static void model_lift_keys(void** a, dim3, dim3)
{
    const int* pix = *(const int**)a[0];
    const int M = *(int*)a[1];
    int* key = *(int**)a[4];
    for (int s = 0; s < M; s++) key[s] = pix[s];
}
static void model_lift_heads(void** a, dim3, dim3) // two positions to a bin
{
    const int T = *(int*)a[2];
    u64* head = *(u64**)a[3];
    for (int r = 0; r < T; r++) head[r] = r % 2 == 0;
}
static void model_lift_count(void** a, dim3, dim3)
{
    const int U = *(int*)a[4];
    u64 *counter = *(u64**)a[5], *sc = *(u64**)a[8];
    for (long long e = 0; e < g_lift_entries; e++) counter[e % std::max(U - 2, 1)]++;
    sc[0] += (u64)g_lift_entries, sc[1] += (u64)g_lift_entries, sc[2] += (u64)g_lift_entries;
}
static void model_lift_scatter(void** a, dim3, dim3)
{
    const int U = *(int*)a[4];
    u64 *cursor = *(u64**)a[5], *ent = *(u64**)a[6];
    const u64 n_ent = *(u64*)a[7];
    for (long long e = 0; e < g_lift_entries; e++) {
        const u64 slot = cursor[e % std::max(U - 2, 1)]++;
        if (slot < n_ent) ent[slot] = ((u64)(e % std::max(U, 1)) << 32) | 1ull; // (column >= row: e % U >= e % (U - 2))
    }
}
// k_lift_reduce over rows whose columns are distinct (the scripted scatter's): every entry is a head
static void model_lift_reduce(void** a, dim3, dim3)
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
// ---- the loop (balance_harness.cpp's scripts): the marginals read every row, every entry and b at every column and row
static void model_marginals(void** a, dim3, dim3)
{
    const Rows r = *(const Rows*)a[0];
    const long long n_rows = *(long long*)a[1], n_ent = *(long long*)a[2];
    const int* done = *(const int**)a[3];
    double* out = *(double**)a[4];
    if (done && *done) return;
    for (long long row = 0; row < n_rows; row++) {
        double s = 0.0;
        for (u64 e = r.rowptr[row]; e < r.rowptr[row + 1] && e < (u64)n_ent; e++) s += (double)r.cnt[e] * r.b[r.col[e]];
        out[row] = 1.0 + s * r.b[row];
    }
}
static void model_mean(void** a, dim3, dim3)
{
    Ctl* ctl = *(Ctl**)a[2];
    if (ctl->done) return;
    ctl->k = (double)*(long long*)a[1], ctl->mean = 1.0;
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
    Ctl* ctl = *(Ctl**)a[2];
    const double tol = *(double*)a[3];
    const int max_iters = *(int*)a[4];
    double* variance = *(double**)a[5];
    if (ctl->done) return;
    const int it = ctl->n_iters;
    const double var = std::ldexp(1.0, -(it + 1));
    variance[it] = var; // (beyond max_iters: a heap overflow the sanitizer reports)
    ctl->n_iters = it + 1;
    if (var < tol) ctl->converged = ctl->done = 1;
    else if (it + 1 >= max_iters) ctl->done = 1;
}

// ---- the data and the rule
struct Map {
    std::vector<int64_t> rowptr, count;
    std::vector<int32_t> col;
    int64_t U() const { return (int64_t)rowptr.size() - 1; }
    int64_t K() const { return (int64_t)col.size(); }
};
// U units: the diagonal at every third, a neighbour, a partner five away, the last unit in every row (a hub column: the last row's
// mirrored entries come from every other row), one count beyond 32 bits
static Map make_map(int U)
{
    Map m;
    m.rowptr.push_back(0);
    for (int u = 0; u < U; u++) {
        std::vector<int> cols;
        if (u % 3 == 0) cols.push_back(u);
        for (int v : {u + 1, u + 5, U - 1})
            if (v > u && v < U && std::find(cols.begin(), cols.end(), v) == cols.end()) cols.push_back(v);
        std::sort(cols.begin(), cols.end());
        for (int v : cols) m.col.push_back(v), m.count.push_back(u == 1 && v == 6 ? (int64_t)1 << 40 : 1 + (u * 7 + v) % 11);
        m.rowptr.push_back((int64_t)m.col.size());
    }
    return m;
}
struct Want {
    std::vector<int64_t> rowptr, count, total;
    std::vector<int32_t> col;
    int64_t sc[5] = {0, 0, 0, 0, 0};
};
static Want rule(const Map& m, int d, int mode, const std::vector<int32_t>& group)
{
    const int64_t U = m.U();
    std::vector<std::vector<std::pair<int32_t, int64_t>>> rows((size_t)U);
    Want w;
    for (int64_t u = 0; u < U; u++)
        for (int64_t e = m.rowptr[(size_t)u]; e < m.rowptr[(size_t)u + 1]; e++) {
            const int64_t v = m.col[(size_t)e], c = m.count[(size_t)e];
            if (u == v) w.sc[NS_WITHIN] += c;
            else if (v - u < d) w.sc[NS_BAND] += c;
            else if (mode != 0 && (group[(size_t)u] == group[(size_t)v]) != (mode == 1)) w.sc[NS_OTHER] += c;
            else {
                w.sc[NS_KEPT] += c, w.sc[NS_ENTRIES] += 2;
                rows[(size_t)u].push_back({(int32_t)v, c}), rows[(size_t)v].push_back({(int32_t)u, c});
            }
        }
    w.rowptr.push_back(0);
    for (auto& r : rows) {
        std::sort(r.begin(), r.end());
        int64_t t = 0;
        for (auto& x : r) w.col.push_back(x.first), w.count.push_back(x.second), t += x.second;
        w.total.push_back(t);
        w.rowptr.push_back((int64_t)w.col.size());
    }
    return w;
}

struct Built {
    int64_t U = -7, E = -7, sc[8];
    std::vector<int64_t> rowptr, nnz, total, count;
    std::vector<int32_t> col;
};
static bool untouched(const Built& b) { return b.U == -7 && b.E == -7 && b.sc[0] == -7 && b.sc[7] == -7; }
static void reset(Built& b)
{
    b.U = b.E = -7;
    for (int k = 0; k < 8; k++) b.sc[k] = -7;
}
static int fetch_rows(ig_ctx* c, Built& b)
{
    b.rowptr.assign((size_t)b.U + 1, -7), b.nnz.assign((size_t)b.U, -7), b.total.assign((size_t)b.U, -7);
    b.col.assign((size_t)b.E + 1, -7), b.count.assign((size_t)b.E + 1, -7);
    CHECK(ig_balance_rows(c, b.rowptr.data(), b.nnz.data(), b.total.data(), b.U + 1) == 0 && ig_balance_rows(c, b.rowptr.data(), b.nnz.data(), b.total.data(), b.U) != 0);
    CHECK(ig_balance_fetch(c, 0, b.E, b.col.data(), b.count.data()) == 0 && b.col[(size_t)b.E] == -7 && b.count[(size_t)b.E] == -7);
    CHECK(ig_balance_fetch(c, 1, b.E, b.col.data(), b.count.data()) != 0);
    b.col.pop_back(), b.count.pop_back();
    return 0;
}
static int debug_build(ig_ctx* c, const Map& m, int d, int mode, const std::vector<int32_t>& group, Built& b)
{
    reset(b);
    return ig_debug_balance_snapshot(c, m.rowptr.data(), m.col.data(), m.count.data(), m.U(), d, mode, group.empty() ? nullptr : group.data(), (int64_t)group.size(), &b.U,
                                     &b.E, b.sc);
}
static int build(ig_ctx* c, int d, int mode, const std::vector<int32_t>& group, Built& b)
{
    reset(b);
    return ig_balance_build_snapshot(c, d, mode, group.empty() ? nullptr : group.data(), (int64_t)group.size(), &b.U, &b.E, b.sc);
}
static int is_the_rule(ig_ctx* c, Built& b, const Map& m, const Want& w)
{
    CHECK(b.U == m.U() && b.E == (int64_t)w.col.size() && b.sc[5] == m.K() && b.sc[6] == m.U() && b.sc[7] == b.E);
    for (int k = 0; k < 5; k++) CHECK(b.sc[k] == w.sc[k]);
    CHECK(fetch_rows(c, b) == 0);
    CHECK(b.rowptr == w.rowptr && b.col == w.col && b.count == w.count && b.total == w.total);
    for (int64_t u = 0; u < b.U; u++) CHECK(b.nnz[(size_t)u] == w.rowptr[(size_t)u + 1] - w.rowptr[(size_t)u]);
    return 0;
}
// the handle's snapshot is the map, byte for byte
static int snapshot_is(ig_ctx* c, const Map& m)
{
    std::vector<int64_t> rowptr((size_t)m.U() + 1, -7), count((size_t)m.K() + 1, -7);
    std::vector<int32_t> col((size_t)m.K() + 1, -7);
    CHECK(ig_assembly_contacts_rows(c, rowptr.data(), m.U() + 1) == 0 && rowptr == m.rowptr);
    CHECK(ig_assembly_contacts_fetch(c, 0, m.K(), col.data(), count.data()) == 0 && col[(size_t)m.K()] == -7);
    col.pop_back(), count.pop_back();
    CHECK(col == m.col && count == m.count);
    return 0;
}
static bool nothing_built(ig_ctx* c)
{
    int32_t col = -7;
    int64_t cnt = -7, w[2] = {-7, -7};
    double one = 1.0, out = 0.0;
    int32_t n = -7, cv = -7;
    return ig_balance_fetch(c, 0, 1, &col, &cnt) != 0 && std::strstr(ig_last_error(), "nothing is built") && ig_balance_rows(c, w, w, w, 2) != 0 &&
           ig_balance_run(c, &one, 1e-5, 4, &out, &out, &out, &n, &cv) != 0 && col == -7 && w[0] == -7 && n == -7;
}
static int run(ig_ctx* c, const Built& b, int group, int want_iters)
{
    const size_t U = (size_t)b.U;
    std::vector<double> b0(U, 1.0), bb(U, -7.0), marg(U, -7.0), var(20, -7.0);
    int32_t n = -7, cv = -7;
    CHECK(ig_debug_balance_group(c, group) == 0);
    CHECK(ig_balance_run(c, b0.data(), 1e-5, 20, bb.data(), marg.data(), var.data(), &n, &cv) == 0);
    CHECK(n == (b.E ? want_iters : 0) && cv == (b.E ? 1 : 0) && var[19] == 0.0);
    for (size_t u = 0; u < U; u++) CHECK(bb[u] != -7.0 && marg[u] != -7.0);
    return 0;
}

int main()
{
    fake_hip::set_model("k_balsnap_emitILb0E", model_emit<false>);
    fake_hip::set_model("k_balsnap_emitILb1E", model_emit<true>);
    fake_hip::set_model("k_balsnap_gather", model_gather);
    fake_hip::set_model("k_scan64_apply", model_scan_apply);
    fake_hip::set_model("k_lift_classifyILb0E", model_classify<false>);
    fake_hip::set_model("k_lift_classifyILb1E", model_classify<true>);
    fake_hip::set_model("k_lift_sort_lds", model_sort_items);
    fake_hip::set_model("k_lift_sort_wave", model_sort_wave);
    fake_hip::set_model("k_lift_merge", model_merge);
    fake_hip::set_model("k_lift_head_totals", model_head_totals);
    fake_hip::set_model("k_zoom_rowstart", model_zoom_rowstart);
    fake_hip::set_model("k_zoom_words", model_zoom_words);
    fake_hip::set_model("k_zoom_reduce", model_zoom_reduce);
    fake_hip::set_model("k_lift_heads", model_lift_heads);
    fake_hip::set_model("k_lift_reduce", model_lift_reduce);
    fake_hip::set_model("k_lift_keys", model_lift_keys);
    fake_hip::set_model("k_lift_passILb0E", model_lift_count);
    fake_hip::set_model("k_lift_passILb1E", model_lift_scatter);
    fake_hip::set_model("k_bal_marginals", model_marginals);
    fake_hip::set_model("k_bal_mean", model_mean);
    fake_hip::set_model("k_bal_update", model_update);
    fake_hip::set_model("k_bal_var", model_var);

    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    Built b;
    const std::vector<int32_t> none;
    const Map m = make_map(23), tiny1 = make_map(1), empty = Map{{0, 0, 0, 0}, {}, {}}, nothing = Map{{0}, {}, {}};
    std::vector<int32_t> group((size_t)m.U());
    for (int64_t u = 0; u < m.U(); u++) group[(size_t)u] = 2 + (int32_t)(u / 6) * 3;

    // ---- a bare handle: no snapshot
    CHECK(build(c, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "no snapshot") && untouched(b) && nothing_built(c));
    float ms[3 * 7];
    CHECK(ig_debug_balance_snapshot_time(c, 1, ms) != 0 && std::strstr(ig_last_error(), "no snapshot"));

    // ---- the build over caller data, every mode, the three sort forms (the hub's row: 22 entries): the rows are the rule's, the run
    // converges as scripted (17 iterations), the snapshot is the data behind each step, a second build from it gives the same rows
    for (int limits = 0; limits < 3; limits++) {
        CHECK(ig_debug_assembly_contacts_limits(c, limits == 0 ? 0 : limits == 1 ? 2 : 1, limits == 0 ? 0 : limits == 1 ? 4 : 1) == 0);
        for (int mode = 0; mode < 3; mode++)
            for (int d : {1, 2, 6}) {
                const Want w = rule(m, d, mode, group);
                CHECK(debug_build(c, m, d, mode, mode ? group : none, b) == 0 && is_the_rule(c, b, m, w) == 0 && snapshot_is(c, m) == 0);
                if (run(c, b, 1 + d, 17)) return 1;
                CHECK(snapshot_is(c, m) == 0);
                CHECK(build(c, d, mode, group, b) == 0 && is_the_rule(c, b, m, w) == 0 && snapshot_is(c, m) == 0); // (mode 0 reads no group)
                CHECK(ig_balance_release(c) == 0 && nothing_built(c) && snapshot_is(c, m) == 0);
            }
    }
    CHECK(ig_debug_assembly_contacts_limits(c, 0, 0) == 0 && ig_debug_balance_group(c, 0) == 0);
    // the smallest maps: one unit with its diagonal, units without an entry, no unit at all -- nothing is launched, the rows are empty
    for (const Map* small : {&tiny1, &empty, &nothing}) {
        const long launches = fake_hip::launches();
        CHECK(debug_build(c, *small, 2, 0, none, b) == 0 && b.E == 0 && b.sc[NS_ENTRIES] == 0 && b.sc[6] == small->U() && is_the_rule(c, b, *small, rule(*small, 2, 0, none)) == 0);
        CHECK(fake_hip::launches() - launches <= 3 + (small->K() ? 2 : 0)); // the scan of the rows' starts (and, with an entry, the two passes that keep none)
        if (small->U() > 0 && run(c, b, 0, 0)) return 1; // (with no entry every marginal is zero: nothing is launched)
        CHECK(snapshot_is(c, *small) == 0);
    }

    // ---- a coarsening behind a balancing sees the snapshot as it was: under the identity map it returns it; the coarsened level is
    // balanced in its turn (what write_pairs_zoom_levels does level by level)
    {
        CHECK(debug_build(c, m, 2, 0, none, b) == 0);
        std::vector<int32_t> ident((size_t)m.U());
        for (int64_t u = 0; u < m.U(); u++) ident[(size_t)u] = (int32_t)u;
        int64_t E = -7, sc[8];
        CHECK(ig_assembly_contacts_coarsen(c, ident.data(), m.U(), m.U(), &E, sc) == 0 && E == m.K() && snapshot_is(c, m) == 0);
        Built again;
        CHECK(fetch_rows(c, b) == 0); // the rows of the build in front of the coarsening are still there
        CHECK(build(c, 2, 1, group, again) == 0 && is_the_rule(c, again, m, rule(m, 2, 1, group)) == 0);
    }

    // ---- the refusals of the build: nothing built, the outputs untouched, the snapshot as it was, the next build works
    {
        CHECK(debug_build(c, m, 2, 0, none, b) == 0);
        std::vector<int32_t> bad = group;
        bad[7] = -1;
        const long before = fake_hip::allocations();
        for (int d : {0, -1}) CHECK(build(c, d, 0, none, b) != 0 && std::strstr(ig_last_error(), "ignore_diags") && untouched(b) && nothing_built(c));
        for (int mode : {-1, 3}) CHECK(build(c, 2, mode, group, b) != 0 && std::strstr(ig_last_error(), "mode is 0") && untouched(b) && nothing_built(c));
        CHECK(build(c, 2, 1, none, b) != 0 && std::strstr(ig_last_error(), "NULL group") && untouched(b));
        CHECK(build(c, 2, 2, std::vector<int32_t>(group.begin(), group.end() - 1), b) != 0 && std::strstr(ig_last_error(), "groups are for 22 units") && untouched(b));
        CHECK(build(c, 2, 1, bad, b) != 0 && std::strstr(ig_last_error(), "negative group") && untouched(b) && nothing_built(c));
        CHECK(ig_balance_build_snapshot(c, 2, 0, nullptr, 0, nullptr, &b.E, b.sc) != 0 && std::strstr(ig_last_error(), "NULL output") && nothing_built(c));
        CHECK(fake_hip::allocations() == before && snapshot_is(c, m) == 0); // none of them reached the device
        // a handle that cannot answer: a nuisance step in flight, a chain in flight, a shard -- both entry points; the debug entry has
        // loaded its data by then, so behind it the snapshot is that data all the same
        for (int which = 0; which < 3; which++) {
            const char* words = which == 0 ? "nuisance step" : which == 1 ? "chain" : "shard 1 of 2";
            if (which == 0) c->nuis_in_flight = true;
            else if (which == 1) c->chain_busy = true;
            else CHECK(ig_set_shard(c, 1, 2) == 0);
            CHECK(build(c, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "ig_balance_build_snapshot") && std::strstr(ig_last_error(), words) && untouched(b));
            CHECK(build(c, 2, 1, group, b) != 0 && std::strstr(ig_last_error(), words) && untouched(b));
            c->nuis_in_flight = c->chain_busy = false; // (nothing_built runs ig_balance_run, which refuses a step in flight with words of its own)
            CHECK(ig_set_shard(c, 0, 1) == 0 && nothing_built(c) && snapshot_is(c, m) == 0);
            if (which == 0) c->nuis_in_flight = true;
            else if (which == 1) c->chain_busy = true;
            else CHECK(ig_set_shard(c, 1, 2) == 0);
            CHECK(debug_build(c, m, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "ig_debug_balance_snapshot") && std::strstr(ig_last_error(), words) && untouched(b));
            c->nuis_in_flight = c->chain_busy = false;
            CHECK(ig_set_shard(c, 0, 1) == 0 && nothing_built(c));
            CHECK(debug_build(c, m, 2, 0, none, b) == 0 && is_the_rule(c, b, m, rule(m, 2, 0, none)) == 0 && snapshot_is(c, m) == 0); // the next one works
        }
        g_free_bytes = 4096; // the rows do not fit beside the snapshot: refused with the bytes named, before anything is allocated by their number
        CHECK(build(c, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "bytes of device memory") && untouched(b) && nothing_built(c) && snapshot_is(c, m) == 0);
        g_free_bytes = (size_t)1 << 34;
        g_extra_entries = 1; // an odd number of entries, then more than two per snapshot entry: device errors, caught before anything is sized by them
        CHECK(build(c, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "device error") && untouched(b) && nothing_built(c));
        g_extra_entries = 2 * (u64)m.K();
        CHECK(build(c, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "device error") && nothing_built(c) && snapshot_is(c, m) == 0);
        g_extra_entries = 0;
        CHECK(build(c, 2, 0, none, b) == 0 && is_the_rule(c, b, m, rule(m, 2, 0, none)) == 0);
        // a unit whose counts do not convert exactly: 2^53 is refused, 2^53 - 1 is built
        const int64_t top = ((int64_t)1 << 53) - 1;
        Map big = Map{{0, 2, 3, 3, 3, 3}, {top - 5, 6, 1}, {2, 3, 4}};
        CHECK(debug_build(c, big, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "2^53") && untouched(b) && nothing_built(c) && snapshot_is(c, big) == 0);
        big.count[1] = 5;
        CHECK(debug_build(c, big, 2, 0, none, b) == 0 && is_the_rule(c, b, big, rule(big, 2, 0, none)) == 0 && b.total[0] == top);
    }

    // ---- the debug entry checks its data on the host; a refusal leaves neither rows nor a snapshot
    {
        int64_t rows1[2] = {-7, -7};
        const auto no_snapshot = [&] { return ig_assembly_contacts_rows(c, rows1, 2) != 0 && std::strstr(ig_last_error(), "nothing is built") && nothing_built(c); };
        Map bad = m;
        bad.rowptr[3] = bad.rowptr[2] - 1;
        CHECK(debug_build(c, bad, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "decreases") && untouched(b) && no_snapshot());
        bad = m, bad.rowptr[0] = 1;
        CHECK(debug_build(c, bad, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "starts at 0") && no_snapshot());
        bad = m, bad.col[(size_t)m.rowptr[4]] = 3;
        CHECK(debug_build(c, bad, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "upper-triangular") && no_snapshot());
        bad = m, bad.col[(size_t)m.rowptr[4]] = (int32_t)m.U();
        CHECK(debug_build(c, bad, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "upper-triangular") && no_snapshot());
        bad = m, bad.col[(size_t)m.rowptr[4] + 1] = bad.col[(size_t)m.rowptr[4]];
        CHECK(debug_build(c, bad, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "ascend strictly") && no_snapshot());
        bad = m, bad.count[5] = -1;
        CHECK(debug_build(c, bad, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "negative count") && no_snapshot());
        bad = m, bad.count[0] = (int64_t)1 << 53; // (on the diagonal: in no total, refused all the same -- the totals are 64-bit sums)
        CHECK(debug_build(c, bad, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "counts 2^53 or more") && no_snapshot());
        bad = Map{{0, 4, 4, 4, 4, 4, 4}, {(int64_t)1 << 62, (int64_t)1 << 62, (int64_t)1 << 62, (int64_t)1 << 62}, {2, 3, 4, 5}}; // a row whose sum wraps 64 bits to 0
        CHECK(debug_build(c, bad, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "counts 2^53 or more") && untouched(b) && no_snapshot());
        CHECK(ig_debug_balance_snapshot(c, m.rowptr.data(), nullptr, m.count.data(), m.U(), 2, 0, nullptr, 0, &b.U, &b.E, b.sc) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(ig_debug_balance_snapshot(c, nullptr, m.col.data(), m.count.data(), m.U(), 2, 0, nullptr, 0, &b.U, &b.E, b.sc) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(ig_debug_balance_snapshot(c, m.rowptr.data(), m.col.data(), m.count.data(), -1, 2, 0, nullptr, 0, &b.U, &b.E, b.sc) != 0 && std::strstr(ig_last_error(), "rows") && no_snapshot());
        // (the arguments of the build are refused behind the load: the data is the snapshot, no rows are built)
        CHECK(debug_build(c, m, 0, 0, none, b) != 0 && std::strstr(ig_last_error(), "ignore_diags") && untouched(b) && nothing_built(c) && snapshot_is(c, m) == 0);
    }

    // ---- every allocation of a load, a build and a run fails once: an error that names hipMalloc, no rows, nothing leaked; a failed
    // build from the resident snapshot leaves the snapshot as it was; the next calls work
    {
        CHECK(ig_debug_assembly_contacts_limits(c, 2, 4) == 0); // (long rows: the scratch buffer and the runs' items are allocated too)
        int failed = 0;
        for (int n = 0; n < 40; n++) {
            fake_hip::fail_allocation_in(n);
            int rc = debug_build(c, m, 2, 1, group, b), rc_run = 0;
            if (!rc) { // (a run that fails comes behind a build that stands: its rows stay)
                std::vector<double> b0((size_t)b.U, 1.0), bb((size_t)b.U), marg((size_t)b.U), var(20);
                int32_t n_it = -7, conv = -7;
                rc_run = ig_balance_run(c, b0.data(), 1e-5, 20, bb.data(), marg.data(), var.data(), &n_it, &conv);
            }
            fake_hip::fail_allocation_in(-1);
            if (rc || rc_run) {
                CHECK(std::strstr(ig_last_error(), "hipMalloc"));
                failed++;
            }
            if (rc) CHECK(nothing_built(c));
            CHECK(debug_build(c, m, 2, 1, group, b) == 0 && is_the_rule(c, b, m, rule(m, 2, 1, group)) == 0);
            fake_hip::fail_allocation_in(n);
            rc = build(c, 1, 0, none, b);
            fake_hip::fail_allocation_in(-1);
            if (rc) {
                CHECK(std::strstr(ig_last_error(), "hipMalloc") && untouched(b) && nothing_built(c));
                failed++;
            }
            CHECK(snapshot_is(c, m) == 0 && build(c, 1, 0, none, b) == 0 && is_the_rule(c, b, m, rule(m, 1, 0, none)) == 0);
        }
        CHECK(failed >= 25);
        CHECK(ig_debug_assembly_contacts_limits(c, 0, 0) == 0);
    }

    // ---- the timed build: the snapshot survives, the last build's rows stay
    {
        for (float& x : ms) x = -7.0f;
        CHECK(ig_debug_balance_snapshot_time(c, 3, ms) == 0 && ms[0] != -7.0f && ms[20] != -7.0f && snapshot_is(c, m) == 0);
        b.U = m.U(), b.E = (int64_t)rule(m, 2, 0, none).col.size();
        CHECK(fetch_rows(c, b) == 0 && b.col == rule(m, 2, 0, none).col);
        CHECK(ig_debug_balance_snapshot_time(c, 0, ms) != 0 && ig_debug_balance_snapshot_time(c, 1, nullptr) != 0);
    }

    // ---- a level 0 snapshot (packed words) is refused; then the level 1 snapshot of the same genome is balanced from
    {
        const Fixture fx;
        ig_ctx* g = nullptr;
        if (fx.fresh(g)) return 1;
        int64_t nu = -7, E = -7, sc[8];
        CHECK(ig_assembly_contacts_build(g, 0, &nu, &E, sc) == 0 && nu == Fixture::M);
        CHECK(build(g, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "level 0") && untouched(b) && nothing_built(g));
        CHECK(ig_assembly_contacts_fetch(g, 0, 0, nullptr, nullptr) == 0); // the snapshot is still there
        CHECK(ig_assembly_contacts_release(g) == 0);
        CHECK(build(g, 2, 0, none, b) != 0 && std::strstr(ig_last_error(), "no snapshot"));
        // level 1 (the placed bins, reduced): what the build made is fetched, and the rows from it are the rule's over exactly that
        CHECK(ig_assembly_contacts_build(g, 1, &nu, &E, sc) == 0 && nu == Fixture::M / 2 && E == g_lift_entries);
        Map lv;
        lv.rowptr.assign((size_t)nu + 1, -7), lv.col.assign((size_t)E, -7), lv.count.assign((size_t)E, -7);
        CHECK(ig_assembly_contacts_rows(g, lv.rowptr.data(), nu + 1) == 0 && ig_assembly_contacts_fetch(g, 0, E, lv.col.data(), lv.count.data()) == 0);
        for (int d : {1, 2, 3}) {
            const Want w = rule(lv, d, 0, none);
            CHECK(w.sc[NS_ENTRIES] > 0 && w.sc[NS_WITHIN] > 0);
            CHECK(build(g, d, 0, none, b) == 0 && is_the_rule(g, b, lv, w) == 0 && snapshot_is(g, lv) == 0);
        }
        ig_destroy(g);
    }

    // ---- ig_destroy behind a failed build, and with a snapshot and rows still built
    CHECK(debug_build(c, m, 2, 0, none, b) == 0);
    CHECK(failed_call_before_destroy(c, 3, [&] { return build(c, 2, 0, none, b); }) != 0);
    CHECK(ig_create(0, &c) == 0 && c);
    CHECK(debug_build(c, m, 2, 2, group, b) == 0 && is_the_rule(c, b, m, rule(m, 2, 2, group)) == 0);
    ig_destroy(c);
    std::printf("balsnap harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
