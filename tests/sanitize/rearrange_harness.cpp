// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the segment edits (csrc/ig_host_edit.inc): a stand-alone program
// on the fake HIP runtime (fake_hip_runtime.cpp: device memory is the heap, so every copy, fill and model write is checked against the
// real allocation sizes).  The models below script what steers the host -- the status of every edit, the id a new contig uses up -- and
// touch the first and the last word of what the kernels write, for every edit of a chunk; the sums mean nothing here, memory safety, the
// chunking of a list at 1, 64, 65 and 130 edits and under a memory limit, the growth and reuse of the buffers, a state of another size
// on the same handle, every refusal and every error path are the subject.  Built and run by tests/test_rearrange_sanitize.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "harness_common.h"
// mirrors of the device structs (ig_kernels_edit.cuh: device code, not included here)
struct Plan {
    int status, rest[27];
};
struct Tabs {
    float *dist, *stot;
    int* len;
    int2* cp;
};
enum { ACC = 5, CHUNK = 64, PASSES = 6 };

static int g_N = Fixture::N;      // bins of the state on the handle
static int g_n = 0;               // edits of the chunk the plan model saw last: the other models size their writes by it
static long g_plans = 0, g_states = 0, g_state_edits = 0, g_tables = 0, g_deltas = 0, g_zeros = 0, g_commits = 0;
static int g_cid_step = 1;        // ids a committed new contig uses up (a large step makes the masks grow)
static size_t g_free_bytes = (size_t)1 << 34; // what the device reports free
// the fake runtime has no hipMemGetInfo (the library refers to it weakly): this program brings its own, so the check runs here
extern "C" hipError_t hipMemGetInfo(size_t* free_bytes, size_t* total_bytes)
{
    *free_bytes = g_free_bytes;
    *total_bytes = (size_t)1 << 34;
    return hipSuccess;
}

static void model_plan(void** a, dim3, dim3)
{
    const int* edits = *(const int**)a[2];
    const int n = *(int*)a[3], N = *(int*)a[4], mask_n = *(int*)a[7];
    Plan* plan = *(Plan**)a[5];
    u64* mask = *(u64**)a[6];
    g_n = n;
    g_plans++;
    for (int e = 0; e < n; e++) {
        std::memset(&plan[e], 0, sizeof(Plan));
        const int fb = edits[5 * e], flip = edits[5 * e + 4];
        plan[e].status = (fb < 0 || fb >= N) ? 1 : (flip < 0 || flip > 1) ? 5 : 0;
        if (plan[e].status == 0) mask[0] |= 1ull << e, mask[mask_n - 1] |= 1ull << e;
    }
}
static void model_state(void** a, dim3 grid, dim3)
{
    const int N = *(int*)a[2];
    int* dyn = *(int**)a[3];
    if ((int)grid.y != g_n) std::abort(); // (one row of workgroups per edit of the chunk)
    for (int e = 0; e < g_n; e++) {
        dyn[(size_t)e * NDYN * N] = 0;
        dyn[(size_t)(e + 1) * NDYN * N - 1] = 1;
    }
    g_states++;
    g_state_edits += g_n;
}
static void model_tables(void** a, dim3, dim3)
{
    const State& st = *(const State*)a[0];
    const Tables& t = *(const Tables*)a[2];
    const int M = *(int*)a[3];
    volatile int x = st.pos[0] + st.ori[g_N - 1];
    (void)x;
    t.dist[0] = t.dist[M - 1] = 1.0f;
    t.stot[0] = t.stot[M - 1] = 0.0f;
    t.len[0] = t.len[M - 1] = 2;
    t.cp[0] = t.cp[M - 1] = make_int2(0, 0);
    g_tables++;
}
static void model_delta(void** a, dim3, dim3)
{
    const Tabs& et = *(const Tabs*)a[4];
    const int M = *(int*)a[5], mask_n = *(int*)a[7];
    const u64* mask = *(const u64**)a[6];
    long long* out = *(long long**)a[11];
    volatile u64 m = mask[0] | mask[mask_n - 1];
    (void)m;
    for (int e = 0; e < g_n; e++) {
        volatile float d = et.dist[(size_t)e * M] + et.dist[(size_t)(e + 1) * M - 1];
        volatile int c = et.cp[(size_t)(e + 1) * M - 1].x;
        (void)d, (void)c;
        out[e * ACC] += e + 1;
        out[e * ACC + 1] += 7;
    }
    g_deltas++;
}
static void model_zero(void** a, dim3, dim3)
{
    const Tabs& et = *(const Tabs*)a[1];
    const int M = *(int*)a[2];
    long long* out = *(long long**)a[8];
    for (int e = 0; e < g_n; e++) {
        volatile int l = et.len[(size_t)(e + 1) * M - 1] + (int)et.stot[(size_t)e * M];
        (void)l;
        out[e * ACC + 2] += 3;
        out[e * ACC + 3] += 5;
        out[e * ACC + 4] += 11;
    }
    out[CHUNK * ACC - 1] += 0; // (the accumulators hold a whole chunk whatever the list's length)
    g_zeros++;
}
static void model_commit(void** a, dim3, dim3)
{
    const State& st = *(const State*)a[0];
    const int* dyn = *(const int**)a[1];
    const int N = *(int*)a[2];
    Glob* g = *(Glob**)a[3];
    const int is_new = *(int*)a[4];
    volatile int x = dyn[0] + dyn[(size_t)NDYN * N - 1];
    (void)x;
    st.pos[0] = 0;
    st.ori[N - 1] = 1;
    if (is_new) g->next_cid += g_cid_step;
    for (int i = 0; i < 12; i++) g->valid_insert[i] = 0;
    g_commits++;
}

struct Out {
    std::vector<int32_t> status;
    std::vector<int64_t> limbs;
    std::vector<double> nz, z;
    void reset(int n)
    {
        const size_t k = (size_t)std::max(n, 1);
        status.assign(k, -7);
        limbs.assign(5 * k, -7);
        nz.assign(k, -7.0);
        z.assign(k, -7.0);
    }
    bool untouched() const
    {
        for (auto v : status) if (v != -7) return false;
        for (auto v : limbs) if (v != -7) return false;
        for (auto v : nz) if (v != -7.0) return false;
        for (auto v : z) if (v != -7.0) return false;
        return true;
    }
};
static std::vector<int32_t> list_of(int n)
{
    std::vector<int32_t> e;
    for (int k = 0; k < n; k++) {
        const int v[5] = {k % g_N, k % g_N, -2, 0, k & 1};
        e.insert(e.end(), v, v + 5);
    }
    return e;
}
static int run(ig_ctx* c, const std::vector<int32_t>& edits, int form, Out& o)
{
    const int n = (int)(edits.size() / 5);
    o.reset(n);
    return ig_edit_score(c, n, edits.data(), form, o.status.data(), o.limbs.data(), o.nz.data(), o.z.data());
}
static void reset_counts() { g_plans = g_states = g_state_edits = g_tables = g_deltas = g_zeros = g_commits = 0; }

int main()
{
    fake_hip::set_model("k_edit_plan", model_plan);
    fake_hip::set_model("k_edit_state", model_state);
    fake_hip::set_model("k_fill_tables", model_tables);
    fake_hip::set_model("k_edit_delta", model_delta);
    fake_hip::set_model("k_edit_zero_delta", model_zero);
    fake_hip::set_model("k_edit_commit", model_commit);

    const Fixture fx;
    const unsigned long long per_edit = (unsigned long long)NDYN * Fixture::N * 4 + 20ull * Fixture::M + 20 + sizeof(Plan);

    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    Out o;
    std::vector<int32_t> edits = list_of(3);
    const auto untouched = [&] { return o.untouched(); };
    if (bring_up_ladder(fx, c, [&](bool) { return run(c, edits, 0, o); }, untouched, true, PARAMS_ALWAYS)) return 1;
    CHECK(fx.params(c) == 0);
    reset_counts();
    CHECK(run(c, edits, 0, o) == 0 && g_plans == 1 && g_states == 1 && g_tables == 3 && g_deltas == 1 && g_zeros == 1);
    CHECK(o.status[0] == 0 && o.limbs[0] == 1 && o.limbs[5] == 2 && o.limbs[10] == 3 && o.limbs[1] == 7 && o.limbs[2] == 3 && o.limbs[3] == 5 && o.limbs[14] == 11);

    // the arguments
    o.reset(3);
    CHECK(ig_edit_score(c, 3, nullptr, 0, o.status.data(), o.limbs.data(), o.nz.data(), o.z.data()) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_edit_score(c, 3, edits.data(), 0, nullptr, o.limbs.data(), o.nz.data(), o.z.data()) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_edit_score(c, 3, edits.data(), 0, o.status.data(), nullptr, o.nz.data(), o.z.data()) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_edit_score(c, 3, edits.data(), 0, o.status.data(), o.limbs.data(), nullptr, o.z.data()) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_edit_score(c, 3, edits.data(), 0, o.status.data(), o.limbs.data(), o.nz.data(), nullptr) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_edit_score(c, -1, edits.data(), 0, o.status.data(), o.limbs.data(), o.nz.data(), o.z.data()) != 0 && o.untouched());
    for (int form : {-1, 2}) CHECK(run(c, edits, form, o) != 0 && std::strstr(ig_last_error(), "form") && o.untouched());
    CHECK(ig_edit_score(c, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == 0); // an empty list: every pointer may be NULL
    // the statuses the plan reports come back, whatever the form; a refused edit gets the sums of the current genome in the whole form
    edits = list_of(4);
    edits[5 * 1] = -1, edits[5 * 2 + 4] = 2;
    for (int form = 0; form < 2; form++) CHECK(run(c, edits, form, o) == 0 && o.status[0] == 0 && o.status[1] == 1 && o.status[2] == 5 && o.status[3] == 0);

    // chunking: 1, 64, 65 and 130 edits in chunks of 64 or fewer; the buffers of the largest chunk seen are kept
    for (int n : {1, 64, 65, 130, 3, 64}) {
        edits = list_of(n);
        for (int form = 0; form < 2; form++) {
            reset_counts();
            CHECK(run(c, edits, form, o) == 0);
            const long chunks = (n + CHUNK - 1) / CHUNK;
            CHECK(g_plans == chunks && g_states == chunks && g_state_edits == n && g_tables == n);
            CHECK(form == 0 ? (g_deltas == chunks && g_zeros == chunks) : (g_deltas == 0 && g_zeros == 0));
            for (int e = 0; e < n; e++) CHECK(o.status[e] == 0 && o.limbs[5 * (size_t)e] == (form == 0 ? e % CHUNK + 1 : 0));
        }
    }
    {
        edits = list_of(17);
        const long before = fake_hip::allocations();
        CHECK(run(c, edits, 0, o) == 0);
        edits = list_of(130);
        CHECK(run(c, edits, 0, o) == 0 && fake_hip::allocations() == before); // (a chunk of 64 was seen: nothing is allocated again)
    }
    // a genome of another size on the same handle (20 bins of four sub-fragments: N changes, M cannot): the buffers sized for the old one
    // are freed and made again, and again on the way back; the arrays of one edit are 11 N words, checked by the models' last writes
    {
        std::vector<float> sub2((size_t)Fixture::M * 4);
        std::vector<int32_t> soa2((size_t)17 * 20, 0);
        for (int f = 0; f < 20; f++) {
            const int v[17] = {0, 0, f, 0, 4000, 4, 0, f, -1, -1, 1, 4, 4000, 1, 0, 1, f};
            for (int k = 0; k < 17; k++) soa2[(size_t)k * 20 + f] = v[k];
            for (int w = 0; w < 4; w++) {
                float* q = &sub2[(size_t)4 * (4 * f + w)];
                q[0] = (float)f, q[1] = 0.5f + (float)w, q[2] = 3.5f - (float)w, q[3] = (float)w;
            }
        }
        CHECK(ig_upload_subfrag_table(c, sub2.data(), Fixture::M) == 0 && ig_upload_state(c, soa2.data(), 20) == 0);
        g_N = 20;
        edits = list_of(70);
        long before = fake_hip::allocations();
        reset_counts();
        CHECK(run(c, edits, 0, o) == 0 && g_plans == 2 && g_state_edits == 70 && o.status[69] == 0 && fake_hip::allocations() - before >= 7);
        before = fake_hip::allocations();
        CHECK(run(c, edits, 1, o) == 0 && fake_hip::allocations() == before);
        CHECK(fx.table(c) == 0 && fx.state(c) == 0);
        g_N = Fixture::N;
        edits = list_of(3);
        before = fake_hip::allocations();
        CHECK(run(c, edits, 0, o) == 0 && o.status[2] == 0 && fake_hip::allocations() - before >= 7);
        edits = list_of(65);
        CHECK(run(c, edits, 0, o) == 0 && o.limbs[5 * 64] == 1); // (a chunk of three was made for the list of three: it grows to 64)
    }
    // sized to the free device memory: a chunk of five edits; one edit that does not fit fails first and names the bytes it needs
    if (fx.fresh(c)) return 1;
    g_free_bytes = (size_t)((1ull << 20) + 5 * per_edit + per_edit / 2);
    edits = list_of(130);
    reset_counts();
    CHECK(run(c, edits, 0, o) == 0 && g_plans == 26 && g_state_edits == 130 && g_deltas == 26);
    for (int e = 0; e < 130; e++) CHECK(o.limbs[5 * (size_t)e] == e % 5 + 1);
    g_free_bytes = (size_t)1 << 34; // (more room now: the next call grows the chunk)
    reset_counts();
    CHECK(run(c, edits, 0, o) == 0 && g_plans == 3);
    if (fx.fresh(c)) return 1;
    g_free_bytes = (size_t)((1ull << 20) + per_edit - 1);
    {
        const long before = fake_hip::allocations();
        char need[64];
        std::snprintf(need, sizeof need, "%llu bytes", per_edit + (1ull << 20));
        CHECK(run(c, edits, 0, o) != 0 && std::strstr(ig_last_error(), need) && o.untouched());
        CHECK(fake_hip::allocations() - before <= 2); // (the masks and the accumulators: nothing sized by the genome)
    }
    g_free_bytes = (size_t)1 << 34;
    CHECK(run(c, edits, 0, o) == 0);

    // the state of one edit, and the commit
    std::vector<int32_t> soa((size_t)17 * Fixture::N, -7);
    int32_t status = -7;
    int64_t limbs5[5] = {-7, -7, -7, -7, -7};
    const int32_t ok[5] = {3, 3, -2, 0, 1}, fresh_contig[5] = {3, 3, -1, 0, 0}, refused[5] = {-1, 3, -2, 0, 0};
    CHECK(ig_edit_state(c, ok, soa.data(), &status) == 0 && status == 0 && soa[7 * Fixture::N + 5] == 5 && soa[4 * Fixture::N] == 2000);
    CHECK(ig_edit_state(c, refused, soa.data(), &status) == 0 && status == 1);
    CHECK(ig_edit_state(c, ok, nullptr, &status) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_edit_state(c, nullptr, soa.data(), &status) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_edit_state(c, ok, soa.data(), nullptr) != 0 && std::strstr(ig_last_error(), "NULL"));
    reset_counts();
    CHECK(ig_edit_apply(c, refused, &status, limbs5) == 0 && status == 1 && g_commits == 0 && limbs5[0] == 0);
    CHECK(ig_edit_apply(c, ok, &status, limbs5) == 0 && status == 0 && g_commits == 1);
    CHECK(ig_edit_apply(c, ok, &status, nullptr) == 0 && status == 0 && g_commits == 2);
    CHECK(ig_edit_apply(c, nullptr, &status, limbs5) != 0 && std::strstr(ig_last_error(), "NULL"));
    CHECK(ig_edit_apply(c, ok, nullptr, limbs5) != 0 && std::strstr(ig_last_error(), "NULL") && g_commits == 2);
    // new contigs use up ids: the masks grow with the largest id
    g_cid_step = 5000;
    for (int k = 0; k < 3; k++) {
        CHECK(ig_edit_apply(c, fresh_contig, &status, limbs5) == 0 && status == 0);
        edits = list_of(65);
        CHECK(run(c, edits, 0, o) == 0 && o.status[64] == 0);
    }
    g_cid_step = 1;

    // the refusals of a handle that cannot answer: a step or a chain in flight, a shard
    edits = list_of(3);
    c->nuis_in_flight = true;
    CHECK(run(c, edits, 0, o) != 0 && std::strstr(ig_last_error(), "nuisance step") && o.untouched());
    CHECK(ig_edit_apply(c, ok, &status, limbs5) != 0 && ig_edit_state(c, ok, soa.data(), &status) != 0);
    c->nuis_in_flight = false;
    c->chain_busy = true;
    CHECK(run(c, edits, 1, o) != 0 && std::strstr(ig_last_error(), "chain") && o.untouched());
    c->chain_busy = false;
    CHECK(ig_upload_contacts(c, fx.row.data(), fx.col.data(), fx.cnt.data(), fx.Z, Fixture::M, 1, 2) == 0);
    CHECK(run(c, edits, 0, o) != 0 && std::strstr(ig_last_error(), "shard 1 of 2") && o.untouched());
    CHECK(ig_edit_apply(c, ok, &status, limbs5) != 0 && std::strstr(ig_last_error(), "shard"));
    CHECK(fx.contacts(c) == 0 && run(c, edits, 0, o) == 0);

    // every allocation of a call fails once: an error, nothing written, nothing leaked, and the next call works
    edits = list_of(12);
    const auto call = [&] { return run(c, edits, 0, o); };
    if (allocation_failure_sweep(fx, c, 24, 12, 3, 4, call, untouched, [&] { return run(c, edits, 0, o) == 0 && o.status[11] == 0; })) return 1;
    // the time entry point: both forms
    std::vector<float> ms(2 * PASSES);
    int64_t ck = 0;
    edits = list_of(70);
    reset_counts();
    CHECK(ig_debug_edit_time(c, 70, edits.data(), 0, 2, ms.data(), &ck) == 0 && ck != 0 && g_deltas == 4);
    CHECK(ig_debug_edit_time(c, 70, edits.data(), 1, 1, ms.data(), nullptr) == 0 && g_deltas == 4);
    CHECK(ig_debug_edit_time(c, 0, nullptr, 0, 1, ms.data(), &ck) == 0 && ck == 0);
    CHECK(ig_debug_edit_time(c, 70, edits.data(), 0, 0, ms.data(), &ck) != 0);
    CHECK(ig_debug_edit_time(c, 70, edits.data(), 0, 1, nullptr, &ck) != 0);
    CHECK(ig_debug_edit_time(c, -1, edits.data(), 0, 1, ms.data(), &ck) != 0);
    CHECK(ig_debug_edit_time(c, 70, edits.data(), 3, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "form"));
    // a failed call right in front of ig_destroy: whatever it left is freed there (LeakSanitizer looks at the exit)
    if (fx.fresh(c)) return 1;
    (void)failed_call_before_destroy(c, 5, call);
    std::printf("rearrange harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
