// What the sanitizer harnesses of tests/sanitize/ share: the library's declarations, CHECK, and -- for the harnesses of the reports on
// the current genome -- the small genome they all work on, the bring-up ladder with its refusals, the sweep that fails every allocation
// of a call once, and the failed call in front of ig_destroy.  A harness keeps its kernel models, its outputs, its own cases and its
// final line.  The helpers CHECK for themselves and return 1 where a CHECK failed: call them as `if (helper(...)) return 1;`.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define ig_fail_msg harness_copy_of_ig_fail_msg /* ig_common.cuh defines it (for ig_draw.cpp): the library object has the real one */
#include "../../instagraal_amd/csrc/ig_common.cuh"
#undef ig_fail_msg
#include "fake_hip_runtime.h"

#define CHECK(x)                                                                                                           \
    do {                                                                                                                   \
        if (!(x)) {                                                                                                        \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s   [last error: %s]\n", __FILE__, __LINE__, #x, ig_last_error()); \
            return 1;                                                                                                      \
        }                                                                                                                  \
    } while (0)

typedef unsigned long long u64;

// A genome of 40 bins of two sub-fragments each in one contig per bin, a few contacts: T = 80 positions.
struct Fixture {
    static constexpr int N = 40, M = 80;
    std::vector<float> sub;
    std::vector<int32_t> soa, row, col, cnt;
    int64_t Z;
    float p8[8] = {50.0f, 9.6f, 1e-3f, -1.5f, 2.0f, 250.0f, 3.0e5f, 5e-3f};
    Fixture() : sub((size_t)M * 4), soa((size_t)17 * N, 0)
    {
        for (int f = 0; f < N; f++) {
            const int v[17] = {0, 0, f, 0, 2000, 2, 0, f, -1, -1, 1, 2, 2000, 1, 0, 1, f};
            for (int k = 0; k < 17; k++) soa[(size_t)k * N + f] = v[k];
            for (int w = 0; w < 2; w++) {
                float* s = &sub[(size_t)4 * (2 * f + w)];
                s[0] = (float)f, s[1] = 0.5f + (float)w, s[2] = 1.5f - (float)w, s[3] = (float)w;
            }
        }
        for (int a = 0; a < M; a++)
            for (int b = a + 1; b < M; b += 7) row.push_back(a), col.push_back(b), cnt.push_back(1 + (a + b) % 5);
        Z = (int64_t)row.size();
    }
    int table(ig_ctx* c) const { return ig_upload_subfrag_table(c, sub.data(), M); }
    int contacts(ig_ctx* c) const { return ig_upload_contacts(c, row.data(), col.data(), cnt.data(), Z, M, 0, 1); }
    int state(ig_ctx* c) const { return ig_upload_state(c, soa.data(), N); }
    int params(ig_ctx* c) const { return ig_set_params(c, p8, 1.8f, 0); }
    // a fresh handle all the way up, in place of the one c held: the genome view's and the report's buffers are made again
    int fresh(ig_ctx*& c) const
    {
        if (c) ig_destroy(c);
        c = nullptr;
        CHECK(ig_create(0, &c) == 0 && table(c) == 0 && contacts(c) == 0);
        CHECK(state(c) == 0 && params(c) == 0);
        return 0;
    }
};

enum NeedsParams { PARAMS_NEVER, PARAMS_WITH_MODEL, PARAMS_ALWAYS };

// From a handle with nothing uploaded to one that lacks the parameters only: the table, the contacts (where the report reads them: a
// report that reads none gets none), the state; before each, run(with_model) fails, ig_last_error() names what is missing and
// untouched() holds.  A report that needs the parameters only with its model (PARAMS_WITH_MODEL) is run without the model up to the
// state and with it then; one that needs them whatever `model` says (PARAMS_ALWAYS), the other way round.  Setting the parameters is
// left to the harness (Fixture::params): some have a case of their own in front of it.
template <class Run, class Untouched>
static int bring_up_ladder(const Fixture& fx, ig_ctx* c, Run run, Untouched untouched, bool needs_contacts, NeedsParams needs_params)
{
    const bool early = needs_params == PARAMS_ALWAYS;
    const char* first = needs_contacts ? "contacts" : "state";
    CHECK(run(early) != 0 && std::strstr(ig_last_error(), first) && untouched()); // nothing uploaded yet
    CHECK(fx.table(c) == 0);
    CHECK(run(early) != 0 && std::strstr(ig_last_error(), first) && untouched());
    if (needs_contacts) {
        CHECK(fx.contacts(c) == 0);
        CHECK(run(early) != 0 && std::strstr(ig_last_error(), "state") && untouched());
    }
    CHECK(fx.state(c) == 0);
    if (needs_params != PARAMS_NEVER) CHECK(run(!early) != 0 && std::strstr(ig_last_error(), "parameters") && untouched());
    return 0;
}

// Every allocation of a call fails once (turn n fails allocation n % modulo): an error that names hipMalloc, nothing written, nothing
// leaked, and the next call works.  fresh_every > 0: a new handle every so many turns, so the allocations of a first call fail too.
template <class Run, class Untouched, class Works>
static int allocation_failure_sweep(const Fixture& fx, ig_ctx*& c, int turns, int modulo, int fresh_every, int min_failed, Run run, Untouched untouched, Works still_works)
{
    int failed = 0;
    for (int n = 0; n < turns; n++) {
        if (fresh_every && n % fresh_every == 0 && fx.fresh(c)) return 1;
        fake_hip::fail_allocation_in(n % modulo);
        const int rc = run();
        fake_hip::fail_allocation_in(-1);
        if (rc) {
            CHECK(std::strstr(ig_last_error(), "hipMalloc") && untouched());
            failed++;
        }
        CHECK(still_works());
    }
    CHECK(failed >= min_failed);
    return 0;
}

// A call whose n-th allocation fails, right in front of ig_destroy: whatever it left is freed there (LeakSanitizer looks at the exit).
// Returns what the call returned.
template <class Run>
static int failed_call_before_destroy(ig_ctx*& c, int n, Run run)
{
    fake_hip::fail_allocation_in(n);
    const int rc = run();
    fake_hip::fail_allocation_in(-1);
    ig_destroy(c);
    c = nullptr;
    return rc;
}
