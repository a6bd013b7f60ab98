// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the expected contact map (csrc/ig_host_emap.inc): a
// stand-alone program on the fake HIP runtime (fake_hip_runtime.cpp: device memory is the heap, so every copy, fill and model write is
// checked against the real allocation sizes).  The models below script what steers the host -- the tiles every pixel lists, the
// monotony flag, the largest model value -- with protocol-conforming values and touch the first and the last word of what the kernels
// write; the sums mean nothing here, memory safety, the sizes of the buffers, their life and every error path are the subject.
// Built and run by tests/test_expected_map_sanitize.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "harness_common.h"
enum { SC_LINEAR = 0, SC_RING = 1, SC_MAXQ = 2, SC_EVAL = 3, SC_CONST = 4, SC_NONMONO = 5 }; // EmapBuf.sc (ig_kernels_emap.cuh: device code, not included here)

static long long g_per_pixel = -1; // tiles every pixel lists; -1: the pixels from itself on (the whole triangle)
static bool g_nonmono = false;     // k_emap_count saw ds decrease
static u64 g_maxq = 1;             // what the passes report as the largest |q|
static long g_rows = 0, g_tiles_short = 0, g_tiles_plain = 0, g_listed = 0; // what ran

static void model_count(void** a, dim3, dim3)
{
    const int T = *(int*)a[2], bin = *(int*)a[3];
    u64 *cnt = *(u64**)a[4], *sc = *(u64**)a[5];
    const int side = (T + bin - 1) / bin;
    if (cnt)
        for (int p = 0; p < side; p++) cnt[p] = g_per_pixel < 0 ? (u64)(side - p) : (u64)g_per_pixel;
    sc[SC_LINEAR] += (u64)T;
    if (g_nonmono) sc[SC_NONMONO] |= 1ull;
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
static void touch_images(void** a, int first, int side)
{
    const size_t px = (size_t)side * (size_t)side;
    for (int k = 0; k < 3; k++) {
        u64* img = *(u64**)a[first + k];
        img[0] += 1;
        img[px - 1] += 1;
    }
}
static void model_rows(void** a, dim3, dim3)
{
    touch_images(a, 6, *(int*)a[4]);
    u64* sc = *(u64**)a[9];
    sc[SC_MAXQ] = std::max(sc[SC_MAXQ], g_maxq);
    g_rows++;
}
static void model_list(void** a, dim3, dim3)
{
    const long long n = *(long long*)a[2];
    int2* list = *(int2**)a[3];
    for (long long t = 0; t < n; t++) list[t] = make_int2(0, 0);
    g_listed = (long)n;
}
template <bool SHORTCUT>
static void model_tiles(void** a, dim3 grid, dim3)
{
    const int2* list = *(const int2**)a[0];
    volatile int last = list[grid.x - 1].x; // (the launch is as wide as the list)
    (void)last;
    touch_images(a, 7, *(int*)a[5]);
    u64* sc = *(u64**)a[10];
    sc[SC_MAXQ] = std::max(sc[SC_MAXQ], g_maxq);
    sc[SHORTCUT ? SC_CONST : SC_EVAL] += grid.x;
    (SHORTCUT ? g_tiles_short : g_tiles_plain)++;
}
static void model_mirror(void** a, dim3, dim3)
{
    u64* img = *(u64**)a[0];
    const int side = *(int*)a[1];
    img[(size_t)side * side - 1] += 0;
}
static void model_checksum(void** a, dim3, dim3)
{
    const u64* img = *(const u64**)a[0];
    const long long n = *(long long*)a[1];
    u64* out = *(u64**)a[2];
    *out += img[0] + img[n - 1];
}

struct Out {
    std::vector<int64_t> img[3];
    int32_t side = -7, bin = -7;
    int64_t sc[8];
};
static int run(ig_ctx* c, int max_side, int64_t cap, Out& o)
{
    for (auto& v : o.img) v.assign((size_t)std::max<int64_t>(cap, 1), -7);
    for (auto& v : o.sc) v = -7;
    o.side = o.bin = -7;
    return ig_expected_map(c, max_side, o.img[0].data(), o.img[1].data(), o.img[2].data(), cap, &o.side, &o.bin, o.sc);
}

int main()
{
    fake_hip::set_model("k_emap_count", model_count);
    fake_hip::set_model("k_scan64_apply", model_scan_apply);
    fake_hip::set_model("k_emap_rows", model_rows);
    fake_hip::set_model("k_emap_list", model_list);
    fake_hip::set_model("k_emap_tilesILb1E", model_tiles<true>);
    fake_hip::set_model("k_emap_tilesILb0E", model_tiles<false>);
    fake_hip::set_model("k_map_mirror", model_mirror);
    fake_hip::set_model("k_emap_checksum", model_checksum);

    const Fixture fx;
    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    Out o;
    const auto small = [&] { return run(c, 8, 64, o); };
    // (no contact is uploaded: none is read)
    if (bring_up_ladder(fx, c, [&](bool) { return small(); }, [&] { return o.side == -7; }, false, PARAMS_ALWAYS)) return 1;
    CHECK(fx.params(c) == 0);
    for (int bad : {0, -3}) CHECK(run(c, bad, 64, o) != 0 && std::strstr(ig_last_error(), "max_side") && o.side == -7);
    CHECK(ig_expected_map(c, 8, o.img[0].data(), o.img[1].data(), o.img[2].data(), 64, nullptr, &o.bin, o.sc) != 0);
    CHECK(ig_expected_map(c, 8, o.img[0].data(), o.img[1].data(), o.img[2].data(), 64, &o.side, &o.bin, nullptr) != 0);
    CHECK(ig_debug_expected_map_form(c, 4) != 0 && ig_debug_expected_map_form(c, -1) != 0);
    // the capacity: the size is reported, nothing else is written, nothing is allocated for the images
    {
        const long before = fake_hip::allocations();
        CHECK(run(c, 8, 63, o) != 0 && std::strstr(ig_last_error(), "hold") && o.side == 8 && o.bin == 10 && o.img[0][0] == -7 && o.sc[0] == -7);
        CHECK(fake_hip::allocations() - before < 12); // (the map's and the law's tables only)
        CHECK(ig_expected_map(c, 8, nullptr, o.img[1].data(), o.img[2].data(), 64, &o.side, &o.bin, o.sc) != 0 && std::strstr(ig_last_error(), "NULL"));
    }
    // every form at several sizes: one position per pixel (always the rows), a partial last pixel, one pixel
    for (int form = 0; form < 4; form++) {
        CHECK(ig_debug_expected_map_form(c, form) == 0);
        for (int max_side : {200, 80, 27, 8, 1}) {
            g_rows = g_tiles_short = g_tiles_plain = 0;
            CHECK(run(c, max_side, 80 * 80, o) == 0);
            CHECK(o.side == (max_side >= 80 ? 80 : max_side == 27 ? 27 : max_side) && o.sc[0] == 80 && o.sc[1] == 80 && o.sc[3] == 1);
            const bool tiles = o.bin > 1 && (form >= 2 || (form == 0 && g_rows == 0)); /* (form 0: whichever the library ships at this pixel size) */
            CHECK(g_rows == (tiles ? 0 : 1) && g_tiles_short == (tiles && form != 3 ? 1 : 0) && g_tiles_plain == (tiles && form == 3 ? 1 : 0));
            if (tiles) CHECK(g_listed == (long)o.side * (o.side + 1) / 2 && o.sc[4] + o.sc[5] == g_listed);
            else CHECK(o.sc[4] == 0 && o.sc[5] == 0);
        }
    }
    CHECK(ig_debug_expected_map_form(c, 2) == 0);
    // the monotony flag: the tiles run without the shortcut
    g_nonmono = true;
    g_tiles_short = g_tiles_plain = 0;
    CHECK(run(c, 8, 64, o) == 0 && g_tiles_short == 0 && g_tiles_plain == 1 && o.sc[5] == 0 && o.sc[4] == 36);
    g_nonmono = false;
    // the size of the work list: fewer tiles than pixels, more than the triangle -- caught before anything is sized by it
    for (long long per : {0ll, 5ll, 1ll << 40}) {
        g_per_pixel = per;
        const long before = fake_hip::allocations();
        g_listed = -1;
        CHECK(run(c, 8, 64, o) != 0 && std::strstr(ig_last_error(), "work list") && g_listed == -1 && o.img[0][0] == -7);
        CHECK(fake_hip::allocations() - before < 12);
    }
    g_per_pixel = 1; // the diagonal alone: the smallest list there is
    CHECK(run(c, 8, 64, o) == 0 && g_listed == 8);
    g_per_pixel = -1;
    // the overflow guard: 2 bin^2 max_q >= 2^62
    g_maxq = 1ull << 55;
    CHECK(run(c, 8, 64, o) != 0 && std::strstr(ig_last_error(), "model value too large for this pixel size") && o.img[0][0] == -7);
    CHECK(run(c, 80, 80 * 80, o) == 0); // (one position per pixel: 2 x 2^55 fits)
    CHECK(ig_debug_expected_map_form(c, 1) == 0 && run(c, 1, 1, o) != 0 && std::strstr(ig_last_error(), "pixel size"));
    g_maxq = 1;
    // every allocation of a call fails once: an error, nothing leaked, and the next call works
    for (int form = 1; form <= 2; form++) {
        CHECK(ig_debug_expected_map_form(c, form) == 0);
        if (allocation_failure_sweep(fx, c, 24, 24, 0, form == 2 ? 6 : 2, small, [&] { return o.img[0][0] == -7; }, [&] { return small() == 0 && o.side == 8; })) return 1;
    }
    // the time entry point
    std::vector<float> ms(3);
    int64_t ck = 0;
    for (int form = 0; form < 4; form++) CHECK(ig_debug_expected_map_time(c, 8, form, 3, ms.data(), &ck) == 0);
    CHECK(ig_debug_expected_map_time(c, 8, 1, 0, ms.data(), &ck) != 0 && ig_debug_expected_map_time(c, 8, 7, 1, ms.data(), &ck) != 0);
    CHECK(ig_debug_expected_map_time(c, 0, 1, 1, ms.data(), &ck) != 0 && ig_debug_expected_map_time(c, 8, 2, 1, ms.data(), nullptr) == 0);
    g_per_pixel = 0;
    CHECK(ig_debug_expected_map_time(c, 8, 2, 1, ms.data(), &ck) != 0 && std::strstr(ig_last_error(), "work list"));
    g_per_pixel = -1;
    // a failed call right in front of ig_destroy: whatever it left is freed there (LeakSanitizer looks at the exit)
    (void)failed_call_before_destroy(c, 3, small);
    std::printf("emap harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
