// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the polished FASTA of the polish step (csrc/ig_host_seq.inc:
// the session, the upload in pieces, the checks of the plan, the windows, the counts): a stand-alone program on the fake HIP runtime
// (fake_hip_runtime.cpp: device memory is the heap, so every copy, fill, load and store is checked against the real allocation sizes).
// The models below run the per-thread functions of csrc/ig_kernels_seq.cuh THEMSELVES (the file is included with SEQ_HOST_MODEL: the
// kernels and the wave step are left out) in the kernels' order of waves, turns and lanes, so every load of the sequence -- the aligned
// word in front of its first base and behind its last included -- every table look-up and every 16-byte store is the kernel's own.  What
// comes out is compared with a per-bin string build.  A second plan lays a file across the offset 2^32 from pieces that use one record
// of a few MiB again and again: only the plan arithmetic and small windows on either side are covered, nothing of 4 GiB exists.
// Built and run by tests/test_polish_sanitize.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "harness_common.h"
// (ig_kernels_pre.cuh is device code and not included here: the letters ABCDGHKMNRSTVWY, a bit per letter, as it defines them)
#define PRE_LETTERS ((1u << 0) | (1u << 1) | (1u << 2) | (1u << 3) | (1u << 6) | (1u << 7) | (1u << 10) | (1u << 12) | (1u << 13) | (1u << 17) | (1u << 18) | (1u << 19) | (1u << 21) | (1u << 22) | (1u << 24))
#define SEQ_HOST_MODEL
#include "../../instagraal_amd/csrc/ig_kernels_seq.cuh"

static size_t g_free_bytes = (size_t)1 << 34;
extern "C" hipError_t hipMemGetInfo(size_t* free_bytes, size_t* total_bytes)
{
    *free_bytes = g_free_bytes;
    *total_bytes = (size_t)1 << 34;
    return hipSuccess;
}

static void model_composition(void** a, dim3 grid, dim3 block)
{
    const unsigned char* seq = *(const unsigned char**)a[0];
    const long long n_runs = *(long long*)a[1];
    const long long* off = *(const long long**)a[2];
    const int R = *(int*)a[3];
    const long long runs_per_wave = *(long long*)a[4];
    u64* counts = *(u64**)a[5];
    const long long waves = (long long)grid.x * (block.x / 64);
    if (waves * runs_per_wave * 64 < n_runs || runs_per_wave > SEQ_COMP_MAX_TURNS) {
        std::fprintf(stderr, "k_seq_composition: %lld waves of %lld turns for %lld runs\n", waves, runs_per_wave, n_runs);
        std::abort();
    }
    for (long long wave = 0; wave < waves; wave++)
        for (int lane = 0; lane < 64; lane++) {
            SeqCounts acc = {-1ll, {0ull, 0ull, 0ull, 0ull}};
            for (long long turn = 0; turn < runs_per_wave; turn++) {
                const long long t = (wave * runs_per_wave + turn) * 64 + lane;
                if (t >= n_runs) break;
                seq_composition_run(seq, t, off, R, acc, counts);
            }
            seq_counts_own(acc, counts);
        }
}

template <bool COUNT>
static void model_stitch(void** a, dim3 grid, dim3 block)
{
    const unsigned char* seq = *(const unsigned char**)a[0];
    const SeqPlan pl = *(SeqPlan*)a[1];
    const long long first_byte = *(long long*)a[2], n_runs = *(long long*)a[3];
    const int runs_per_wave = *(int*)a[4];
    unsigned char* out = *(unsigned char**)a[5];
    u64* out_counts = *(u64**)a[6];
    unsigned char comp[256];
    for (unsigned b = 0; b < 256; b++) comp[b] = (unsigned char)seq_complement(b);
    const long long waves = (long long)grid.x * (block.x / 64);
    if ((waves * runs_per_wave) * 64 < n_runs) {
        std::fprintf(stderr, "k_seq_stitch: %lld waves of %d turns do not cover %lld runs\n", waves, runs_per_wave, n_runs);
        std::abort();
    }
    for (long long wave = 0; wave < waves; wave++)
        for (int lane = 0; lane < 64; lane++) {
            SeqCounts acc = {-1ll, {0ull, 0ull, 0ull, 0ull}};
            SeqState st;
            st.j = st.p = -1;
            for (int turn = 0; turn < runs_per_wave; turn++) {
                const long long t = (wave * runs_per_wave + turn) * 64 + lane;
                if (t >= n_runs) break;
                const seq_u128 o = seq_stitch_run<COUNT>(seq, pl, comp, first_byte + t * SEQ_RUN, st, acc, out_counts);
                std::memcpy(out + 16 * t, &o, 16);
            }
            if (COUNT) seq_counts_own(acc, out_counts);
        }
}

// ---- the rule, as strings
struct Genome {
    std::vector<std::string> rec;
    std::vector<uint8_t> buf;
    std::vector<int64_t> off;
    std::vector<int32_t> len;
    void finish()
    {
        for (auto& r : rec) {
            off.push_back((int64_t)buf.size());
            len.push_back((int32_t)r.size());
            buf.insert(buf.end(), r.begin(), r.end());
            buf.push_back(0);
        }
    }
};
struct Plan {
    int32_t width = 60;
    std::vector<int64_t> rec_off{0}, hdr_lit, body_len, piece_first{0}, start, length, body;
    std::vector<int32_t> hdr_len, src, ori;
    std::vector<uint8_t> lit;
    std::string file; // what the rule makes of it (left empty for the plan beyond 2^32)
    std::vector<int64_t> counts;
    int upload(ig_ctx* c) const
    {
        return ig_seq_plan(c, (int32_t)hdr_len.size(), width, rec_off.data(), hdr_len.data(), hdr_lit.data(), body_len.data(), piece_first.data(), (int64_t)src.size(), src.data(),
                           start.data(), length.data(), ori.data(), body.data(), lit.data(), (int64_t)lit.size());
    }
};
static char comp_of(char ch)
{
    const char* from = "ABCDGHKMNRSTVWY";
    const char* to = "TVGHCDMKNYSABWR";
    const char up = (char)(ch & ~0x20);
    const char* f = std::strchr(from, up);
    return f && up ? (char)(to[f - from] | (ch & 0x20)) : ch;
}
static void count_into(std::vector<int64_t>& counts, size_t j, const std::string& bases)
{
    for (char ch : bases) {
        const char up = (char)(ch & ~0x20);
        if (!up || !std::strchr("ABCDGHKMNRSTVWY", up)) continue;
        const char* plain = std::strchr("ACGTN", up);
        counts[j * 8 + (plain ? (size_t)(plain - "ACGTN") : 5)]++;
        counts[j * 8 + 6] += (ch & 0x20) ? 1 : 0;
        counts[j * 8 + 7]++;
    }
}
struct Bin {
    int src; // -1: the junction
    long long start, len;
    int ori;
};
static void add_record(Plan& pl, const Genome& g, const std::string& name, const std::vector<Bin>& bins, const std::string& junction, bool make_file)
{
    const std::string header = ">" + name + "\n";
    pl.hdr_lit.push_back((int64_t)pl.lit.size());
    pl.hdr_len.push_back((int32_t)header.size());
    pl.lit.insert(pl.lit.end(), header.begin(), header.end());
    std::string bases;
    long long at = 0;
    for (const Bin& b : bins) {
        pl.src.push_back(b.src), pl.start.push_back(b.start), pl.length.push_back(b.len), pl.ori.push_back(b.ori), pl.body.push_back(at);
        at += b.len;
        if (!make_file) continue;
        std::string part = b.src < 0 ? junction.substr((size_t)b.start, (size_t)b.len) : g.rec[(size_t)b.src].substr((size_t)b.start, (size_t)b.len);
        if (b.ori < 0) {
            std::reverse(part.begin(), part.end());
            for (char& ch : part) ch = comp_of(ch);
        }
        bases += part;
    }
    pl.body_len.push_back(at);
    pl.piece_first.push_back((int64_t)pl.src.size());
    pl.rec_off.push_back(pl.rec_off.back() + (int64_t)header.size() + at + (at + pl.width - 1) / pl.width);
    if (!make_file) return;
    pl.file += header;
    for (size_t i = 0; i < bases.size(); i += (size_t)pl.width) pl.file += bases.substr(i, (size_t)pl.width) + "\n";
    pl.counts.resize(pl.hdr_len.size() * 8, 0);
    count_into(pl.counts, pl.hdr_len.size() - 1, bases);
}

static int walk(ig_ctx* c, const Plan& pl, long long window)
{
    std::string got;
    const long long total = pl.rec_off.back();
    for (long long first = 0; first < total; first += window) {
        const long long n = std::min(window, total - first);
        std::vector<uint8_t> out((size_t)n, 0xee); // (exactly n bytes: a byte written behind them is an error)
        CHECK(ig_seq_window(c, first, n, out.data(), nullptr) == 0);
        got.append(out.begin(), out.end());
    }
    if (got != pl.file) {
        size_t k = 0;
        while (k < got.size() && k < pl.file.size() && got[k] == pl.file[k]) k++;
        std::fprintf(stderr, "window %lld: the file differs from the rule's at byte %zu of %zu\n", window, k, pl.file.size());
        return 1;
    }
    return 0;
}

static int small_genome_cases()
{
    Genome g;
    unsigned x = 12345;
    auto letters = [&](size_t n) {
        std::string s;
        const char* alphabet = "ACGTACGTACGTNRYSWKMBDHVacgtnryswkmbdhv";
        for (size_t i = 0; i < n; i++) x = x * 1103515245u + 12345u, s += alphabet[(x >> 16) % 38];
        return s;
    };
    for (size_t n : {(size_t)1, (size_t)70000, (size_t)15, (size_t)16, (size_t)17, (size_t)4097, (size_t)1}) g.rec.push_back(letters(n));
    g.finish();
    const int R = (int)g.rec.size();
    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0);
    std::vector<int64_t> counts((size_t)R * 8), out_counts;
    CHECK(ig_seq_end(c) != 0 && std::strstr(ig_last_error(), "no session"));
    CHECK(ig_seq_composition(c, counts.data(), nullptr) != 0 && std::strstr(ig_last_error(), "no session"));
    // the refusals of the records are ig_pre_begin's
    {
        std::vector<int64_t> off = g.off;
        off[1]++;
        CHECK(ig_seq_begin(c, g.buf.data(), (int64_t)g.buf.size(), off.data(), g.len.data(), R) != 0 && std::strstr(ig_last_error(), "ig_seq_begin: record 1 starts at"));
        std::vector<uint8_t> buf = g.buf;
        buf[5] = 'U';
        CHECK(ig_seq_begin(c, buf.data(), (int64_t)buf.size(), g.off.data(), g.len.data(), R) != 0 && std::strstr(ig_last_error(), "record 1, position 4"));
        g_free_bytes = 1000;
        CHECK(ig_seq_begin(c, g.buf.data(), (int64_t)g.buf.size(), g.off.data(), g.len.data(), R) != 0 && std::strstr(ig_last_error(), "are free"));
        g_free_bytes = (size_t)1 << 34;
    }
    for (int n = 0; n < 4; n++) { // every allocation of begin fails once: nothing leaked, no session left
        fake_hip::fail_allocation_in(n);
        const int rc = ig_seq_begin(c, g.buf.data(), (int64_t)g.buf.size(), g.off.data(), g.len.data(), R);
        fake_hip::fail_allocation_in(-1);
        if (rc) CHECK(std::strstr(ig_last_error(), "hipMalloc") && ig_seq_end(c) != 0);
        else CHECK(n == 3 && ig_seq_end(c) == 0);
    }
    CHECK(ig_seq_begin(c, g.buf.data(), (int64_t)g.buf.size(), g.off.data(), g.len.data(), R) == 0);
    CHECK(ig_seq_begin(c, g.buf.data(), (int64_t)g.buf.size(), g.off.data(), g.len.data(), R) != 0 && std::strstr(ig_last_error(), "a session is open"));
    CHECK(ig_seq_composition(c, counts.data(), nullptr) == 0);
    {
        std::vector<int64_t> want((size_t)R * 8, 0);
        for (int r = 0; r < R; r++) count_into(want, (size_t)r, g.rec[(size_t)r]);
        CHECK(counts == want);
    }
    uint8_t byte = 0;
    CHECK(ig_seq_window(c, 0, 1, &byte, nullptr) != 0 && std::strstr(ig_last_error(), "no plan"));

    const std::string junction = "NNNNNNacgtRYKMnnnn" + std::string(112, 'N');
    for (int width : {60, 1, 15, 16}) {
        Plan pl;
        pl.width = width;
        pl.lit.assign(junction.begin(), junction.end());
        // the first and the last base of the buffer, reversed and forward; pieces of every length around a run and a line
        std::vector<Bin> bins = {{0, 0, 1, -1}, {6, 0, 1, 1}, {1, 0, 200, -1}, {1, 70000 - 200, 200, 1}, {1, 0, 33, 1}, {-1, 0, 6, 1}, {5, 4097 - 40, 40, -1}, {-1, 0, 130, 1}};
        long long at = 100;
        for (int n : {1, 15, 16, 17, 59, 60, 61, 119, 120, 121, 122})
            for (int ori : {1, -1}) bins.push_back({1, at, n, ori}), at += n + 5;
        add_record(pl, g, "edges", bins, junction, true);
        add_record(pl, g, "b", {{0, 0, 1, 1}}, junction, true);
        add_record(pl, g, "a_header_that_is_longer_than_a_line_of_sixty_bases_and_than_sixteen_bytes", {{2, 0, 15, -1}, {3, 0, 16, -1}, {4, 0, 17, -1}, {-1, 0, 1, 1}, {5, 0, 4097, 1}},
                   junction, true);
        add_record(pl, g, "empty", {}, junction, true);
        std::vector<Bin> align; // reversed and forward pieces at every source alignment; the destination walks by 45 and 46
        for (int k = 0; k < 512; k++) align.push_back({1, 1000 + 16 * (long long)k + k % 16, 45 + (k % 16 == 15), k < 256 ? -1 : 1});
        add_record(pl, g, "align", align, junction, true);
        add_record(pl, g, "long", {{1, 3, 69990, -1}, {1, 7, 69000, 1}}, junction, true); // across a wave's kilobyte, a workgroup's span and every window
        CHECK(pl.upload(c) == 0);
        out_counts.assign(pl.hdr_len.size() * 8, -1);
        CHECK(ig_seq_out_composition(c, out_counts.data(), (int64_t)out_counts.size()) != 0 && std::strstr(ig_last_error(), "up to the file's end first"));
        if (walk(c, pl, 4096)) return 1;
        CHECK(ig_seq_out_composition(c, out_counts.data(), (int64_t)out_counts.size() - 1) != 0 && std::strstr(ig_last_error(), "capacity"));
        CHECK(ig_seq_out_composition(c, out_counts.data(), (int64_t)out_counts.size()) == 0 && out_counts == pl.counts);
        if (walk(c, pl, 1ll << 28)) return 1; // stitched again: not counted again
        if (width == 60 && walk(c, pl, 16)) return 1;
        CHECK(ig_seq_out_composition(c, out_counts.data(), (int64_t)out_counts.size()) == 0 && out_counts == pl.counts);
        CHECK(pl.upload(c) == 0); // a plan anew: the counts begin again
        if (walk(c, pl, 65536 + 16)) return 1;
        CHECK(ig_seq_out_composition(c, out_counts.data(), (int64_t)out_counts.size()) == 0 && out_counts == pl.counts);
        // the windows that are refused
        std::vector<uint8_t> out((size_t)pl.rec_off.back());
        CHECK(ig_seq_window(c, 8, 16, out.data(), nullptr) != 0 && std::strstr(ig_last_error(), "multiple of 16"));
        CHECK(ig_seq_window(c, 0, 40, out.data(), nullptr) != 0 && std::strstr(ig_last_error(), "multiple of 16"));
        CHECK(ig_seq_window(c, 16, pl.rec_off.back(), out.data(), nullptr) != 0 && std::strstr(ig_last_error(), "of a file of"));
        CHECK(ig_seq_window(c, 0, 0, out.data(), nullptr) != 0 && ig_seq_window(c, -16, 16, out.data(), nullptr) != 0 && ig_seq_window(c, 0, 16, nullptr, nullptr) != 0);

        // every refusal of the plan: a refused plan leaves none behind
        auto refused = [&](const Plan& bad, const char* what) {
            if (bad.upload(c) == 0 || !std::strstr(ig_last_error(), what)) {
                std::fprintf(stderr, "a plan that should be refused with '%s': %s\n", what, ig_last_error());
                return 1;
            }
            uint8_t b16[16];
            return ig_seq_window(c, 0, 16, b16, nullptr) != 0 && std::strstr(ig_last_error(), "no plan") ? 0 : 1;
        };
        Plan bad = pl;
        bad.start[2] = 69900; // piece 2: 200 bases of record 1 from 69 900
        CHECK(refused(bad, "piece 2 is 69900 .. 70100 of record 1") == 0);
        bad = pl, bad.start[3] = -1;
        CHECK(refused(bad, "piece 3 is -1") == 0);
        bad = pl, bad.start[5] = (int64_t)bad.lit.size() - 5;
        CHECK(refused(bad, "of the literal buffer") == 0);
        bad = pl, bad.src[4] = R;
        CHECK(refused(bad, "piece 4 is of record 7 of 7") == 0);
        bad = pl, bad.src[4] = -2;
        CHECK(refused(bad, "piece 4 is of record -2") == 0);
        bad = pl, bad.body[3] += 1;
        CHECK(refused(bad, "a gap or an overlap") == 0);
        bad = pl, bad.body[3] -= 1;
        CHECK(refused(bad, "a gap or an overlap") == 0);
        bad = pl, std::swap(bad.body[2], bad.body[3]);
        CHECK(refused(bad, "a gap or an overlap") == 0);
        bad = pl, bad.length[6] = 0;
        CHECK(refused(bad, "piece 6 has 0 bases") == 0);
        bad = pl, bad.length[6] = 1ll << 31;
        CHECK(refused(bad, "piece 6 has 2147483648 bases") == 0);
        bad = pl, bad.ori[6] = 0;
        CHECK(refused(bad, "orientation 0") == 0);
        bad = pl, bad.ori[5] = -1;
        CHECK(refused(bad, "a literal piece is never reversed") == 0);
        bad = pl, bad.body_len[0] += 1;
        CHECK(refused(bad, "not monotone") == 0);
        bad = pl, bad.rec_off[2] -= 1;
        CHECK(refused(bad, "not monotone") == 0);
        bad = pl, bad.rec_off[0] = 16;
        CHECK(refused(bad, "not at 0 with 0") == 0);
        bad = pl, bad.piece_first[1] -= 1;
        CHECK(refused(bad, "hold") == 0);
        bad = pl, bad.piece_first[2] = bad.piece_first[1] - 1;
        CHECK(refused(bad, "in the pieces") == 0);
        bad = pl, bad.piece_first.back() += 1;
        CHECK(refused(bad, "in the pieces") == 0);
        bad = pl, bad.hdr_lit[1] = (int64_t)bad.lit.size() - 1;
        CHECK(refused(bad, "the header of record 1") == 0);
        bad = pl, bad.hdr_len[1] = 0;
        CHECK(refused(bad, "the header of record 1") == 0);
        bad = pl, bad.width = 0;
        CHECK(refused(bad, "width 0") == 0);
        CHECK(ig_seq_plan(c, 0, 60, pl.rec_off.data(), pl.hdr_len.data(), pl.hdr_lit.data(), pl.body_len.data(), pl.piece_first.data(), 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                          pl.lit.data(), (int64_t)pl.lit.size()) != 0 && std::strstr(ig_last_error(), "bad sizes"));
        CHECK(ig_seq_plan(c, 1, 60, nullptr, pl.hdr_len.data(), pl.hdr_lit.data(), pl.body_len.data(), pl.piece_first.data(), 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                          pl.lit.data(), (int64_t)pl.lit.size()) != 0 && std::strstr(ig_last_error(), "NULL"));
        g_free_bytes = 1000;
        CHECK(refused(pl, "are free") == 0);
        g_free_bytes = (size_t)1 << 34;
        for (int n = 0; n < 9; n++) { // every allocation of the plan fails once
            fake_hip::fail_allocation_in(n);
            const int rc = pl.upload(c);
            fake_hip::fail_allocation_in(-1);
            if (rc) CHECK(std::strstr(ig_last_error(), "hipMalloc") && ig_seq_window(c, 0, 16, out.data(), nullptr) != 0);
            else CHECK(n == 8);
        }
        CHECK(ig_seq_end(c) == 0); // (the window buffer anew, failing once)
        CHECK(ig_seq_begin(c, g.buf.data(), (int64_t)g.buf.size(), g.off.data(), g.len.data(), R) == 0 && pl.upload(c) == 0);
        fake_hip::fail_allocation_in(0);
        CHECK(ig_seq_window(c, 0, 16, out.data(), nullptr) != 0 && std::strstr(ig_last_error(), "hipMalloc"));
        fake_hip::fail_allocation_in(-1);
        if (walk(c, pl, 4096)) return 1;
    }
    ig_destroy(c); // a live session with a plan and a window: freed there (LeakSanitizer looks at the exit)
    return 0;
}

// A file across the offset 2^32: one record of 4 MiB, used by 1 100 pieces of one body, forward and reversed in turn, and a second
// output record behind it.  The expected bytes come from the arithmetic of the layout, not from a file.
static int beyond_4gib()
{
    const long long PL = 4ll << 20, NP = 1100;
    const int width = 60;
    Genome g;
    g.rec.push_back(std::string((size_t)PL, 'A'));
    unsigned x = 99;
    for (char& ch : g.rec[0]) x = x * 1103515245u + 12345u, ch = "ACGTacgtNRYKMn"[(x >> 16) % 14];
    g.rec.push_back("GATTACA");
    g.finish();
    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && ig_seq_begin(c, g.buf.data(), (int64_t)g.buf.size(), g.off.data(), g.len.data(), 2) == 0);
    Plan pl;
    pl.width = width;
    std::vector<Bin> bins;
    for (long long k = 0; k < NP; k++) bins.push_back({0, 0, PL, k % 2 ? -1 : 1});
    add_record(pl, g, "huge", bins, "", false);
    add_record(pl, g, "behind", {{1, 0, 7, -1}}, "", false);
    CHECK(pl.rec_off[1] > (1ll << 32) + (1ll << 28) && pl.rec_off[2] == pl.rec_off[1] + 8 + 7 + 1);
    CHECK(pl.upload(c) == 0);
    auto expected = [&](long long f) -> unsigned char {
        const std::string h0 = ">huge\n", h1 = ">behind\n", tail = "TGTAATC\n";
        if (f < (long long)h0.size()) return (unsigned char)h0[(size_t)f];
        if (f >= pl.rec_off[1]) {
            const long long k = f - pl.rec_off[1];
            return (unsigned char)(k < (long long)h1.size() ? h1[(size_t)k] : tail[(size_t)(k - (long long)h1.size())]);
        }
        const long long q = f - (long long)h0.size();
        if (q % (width + 1) == width || f == pl.rec_off[1] - 1) return '\n';
        const long long b = q - q / (width + 1), piece = b / PL, k = b % PL;
        return (unsigned char)(piece % 2 ? comp_of(g.rec[0][(size_t)(PL - 1 - k)]) : g.rec[0][(size_t)k]);
    };
    const long long edge = 1ll << 32, total = pl.rec_off[2];
    const long long firsts[] = {0, edge - 4096, edge, ((pl.rec_off[1] - 100) / 16) * 16, 16 * ((6 + 3 * (PL + PL / width)) / 16)};
    for (long long first : firsts) {
        const long long n = std::min<long long>(4096, total - first);
        std::vector<uint8_t> out((size_t)n, 0xee);
        CHECK(ig_seq_window(c, first, n, out.data(), nullptr) == 0);
        for (long long k = 0; k < n; k++)
            if (out[(size_t)k] != expected(first + k)) {
                std::fprintf(stderr, "beyond 4 GiB: the file byte %lld is %d, the layout says %d\n", first + k, (int)out[(size_t)k], (int)expected(first + k));
                return 1;
            }
    }
    Plan bad = pl;
    bad.rec_off[1] -= 1ll << 32; // an offset that lost its upper half
    CHECK(bad.upload(c) != 0 && std::strstr(ig_last_error(), "not monotone"));
    CHECK(ig_seq_end(c) == 0);
    ig_destroy(c);
    return 0;
}

int main()
{
    fake_hip::set_model("k_seq_composition", model_composition);
    fake_hip::set_model("k_seq_stitchILb1E", model_stitch<true>);
    fake_hip::set_model("k_seq_stitchILb0E", model_stitch<false>);
    if (small_genome_cases()) return 1;
    if (beyond_4gib()) return 1;
    std::printf("seq harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
