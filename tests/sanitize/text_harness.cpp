// AddressSanitizer / UBSan / LeakSanitizer harness for the HOST logic of the reader of 4DN pairs text (csrc/ig_host_text.inc: the
// session, the vocabulary's table, the upload in pieces, the buffers that grow with the bytes and with the lines of a chunk, the two
// scans, the fetch): a stand-alone program on the fake HIP runtime (fake_hip_runtime.cpp: device memory is the heap, so every copy and
// model access is checked against the real allocation sizes).  The models below do what the five kernels do, load for load and word for
// word -- a run's two 16-byte loads at the buffer's end, the staging of a workgroup's lines in 16-byte pieces from the aligned start --
// and what comes out is compared with a line-by-line brute force.  Built and run by tests/test_pairs_text_sanitize.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "harness_common.h"
// mirrors of the device structs and constants (ig_kernels_text.cuh: device code, not included here)
struct Cols {
    int c[6], need, last;
};
struct Names {
    const unsigned char* bytes;
    const long long* off;
    const int* id;
    const int* table;
    unsigned mask;
};
struct Raw {
    int *c1, *c2;
    long long *p1, *p2;
    unsigned char* strands;
};
static const unsigned THREADS = 256, SPAN = 32768;
enum { DATA = 0, COMMENT = 1, MALFORMED = 2, DEFERRED = 3 };

static size_t g_free_bytes = (size_t)1 << 34;
extern "C" hipError_t hipMemGetInfo(size_t* free_bytes, size_t* total_bytes)
{
    *free_bytes = g_free_bytes;
    *total_bytes = (size_t)1 << 34;
    return hipSuccess;
}

static void model_mark(void** a, dim3 grid, dim3)
{
    const unsigned char* bytes = *(const unsigned char**)a[0];
    const unsigned n = *(unsigned*)a[1];
    unsigned short* nl_bits = *(unsigned short**)a[2];
    u64* blk = *(u64**)a[3];
    unsigned* sc = *(unsigned**)a[4];
    for (unsigned b = 0; b < grid.x; b++) {
        unsigned count = 0;
        for (unsigned t = 0; t < THREADS; t++) {
            const unsigned run = b * THREADS + t, at = run * 16;
            if (at >= n) continue;
            unsigned char w[32];
            std::memcpy(w, bytes + 16 * (size_t)run, 16);            // the run's own load ...
            std::memcpy(w + 16, bytes + 16 * ((size_t)run + 1), 16); // ... and the one behind it: both inside the allocation
            const unsigned live = std::min(n - at, 16u);
            unsigned nl = 0, hash = 0;
            for (unsigned i = 0; i < live; i++) {
                if (w[i] == '\n') nl |= 1u << i;
                if (w[i] == '#') hash |= 1u << i;
                if (w[i] == '\r' || w[i] >= 0x80) sc[0] |= 1u;
            }
            if (hash) {
                const unsigned prev = at == 0 ? 1u : (bytes[at - 1] == '\n' ? 1u : 0u);
                const unsigned starts = hash & ((nl << 1) | prev);
                for (unsigned i = 0; i < 16; i++)
                    if (((starts >> i) & 1u) && at + i + 9 <= n && std::memcmp(w + i + 1, "columns:", 8) == 0) sc[1] = std::min(sc[1], at + i);
            }
            nl_bits[run] = (unsigned short)nl;
            count += (unsigned)__builtin_popcount(nl);
        }
        blk[b] = count;
    }
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
static void model_lines(void** a, dim3 grid, dim3)
{
    const unsigned short* nl_bits = *(const unsigned short**)a[0];
    const unsigned n = *(unsigned*)a[1];
    const u64* blk_incl = *(const u64**)a[2];
    int* line_start = *(int**)a[3];
    const unsigned n_lines = *(unsigned*)a[4];
    for (unsigned b = 0; b < grid.x; b++) {
        unsigned rank = b ? (unsigned)blk_incl[b - 1] : 0u;
        for (unsigned t = 0; t < THREADS; t++) {
            const unsigned run = b * THREADS + t, at = run * 16;
            const unsigned nl = at < n ? nl_bits[run] : 0u;
            for (unsigned i = 0; i < 16; i++)
                if ((nl >> i) & 1u) {
                    if (rank + 1 <= n_lines) line_start[rank + 1] = (int)(at + i + 1);
                    rank++;
                }
        }
    }
    line_start[0] = 0;
    line_start[n_lines] = (int)n;
}
static bool model_int(const unsigned char* p, unsigned bias, unsigned a, unsigned b, long long* out)
{
    bool minus = false;
    if (a < b && (p[a - bias] == '+' || p[a - bias] == '-')) minus = p[a - bias] == '-', a++;
    if (a >= b || b - a > 18) return false;
    long long v = 0;
    for (unsigned i = a; i < b; i++) {
        if (p[i - bias] < '0' || p[i - bias] > '9') return false;
        v = v * 10 + (p[i - bias] - '0');
    }
    *out = minus ? -v : v;
    return true;
}
static int model_name(const unsigned char* p, unsigned bias, unsigned a, unsigned b, const Names& nm)
{
    u64 h = 1469598103934665603ull;
    for (unsigned i = a; i < b; i++) h = (h ^ p[i - bias]) * 1099511628211ull;
    for (unsigned slot = (unsigned)h & nm.mask, probes = 0; probes <= nm.mask; slot = (slot + 1) & nm.mask, probes++) {
        const int k = nm.table[slot];
        if (k < 0) return -1;
        if (nm.off[k + 1] - nm.off[k] != (long long)(b - a)) continue;
        if (b == a || std::memcmp(nm.bytes + nm.off[k], p + (a - bias), b - a) == 0) return nm.id[k];
    }
    return -1;
}
static void model_parse(void** a, dim3 grid, dim3)
{
    const unsigned char* bytes = *(const unsigned char**)a[0];
    const int* line_start = *(const int**)a[2];
    const unsigned n_lines = *(unsigned*)a[3];
    const Cols cols = *(Cols*)a[4];
    const Names nm = *(Names*)a[5];
    unsigned char* status = *(unsigned char**)a[6];
    const Raw raw = *(Raw*)a[7];
    u64* blk = *(u64**)a[8];
    const unsigned n_blocks = *(unsigned*)a[9];
    unsigned* sc = *(unsigned**)a[10];
    std::vector<unsigned char> stage((SPAN / 16 + 1) * 16);
    for (unsigned b = 0; b < grid.x; b++) {
        const unsigned first = b * THREADS, lo = (unsigned)line_start[first], hi = (unsigned)line_start[std::min(first + THREADS, n_lines)];
        const bool staged = hi - lo <= SPAN;
        const unsigned lo16 = lo & ~15u;
        if (staged)
            for (unsigned q = 0; lo16 + 16 * q < hi; q++) std::memcpy(&stage.at(16 * q), bytes + lo16 + 16 * (size_t)q, 16); // the 16-byte loads from the aligned start
        unsigned count[4] = {0, 0, 0, 0};
        for (unsigned t = 0; t < THREADS && first + t < n_lines; t++) {
            const unsigned line = first + t, s = (unsigned)line_start[line];
            unsigned e = (unsigned)line_start[line + 1];
            if (s >= sc[1]) {
                if (s == sc[1]) sc[2] = line;
                status[line] = COMMENT;
                continue;
            }
            const unsigned char* p = staged ? stage.data() : bytes;
            const unsigned bias = staged ? lo16 : 0;
            if (e > s && p[e - 1 - bias] == '\n') e--;
            int st;
            if (s < e && p[s - bias] == '#') st = COMMENT;
            else {
                unsigned fs[6], fe[6], start = s;
                for (int k = 0; k < 6; k++) fs[k] = fe[k] = s;
                int f = 0;
                for (unsigned i = s; i <= e; i++) {
                    if (i < e && p[i - bias] != '\t') continue;
                    for (int k = 0; k < 6; k++)
                        if (f == cols.c[k]) fs[k] = start, fe[k] = i;
                    f++, start = i + 1;
                    if (f > cols.last) break;
                }
                long long p1 = 0, p2 = 0;
                if (f < cols.need) st = MALFORMED;
                else if (!model_int(p, bias, fs[1], fe[1], &p1) || !model_int(p, bias, fs[3], fe[3], &p2)) st = DEFERRED;
                else {
                    st = DATA;
                    raw.strands[line] = (unsigned char)(((cols.c[4] < f && fe[4] - fs[4] == 1 && p[fs[4] - bias] == '-') ? 1 : 0) | ((cols.c[5] < f && fe[5] - fs[5] == 1 && p[fs[5] - bias] == '-') ? 2 : 0));
                    raw.c1[line] = model_name(p, bias, fs[0], fe[0], nm), raw.c2[line] = model_name(p, bias, fs[2], fe[2], nm);
                    raw.p1[line] = p1, raw.p2[line] = p2;
                }
            }
            status[line] = (unsigned char)st;
            count[st]++;
        }
        for (int k = 0; k < 4; k++) sc[3 + k] += count[k];
        blk[b] = count[DATA], blk[n_blocks + b] = count[DEFERRED];
    }
}
static void model_compact(void** a, dim3 grid, dim3)
{
    const unsigned char* status = *(const unsigned char**)a[0];
    const unsigned n_lines = *(unsigned*)a[1], cols_line = *(unsigned*)a[2];
    const Raw raw = *(Raw*)a[3];
    const u64* blk_incl = *(const u64**)a[4];
    const unsigned n_blocks = *(unsigned*)a[5];
    const Raw out = *(Raw*)a[6];
    const unsigned n_data = *(unsigned*)a[7];
    int* deferred = *(int**)a[8];
    const unsigned n_deferred = *(unsigned*)a[9];
    for (unsigned b = 0; b < grid.x; b++) {
        unsigned d = b ? (unsigned)blk_incl[b - 1] : 0u, f = b ? (unsigned)blk_incl[n_blocks + b - 1] : 0u;
        for (unsigned line = b * THREADS; line < std::min((b + 1) * THREADS, n_lines); line++) {
            if (line >= cols_line) continue;
            if (status[line] == DATA) {
                if (d < n_data) out.c1[d] = raw.c1[line], out.p1[d] = raw.p1[line], out.c2[d] = raw.c2[line], out.p2[d] = raw.p2[line], out.strands[d] = raw.strands[line];
                d++;
            } else if (status[line] == DEFERRED) {
                if (f < n_deferred) deferred[f] = (int)line;
                f++;
            }
        }
    }
}

// ---- the brute force: line by line with the standard library
struct Want {
    std::vector<uint8_t> status, strands;
    std::vector<int32_t> line_start, c1, c2, deferred;
    std::vector<int64_t> p1, p2;
    int64_t sc[8];
};
static bool brute_int(const std::string& s, int64_t* v)
{
    size_t i = (!s.empty() && (s[0] == '+' || s[0] == '-')) ? 1 : 0;
    if (s.size() - i < 1 || s.size() - i > 18 || s.find_first_not_of("0123456789", i) != std::string::npos) return false;
    *v = std::strtoll(s.c_str(), nullptr, 10);
    return true;
}
static Want brute(const std::string& text, const int cols[6], const std::map<std::string, int>& names)
{
    Want w;
    for (int k = 0; k < 8; k++) w.sc[k] = 0;
    w.sc[5] = -1;
    if (text.find('\r') != std::string::npos || std::any_of(text.begin(), text.end(), [](char ch) { return (unsigned char)ch >= 0x80; })) {
        w.sc[6] = 1;
        return w;
    }
    size_t at = 0;
    w.line_start.push_back(0);
    while (at < text.size()) {
        const size_t nl = text.find('\n', at), end = nl == std::string::npos ? text.size() : nl;
        const std::string line = text.substr(at, end - at);
        at = nl == std::string::npos ? text.size() : nl + 1;
        w.line_start.push_back((int32_t)at);
        const int j = (int)w.status.size();
        if (w.sc[5] >= 0 || line.compare(0, 9, "#columns:") == 0) {
            if (w.sc[5] < 0) w.sc[5] = j;
            w.status.push_back(COMMENT);
            continue;
        }
        if (!line.empty() && line[0] == '#') {
            w.status.push_back(COMMENT), w.sc[2]++;
            continue;
        }
        std::vector<std::string> f;
        for (size_t s = 0;;) {
            const size_t t = line.find('\t', s);
            f.push_back(line.substr(s, t == std::string::npos ? std::string::npos : t - s));
            if (t == std::string::npos) break;
            s = t + 1;
        }
        int64_t p1, p2;
        if ((int)f.size() <= std::max(std::max(cols[0], cols[1]), std::max(cols[2], cols[3]))) w.status.push_back(MALFORMED), w.sc[3]++;
        else if (!brute_int(f[(size_t)cols[1]], &p1) || !brute_int(f[(size_t)cols[3]], &p2)) w.status.push_back(DEFERRED), w.sc[4]++, w.deferred.push_back(j);
        else {
            auto id = [&](const std::string& s) { return names.count(s) ? names.at(s) : -1; };
            auto minus = [&](int c) { return c < (int)f.size() && f[(size_t)c] == "-"; };
            w.status.push_back(DATA), w.sc[1]++;
            w.c1.push_back(id(f[(size_t)cols[0]])), w.c2.push_back(id(f[(size_t)cols[2]])), w.p1.push_back(p1), w.p2.push_back(p2);
            w.strands.push_back((uint8_t)((minus(cols[4]) ? 1 : 0) | (minus(cols[5]) ? 2 : 0)));
        }
    }
    w.sc[0] = (int64_t)w.status.size();
    return w;
}

struct Vocabulary {
    std::map<std::string, int> names;
    std::vector<uint8_t> bytes;
    std::vector<int64_t> off = {0};
    std::vector<int32_t> id;
    void add(const std::string& s, int v)
    {
        names[s] = v; // (the later id wins)
        bytes.insert(bytes.end(), s.begin(), s.end());
        off.push_back((int64_t)bytes.size()), id.push_back(v);
    }
    int begin(ig_ctx* c) const { return ig_text_begin(c, bytes.data(), off.data(), id.data(), (int32_t)id.size()); }
};
static const int kCols[6] = {1, 2, 3, 4, 5, 6};

// one chunk through ig_text_parse and ig_text_fetch against the brute force; the outputs are one element longer than the result
static int chunk_agrees(ig_ctx* c, const std::string& text, const int cols[6], const Vocabulary& v)
{
    const Want w = brute(text, cols, v.names);
    int64_t sc[8];
    float ms[4] = {-7, -7, -7, -7};
    std::vector<uint8_t> exact(text.begin(), text.end()); // (a heap block of exactly n bytes: a read beyond the chunk on the host side is caught)
    CHECK(ig_text_parse(c, exact.data(), (int64_t)exact.size(), cols, sc, ms) == 0 && ms[3] != -7.0f);
    for (int k = 0; k < 8; k++) CHECK(sc[k] == w.sc[k] || (w.sc[6] && k != 6));
    if (w.sc[6]) {
        CHECK(ig_text_fetch(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0 && std::strstr(ig_last_error(), "to_host"));
        return 0;
    }
    const size_t L = w.status.size(), D = w.c1.size(), F = w.deferred.size();
    std::vector<uint8_t> status(L + 1, 77), strands(D + 1, 77);
    std::vector<int32_t> ls(L + 2, -7), c1(D + 1, -7), c2(D + 1, -7), def(F + 1, -7);
    std::vector<int64_t> p1(D + 1, -7), p2(D + 1, -7);
    CHECK(ig_text_fetch(c, status.data(), ls.data(), c1.data(), p1.data(), c2.data(), p2.data(), strands.data(), def.data()) == 0);
    CHECK(status[L] == 77 && strands[D] == 77 && ls[L + 1] == -7 && c1[D] == -7 && c2[D] == -7 && def[F] == -7 && p1[D] == -7 && p2[D] == -7);
    status.resize(L), strands.resize(D), ls.resize(L + 1), c1.resize(D), c2.resize(D), def.resize(F), p1.resize(D), p2.resize(D);
    CHECK(status == w.status && ls == w.line_start && c1 == w.c1 && p1 == w.p1 && c2 == w.c2 && p2 == w.p2 && strands == w.strands && def == w.deferred);
    CHECK(ig_text_fetch(c, nullptr, nullptr, nullptr, p1.data(), nullptr, nullptr, nullptr, nullptr) == 0 && p1 == w.p1); // any pointer may be NULL
    return 0;
}

static std::string lines(int n, unsigned seed, int pad = 0)
{
    unsigned x = seed;
    auto next = [&] { return (x = x * 1664525u + 1013904223u) >> 8; };
    const char* name[] = {"chr1", "chr11", "chr", "a", "", "unknown", "chr2"};
    const char* pos[] = {"5", "+7", "-3", "007", "123456789012345678", "1234567890123456789", "12x", " 9", "", "1_0", "44444", "2147483648"};
    std::string out;
    for (int k = 0; k < n; k++) {
        const unsigned kind = next() % 40;
        if (kind == 0) out += "#a comment\n";
        else if (kind == 1) out += "\n";
        else if (kind == 2) out += "r\tchr1\t5\n";
        else {
            out += "r" + std::string((size_t)pad, 'x') + std::to_string(next() % 100000) + "\t" + name[next() % 7] + "\t" + pos[kind < 30 ? 10 : next() % 12] + "\t" + name[next() % 7] + "\t" +
                   pos[kind < 30 ? 0 : next() % 12];
            if (next() % 4) out += std::string("\t") + "+-.-"[next() % 4] + "\t" + "+-"[next() % 2];
            if (next() % 3 == 0) out += "\tUU\t60";
            out += "\n";
        }
    }
    return out;
}

int main()
{
    fake_hip::set_model("k_text_mark", model_mark);
    fake_hip::set_model("k_text_lines", model_lines);
    fake_hip::set_model("k_text_parse", model_parse);
    fake_hip::set_model("k_text_compact", model_compact);
    fake_hip::set_model("k_scan64_apply", model_scan_apply);

    const Fixture fx;
    Vocabulary v;
    for (const char* s : {"chr1", "chr11", "chr2", "a", "chr1"}) v.add(s, (int)v.id.size() + 10);
    for (int k = 0; k < 300; k++) v.add("ctg" + std::to_string(k), k); // probes longer than one
    ig_ctx* c = nullptr;
    CHECK(ig_create(0, &c) == 0 && c);
    int64_t sc[8] = {-7, -7, -7, -7, -7, -7, -7, -7};
    const uint8_t one = 'x';

    // ---- nothing without a session; end without one is harmless; the refusals of the vocabulary, on the host
    CHECK(ig_text_end(c) == 0);
    CHECK(ig_text_parse(c, &one, 1, kCols, sc, nullptr) != 0 && std::strstr(ig_last_error(), "no session") && sc[0] == -7);
    CHECK(ig_text_fetch(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0 && ig_text_feed_pre(c, sc, nullptr) != 0 && ig_text_feed_pairs(c, sc) != 0);
    {
        const long before = fake_hip::allocations();
        std::vector<int64_t> bad = v.off;
        bad[3] = bad[2] - 1;
        CHECK(ig_text_begin(c, v.bytes.data(), bad.data(), v.id.data(), (int32_t)v.id.size()) != 0 && std::strstr(ig_last_error(), "decreases"));
        CHECK(ig_text_begin(c, v.bytes.data(), nullptr, v.id.data(), 3) != 0 && ig_text_begin(c, nullptr, v.off.data(), v.id.data(), 3) != 0 && std::strstr(ig_last_error(), "NULL"));
        CHECK(ig_text_begin(c, v.bytes.data(), v.off.data(), v.id.data(), -1) != 0 && fake_hip::allocations() == before && ig_text_begin(nullptr, nullptr, nullptr, nullptr, 0) != 0);
    }
    CHECK(v.begin(c) == 0);
    CHECK(v.begin(c) != 0 && std::strstr(ig_last_error(), "a session is open"));

    // ---- the refusals of a chunk: on the arguments, nothing allocated by them
    {
        const long before = fake_hip::allocations();
        CHECK(ig_text_parse(c, &one, ((int64_t)1 << 30) + 1, kCols, sc, nullptr) != 0 && std::strstr(ig_last_error(), "2^30") && sc[0] == -7);
        CHECK(ig_text_parse(c, &one, -1, kCols, sc, nullptr) != 0 && ig_text_parse(c, nullptr, 1, kCols, sc, nullptr) != 0 && ig_text_parse(c, &one, 1, nullptr, sc, nullptr) != 0);
        const int neg[6] = {1, 2, 3, -4, 5, 6};
        CHECK(ig_text_parse(c, &one, 1, neg, sc, nullptr) != 0 && std::strstr(ig_last_error(), "column 3") && ig_text_parse(c, &one, 1, kCols, nullptr, nullptr) != 0);
        g_free_bytes = 1024;
        CHECK(ig_text_parse(c, &one, 1, kCols, sc, nullptr) != 0 && std::strstr(ig_last_error(), "bytes of device memory") && sc[0] == -7);
        g_free_bytes = (size_t)1 << 34;
        CHECK(fake_hip::allocations() == before);
        CHECK(ig_text_fetch(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0 && std::strstr(ig_last_error(), "nothing is parsed"));
    }

    // ---- chunks whose last 16-byte run is partly, wholly and just beyond filled, against the real allocation; growth across chunks
    CHECK(chunk_agrees(c, "", kCols, v) == 0);
    CHECK(chunk_agrees(c, "\n", kCols, v) == 0 && chunk_agrees(c, "r\tchr1\t5\tchr2\t6", kCols, v) == 0 && chunk_agrees(c, "#a\n##b\n#c", kCols, v) == 0);
    const std::string body = lines(900, 7);
    for (size_t n : {15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8193})
        CHECK(chunk_agrees(c, body.substr(0, n), kCols, v) == 0);
    CHECK(chunk_agrees(c, body, kCols, v) == 0);                 // more lines and more bytes than any chunk before: both sets of buffers grow
    CHECK(chunk_agrees(c, body.substr(0, 100), kCols, v) == 0);  // a small chunk in the grown buffers: the bytes behind it are the last chunk's
    CHECK(chunk_agrees(c, lines(3000, 8), kCols, v) == 0);
    const int reordered[6] = {3, 4, 1, 2, 6, 5};
    CHECK(chunk_agrees(c, body, reordered, v) == 0);
    // #columns: at the start, in the middle, as the last line without a newline, twice; "#columns" without the colon is a comment
    CHECK(chunk_agrees(c, "#columns: a b\n" + body.substr(0, 500), kCols, v) == 0 && chunk_agrees(c, lines(40, 9) + "#columns: x\n" + lines(40, 10) + "#columns: y\n", kCols, v) == 0);
    CHECK(chunk_agrees(c, lines(20, 11) + "#columns:", kCols, v) == 0 && chunk_agrees(c, lines(20, 11) + "#columns\n" + lines(5, 12) + "x#columns:\n", kCols, v) == 0);
    // the direct form: a workgroup's lines beyond the span, next to staged ones; the span's two sides by the readID's padding
    CHECK(chunk_agrees(c, lines(300, 13) + "r" + std::string(SPAN + 5, 'L') + "\tchr1\t5\tchr2\t6\t-\t-\n" + lines(300, 14), kCols, v) == 0);
    CHECK(chunk_agrees(c, lines(600, 15, 90), kCols, v) == 0 && chunk_agrees(c, lines(600, 15, 140), kCols, v) == 0);
    // the chunks that are Python's
    CHECK(chunk_agrees(c, body.substr(0, 300) + "\r\n", kCols, v) == 0 && chunk_agrees(c, "\xc3\xa9" + body.substr(0, 300), kCols, v) == 0);
    CHECK(chunk_agrees(c, body.substr(0, 17), kCols, v) == 0); // ... and the next chunk is parsed again
    CHECK(ig_text_feed_pre(c, sc, nullptr) != 0 && std::strstr(ig_last_error(), "ig_pre_begin first") && ig_text_feed_pairs(c, sc) != 0 && std::strstr(ig_last_error(), "ig_pairs_begin first"));
    CHECK(ig_text_end(c) == 0 && ig_text_end(c) == 0);

    // ---- every allocation of a session fails once: an error that names hipMalloc, nothing leaked, and the next session works
    {
        const std::string small = lines(50, 16), big = lines(1200, 17);
        const auto session = [&]() -> int {
            (void)ig_text_end(c);
            int64_t s8[8];
            int rc = v.begin(c);
            std::vector<uint8_t> a(small.begin(), small.end()), b(big.begin(), big.end());
            if (!rc) rc = ig_text_parse(c, a.data(), (int64_t)a.size(), kCols, s8, nullptr);
            if (!rc) rc = ig_text_parse(c, b.data(), (int64_t)b.size(), kCols, s8, nullptr); // both sets of buffers grow
            return rc;
        };
        if (allocation_failure_sweep(fx, c, 130, 65, 40, 40, session, [&] { return true; }, [&] { return session() == 0 && chunk_agrees(c, big, kCols, v) == 0; })) return 1;
    }

    // ---- a failed parse in front of ig_destroy; a live session with a parsed chunk in front of ig_destroy
    (void)ig_text_end(c);
    CHECK(v.begin(c) == 0 && chunk_agrees(c, body.substr(0, 200), kCols, v) == 0);
    {
        std::vector<uint8_t> b(body.begin(), body.end());
        CHECK(failed_call_before_destroy(c, 2, [&] { return ig_text_parse(c, b.data(), (int64_t)b.size(), kCols, sc, nullptr); }) != 0);
    }
    CHECK(ig_create(0, &c) == 0 && v.begin(c) == 0 && chunk_agrees(c, body, kCols, v) == 0);
    ig_destroy(c);
    std::printf("text harness ok (%ld launches, %ld allocations)\n", fake_hip::launches(), fake_hip::allocations());
    return 0;
}
