/* ig_host_text.inc -- part of ig_hip.hip (one translation unit; included there in order): 4DN pairs text on the device
 * (ig_kernels_text.cuh; the rule: instagraal_amd/pairs_text.py; DESIGN.md 4.30).  A session on a created handle with nothing uploaded:
 * the vocabulary and its table (ig_text_begin), one chunk of bytes at a time through the four passes mark, scan, parse, compact
 * (ig_text_parse), its result to the host (ig_text_fetch) or straight into the live pre store or pairs session (ig_text_feed_pre,
 * ig_text_feed_pairs: pre_add_impl of ig_host_pre.inc, pairs_lift_staged of ig_host_pairs.inc). */

#define TEXT_UPLOAD_PIECE (1ll << 28) /* bytes per copy */
/* the passes ig_text_parse times, in this order */
#define TEXT_P_MARK 0
#define TEXT_P_SCAN 1
#define TEXT_P_PARSE 2
#define TEXT_P_COMPACT 3
#define TEXT_PASSES 4
/* per line: line_start, status, the raw and the compacted fields (4 + 8 + 4 + 8 + 1 each), a deferred index; per 256 lines six words */
#define TEXT_LINE_BYTES (4 + 1 + 2 * 25 + 4 + 1)

static void text_free_bytes(TextBuf& t)
{
    hipFree(t.bytes);
    hipFree(t.nl_bits);
    hipFree(t.blk);
    hipFree(t.blk_incl);
    hipFree(t.tot);
    t.bytes = nullptr, t.nl_bits = nullptr, t.blk = t.blk_incl = t.tot = nullptr, t.bytes_cap = 0;
}

static void text_free_lines(TextBuf& t)
{
    hipFree(t.line_start);
    hipFree(t.status);
    hipFree(t.deferred);
    hipFree(t.raw_s);
    hipFree(t.out_s);
    hipFree(t.lblk);
    hipFree(t.lblk_incl);
    hipFree(t.ltot);
    for (int k = 0; k < 2; k++) {
        hipFree(t.raw_c[k]), hipFree(t.out_c[k]), hipFree(t.raw_p[k]), hipFree(t.out_p[k]);
        t.raw_c[k] = t.out_c[k] = nullptr, t.raw_p[k] = t.out_p[k] = nullptr;
    }
    t.line_start = t.deferred = nullptr, t.status = t.raw_s = t.out_s = nullptr, t.lblk = t.lblk_incl = t.ltot = nullptr, t.line_cap = 0;
}

static void free_text_buffers(ig_ctx* c)
{
    TextBuf& t = c->text;
    hipFree(t.names);
    hipFree(t.name_off);
    hipFree(t.name_id);
    hipFree(t.table);
    hipFree(t.sc);
    text_free_bytes(t);
    text_free_lines(t);
    t = TextBuf{};
}

static int text_usable(ig_ctx* c, const char* who)
{
    if (!c->text.live) return fail("%s: no session (ig_text_begin first)", who);
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    return 0;
}

static inline unsigned long long text_hash(const uint8_t* b, long long n)
{
    unsigned long long h = TEXT_FNV_BASIS;
    for (long long i = 0; i < n; i++) h = (h ^ (unsigned long long)b[i]) * TEXT_FNV_PRIME;
    return h;
}

static inline long long text_byte_blocks(long long n_bytes) { return (n_bytes + TEXT_BLOCK_BYTES - 1) / TEXT_BLOCK_BYTES; }
static inline long long text_line_blocks(long long n_lines) { return (n_lines + TEXT_LINES - 1) / TEXT_LINES; }

/* grow-only: a buffer too small is freed and made anew (its contents are the last chunk's: nothing to keep).  The bytes are allocated
 * to a multiple of 16, plus 16: k_text_mark's two 16-byte loads of the last run stay inside */
static int text_reserve_bytes(TextBuf& t, long long n_bytes)
{
    const long long cap = ((n_bytes + 15) / 16) * 16 + 16;
    if (cap <= t.bytes_cap) return 0;
    text_free_bytes(t);
    const long long nb = text_byte_blocks(cap);
    DALLOC(t.bytes, (size_t)cap);
    DALLOC(t.nl_bits, (size_t)(cap / 16));
    DALLOC(t.blk, (size_t)nb);
    DALLOC(t.blk_incl, (size_t)nb);
    DALLOC(t.tot, (size_t)scan_chunks(nb));
    t.bytes_cap = cap;
    return 0;
}

static int text_reserve_lines(TextBuf& t, long long n_lines)
{
    if (n_lines <= t.line_cap) return 0;
    text_free_lines(t);
    const size_t n = (size_t)n_lines, nb = (size_t)text_line_blocks(n_lines);
    DALLOC(t.line_start, n + 1);
    DALLOC(t.status, n);
    DALLOC(t.deferred, n);
    DALLOC(t.raw_s, n);
    DALLOC(t.out_s, n);
    for (int k = 0; k < 2; k++) {
        DALLOC(t.raw_c[k], n);
        DALLOC(t.out_c[k], n);
        DALLOC(t.raw_p[k], n);
        DALLOC(t.out_p[k], n);
    }
    DALLOC(t.lblk, 2 * nb);
    DALLOC(t.lblk_incl, 2 * nb);
    DALLOC(t.ltot, (size_t)2 * scan_chunks((long long)nb));
    t.line_cap = n_lines;
    return 0;
}

/* name k is name_bytes[name_off[k] .. name_off[k + 1]) with the id name_id[k].  Where a name stands twice the later id wins, as a dict
 * does: resolved here, before the table is built. */
extern "C" int ig_text_begin(ig_ctx* c, const uint8_t* name_bytes, const int64_t* name_off, const int32_t* name_id, int32_t n_names)
{
    if (!c) return fail("ig_text_begin: NULL handle");
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_text_begin";
    TextBuf& t = c->text;
    if (t.live) return fail("%s: a session is open (ig_text_end first)", who);
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    if (n_names < 0 || n_names > (1 << 28)) return fail("%s: 0 .. 2^28 names (got %d)", who, n_names);
    if (!name_off || (n_names > 0 && !name_id)) return fail("%s: NULL argument", who);
    const int n = n_names;
    if (name_off[0] != 0) return fail("%s: name_off starts at 0 (got %lld)", who, (long long)name_off[0]);
    for (int k = 0; k < n; k++)
        if (name_off[k + 1] < name_off[k]) return fail("%s: name_off decreases behind name %d", who, k);
    const long long total = name_off[n];
    if (total > 0 && !name_bytes) return fail("%s: NULL argument", who);
    unsigned slots = 2;
    while ((unsigned long long)slots < 2ull * (unsigned long long)n) slots <<= 1; /* load <= 0.5 */
    std::vector<int> table((size_t)slots, -1), ids(name_id, name_id + n);
    for (int k = 0; k < n; k++) {
        const uint8_t* b = name_bytes + name_off[k];
        const long long len = name_off[k + 1] - name_off[k];
        for (unsigned slot = (unsigned)text_hash(b, len) & (slots - 1);; slot = (slot + 1) & (slots - 1)) {
            const int q = table[slot];
            if (q < 0) {
                table[slot] = k;
                break;
            }
            if (name_off[q + 1] - name_off[q] == len && (len == 0 || memcmp(name_bytes + name_off[q], b, (size_t)len) == 0)) {
                ids[(size_t)q] = name_id[k]; /* the same name again: the later id wins */
                break;
            }
        }
    }
    const int rc = [&]() -> int {
        DALLOC(t.names, (size_t)total);
        DALLOC(t.name_off, (size_t)n + 1);
        DALLOC(t.name_id, (size_t)n);
        DALLOC(t.table, (size_t)slots);
        DALLOC(t.sc, (size_t)TEXT_SC_WORDS);
        if (total > 0) HIPCK(hipMemcpyAsync(t.names, name_bytes, (size_t)total, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(t.name_off, name_off, ((size_t)n + 1) * sizeof(long long), hipMemcpyHostToDevice, c->stream));
        if (n > 0) HIPCK(hipMemcpyAsync(t.name_id, ids.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(t.table, table.data(), (size_t)slots * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        return 0;
    }();
    if (rc) {
        free_text_buffers(c);
        return rc;
    }
    t.live = true;
    t.n_names = n, t.table_mask = slots - 1;
    return 0;
}

static inline TextRaw text_raw(TextBuf& t) { return TextRaw{t.raw_c[0], t.raw_c[1], t.raw_p[0], t.raw_p[1], t.raw_s}; }
static inline TextRaw text_out(TextBuf& t) { return TextRaw{t.out_c[0], t.out_c[1], t.out_p[0], t.out_p[1], t.out_s}; }

/* the four passes over a chunk of n_bytes >= 1; sc: the eight scalars */
static int text_parse_impl(ig_ctx* c, const char* who, const uint8_t* bytes, long long n_bytes, const TextCols& cols, long long sc[8], float* ms)
{
    TextBuf& t = c->text;
    if (pre_memory_guard(who, (unsigned long long)n_bytes + (unsigned long long)n_bytes / 8 + 64, "the chunk (a smaller chunk)")) return -1;
    if (text_reserve_bytes(t, n_bytes)) return -1;
    const long long nb = text_byte_blocks(n_bytes);
    LiftTimer timer(c, ms, TEXT_PASSES);
    unsigned h_sc[TEXT_SC_WORDS] = {0u, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u, 0u};
    HIPCK(hipMemcpyAsync(t.sc, h_sc, sizeof(h_sc), hipMemcpyHostToDevice, c->stream));
    for (long long o = 0; o < n_bytes; o += TEXT_UPLOAD_PIECE)
        HIPCK(hipMemcpyAsync(t.bytes + o, bytes + o, (size_t)std::min<long long>(TEXT_UPLOAD_PIECE, n_bytes - o), hipMemcpyHostToDevice, c->stream));
    timer.begin();
    hipLaunchKernelGGL(k_text_mark, dim3((unsigned)nb), dim3(TEXT_THREADS), 0, c->stream, (const unsigned char*)t.bytes, (unsigned)n_bytes, t.nl_bits, t.blk, t.sc);
    timer.end(TEXT_P_MARK);
    timer.begin();
    scan64_enqueue(c, t.blk, t.blk_incl, nb, (int)nb, 1, t.tot);
    unsigned long long n_newlines = 0;
    HIPCK(hipMemcpyAsync(&n_newlines, t.blk_incl + (nb - 1), sizeof(n_newlines), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(h_sc, t.sc, sizeof(h_sc), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (n_newlines > (unsigned long long)n_bytes) return fail("%s: %llu newlines in %lld bytes (device error)", who, n_newlines, n_bytes);
    if (h_sc[TEXT_SC_TO_HOST]) { /* a '\r' or a byte >= 0x80: the chunk is Python's, nothing else of the result is defined */
        timer.end(TEXT_P_SCAN);
        t.to_host = true;
        sc[6] = 1;
        return 0;
    }
    const long long n_lines = (long long)n_newlines + (bytes[n_bytes - 1] != '\n' ? 1 : 0), nlb = text_line_blocks(n_lines);
    if (pre_memory_guard(who, (unsigned long long)n_lines * TEXT_LINE_BYTES, "the lines of the chunk (a smaller chunk)")) return -1;
    if (text_reserve_lines(t, n_lines)) return -1;
    hipLaunchKernelGGL(k_text_lines, dim3((unsigned)nb), dim3(TEXT_THREADS), 0, c->stream, (const unsigned short*)t.nl_bits, (unsigned)n_bytes,
                       (const unsigned long long*)t.blk_incl, t.line_start, (unsigned)n_lines);
    timer.end(TEXT_P_SCAN);
    const TextNames names = {t.names, t.name_off, t.name_id, t.table, t.table_mask};
    timer.begin();
    hipLaunchKernelGGL(k_text_parse, dim3((unsigned)nlb), dim3(TEXT_THREADS), 0, c->stream, (const unsigned char*)t.bytes, (unsigned)n_bytes, (const int*)t.line_start,
                       (unsigned)n_lines, cols, names, t.status, text_raw(t), t.lblk, (unsigned)nlb, t.sc);
    timer.end(TEXT_P_PARSE);
    timer.begin();
    scan64_enqueue(c, t.lblk, t.lblk_incl, nlb, (int)nlb, 2, t.ltot);
    HIPCK(hipMemcpyAsync(h_sc, t.sc, sizeof(h_sc), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    const long long first_cols = h_sc[TEXT_SC_COLS_LINE] == 0xffffffffu ? -1 : (long long)h_sc[TEXT_SC_COLS_LINE];
    const unsigned* count = h_sc + TEXT_SC_COUNT;
    const long long counted = (long long)count[TEXT_DATA] + count[TEXT_COMMENT] + count[TEXT_MALFORMED] + count[TEXT_DEFERRED];
    if ((h_sc[TEXT_SC_COLS_OFF] == 0xffffffffu) != (first_cols < 0) || first_cols >= n_lines || counted != (first_cols < 0 ? n_lines : first_cols))
        return fail("%s: %lld lines counted of %lld, the first #columns: line is %lld (device error)", who, counted, n_lines, first_cols);
    hipLaunchKernelGGL(k_text_compact, dim3((unsigned)nlb), dim3(TEXT_THREADS), 0, c->stream, (const unsigned char*)t.status, (unsigned)n_lines, h_sc[TEXT_SC_COLS_LINE],
                       text_raw(t), (const unsigned long long*)t.lblk_incl, (unsigned)nlb, text_out(t), count[TEXT_DATA], t.deferred, count[TEXT_DEFERRED]);
    timer.end(TEXT_P_COMPACT);
    HIPCK(hipStreamSynchronize(c->stream));
    t.n_lines = n_lines, t.n_data = count[TEXT_DATA], t.n_deferred = count[TEXT_DEFERRED];
    sc[0] = n_lines, sc[1] = count[TEXT_DATA], sc[2] = count[TEXT_COMMENT], sc[3] = count[TEXT_MALFORMED], sc[4] = count[TEXT_DEFERRED], sc[5] = first_cols;
    return 0;
}

/* One chunk of whole lines, 0 <= n_bytes <= 2^30.  cols: the six column indices of read_pairs (chr1, pos1, chr2, pos2, strand1,
 * strand2).  scalars: {lines, data, comment, malformed, deferred, first_columns_line (-1: none), to_host, 0}; with to_host nothing else
 * of the result is defined.  ms (may be null): the four passes {mark, scan, parse, compact}. */
extern "C" int ig_text_parse(ig_ctx* c, const uint8_t* bytes, int64_t n_bytes, const int32_t cols[6], int64_t scalars[8], float* ms)
{
    if (!c) return fail("ig_text_parse: NULL handle");
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_text_parse";
    if (text_usable(c, who)) return -1;
    TextBuf& t = c->text;
    t.parsed = false;
    if (!scalars || !cols) return fail("%s: NULL argument", who);
    if (n_bytes < 0 || n_bytes > TEXT_MAX_BYTES) return fail("%s: a chunk has 0 .. 2^30 bytes (got %lld)", who, (long long)n_bytes); /* (before anything is allocated by it) */
    if (n_bytes > 0 && !bytes) return fail("%s: NULL argument", who);
    TextCols tc = {};
    for (int k = 0; k < 6; k++) {
        if (cols[k] < 0 || cols[k] > 0xffff) return fail("%s: column %d is %d: 0 .. 65535", who, k, cols[k]);
        tc.c[k] = cols[k];
        tc.last = std::max(tc.last, cols[k]);
        if (k < 4) tc.need = std::max(tc.need, cols[k] + 1);
    }
    long long sc[8] = {0, 0, 0, 0, 0, -1, 0, 0};
    t.to_host = false, t.n_bytes = n_bytes, t.n_lines = t.n_data = t.n_deferred = 0;
    if (ms)
        for (int k = 0; k < TEXT_PASSES; k++) ms[k] = 0.0f;
    if (n_bytes > 0 && text_parse_impl(c, who, bytes, n_bytes, tc, sc, ms)) {
        hipStreamSynchronize(c->stream);
        return -1;
    }
    t.parsed = true;
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    return 0;
}

static int text_result(ig_ctx* c, const char* who)
{
    if (text_usable(c, who)) return -1;
    if (!c->text.parsed) return fail("%s: nothing is parsed (ig_text_parse first)", who);
    if (c->text.to_host) return fail("%s: the last chunk was refused (to_host): it has no result", who);
    return 0;
}

/* the last chunk's result: status [lines], line_start [lines + 1], the five arrays of the DATA lines [data], the indices of the
 * DEFERRED lines [deferred]; any pointer may be NULL */
extern "C" int ig_text_fetch(ig_ctx* c, uint8_t* status, int32_t* line_start, int32_t* c1, int64_t* p1, int32_t* c2, int64_t* p2, uint8_t* strands, int32_t* deferred)
{
    if (!c) return fail("ig_text_fetch: NULL handle");
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_text_fetch";
    if (text_result(c, who)) return -1;
    TextBuf& t = c->text;
    if (t.n_lines == 0) { /* (a chunk of 0 bytes: nothing is on the device) */
        if (line_start) line_start[0] = 0;
        return 0;
    }
    const size_t L = (size_t)t.n_lines, D = (size_t)t.n_data, F = (size_t)t.n_deferred;
    if (status) HIPCK(hipMemcpyAsync(status, t.status, L, hipMemcpyDeviceToHost, c->stream));
    if (line_start) HIPCK(hipMemcpyAsync(line_start, t.line_start, (L + 1) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (c1 && D) HIPCK(hipMemcpyAsync(c1, t.out_c[0], D * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (p1 && D) HIPCK(hipMemcpyAsync(p1, t.out_p[0], D * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    if (c2 && D) HIPCK(hipMemcpyAsync(c2, t.out_c[1], D * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (p2 && D) HIPCK(hipMemcpyAsync(p2, t.out_p[1], D * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    if (strands && D) HIPCK(hipMemcpyAsync(strands, t.out_s, D, hipMemcpyDeviceToHost, c->stream));
    if (deferred && F) HIPCK(hipMemcpyAsync(deferred, t.deferred, F * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return 0;
}

/* The DATA pairs of the last chunk into the live pre store, as ig_pre_add_pairs takes them from pre.run_pre: the positions clipped to
 * 0 .. 2^31 - 1 on the device.  scalars, ms: ig_pre_add_pairs'. */
extern "C" int ig_text_feed_pre(ig_ctx* c, int64_t scalars[8], float* ms)
{
    if (!c) return fail("ig_text_feed_pre: NULL handle");
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_text_feed_pre";
    if (text_result(c, who)) return -1;
    if (pre_usable(c, who)) return -1;
    PreBuf& p = c->pre;
    TextBuf& t = c->text;
    if (!p.digested) return fail("%s: nothing is digested (ig_pre_digest first)", who);
    if (!scalars) return fail("%s: NULL output", who);
    return pre_add_impl(c, who, t.n_data, scalars, ms, [&](long long o, long long m) -> int {
        hipLaunchKernelGGL(k_text_convert, dim3(lift_blocks(m)), dim3(TEXT_THREADS), 0, c->stream, text_out(t), o, m, TEXT_FEED_PRE, p.in[0], p.in[1], p.in[2], p.in[3],
                           (unsigned char*)nullptr);
        return 0;
    });
}

/* The DATA pairs of the last chunk into the live pairs session, as ig_pairs_lift takes them from Context.pairs_lift without outputs: a
 * position outside 1 .. 2^31 - 1 as 0, a negative id as -1, with the strand codes.  scalars: ig_pairs_lift's. */
extern "C" int ig_text_feed_pairs(ig_ctx* c, int64_t scalars[8])
{
    if (!c) return fail("ig_text_feed_pairs: NULL handle");
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_text_feed_pairs";
    if (!scalars) return fail("%s: NULL output", who);
    if (text_result(c, who)) return -1;
    if (pairs_usable(c, who)) return -1;
    PairsBuf& p = c->pairs;
    TextBuf& t = c->text;
    int32_t* const no_i[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint8_t* const no_b[3] = {nullptr, nullptr, nullptr};
    long long sc[8];
    LiftTimer timer(c, nullptr, PAIRS_PASSES);
    const int rc = pairs_lift_staged(c, who, true, t.n_data, [&](long long o, long long m) -> int {
        hipLaunchKernelGGL(k_text_convert, dim3(lift_blocks(m)), dim3(TEXT_THREADS), 0, c->stream, text_out(t), o, m, TEXT_FEED_PAIRS, p.in[0], p.in[1], p.in[2], p.in[3],
                           p.in_strands);
        return 0;
    }, no_i, no_b, sc, timer);
    if (rc) return rc;
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    return 0;
}

/* ends the session; without one there is nothing to do */
extern "C" int ig_text_end(ig_ctx* c)
{
    if (!c) return fail("ig_text_end: NULL handle");
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->text.live) return 0;
    HIPCK(hipStreamSynchronize(c->stream));
    free_text_buffers(c);
    return 0;
}
