/* ig_host_pre.inc -- part of ig_hip.hip (one translation unit; included there in order): the input folder from an assembly FASTA and
 * read pairs (ig_kernels_pre.cuh; the rule: instagraal_amd/pre.py; DESIGN.md 4.26).  A session on a created handle with nothing
 * uploaded: the sequence bytes (ig_pre_begin), the digest and G+C (ig_pre_digest, ig_pre_fragments), the fragments of the pair ends
 * into a store that grows (ig_pre_add_pairs), the pixels through the row builder (rows_build, ig_host_rows.inc) into the session's own
 * rows (ig_pre_pixels_build, _rows, _fetch). */

/* PreBuf.sc, in 64-bit words */
#define PRE_SC_CURSOR 0
#define PRE_SC_ASSIGN 1
#define PRE_SC_EMIT (PRE_SC_ASSIGN + PRE_NS)
#define PRE_SC_WORDS (PRE_SC_EMIT + 2)
#define PRE_PIECE (1ll << 22)          /* pairs of a chunk that go through the staging arrays at a time */
#define PRE_UPLOAD_PIECE (1ll << 28)   /* sequence bytes per copy */
#define PRE_MAX_STORE 0x7fffffffll
#define PRE_MAX_RECORD 0x7ffffffe      /* pre.MAX_RECORD */
/* the passes ig_pre_digest times, in this order */
#define PRE_P_SITES 0
#define PRE_P_SCAN 1
#define PRE_P_CUTS 2
#define PRE_P_FRAGS 3
#define PRE_DIGEST_PASSES 4

static void pre_free_digest(PreBuf& p)
{
    hipFree(p.rec_first);
    hipFree(p.frag_rec);
    hipFree(p.start);
    hipFree(p.end);
    hipFree(p.gc);
    p.rec_first = nullptr;
    p.frag_rec = p.start = p.end = p.gc = nullptr;
    p.digested = false;
    p.n_frags = 0;
}

static void pre_free_pixels(PreBuf& p)
{
    rows_free(p.rows);
    p.built = false;
    p.n_out = 0;
}

static void free_pre_buffers(ig_ctx* c)
{
    PreBuf& p = c->pre;
    hipFree(p.seq);
    hipFree(p.off);
    hipFree(p.len);
    hipFree(p.store);
    hipFree(p.sc);
    for (int k = 0; k < 4; k++) hipFree(p.in[k]);
    pre_free_digest(p);
    pre_free_pixels(p);
    p = PreBuf{};
}

static int pre_usable(ig_ctx* c, const char* who)
{
    if (!c->pre.live) return fail("%s: no session (ig_pre_begin first)", who);
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    return 0;
}

static int pre_memory_guard(const char* who, unsigned long long bytes, const char* what)
{
    size_t free_b = ~(size_t)0, total_b = 0;
    if (&hipMemGetInfo != nullptr) HIPCK(hipMemGetInfo(&free_b, &total_b));
    if (bytes + (1ull << 20) > (unsigned long long)free_b) return fail("%s: %s needs %llu bytes of device memory, %zu are free", who, what, bytes, free_b);
    return 0;
}

/* the code of a byte on the host (pre.CODE; pre_code in ig_kernels_pre.cuh): 0 is no letter of the alphabet */
static inline bool pre_host_valid(unsigned char b)
{
    const unsigned i = (b & 0x1fu) - 1u;
    return (b & 0xc0u) == 0x40u && i < 26u && ((PRE_LETTERS >> i) & 1u);
}

/* whether each of the eight bytes of w is A, C, G, T or N in either case: per letter, the bytes equal to it get their top bit set
 * (a byte x is zero where ((x & 0x7f) + 0x7f) | x has its top bit clear: no carry leaves a byte) */
static inline bool pre_host_plain8(uint64_t w)
{
    const uint64_t ones = 0x0101010101010101ull, low7 = 0x7f7f7f7f7f7f7f7full, top = 0x8080808080808080ull;
    const uint64_t up = w & ~(0x20ull * ones);
    uint64_t hit = 0;
    for (const unsigned char letter : {'A', 'C', 'G', 'T', 'N'}) {
        const uint64_t x = up ^ (letter * ones);
        hit |= ~(((x & low7) + low7) | x) & top;
    }
    return hit == top;
}

/* the layout ig_pre_begin and ig_seq_begin take, checked before anything is allocated: the records one behind the other with a zero
 * byte behind each, every base a letter of the alphabet */
static int records_layout_check(const char* who, const uint8_t* seq, int64_t n_bytes, const int64_t* rec_off, const int32_t* rec_len, int32_t n_records)
{
    if (n_records < 1 || n_bytes < 2) return fail("%s: bad sizes (%d records, %lld bytes)", who, n_records, (long long)n_bytes);
    if (!seq || !rec_off || !rec_len) return fail("%s: NULL argument", who);
    const int R = n_records;
    long long at = 0;
    for (int r = 0; r < R; r++) {
        if (rec_len[r] < 1) return fail("%s: record %d is empty (length %d)", who, r, rec_len[r]);
        if (rec_len[r] > PRE_MAX_RECORD) return fail("%s: record %d has %d bases: more than 2^31 - 2 (the position 2^31 - 1 lies beyond every record)", who, r, rec_len[r]);
        if (rec_off[r] != at) return fail("%s: record %d starts at %lld, the records before it and their separators end at %lld", who, r, (long long)rec_off[r], at);
        at += (long long)rec_len[r] + 1;
        if (at > n_bytes) return fail("%s: record %d ends at %lld of %lld bytes", who, r, at, (long long)n_bytes);
        if (seq[at - 1] != 0) return fail("%s: the byte behind record %d is %d, not the separator 0", who, r, (int)seq[at - 1]);
    }
    if (at != n_bytes) return fail("%s: the records and their separators are %lld bytes, not %lld", who, at, (long long)n_bytes);
    for (int r = 0; r < R; r++) { /* the rule's refusal of a character outside the alphabet, before anything is allocated */
        long long k = rec_off[r];
        const long long e = rec_off[r] + rec_len[r];
        while (k < e) {
            if (e - k >= 8) { /* eight bytes at a time where all of them are A, C, G, T or N of either case: nearly every word of a genome */
                uint64_t w;
                memcpy(&w, seq + k, 8);
                if (pre_host_plain8(w)) {
                    k += 8;
                    continue;
                }
            }
            if (!pre_host_valid(seq[k])) return fail("%s: record %d, position %lld: the character 0x%02x is not one of ABCDGHKMNRSTVWY", who, r, k - rec_off[r] + 1, (unsigned)seq[k]);
            k++;
        }
    }
    return 0;
}

/* seq: n_bytes bytes, the records one behind the other with a zero byte behind each: rec_off[0] == 0, rec_off[r + 1] == rec_off[r] +
 * rec_len[r] + 1, n_bytes == rec_off[R - 1] + rec_len[R - 1] + 1.  The bytes go to the device in pieces. */
extern "C" int ig_pre_begin(ig_ctx* c, const uint8_t* seq, int64_t n_bytes, const int64_t* rec_off, const int32_t* rec_len, int32_t n_records)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pre_begin";
    PreBuf& p = c->pre;
    if (p.live) return fail("%s: a session is open (ig_pre_end first)", who);
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    if (records_layout_check(who, seq, n_bytes, rec_off, rec_len, n_records)) return -1;
    const int R = n_records;
    const long long n_runs = (n_bytes + PRE_RUN - 1) / PRE_RUN, W = (n_runs + 3) / 4 + 1;
    if (W > 0x7fffffffll) return fail("%s: %lld bytes make %lld bitmap words, more than 2^31 - 1", who, (long long)n_bytes, W);
    const unsigned long long padded = (unsigned long long)(n_runs + 1) * PRE_RUN;
    /* the bytes, and what a digest adds: two bitmaps, their counts and prefix sums (8 bytes a word each) */
    if (pre_memory_guard(who, padded + (unsigned long long)W * 8 * 6 + (unsigned long long)R * 12, "the sequence and its digest")) return -1;
    const int rc = [&]() -> int {
        DALLOC(p.seq, (size_t)padded);
        DALLOC(p.off, (size_t)R);
        DALLOC(p.len, (size_t)R);
        DALLOC(p.sc, (size_t)PRE_SC_WORDS);
        HIPCK(hipMemsetAsync(p.seq + (padded - 2 * PRE_RUN), 0, 2 * PRE_RUN, c->stream)); /* (the tail the bytes do not cover) */
        for (long long o = 0; o < n_bytes; o += PRE_UPLOAD_PIECE)
            HIPCK(hipMemcpyAsync(p.seq + o, seq + o, (size_t)std::min<long long>(PRE_UPLOAD_PIECE, n_bytes - o), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(p.off, rec_off, (size_t)R * sizeof(long long), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(p.len, rec_len, (size_t)R * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemsetAsync(p.sc, 0, PRE_SC_WORDS * sizeof(unsigned long long), c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        return 0;
    }();
    if (rc) {
        free_pre_buffers(c);
        return rc;
    }
    p.live = true;
    p.R = R, p.n_bytes = n_bytes, p.n_runs = n_runs, p.W = W;
    return 0;
}

/* the digest of the session's records under n_enzymes sites: site_len[e] letters, the cut behind cut[e] of them, masks[e][16] (a
 * letter's mask: the bits A 1, C 2, G 4, T 8 it accepts, or 16: any letter).  frags_per_record: [R]; ms (may be null):
 * PRE_DIGEST_PASSES words.  An earlier digest, the store and the pixels of the session are gone. */
static int pre_digest_impl(ig_ctx* c, const char* who, const PreSites& sites, float* ms)
{
    PreBuf& p = c->pre;
    const long long W = p.W;
    unsigned long long *cutbits = nullptr, *gcbits = nullptr, *cnt = nullptr, *incl = nullptr, *tot = nullptr;
    long long* cuts = nullptr;
    const int rc = [&]() -> int {
        DALLOC(cutbits, (size_t)W);
        DALLOC(gcbits, (size_t)W);
        DALLOC(cnt, (size_t)2 * W);
        DALLOC(incl, (size_t)2 * W);
        DALLOC(tot, (size_t)2 * scan_chunks(W));
        LiftTimer timer(c, ms, PRE_DIGEST_PASSES);
        timer.begin();
        HIPCK(hipMemsetAsync(cutbits, 0, (size_t)W * sizeof(unsigned long long), c->stream));
        HIPCK(hipMemsetAsync(gcbits, 0, (size_t)W * sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(k_pre_sites, dim3((unsigned)std::min<long long>((p.n_runs + PRE_THREADS - 1) / PRE_THREADS, 1ll << 20)), dim3(PRE_THREADS), 0, c->stream,
                           (const unsigned char*)p.seq, p.n_runs, sites, cutbits, (unsigned short*)gcbits);
        hipLaunchKernelGGL(k_pre_marks, dim3((unsigned)((p.R + PRE_THREADS - 1) / PRE_THREADS)), dim3(PRE_THREADS), 0, c->stream, (const long long*)p.off, (const int*)p.len,
                           p.R, cutbits);
        timer.end(PRE_P_SITES);
        timer.begin();
        hipLaunchKernelGGL(k_pre_popc, dim3(lift_blocks(W)), dim3(PRE_THREADS), 0, c->stream, (const unsigned long long*)cutbits, (const unsigned long long*)gcbits, W, cnt);
        scan64_enqueue(c, cnt, incl, W, (int)W, 2, tot);
        timer.end(PRE_P_SCAN);
        unsigned long long n_bits = 0;
        HIPCK(hipMemcpyAsync(&n_bits, incl + (W - 1), sizeof(n_bits), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        const long long n_cuts = (long long)n_bits, n_frags = n_cuts - p.R;
        if (n_cuts < 2ll * p.R || n_cuts > p.n_bytes) return fail("%s: %lld cuts of %d records in %lld bytes (device error)", who, n_cuts, p.R, p.n_bytes);
        if (n_frags > 0x7fffffffll) return fail("%s: %lld fragments are more than 2^31 - 1", who, n_frags);
        if (pre_memory_guard(who, (unsigned long long)n_cuts * 8 + (unsigned long long)n_frags * 16 + (unsigned long long)(p.R + 1) * 8, "the fragment table")) return -1;
        DALLOC(cuts, (size_t)n_cuts);
        DALLOC(p.rec_first, (size_t)p.R + 1);
        DALLOC(p.frag_rec, (size_t)n_frags);
        DALLOC(p.start, (size_t)n_frags);
        DALLOC(p.end, (size_t)n_frags);
        DALLOC(p.gc, (size_t)n_frags);
        timer.begin();
        hipLaunchKernelGGL(k_pre_cuts, dim3(lift_blocks(W)), dim3(PRE_THREADS), 0, c->stream, (const unsigned long long*)cutbits, (const unsigned long long*)incl, W, cuts, n_cuts);
        timer.end(PRE_P_CUTS);
        timer.begin();
        HIPCK(hipMemcpyAsync(p.rec_first + p.R, &n_frags, sizeof(long long), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_pre_frags, dim3(lift_blocks(n_cuts)), dim3(PRE_THREADS), 0, c->stream, (const long long*)cuts, n_cuts, (const long long*)p.off, (const int*)p.len,
                           p.R, (const unsigned long long*)gcbits, (const unsigned long long*)(incl + W), n_frags, p.rec_first, p.frag_rec, p.start, p.end, p.gc);
        timer.end(PRE_P_FRAGS);
        p.h_first.assign((size_t)p.R + 1, 0);
        HIPCK(hipMemcpyAsync(p.h_first.data(), p.rec_first, ((size_t)p.R + 1) * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        if (p.h_first[0] != 0 || p.h_first[(size_t)p.R] != n_frags) return fail("%s: the records' first fragments run from %lld to %lld of %lld (device error)", who, p.h_first[0], p.h_first[(size_t)p.R], n_frags);
        for (int r = 0; r < p.R; r++)
            if (p.h_first[(size_t)r + 1] <= p.h_first[(size_t)r]) return fail("%s: record %d has no fragment (device error)", who, r);
        p.n_frags = n_frags;
        return 0;
    }();
    hipStreamSynchronize(c->stream);
    hipFree(cutbits);
    hipFree(gcbits);
    hipFree(cnt);
    hipFree(incl);
    hipFree(tot);
    hipFree(cuts);
    return rc;
}

extern "C" int ig_pre_digest(ig_ctx* c, int32_t n_enzymes, const int32_t* site_len, const int32_t* cut, const uint8_t* masks, int64_t* frags_per_record, int64_t* n_frags,
                             float* ms)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pre_digest";
    if (pre_usable(c, who)) return -1;
    PreBuf& p = c->pre;
    if (n_enzymes < 1 || n_enzymes > PRE_MAX_ENZYMES) return fail("%s: 1 .. %d enzymes (got %d)", who, PRE_MAX_ENZYMES, n_enzymes);
    if (!site_len || !cut || !masks || !frags_per_record || !n_frags) return fail("%s: NULL argument", who);
    PreSites sites = {};
    sites.n = n_enzymes;
    for (int e = 0; e < n_enzymes; e++) {
        if (site_len[e] < 1 || site_len[e] > PRE_MAX_SITE) return fail("%s: the site of enzyme %d has %d letters: 1 .. %d", who, e, site_len[e], PRE_MAX_SITE);
        if (cut[e] < 0 || cut[e] > site_len[e]) return fail("%s: enzyme %d cuts behind %d of %d letters", who, e, cut[e], site_len[e]);
        sites.len[e] = site_len[e], sites.cut[e] = cut[e];
        for (int j = 0; j < site_len[e]; j++) {
            const unsigned m = masks[e * PRE_MAX_SITE + j];
            if (m == 0 || (m != PRE_BIT_VALID && m > 15u)) return fail("%s: enzyme %d, letter %d: the mask 0x%02x is neither a set of A, C, G, T nor 16 (any letter)", who, e, j, m);
            sites.mask[e][j] = (unsigned char)m;
        }
    }
    pre_free_digest(p);
    pre_free_pixels(p);
    p.size = 0;
    for (int k = 0; k < PRE_NS; k++) p.totals[k] = 0;
    if (pre_digest_impl(c, who, sites, ms)) {
        pre_free_digest(p);
        return -1;
    }
    p.digested = true;
    for (int r = 0; r < p.R; r++) frags_per_record[r] = p.h_first[(size_t)r + 1] - p.h_first[(size_t)r];
    *n_frags = p.n_frags;
    return 0;
}

/* the fragments first .. first + n - 1 of the digest: record, start, end (0-based, half-open, inside the record), G + C */
extern "C" int ig_pre_fragments(ig_ctx* c, int64_t first, int64_t n, int32_t* frag_rec, int32_t* start, int32_t* end, int32_t* gc_count)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pre_fragments";
    if (pre_usable(c, who)) return -1;
    PreBuf& p = c->pre;
    if (!p.digested) return fail("%s: nothing is digested (ig_pre_digest first)", who);
    if (first < 0 || n < 0 || first > p.n_frags || n > p.n_frags - first) return fail("%s: fragments %lld .. %lld of %lld", who, (long long)first, (long long)(first + n), p.n_frags);
    if (n > 0 && (!frag_rec || !start || !end || !gc_count)) return fail("%s: NULL output", who);
    if (n == 0) return 0;
    HIPCK(hipMemcpyAsync(frag_rec, p.frag_rec + first, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(start, p.start + first, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(end, p.end + first, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(gc_count, p.gc + first, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return 0;
}

/* room for `need` pairs in all: the array made anew, the stored pairs copied over; a refusal leaves the store as it was */
static int pre_grow_store(ig_ctx* c, const char* who, long long need)
{
    PreBuf& p = c->pre;
    if (need <= p.cap) return 0;
    if (need > PRE_MAX_STORE) return fail("%s: %lld pairs are more than a session stores (2^31 - 1)", who, need);
    const long long cap = std::min<long long>(std::max(need, p.cap + p.cap / 2), PRE_MAX_STORE);
    if (pre_memory_guard(who, (unsigned long long)cap * sizeof(int2), "the store of the pairs")) return -1;
    int2* store = nullptr;
    const int rc = [&]() -> int {
        DALLOC(store, (size_t)cap);
        if (p.size > 0) HIPCK(hipMemcpyAsync(store, p.store, (size_t)p.size * sizeof(int2), hipMemcpyDeviceToDevice, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        return 0;
    }();
    if (rc) {
        hipFree(store);
        return rc;
    }
    hipFree(p.store);
    p.store = store, p.cap = cap;
    return 0;
}

static int pre_reserve_piece(PreBuf& p, long long n)
{
    if (n <= p.piece_cap) return 0;
    for (int k = 0; k < 4; k++) hipFree(p.in[k]), p.in[k] = nullptr;
    p.piece_cap = 0;
    for (int k = 0; k < 4; k++) DALLOC(p.in[k], (size_t)n);
    p.piece_cap = n;
    return 0;
}

/* One chunk of n pairs behind the checks of its arguments: stage(o, m) enqueues the pairs o .. o + m - 1 into the staging arrays (a copy
 * from the host, or ig_text_feed_pre's conversion on the device).  The kept pairs are appended to the store; scalars: the chunk's
 * pairs_in, pairs_kept, end1_without_fragment, end2_without_fragment, ends_beyond_record, then the pairs stored in all, 0, 0.  ms (may
 * be null): the assign kernel's time, summed over the pieces.  An earlier build's pixels are gone. */
template <class Stage>
static int pre_add_impl(ig_ctx* c, const char* who, long long n, int64_t scalars[8], float* ms, Stage stage)
{
    PreBuf& p = c->pre;
    pre_free_pixels(p);
    if (pre_grow_store(c, who, p.size + n)) return -1;
    if (pre_reserve_piece(p, std::min<long long>(std::max<long long>(n, 1), PRE_PIECE))) return -1;
    const long long before = p.size;
    unsigned long long h_sc[PRE_SC_WORDS] = {0};
    h_sc[PRE_SC_CURSOR] = (unsigned long long)before;
    HIPCK(hipMemcpyAsync(p.sc, h_sc, sizeof(h_sc), hipMemcpyHostToDevice, c->stream));
    LiftTimer timer(c, ms, 1);
    for (long long o = 0; o < n; o += PRE_PIECE) {
        const long long m = std::min<long long>(PRE_PIECE, n - o);
        if (stage(o, m)) return -1;
        timer.begin();
        hipLaunchKernelGGL(k_pre_assign, dim3(lift_blocks(m)), dim3(PRE_THREADS), 0, c->stream, (const int*)p.in[0], (const int*)p.in[1], (const int*)p.in[2],
                           (const int*)p.in[3], m, (const long long*)p.rec_first, (const int*)p.len, p.R, (const int*)p.start, p.store, p.sc + PRE_SC_CURSOR,
                           (unsigned long long)p.cap, p.sc + PRE_SC_ASSIGN);
        timer.end(0);
        HIPCK(hipStreamSynchronize(c->stream)); /* (the staging arrays are the next piece's) */
    }
    HIPCK(hipMemcpyAsync(h_sc, p.sc, sizeof(h_sc), hipMemcpyDeviceToHost, c->stream)); /* (on the stream: behind the upload of the words even where no piece ran) */
    HIPCK(hipStreamSynchronize(c->stream));
    const unsigned long long* s = h_sc + PRE_SC_ASSIGN;
    if (s[PRE_IN] != (unsigned long long)n || s[PRE_KEPT] + s[PRE_MISS1] + s[PRE_MISS2] != (unsigned long long)n || s[PRE_BEYOND] > 2ull * (unsigned long long)n ||
        h_sc[PRE_SC_CURSOR] != (unsigned long long)before + s[PRE_KEPT] || h_sc[PRE_SC_CURSOR] > (unsigned long long)p.cap)
        return fail("%s: %llu pairs counted of %lld, %llu kept, the store's cursor at %llu of %lld (device error)", who, s[PRE_IN], (long long)n, s[PRE_KEPT],
                    h_sc[PRE_SC_CURSOR], p.cap);
    p.size = (long long)h_sc[PRE_SC_CURSOR];
    for (int k = 0; k < PRE_NS; k++) {
        scalars[k] = (long long)s[k];
        p.totals[k] += (long long)s[k];
    }
    scalars[5] = p.size;
    scalars[6] = scalars[7] = 0;
    return 0;
}

/* One chunk of pairs from the host: record (-1: unknown) and 1-based position of both ends */
extern "C" int ig_pre_add_pairs(ig_ctx* c, const int32_t* c1, const int32_t* p1, const int32_t* c2, const int32_t* p2, int64_t n, int64_t scalars[8], float* ms)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pre_add_pairs";
    if (pre_usable(c, who)) return -1;
    PreBuf& p = c->pre;
    if (!p.digested) return fail("%s: nothing is digested (ig_pre_digest first)", who);
    if (!scalars) return fail("%s: NULL output", who);
    if (n < 0 || (n > 0 && (!c1 || !p1 || !c2 || !p2))) return fail("%s: bad arguments (%lld pairs)", who, (long long)n);
    const int32_t* in[4] = {c1, p1, c2, p2};
    return pre_add_impl(c, who, n, scalars, ms, [&](long long o, long long m) -> int {
        for (int k = 0; k < 4; k++) HIPCK(hipMemcpyAsync(p.in[k], in[k] + o, (size_t)m * sizeof(int), hipMemcpyHostToDevice, c->stream));
        return 0;
    });
}

/* The pixels of the store: rows_build with the sum of the equal columns, into the session's own rows.  scalars: the six of
 * pre.SCALARS over every chunk since the digest (or ig_pre_clear), then the fragments and the stored pairs.  ms (may be null):
 * LIFT_PASSES words. */
extern "C" int ig_pre_pixels_build(ig_ctx* c, int64_t* n_pixels, int64_t scalars[8], float* ms)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pre_pixels_build";
    if (pre_usable(c, who)) return -1;
    PreBuf& p = c->pre;
    pre_free_pixels(p); /* whatever happens, the result of an earlier build is gone */
    if (!p.digested) return fail("%s: nothing is digested (ig_pre_digest first)", who);
    if (!n_pixels || !scalars) return fail("%s: NULL output", who);
    const int U = (int)p.n_frags;
    const long long S = p.size;
    const int rc = [&]() -> int {
        unsigned long long* d_sc = p.sc + PRE_SC_EMIT;
        HIPCK(hipMemsetAsync(d_sc, 0, 2 * sizeof(unsigned long long), c->stream));
        auto emit = [&](bool scatter, unsigned long long* slots, unsigned long long* ent, unsigned long long n_ent) {
            if (S == 0) return; /* an empty store: nothing to launch, the rows stay empty */
            const dim3 grid(lift_blocks(S)), block(PRE_THREADS);
            if (!scatter) hipLaunchKernelGGL((k_pre_emit<false>), grid, block, 0, c->stream, (const int2*)p.store, S, U, slots, ent, n_ent, d_sc);
            else hipLaunchKernelGGL((k_pre_emit<true>), grid, block, 0, c->stream, (const int2*)p.store, S, U, slots, ent, n_ent, d_sc);
        };
        auto check = [&](long long E) { return E != S ? fail("%s: %lld entries of %lld stored pairs (a fragment outside 0 .. %d: device error)", who, E, S, U - 1) : 0; };
        /* per entry: the word, the long rows' scratch and their runs' items (8 bytes each), a bit, a summed entry (12 bytes) */
        const RowsSpec spec = {d_sc, 2, 0, 37, " (the pixels' temporaries: fewer pairs per session)", true, {LIFT_P_COUNT, LIFT_P_SCAN, LIFT_P_SCATTER, LIFT_P_SORT_SHORT, LIFT_P_REDUCE}};
        LiftTimer timer(c, ms, LIFT_PASSES);
        unsigned long long h_sc[2];
        long long E = 0, n_out = 0;
        if (rows_build(c, who, p.rows, U, spec, h_sc, check, emit, timer, p.forms, &E, &n_out)) return -1;
        HIPCK(hipStreamSynchronize(c->stream));
        p.n_out = n_out;
        return 0;
    }();
    hipStreamSynchronize(c->stream);
    rows_free_temp(p.rows);
    if (rc) {
        pre_free_pixels(p);
        return rc;
    }
    p.built = true;
    const long long sc[8] = {p.totals[PRE_IN], p.totals[PRE_KEPT], p.totals[PRE_MISS1], p.totals[PRE_MISS2], p.totals[PRE_BEYOND], p.n_out, p.n_frags, S};
    for (int k = 0; k < 8; k++) scalars[k] = sc[k];
    *n_pixels = p.n_out;
    return 0;
}

/* rowptr[n_frags + 1] of the built pixels (n_rowptr: the caller's capacity) */
extern "C" int ig_pre_pixels_rows(ig_ctx* c, int64_t* rowptr, int64_t n_rowptr)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pre_pixels_rows";
    if (pre_usable(c, who)) return -1;
    PreBuf& p = c->pre;
    if (!p.built) return fail("%s: nothing is built (ig_pre_pixels_build first)", who);
    if (!rowptr || n_rowptr < p.n_frags + 1) return fail("%s: the result has %lld row words, the caller's capacity is %lld", who, p.n_frags + 1, (long long)n_rowptr);
    HIPCK(hipMemcpy(rowptr, p.rows.rowptr, ((size_t)p.n_frags + 1) * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}

/* the pixels first .. first + n - 1 of the built result, in the order of (bin1, bin2): bin2 and the count */
extern "C" int ig_pre_pixels_fetch(ig_ctx* c, int64_t first, int64_t n, int32_t* col, int64_t* count)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_pre_pixels_fetch";
    if (pre_usable(c, who)) return -1;
    PreBuf& p = c->pre;
    if (!p.built) return fail("%s: nothing is built (ig_pre_pixels_build first)", who);
    if (first < 0 || n < 0 || first > p.n_out || n > p.n_out - first) return fail("%s: pixels %lld .. %lld of %lld", who, (long long)first, (long long)(first + n), p.n_out);
    if (n > 0 && (!col || !count)) return fail("%s: NULL output", who);
    if (n == 0) return 0;
    HIPCK(hipMemcpy(col, p.rows.out_col + first, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(count, p.rows.out_cnt + first, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}

/* empties the store and its scalars, drops the pixels: the sequence, the digest and the buffers stay */
extern "C" int ig_pre_clear(ig_ctx* c)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->pre.live) return fail("ig_pre_clear: no session (ig_pre_begin first)");
    HIPCK(hipStreamSynchronize(c->stream));
    PreBuf& p = c->pre;
    p.size = 0;
    for (int k = 0; k < PRE_NS; k++) p.totals[k] = 0;
    pre_free_pixels(p);
    return 0;
}

extern "C" int ig_pre_end(ig_ctx* c)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->pre.live) return fail("ig_pre_end: no session (ig_pre_begin first)");
    HIPCK(hipStreamSynchronize(c->stream));
    free_pre_buffers(c);
    return 0;
}
