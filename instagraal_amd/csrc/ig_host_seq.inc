/* ig_host_seq.inc -- part of ig_hip.hip (one translation unit; included there in order): the polished FASTA of the polish step
 * (ig_kernels_seq.cuh; the rule: instagraal_amd/scaffold_polish.py; DESIGN.md 4.27).  A session on a created handle with nothing
 * uploaded, like ig_pre_*: the sequence bytes (ig_seq_begin, the layout, the checks, the upload pieces and the memory guard of
 * ig_pre_begin), the composition of the input records (ig_seq_composition), the plan of the output file (ig_seq_plan: every table
 * checked on the host, so that no kernel reads outside a buffer), the file's bytes window by window (ig_seq_window) and the composition
 * of the stitched bodies (ig_seq_out_composition), counted while the windows are stitched in file order. */

#define SEQ_MAX_WIDTH (1 << 30)
#define SEQ_WAVE_TURNS 16 /* consecutive kilobytes a wave of k_seq_stitch walks */

static void seq_free_plan(SeqBuf& s)
{
    hipFree(s.rec_off);
    hipFree(s.hdr_len);
    hipFree(s.hdr_lit);
    hipFree(s.piece_first);
    hipFree(s.p_body);
    hipFree(s.piece);
    hipFree(s.lit);
    hipFree(s.out_counts);
    s.rec_off = s.hdr_lit = s.piece_first = s.p_body = nullptr;
    s.hdr_len = nullptr;
    s.piece = nullptr;
    s.lit = nullptr;
    s.out_counts = nullptr;
    s.planned = false;
    s.n_out = 0, s.width = 0;
    s.n_pieces = s.file_bytes = s.counted = 0;
}

static void free_seq_buffers(ig_ctx* c)
{
    SeqBuf& s = c->seq;
    seq_free_plan(s);
    hipFree(s.base);
    hipFree(s.off);
    hipFree(s.counts);
    hipFree(s.win);
    s = SeqBuf{};
}

static int seq_usable(ig_ctx* c, const char* who)
{
    if (!c->seq.live) return fail("%s: no session (ig_seq_begin first)", who);
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    return 0;
}

extern "C" int ig_seq_begin(ig_ctx* c, const uint8_t* seq, int64_t n_bytes, const int64_t* rec_off, const int32_t* rec_len, int32_t n_records)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_seq_begin";
    SeqBuf& s = c->seq;
    if (s.live) return fail("%s: a session is open (ig_seq_end first)", who);
    if (c->nuis_in_flight || c->chain_busy) return fail("%s: a nuisance step or a chain is in flight", who);
    if (records_layout_check(who, seq, n_bytes, rec_off, rec_len, n_records)) return -1;
    const int R = n_records;
    const long long n_runs = (n_bytes + SEQ_RUN - 1) / SEQ_RUN;
    const unsigned long long padded = (unsigned long long)SEQ_FRONT + (unsigned long long)(n_runs + 1) * SEQ_RUN;
    if (pre_memory_guard(who, padded + (unsigned long long)R * (8 + 8 * SEQ_NC), "the sequence")) return -1;
    const int rc = [&]() -> int {
        DALLOC(s.base, (size_t)padded);
        DALLOC(s.off, (size_t)R);
        DALLOC(s.counts, (size_t)R * SEQ_NC);
        HIPCK(hipMemsetAsync(s.base, 0, SEQ_FRONT, c->stream));
        HIPCK(hipMemsetAsync(s.base + (padded - 2 * SEQ_RUN), 0, 2 * SEQ_RUN, c->stream)); /* (the tail the bytes do not cover) */
        for (long long o = 0; o < n_bytes; o += PRE_UPLOAD_PIECE)
            HIPCK(hipMemcpyAsync(s.base + SEQ_FRONT + o, seq + o, (size_t)std::min<long long>(PRE_UPLOAD_PIECE, n_bytes - o), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(s.off, rec_off, (size_t)R * sizeof(long long), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        return 0;
    }();
    if (rc) {
        free_seq_buffers(c);
        return rc;
    }
    s.h_off.assign(rec_off, rec_off + R);
    s.h_len.assign(rec_len, rec_len + R);
    s.live = true;
    s.R = R, s.n_bytes = n_bytes, s.n_runs = n_runs;
    return 0;
}

/* counts[n_records][SEQ_NC]: A, C, G, T, N of either case, the other letters, the lower-case letters, all bases; ms (may be null): the
 * kernel's time */
extern "C" int ig_seq_composition(ig_ctx* c, int64_t* counts, float* ms)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_seq_composition";
    if (seq_usable(c, who)) return -1;
    if (!counts) return fail("%s: NULL output", who);
    SeqBuf& s = c->seq;
    HIPCK(hipMemsetAsync(s.counts, 0, (size_t)s.R * SEQ_NC * sizeof(unsigned long long), c->stream));
    LiftTimer timer(c, ms, 1);
    timer.begin();
    /* 2048 workgroups walk the sequence, a wave one stretch of it; more of them where a stretch would outgrow the 32-bit sums */
    const long long wave_turns = (s.n_runs + 63) / 64, per_block = SEQ_THREADS / 64;
    const long long blocks = std::max<long long>(std::min<long long>((wave_turns + per_block - 1) / per_block, 2048), (wave_turns + per_block * SEQ_COMP_MAX_TURNS - 1) / (per_block * SEQ_COMP_MAX_TURNS));
    const long long runs_per_wave = (wave_turns + blocks * per_block - 1) / (blocks * per_block);
    hipLaunchKernelGGL(k_seq_composition, dim3((unsigned)blocks), dim3(SEQ_THREADS), 0, c->stream, (const unsigned char*)(s.base + SEQ_FRONT), s.n_runs, (const long long*)s.off,
                       s.R, runs_per_wave, s.counts);
    timer.end(0);
    HIPCK(hipMemcpyAsync(counts, s.counts, (size_t)s.R * SEQ_NC * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    for (int r = 0; r < s.R; r++)
        if (counts[(size_t)r * SEQ_NC + 7] != s.h_len[(size_t)r])
            return fail("%s: %lld letters counted in record %d of %d bases (device error)", who, (long long)counts[(size_t)r * SEQ_NC + 7], r, s.h_len[(size_t)r]);
    return 0;
}

/* The plan of the output file (scaffold_polish.stitch_plan).  Per output record j: its header is literal[hdr_lit[j] .. + hdr_len[j]),
 * its body has body_len[j] bases and its pieces are piece_first[j] .. piece_first[j + 1] - 1; rec_off[n_out + 1]: the file offset of
 * every header, the file's size last.  Per piece: src (an input record, -1: the literal buffer), start (inside it), length (>= 1), ori
 * (1, -1: the reverse complement; a literal piece is never reversed), body (the offset of its first base in its body).  Refused unless
 * every piece lies inside its source, the pieces of a record tile its body without gap or overlap in ascending order, and rec_off[j + 1]
 * == rec_off[j] + hdr_len[j] + L + ceil(L / width).  An earlier plan of the session and its counts are gone. */
extern "C" int ig_seq_plan(ig_ctx* c, int32_t n_out, int32_t width, const int64_t* rec_off, const int32_t* hdr_len, const int64_t* hdr_lit, const int64_t* body_len,
                           const int64_t* piece_first, int64_t n_pieces, const int32_t* src, const int64_t* start, const int64_t* length, const int32_t* ori,
                           const int64_t* body, const uint8_t* literal, int64_t n_literal)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_seq_plan";
    if (seq_usable(c, who)) return -1;
    SeqBuf& s = c->seq;
    seq_free_plan(s);
    if (n_out < 1 || n_pieces < 0 || n_literal < 0) return fail("%s: bad sizes (%d records, %lld pieces, %lld literal bytes)", who, n_out, (long long)n_pieces, (long long)n_literal);
    if (width < 1 || width > SEQ_MAX_WIDTH) return fail("%s: a line has 1 .. 2^30 bases (width %d)", who, width);
    if (!rec_off || !hdr_len || !hdr_lit || !body_len || !piece_first || !literal) return fail("%s: NULL argument", who);
    if (n_pieces > 0 && (!src || !start || !length || !ori || !body)) return fail("%s: NULL argument", who);
    if (rec_off[0] != 0 || piece_first[0] != 0) return fail("%s: the first record starts at byte %lld with piece %lld, not at 0 with 0", who, (long long)rec_off[0], (long long)piece_first[0]);
    std::vector<SeqPiece> pieces((size_t)n_pieces);
    for (int j = 0; j < n_out; j++) {
        const long long L = body_len[j], pf = piece_first[j], pe = piece_first[j + 1];
        if (hdr_len[j] < 1 || hdr_lit[j] < 0 || hdr_lit[j] > n_literal - hdr_len[j])
            return fail("%s: the header of record %d is the literal bytes %lld .. %lld of %lld", who, j, (long long)hdr_lit[j], (long long)hdr_lit[j] + hdr_len[j], (long long)n_literal);
        if (L < 0 || pe < pf || pe > n_pieces) return fail("%s: record %d has %lld bases in the pieces %lld .. %lld of %lld", who, j, L, pf, pe, (long long)n_pieces);
        if (rec_off[j + 1] != rec_off[j] + hdr_len[j] + L + (L + width - 1) / width)
            return fail("%s: record %d at byte %lld with a header of %d and %lld bases in lines of %d ends at %lld, not at %lld (the offsets are not monotone)", who, j,
                        (long long)rec_off[j], hdr_len[j], L, width, (long long)(rec_off[j] + hdr_len[j] + L + (L + width - 1) / width), (long long)rec_off[j + 1]);
        long long at = 0;
        for (long long p = pf; p < pe; p++) {
            if (length[p] < 1 || length[p] > 0x7fffffffll) return fail("%s: piece %lld has %lld bases", who, p, (long long)length[p]);
            if (body[p] != at) return fail("%s: piece %lld of record %d begins at base %lld of the body, the pieces before it end at %lld (a gap or an overlap)", who, p, j, (long long)body[p], at);
            at += length[p];
            const bool lit = src[p] == -1;
            if (!lit && (src[p] < 0 || src[p] >= s.R)) return fail("%s: piece %lld is of record %d of %d", who, p, src[p], s.R);
            const long long room = lit ? (long long)n_literal : (long long)s.h_len[(size_t)src[p]];
            if (start[p] < 0 || start[p] > room - length[p])
                return fail("%s: piece %lld is %lld .. %lld of %s %d, which has %lld", who, p, (long long)start[p], (long long)(start[p] + length[p]), lit ? "the literal buffer" : "record", src[p], room);
            if (ori[p] != 1 && !(ori[p] == -1 && !lit)) return fail("%s: piece %lld has the orientation %d%s", who, p, ori[p], lit ? " (a literal piece is never reversed)" : "");
            pieces[(size_t)p] = SeqPiece{lit ? start[p] : s.h_off[(size_t)src[p]] + start[p], (int)length[p], (lit ? SEQ_PIECE_LITERAL : 0) | (ori[p] < 0 ? SEQ_PIECE_REVERSE : 0)};
        }
        if (at != L) return fail("%s: the pieces of record %d hold %lld bases, its body %lld", who, j, at, L);
    }
    if (piece_first[n_out] != n_pieces) return fail("%s: the records hold %lld pieces of %lld", who, (long long)piece_first[n_out], (long long)n_pieces);
    if (pre_memory_guard(who, (unsigned long long)n_out * (36 + 8 * SEQ_NC) + (unsigned long long)n_pieces * 24 + (unsigned long long)n_literal + 64, "the plan")) return -1;
    const int rc = [&]() -> int {
        DALLOC(s.rec_off, (size_t)n_out + 1);
        DALLOC(s.hdr_len, (size_t)n_out);
        DALLOC(s.hdr_lit, (size_t)n_out);
        DALLOC(s.piece_first, (size_t)n_out + 1);
        DALLOC(s.p_body, (size_t)n_pieces);
        DALLOC(s.piece, (size_t)n_pieces);
        DALLOC(s.lit, (size_t)n_literal);
        DALLOC(s.out_counts, (size_t)n_out * SEQ_NC);
        HIPCK(hipMemcpyAsync(s.rec_off, rec_off, ((size_t)n_out + 1) * sizeof(long long), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(s.hdr_len, hdr_len, (size_t)n_out * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(s.hdr_lit, hdr_lit, (size_t)n_out * sizeof(long long), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(s.piece_first, piece_first, ((size_t)n_out + 1) * sizeof(long long), hipMemcpyHostToDevice, c->stream));
        if (n_pieces) HIPCK(hipMemcpyAsync(s.p_body, body, (size_t)n_pieces * sizeof(long long), hipMemcpyHostToDevice, c->stream));
        if (n_pieces) HIPCK(hipMemcpyAsync(s.piece, pieces.data(), (size_t)n_pieces * sizeof(SeqPiece), hipMemcpyHostToDevice, c->stream));
        if (n_literal) HIPCK(hipMemcpyAsync(s.lit, literal, (size_t)n_literal, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemsetAsync(s.out_counts, 0, (size_t)n_out * SEQ_NC * sizeof(unsigned long long), c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        return 0;
    }();
    if (rc) {
        hipStreamSynchronize(c->stream);
        seq_free_plan(s);
        return rc;
    }
    s.planned = true;
    s.n_out = n_out, s.width = width, s.n_pieces = n_pieces, s.file_bytes = rec_off[n_out], s.counted = 0;
    return 0;
}

/* The file bytes first_byte .. first_byte + n_bytes - 1 into out (host memory).  first_byte is a multiple of 16, and so is n_bytes
 * unless the window ends with the file.  The window that begins where the last counted one ended is counted as it is stitched
 * (ig_seq_out_composition); any other is only stitched.  ms (may be null): the kernel's time. */
extern "C" int ig_seq_window(ig_ctx* c, int64_t first_byte, int64_t n_bytes, uint8_t* out, float* ms)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_seq_window";
    if (seq_usable(c, who)) return -1;
    SeqBuf& s = c->seq;
    if (!s.planned) return fail("%s: no plan (ig_seq_plan first)", who);
    if (!out) return fail("%s: NULL output", who);
    if (first_byte < 0 || n_bytes < 1 || first_byte > s.file_bytes || n_bytes > s.file_bytes - first_byte)
        return fail("%s: the bytes %lld .. %lld of a file of %lld", who, (long long)first_byte, (long long)(first_byte + n_bytes), s.file_bytes);
    if (first_byte % SEQ_RUN || (n_bytes % SEQ_RUN && first_byte + n_bytes != s.file_bytes))
        return fail("%s: a window begins at a multiple of 16 and, unless it ends with the file, holds a multiple of 16 bytes (%lld, %lld)", who, (long long)first_byte, (long long)n_bytes);
    const long long n_runs = (n_bytes + SEQ_RUN - 1) / SEQ_RUN;
    if (n_runs * SEQ_RUN > s.win_cap) {
        if (pre_memory_guard(who, (unsigned long long)n_runs * SEQ_RUN, "the window")) return -1;
        hipFree(s.win);
        s.win = nullptr, s.win_cap = 0;
        DALLOC(s.win, (size_t)n_runs * SEQ_RUN);
        s.win_cap = n_runs * SEQ_RUN;
    }
    const SeqPlan pl = {s.rec_off, s.hdr_len, s.hdr_lit, s.piece_first, s.p_body, s.piece, s.lit, s.file_bytes, s.n_out, s.width};
    const bool count = first_byte == s.counted;
    const long long n_waves = (n_runs + 63) / 64, waves = (n_waves + SEQ_WAVE_TURNS - 1) / SEQ_WAVE_TURNS;
    const dim3 grid((unsigned)((waves + SEQ_THREADS / 64 - 1) / (SEQ_THREADS / 64))), block(SEQ_THREADS);
    LiftTimer timer(c, ms, 1);
    timer.begin();
    if (count) hipLaunchKernelGGL((k_seq_stitch<true>), grid, block, 0, c->stream, (const unsigned char*)(s.base + SEQ_FRONT), pl, (long long)first_byte, n_runs, SEQ_WAVE_TURNS, (uint4*)s.win, s.out_counts);
    else hipLaunchKernelGGL((k_seq_stitch<false>), grid, block, 0, c->stream, (const unsigned char*)(s.base + SEQ_FRONT), pl, (long long)first_byte, n_runs, SEQ_WAVE_TURNS, (uint4*)s.win, s.out_counts);
    timer.end(0);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(out, s.win, (size_t)n_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (count) s.counted = first_byte + n_bytes;
    return 0;
}

/* counts[n_out][SEQ_NC] of the stitched bodies (junctions included, headers and newlines not): every window of the file has gone
 * through ig_seq_window, in file order */
extern "C" int ig_seq_out_composition(ig_ctx* c, int64_t* counts, int64_t n_counts)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    const char* who = "ig_seq_out_composition";
    if (seq_usable(c, who)) return -1;
    SeqBuf& s = c->seq;
    if (!s.planned) return fail("%s: no plan (ig_seq_plan first)", who);
    if (!counts || n_counts < (long long)s.n_out * SEQ_NC) return fail("%s: the result has %lld words, the caller's capacity is %lld", who, (long long)s.n_out * SEQ_NC, (long long)n_counts);
    if (s.counted != s.file_bytes) return fail("%s: the windows stitched in file order end at byte %lld of %lld (ig_seq_window up to the file's end first)", who, s.counted, s.file_bytes);
    HIPCK(hipMemcpyAsync(counts, s.out_counts, (size_t)s.n_out * SEQ_NC * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int ig_seq_end(ig_ctx* c)
{
    IG_JOIN(c);
    HIPCK(hipSetDevice(c->device));
    if (!c->seq.live) return fail("ig_seq_end: no session (ig_seq_begin first)");
    HIPCK(hipStreamSynchronize(c->stream));
    free_seq_buffers(c);
    return 0;
}
