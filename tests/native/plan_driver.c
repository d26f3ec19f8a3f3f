/* plan_driver.c -- stand-alone driver of the device planner's host-visible
 * code for the sanitizer build (make -C somatic-sniper_amd sanitize ->
 * build/san/plan-asan): the shared core (csrc/ss_plan_core.h, the code the GPU
 * kernels run), its CPU twin ss_pileup_split_cpu and ss_bam_header_scan
 * (csrc/ss_pileup_plan.c).
 *
 *   plan-asan corpus.bin
 *
 * corpus.bin (tests/plan_cases.py write_corpus): u32 n_spans, per span u32
 * chunk, i32 n_ref, u64 len + the bytes; then u32 n_headers, per header u64
 * len + whole uncompressed BAM bytes, i32 n_ref, u64 records_at.  Every input
 * gets a heap block of exactly its length, so a read outside it is an ASan
 * report; UBSan watches the loads, shifts and arithmetic.
 *
 * Per span: the twin at the span's chunk size, at 64 bytes and at
 * SS_PLAN_CHUNK against a plain walk; the guess rule at every offset; and the
 * device's plan (the records' scan elements, the two scans joined in blocks of
 * three so that the join's associativity is used, the rules, the ranks and
 * the closing step -- all functions of the core) against ss_pileup_plan, for
 * several masks, thresholds, capacities and in-states.  Prints
 * "ok=1 spans=N headers=M" and exits 0 when everything matched. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sniper_amd.h"
#include "ss_plan_core.h"

static int rd(FILE *f, void *p, size_t n) { return n && fread(p, 1, n, f) != n ? -1 : 0; }

static void *exact(size_t n)
{
    void *p = malloc(n ? n : 1);
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    return p;
}

static int fail(const char *what, uint32_t i, long a, long b)
{
    fprintf(stderr, "span/header %u: %s (%ld vs %ld)\n", i, what, a, b);
    return 0;
}

/* the plain walk: offsets (cap entries), their count, the end and whether a block_size < 32 ended it */
static uint64_t plain_walk(const uint8_t *b, uint64_t len, uint64_t *off, uint64_t *end_at, int *bad)
{
    uint64_t at = 0, n = 0;
    *bad = 0;
    while (len - at >= 4) {
        const int32_t block = (int32_t)ssp_le32(b + at);
        if (block < 32) { *bad = 1; break; }
        if (len - at - 4 < (uint64_t)block) break;
        off[n++] = at;
        at += 4 + (uint64_t)block;
    }
    *end_at = at;
    return n;
}

static int check_twin(uint32_t i, const uint8_t *b, uint64_t len, int32_t n_ref, uint32_t chunk, const uint64_t *want,
                      uint64_t n_want, uint64_t want_end, int want_bad)
{
    uint64_t *off = (uint64_t *)exact(sizeof(uint64_t) * n_want);
    uint64_t n = 0, end_at = 0;
    int why = 0, ok = 1;
    uint32_t rep = 0;
    const int rc = ss_pileup_split_cpu(b, len, n_ref, chunk, off, n_want, &n, &end_at, &why, &rep);
    if (rc != SS_OK) ok = fail("twin return code", i, rc, 0);
    else if (n != n_want) ok = fail("twin record count", i, (long)n, (long)n_want);
    else if (memcmp(off, want, sizeof(uint64_t) * n_want)) ok = fail("twin offsets", i, chunk, 0);
    else if (end_at != want_end) ok = fail("twin end", i, (long)end_at, (long)want_end);
    else if (why != (want_bad ? SS_PLAN_END_BLOCK : SS_PLAN_END_DATA)) ok = fail("twin end reason", i, why, want_bad);
    else if (rep > (len + chunk - 1) / chunk) ok = fail("twin repairs", i, rep, 0);
    if (ok && n_want) {                       /* one too small: the count, and nothing past the capacity */
        uint64_t *few = (uint64_t *)exact(sizeof(uint64_t) * (n_want - 1));
        if (ss_pileup_split_cpu(b, len, n_ref, chunk, few, n_want - 1, &n, &end_at, &why, &rep) != SS_E_CAPACITY ||
            n != n_want)
            ok = fail("twin capacity", i, (long)n, (long)n_want);
        free(few);
    }
    free(off);
    return ok;
}

/* the device's plan on the host, from the records' offsets */
static int model_plan(const uint8_t *b, const uint64_t *off, uint32_t R, uint64_t chain_end, int chain_bad, int mask,
                      int thresh, const ss_pileup_state_t *in, uint32_t cap, uint64_t *o_off, int32_t *o_from,
                      int32_t *o_tid, ssp_plan_res_t *res)
{
    const uint32_t flag_mask = mask < 0 ? (4u | 256u | 512u | 1024u) : (4u | (uint32_t)mask);
    const int mapq_thresh = thresh < 0 ? 0 : thresh;
    const int32_t t0 = in->has_prev ? in->tid : 0, max0 = in->has_prev ? in->max_tid : -1;
    const int64_t w0 = in->has_prev ? in->w : 0;
    memset(res, 0, sizeof *res);
    res->tid = t0;
    res->w = w0;
    res->max_tid = max0;
    res->first_err = res->cut = SSP_NO_RECORD;
    if (!cap || !R) {
        res->consumed = cap ? chain_end : 0;
        res->code = cap && chain_bad ? -1 : 0;
        return 0;
    }
    int32_t *tid = (int32_t *)exact(4 * (size_t)R), *beg = (int32_t *)exact(4 * (size_t)R);
    int32_t *end = (int32_t *)exact(4 * (size_t)R), *maxt = (int32_t *)exact(4 * (size_t)R);
    int32_t *from = (int32_t *)exact(4 * (size_t)R);
    uint32_t *fl = (uint32_t *)exact(4 * (size_t)R), *rank = (uint32_t *)exact(4 * ((size_t)R + 1));
    ssp_seg_t *seg = (ssp_seg_t *)exact(sizeof(ssp_seg_t) * R);
    for (uint32_t i = 0; i < R; ++i) {
        fl[i] = ssp_plan_record(b + off[i], flag_mask, mapq_thresh, &tid[i], &beg[i], &end[i]);
        seg[i] = ssp_seg_of(fl[i], tid[i], beg[i]);
        maxt[i] = ssp_maxt_of(fl[i], tid[i]);
    }
    /* inclusive scans, joined in blocks of three: block sums first, then the prefix into each block */
    ssp_seg_t carry = ssp_seg_none();
    for (uint32_t a = 0; a < R; a += 3) {
        ssp_seg_t local = ssp_seg_none();
        const uint32_t e = a + 3 < R ? a + 3 : R;
        for (uint32_t i = a; i < e; ++i) local = ssp_seg_join(local, seg[i]);
        ssp_seg_t run = carry;
        for (uint32_t i = a; i < e; ++i) seg[i] = run = ssp_seg_join(run, seg[i]);
        carry = ssp_seg_join(carry, local);
        if (memcmp(&carry, &seg[e - 1], sizeof carry)) {
            fprintf(stderr, "ssp_seg_join is not associative at record %u\n", a);
            exit(1);
        }
    }
    for (uint32_t i = 1; i < R; ++i)
        if (maxt[i - 1] > maxt[i]) maxt[i] = maxt[i - 1];
    uint32_t kept = 0;
    for (uint32_t i = 0; i < R; ++i) {
        uint32_t k;
        rank[i] = kept;
        if (ssp_plan_rules(fl[i], tid[i], beg[i], end[i], i ? seg[i - 1] : ssp_seg_none(), i ? maxt[i - 1] : INT32_MIN,
                           t0, w0, max0, &k, &from[i]) &&
            i < res->first_err)
            res->first_err = i;
        kept += k;
    }
    rank[R] = kept;
    for (uint32_t i = 0; i < R; ++i) {
        const uint32_t r = rank[i];
        if (rank[i + 1] == r || i >= res->first_err || r >= cap) continue;
        o_off[r] = off[i];
        o_from[r] = from[i];
        o_tid[r] = tid[i];
        if (r == cap - 1) res->cut = i;
    }
    ssp_plan_finish(b, R, t0, w0, max0, chain_end, chain_bad, off, rank, seg, maxt, res);
    free(tid); free(beg); free(end); free(maxt); free(from); free(fl); free(rank); free(seg);
    return 0;
}

static int check_plan(uint32_t i, const uint8_t *b, uint64_t len, const uint64_t *off, uint64_t n_rec, uint64_t end_at,
                      int bad)
{
    static const int masks[3] = {-1, 0x400, 0}, threshs[3] = {0, 20, 61};
    int ok = 1;
    for (int m = 0; m < 3 && ok; ++m) {
        ss_pileup_state_t in[3];
        memset(in, 0, sizeof in);
        in[1].has_prev = 1; in[1].tid = 0; in[1].w = 25; in[1].max_tid = 0;
        in[2].has_prev = 1; in[2].tid = 2; in[2].w = -7; in[2].max_tid = -1;
        for (int s = 0; s < 3 && ok; ++s) {
            /* capacities: all records; then one below the kept count, and 1 */
            uint32_t caps[3] = {(uint32_t)n_rec + 1, 0, 1};
            for (int c = 0; c < 3 && ok; ++c) {
                const uint32_t cap = caps[c];
                uint64_t *h_off = (uint64_t *)exact(8 * (size_t)cap), *d_off = (uint64_t *)exact(8 * (size_t)cap);
                int32_t *h_from = (int32_t *)exact(4 * (size_t)cap), *d_from = (int32_t *)exact(4 * (size_t)cap);
                int32_t *h_tid = (int32_t *)exact(4 * (size_t)cap), *d_tid = (int32_t *)exact(4 * (size_t)cap);
                ss_pileup_state_t st = in[s];
                uint32_t n = 0;
                size_t used = 0;
                const int rc = ss_pileup_plan(b, (size_t)len, masks[m], threshs[m], &st, h_off, h_from, h_tid, cap, &n,
                                              &used);
                ssp_plan_res_t res;
                model_plan(b, off, (uint32_t)n_rec, end_at, bad, masks[m], threshs[m], &in[s], cap, d_off, d_from, d_tid,
                           &res);
                if (rc != res.code) ok = fail("plan code", i, rc, res.code);
                else if (n != res.n) ok = fail("plan n", i, n, res.n);
                else if (used != res.consumed) ok = fail("plan consumed", i, (long)used, (long)res.consumed);
                else if (st.tid != res.tid || st.w != res.w || st.max_tid != res.max_tid)
                    ok = fail("plan state", i, (long)st.w, (long)res.w);
                else if (n && (memcmp(h_off, d_off, 8 * (size_t)n) || memcmp(h_from, d_from, 4 * (size_t)n) ||
                               memcmp(h_tid, d_tid, 4 * (size_t)n)))
                    ok = fail("plan arrays", i, m, c);
                if (c == 0) caps[1] = n ? n - 1 : 0;
                free(h_off); free(d_off); free(h_from); free(d_from); free(h_tid); free(d_tid);
            }
        }
    }
    return ok;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t n_spans = 0, n_headers = 0;
    int ok = 1;
    if (rd(f, &n_spans, 4)) return 2;
    for (uint32_t i = 0; i < n_spans && ok; ++i) {
        uint32_t chunk;
        int32_t n_ref;
        uint64_t len;
        if (rd(f, &chunk, 4) || rd(f, &n_ref, 4) || rd(f, &len, 8) || len > (1u << 28)) return 2;
        uint8_t *b = (uint8_t *)exact((size_t)len);
        if (rd(f, b, (size_t)len)) return 2;
        uint64_t *want = (uint64_t *)exact(sizeof(uint64_t) * (size_t)(len / 36 + 1));
        uint64_t end_at;
        int bad;
        const uint64_t n_want = plain_walk(b, len, want, &end_at, &bad);
        const uint32_t chunks[3] = {chunk, 64, SS_PLAN_CHUNK};
        for (int c = 0; c < 3 && ok; ++c) ok = check_twin(i, b, len, n_ref, chunks[c], want, n_want, end_at, bad);
        /* the guess rule at every offset, the end included, with and without the contig count */
        uint64_t accepted = 0;
        for (uint64_t o = 0; o <= len; ++o)
            accepted += (uint64_t)(ssp_guess_ok(b, len, o, n_ref) + ssp_guess_ok(b, len, o, 0));
        if (len >= 4 && !accepted) ok = fail("no offset accepted", i, 0, 0);
        if (ok) ok = check_plan(i, b, len, want, n_want, end_at, bad);
        int32_t refs;
        size_t at;
        (void)ss_bam_header_scan(b, (size_t)len, &refs, &at);     /* record bytes are no header: any code */
        free(want);
        free(b);
    }
    if (rd(f, &n_headers, 4)) return 2;
    for (uint32_t i = 0; i < n_headers && ok; ++i) {
        uint64_t len, want_at;
        int32_t want_ref;
        if (rd(f, &len, 8) || len > (1u << 28)) return 2;
        uint8_t *whole = (uint8_t *)exact((size_t)len);
        if (rd(f, whole, (size_t)len) || rd(f, &want_ref, 4) || rd(f, &want_at, 8) || want_at > len) return 2;
        for (uint64_t cut = 0; cut <= want_at + 8 && cut <= len && ok; ++cut) {     /* every prefix, exactly sized */
            uint8_t *p = (uint8_t *)exact((size_t)cut);
            memcpy(p, whole, (size_t)cut);
            int32_t refs = -1;
            size_t at = 0;
            const int rc = ss_bam_header_scan(p, (size_t)cut, &refs, &at);
            if (cut < want_at ? rc != SS_BAM_MORE : (rc != SS_OK || refs != want_ref || at != want_at))
                ok = fail("header scan", i, rc, (long)cut);
            free(p);
        }
        free(whole);
    }
    fclose(f);
    printf("ok=%d spans=%u headers=%u\n", ok, n_spans, n_headers);
    return ok ? 0 : 1;
}
