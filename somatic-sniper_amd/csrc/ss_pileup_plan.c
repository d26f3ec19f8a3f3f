/*
 * ss_pileup_plan.c -- the host side of the record pileup that needs no GPU
 * (include/sniper_amd.h, "pileup columns from BAM records"): ss_pileup_plan,
 * one sample's load rules over uncompressed BAM records;
 * ss_pileup_region_cpu, the shared core (ss_pileup_core.h) run on the calling
 * thread -- the twin the device path is compared with; and for the device
 * planner (ss_plan_core.h) the stitch it shares with its own twin
 * ss_pileup_split_cpu, and ss_bam_header_scan.
 */
#include <stdlib.h>
#include <string.h>

#include "sniper_amd.h"
#include "ss_pileup_core.h"
#include "ss_plan_core.h"

#define FUNMAP 4u
#define DEF_MASK (4u | 256u | 512u | 1024u)      /* samtools-0.1.6/bam.h:121 */

int ss_pileup_plan(const uint8_t *bytes, size_t len, int mask, int thresh, ss_pileup_state_t *state,
                   uint64_t *rec_off, int32_t *from, int32_t *tid, uint32_t cap, uint32_t *n, size_t *consumed)
{
    if ((!bytes && len) || !state || !n || (cap && (!rec_off || !from || !tid))) return SS_E_INVAL;
    const uint32_t flag_mask = mask < 0 ? DEF_MASK : (FUNMAP | (uint32_t)mask);
    const int mapq_thresh = thresh < 0 ? 0 : thresh;
    int32_t T = 0, max_tid = -1;
    int64_t W = 0;
    if (state->has_prev) {
        T = state->tid;
        W = state->w;
        max_tid = state->max_tid;
    }
    size_t at = 0;
    uint32_t k = 0;
    int rc = SS_OK;
    while (k < cap && len - at >= 4) {
        const uint8_t *r = bytes + at;
        const int32_t block = (int32_t)ssp_le32(r);
        if (block < 32) { rc = SS_E_INVAL; break; }
        if (len - at - 4 < (size_t)block) break;               /* incomplete */
        const size_t next = at + 4 + (size_t)block;
        ssp_head_t hd;
        ssp_head(r, &hd);
        const int32_t rtid = hd.tid, pos = hd.pos;
        const uint32_t l_name = hd.l_name, mapq = hd.mapq, n_cigar = hd.n_cigar, flag = hd.flag;
        if ((flag & flag_mask) || (int)mapq < mapq_thresh) { at = next; continue; }
        if (32u + (uint64_t)l_name + 4u * (uint64_t)n_cigar > (uint64_t)block) { rc = SS_E_INVAL; break; }
        if (rtid < max_tid) { rc = SS_E_INVAL; break; }        /* not sorted by contig */
        max_tid = rtid;
        const int64_t beg = pos;
        const int64_t end = (int64_t)(int32_t)(uint32_t)ssp_ref_end(r + 36 + l_name, n_cigar, pos);
        const int keep = end > W;
        int64_t f = beg > W ? beg : W;
        if (rtid != T) {                 /* a later contig */
            T = rtid;
            f = beg;
            W = beg > 0 ? beg : 0;
        } else if (beg > W) {
            W = beg;
        }
        if (keep) {
            rec_off[k] = (uint64_t)at;
            from[k] = (int32_t)f;
            tid[k] = rtid;
            ++k;
        }
        at = next;
    }
    state->has_prev = 1;
    state->tid = T;
    state->w = W;
    state->max_tid = max_tid;
    *n = k;
    if (consumed) *consumed = at;
    return rc;
}

/* ---- the CPU twin --------------------------------------------------------- */
typedef struct {
    ssp_desc_t *desc;
    int32_t *max_end;
    uint64_t n_invalid;
} indexed_t;

/* shared with ss_pileup.hip: the checks ss_pileup_region_host makes before any copy */
int ssp_sample_args_ok(const ss_pileup_sample_t *s);
int ssp_sample_args_ok(const ss_pileup_sample_t *s)
{
    if (!s || s->n > SS_PILEUP_MAX_RECORDS || s->n_bytes > 0xffffffffull) return 0;
    if (s->n && (!s->bytes || !s->rec_off || !s->from)) return 0;
    for (uint32_t i = 0; i < s->n; ++i) {
        if (s->rec_off[i] >= s->n_bytes) return 0;
        if (i && s->from[i] < s->from[i - 1]) return 0;
    }
    return 1;
}

static int index_sample(const ss_pileup_sample_t *s, indexed_t *x)
{
    x->desc = (ssp_desc_t *)malloc(sizeof(ssp_desc_t) * ((size_t)s->n + 1));
    x->max_end = (int32_t *)malloc(sizeof(int32_t) * ((size_t)s->n + 1));
    x->n_invalid = 0;
    if (!x->desc || !x->max_end) return SS_E_NOMEM;
    int32_t m = 0;
    for (uint32_t i = 0; i < s->n; ++i) {
        if (!ssp_index(s->bytes, s->n_bytes, s->rec_off[i], s->from[i], &x->desc[i])) ++x->n_invalid;
        if (x->desc[i].end > m) m = x->desc[i].end;
        x->max_end[i] = m;
    }
    return SS_OK;
}

int ss_pileup_region_cpu(const ss_pileup_sample_t *tumor, const ss_pileup_sample_t *normal, const uint8_t *ref,
                         int64_t ref_len, int32_t lo, int32_t hi, ss_pileup_out_t *out)
{
    if (!out || lo < 0 || hi <= lo || (uint32_t)(hi - lo) > SS_PILEUP_MAX_SPAN) return SS_E_INVAL;
    if (!ssp_sample_args_ok(tumor) || !ssp_sample_args_ok(normal)) return SS_E_INVAL;
    indexed_t xt = {0, 0, 0}, xn = {0, 0, 0};
    const uint32_t span = (uint32_t)(hi - lo);
    uint32_t *cnt = (uint32_t *)malloc(sizeof(uint32_t) * 4 * (size_t)span);     /* raw_t raw_n npk_t npk_n */
    int rc = cnt ? SS_OK : SS_E_NOMEM;
    if (rc == SS_OK) rc = index_sample(tumor, &xt);
    if (rc == SS_OK) rc = index_sample(normal, &xn);
    if (rc != SS_OK) goto done;
    /* pass 1: every column's counts */
    uint64_t n_sites = 0, nt = 0, nn = 0;
    for (int32_t t_lo = lo; t_lo < hi; t_lo = t_lo > hi - SSP_TILE ? hi : t_lo + SSP_TILE) {
        const int32_t t_hi = t_lo > hi - SSP_TILE ? hi : t_lo + SSP_TILE;
        uint32_t lbt, ubt, lbn, ubn;
        ssp_candidates(xt.desc, xt.max_end, tumor->n, t_lo, t_hi, &lbt, &ubt);
        ssp_candidates(xn.desc, xn.max_end, normal->n, t_lo, t_hi, &lbn, &ubn);
        for (int32_t p = t_lo; p < t_hi; ++p) {
            uint32_t *c = cnt + 4 * (size_t)(p - lo);
            c[2] = ssp_column(tumor->bytes, xt.desc, lbt, ubt, p, &c[0], NULL, 0);
            c[3] = ssp_column(normal->bytes, xn.desc, lbn, ubn, p, &c[1], NULL, 0);
            if (c[0] && c[1]) {
                ++n_sites;
                nt += c[2];
                nn += c[3];
            }
        }
    }
    out->n_sites = n_sites;
    out->n_reads_t = nt;
    out->n_reads_n = nn;
    out->n_invalid = xt.n_invalid + xn.n_invalid;
    if (nt > SS_PILEUP_MAX_READS || nn > SS_PILEUP_MAX_READS || n_sites > out->cap_sites || nt > out->cap_reads_t ||
        nn > out->cap_reads_n) {
        rc = SS_E_CAPACITY;
        goto done;
    }
    if (!out->pos || !out->ref || !out->raw_t || !out->raw_n || !out->off_t || !out->off_n ||
        (nt && !out->reads_t) || (nn && !out->reads_n)) {
        rc = SS_E_INVAL;
        goto done;
    }
    /* pass 2: the sites and their entries */
    {
        uint64_t s = 0, ot = 0, on = 0;
        for (int32_t t_lo = lo; t_lo < hi; t_lo = t_lo > hi - SSP_TILE ? hi : t_lo + SSP_TILE) {
            const int32_t t_hi = t_lo > hi - SSP_TILE ? hi : t_lo + SSP_TILE;
            uint32_t lbt, ubt, lbn, ubn;
            ssp_candidates(xt.desc, xt.max_end, tumor->n, t_lo, t_hi, &lbt, &ubt);
            ssp_candidates(xn.desc, xn.max_end, normal->n, t_lo, t_hi, &lbn, &ubn);
            for (int32_t p = t_lo; p < t_hi; ++p) {
                const uint32_t *c = cnt + 4 * (size_t)(p - lo);
                if (!c[0] || !c[1]) continue;
                uint32_t raw;
                out->pos[s] = p;
                out->ref[s] = (uint8_t)((ref && p < ref_len) ? ref[p] : 'N');
                out->raw_t[s] = c[0];
                out->raw_n[s] = c[1];
                out->off_t[s] = (uint32_t)ot;
                out->off_n[s] = (uint32_t)on;
                if (c[2]) ssp_column(tumor->bytes, xt.desc, lbt, ubt, p, &raw, out->reads_t + ot, c[2]);
                if (c[3]) ssp_column(normal->bytes, xn.desc, lbn, ubn, p, &raw, out->reads_n + on, c[3]);
                ot += c[2];
                on += c[3];
                ++s;
            }
        }
        out->off_t[s] = (uint32_t)ot;
        out->off_n[s] = (uint32_t)on;
    }
    if (out->n_invalid) rc = SS_E_INVAL;
done:
    free(cnt);
    free(xt.desc);
    free(xt.max_end);
    free(xn.desc);
    free(xn.max_end);
    return rc;
}

/* ---- the device planner's host parts ----------------------------------------- */
typedef int (*ssp_rewalk_fn)(void *ctx, uint32_t k, uint64_t entry, ssp_chunk_t *c);

/* The stitch, shared with ss_pileup.hip.  c[k] is chunk k's walk from its
 * guess.  Follows the true chain from offset 0: a chunk the chain passes over
 * contributes nothing (SSP_WALK_SKIP, count 0); a chunk whose guess is not
 * where the chain enters it is walked again from there (rewalk; counted in
 * *n_repaired); the chain ends where a kept chunk's walk broke, or after the
 * last chunk.  Afterwards the kept chunks' entries and counts are the
 * chain's.  One pass: every chunk is looked at once and walked at most twice. */
int ssp_plan_stitch(ssp_chunk_t *c, uint32_t n_chunks, uint64_t chunk, uint64_t len, ssp_rewalk_fn rewalk, void *ctx,
                    uint64_t *n_rec, uint64_t *end_at, uint32_t *end_status, uint32_t *n_repaired);
int ssp_plan_stitch(ssp_chunk_t *c, uint32_t n_chunks, uint64_t chunk, uint64_t len, ssp_rewalk_fn rewalk, void *ctx,
                    uint64_t *n_rec, uint64_t *end_at, uint32_t *end_status, uint32_t *n_repaired)
{
    uint64_t e = 0, total = 0;
    uint32_t st = SSP_WALK_END, rep = 0, k = 0;
    for (; k < n_chunks; ++k) {
        const uint64_t lim = ((uint64_t)k + 1) * chunk;
        const uint64_t end = lim < len ? lim : len;
        if (e >= end) {
            c[k].count = 0;
            c[k].status = SSP_WALK_SKIP;
            continue;
        }
        if (c[k].entry != e) {
            const int rc = rewalk(ctx, k, e, &c[k]);
            if (rc != SS_OK) return rc;
            ++rep;
        }
        total += c[k].count;
        e = c[k].exit;
        if (c[k].status != SSP_WALK_EXIT) {
            st = c[k].status;
            ++k;
            break;
        }
    }
    for (; k < n_chunks; ++k) {
        c[k].count = 0;
        c[k].status = SSP_WALK_SKIP;
    }
    *n_rec = total;
    *end_at = e;
    *end_status = st == SSP_WALK_BAD ? SSP_WALK_BAD : SSP_WALK_END;
    *n_repaired = rep;
    return SS_OK;
}

typedef struct {
    const uint8_t *bytes;
    uint64_t len, chunk;
} split_t;

static void split_walk(const split_t *s, uint32_t k, uint64_t entry, uint32_t *rel, uint32_t rel_cap, ssp_chunk_t *c)
{
    const uint64_t start = (uint64_t)k * s->chunk, lim = start + s->chunk;
    const uint64_t end = lim < s->len ? lim : s->len;
    c->entry = entry;
    c->exit = entry;
    c->count = 0;
    c->status = SSP_WALK_EXIT;
    if (entry != SSP_NO_GUESS)
        c->status = ssp_walk(s->bytes, 0, s->len, start, entry, end, rel, rel_cap, &c->exit, &c->count);
}

static int split_rewalk(void *ctx, uint32_t k, uint64_t entry, ssp_chunk_t *c)
{
    split_walk((const split_t *)ctx, k, entry, NULL, 0, c);
    return SS_OK;
}

int ss_pileup_split_cpu(const uint8_t *bytes, uint64_t len, int32_t n_ref, uint32_t chunk, uint64_t *rec_off,
                        uint64_t cap, uint64_t *n, uint64_t *end_at, int *end_why, uint32_t *n_repaired)
{
    if ((!bytes && len) || !chunk || !n || !end_at || !end_why || !n_repaired || (cap && !rec_off)) return SS_E_INVAL;
    const uint64_t nc64 = (len + chunk - 1) / chunk;
    if (nc64 > 0x7fffffffull) return SS_E_INVAL;
    const uint32_t n_chunks = (uint32_t)nc64, rel_cap = chunk / 36u + 2u;
    const split_t s = {bytes, len, chunk};
    ssp_chunk_t *c = (ssp_chunk_t *)malloc(sizeof(ssp_chunk_t) * ((size_t)n_chunks + 1));
    uint32_t *rel = (uint32_t *)malloc(sizeof(uint32_t) * rel_cap);
    int rc = (c && rel) ? SS_OK : SS_E_NOMEM;
    uint64_t total = 0, at = 0;
    uint32_t st = SSP_WALK_END, rep = 0;
    if (rc == SS_OK) {
        for (uint32_t k = 0; k < n_chunks; ++k) {
            const uint64_t start = (uint64_t)k * chunk, lim = start + chunk;
            split_walk(&s, k, k ? ssp_guess(bytes, len, start, lim < len ? lim : len, n_ref) : 0, NULL, 0, &c[k]);
        }
        rc = ssp_plan_stitch(c, n_chunks, chunk, len, split_rewalk, (void *)&s, &total, &at, &st, &rep);
    }
    if (rc == SS_OK) {
        uint64_t base = 0;
        for (uint32_t k = 0; k < n_chunks; ++k) {
            if (c[k].status == SSP_WALK_SKIP) continue;
            ssp_chunk_t again;
            split_walk(&s, k, c[k].entry, rel, rel_cap, &again);
            for (uint32_t i = 0; i < again.count && i < rel_cap; ++i)
                if (base + i < cap) rec_off[base + i] = (uint64_t)k * chunk + rel[i];
            base += again.count;
        }
        *n = total;
        *end_at = at;
        *end_why = st == SSP_WALK_BAD ? SS_PLAN_END_BLOCK : SS_PLAN_END_DATA;
        *n_repaired = rep;
        if (total > cap) rc = SS_E_CAPACITY;
    }
    free(c);
    free(rel);
    return rc;
}

int ss_bam_header_scan(const uint8_t *bytes, size_t len, int32_t *n_ref, size_t *records_at)
{
    if ((!bytes && len) || !n_ref || !records_at) return SS_E_INVAL;
    const size_t m = len < 4 ? len : 4;
    if (m && memcmp(bytes, "BAM\1", m) != 0) return SS_E_INVAL;
    if (len < 8) return SS_BAM_MORE;
    const int32_t l_text = (int32_t)ssp_le32(bytes + 4);
    if (l_text < 0) return SS_E_INVAL;
    size_t at = 8 + (size_t)l_text;
    if (len < at || len - at < 4) return SS_BAM_MORE;
    const int32_t refs = (int32_t)ssp_le32(bytes + at);
    if (refs < 0) return SS_E_INVAL;
    at += 4;
    for (int32_t i = 0; i < refs; ++i) {
        if (len - at < 4) return SS_BAM_MORE;
        const int32_t l_name = (int32_t)ssp_le32(bytes + at);
        if (l_name < 0) return SS_E_INVAL;
        if (len - at - 4 < (size_t)l_name + 4) return SS_BAM_MORE;
        at += 8 + (size_t)l_name;
    }
    *n_ref = refs;
    *records_at = at;
    return SS_OK;
}
