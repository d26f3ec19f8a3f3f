/*
 * ss_plan_core.h -- the record index of the planner, shared verbatim by the
 * host (ss_pileup_plan, ss_pileup_split_cpu, tests/native/plan_driver.c) and
 * the device (ss_pileup.hip), so both find the same records and apply the same
 * load rules.  Integer code only, no library calls.  DESIGN.md section 14.
 *
 * The chain next = at + 4 + block_size is serial.  The byte span is cut into
 * chunks; every chunk but the first guesses where the chain enters it
 * (ssp_guess), walks from there (ssp_walk), and a serial stitch over the
 * chunks' results (ssp_plan_stitch, ss_pileup_plan.c) keeps a chunk only when
 * the chain really arrives at its guess, and walks it again from the true
 * entry otherwise.  The guess decides how much is walked twice, never what
 * comes out.
 *
 * Record layout: see ss_pileup_core.h.
 */
#ifndef SS_PLAN_CORE_H
#define SS_PLAN_CORE_H

#include "ss_pileup_core.h"

#define SSP_WALK_EXIT 0u                /* the chain left the chunk                              */
#define SSP_WALK_END  1u                /* fewer than 4 bytes left, or a record the bytes do not hold whole */
#define SSP_WALK_BAD  2u                /* block_size < 32                                       */
#define SSP_WALK_SKIP 3u                /* set by the stitch: the chain passes over the chunk    */

#define SSP_NO_GUESS (~(uint64_t)0)

#define SSP_R_PASS 1u                   /* the record passes the flag / mapq filter */
#define SSP_R_ERR  2u                   /* ... and its name + CIGAR pass its block  */

/* One chunk's walk. */
typedef struct ssp_chunk {
    uint64_t entry;                     /* where the walk began (the guess, or the true entry after a repair) */
    uint64_t exit;                      /* where it stopped: the first offset at or past the chunk's end, or the break */
    uint32_t count;                     /* whole records met */
    uint32_t status;                    /* SSP_WALK_* */
} ssp_chunk_t;

/* The fixed fields the planner reads.  r points at a record's block_size; 20
 * bytes are read. */
typedef struct ssp_head {
    int32_t  block, tid, pos;
    uint32_t l_name, mapq, n_cigar, flag;
} ssp_head_t;

SSP_HD void ssp_head(const uint8_t *r, ssp_head_t *h)
{
    h->block = (int32_t)ssp_le32(r);
    h->tid = (int32_t)ssp_le32(r + 4);
    h->pos = (int32_t)ssp_le32(r + 8);
    h->l_name = r[12];
    h->mapq = r[13];
    h->n_cigar = (uint32_t)r[16] | (uint32_t)r[17] << 8;
    h->flag = (uint32_t)r[18] | (uint32_t)r[19] << 8;
}

/* The load rules' view of one whole record (block_size >= 32, all of it inside
 * the bytes): SSP_R_* bits, and for a passing record without SSP_R_ERR its
 * contig, pos and reference end truncated to int32 as ss_pileup_plan has it. */
SSP_HD uint32_t ssp_plan_record(const uint8_t *r, uint32_t flag_mask, int mapq_thresh, int32_t *tid, int32_t *beg,
                                int32_t *end)
{
    ssp_head_t h;
    ssp_head(r, &h);
    *tid = h.tid;
    *beg = h.pos;
    *end = h.pos;
    if ((h.flag & flag_mask) || (int)h.mapq < mapq_thresh) return 0u;
    if (32u + (uint64_t)h.l_name + 4u * (uint64_t)h.n_cigar > (uint64_t)h.block) return SSP_R_PASS | SSP_R_ERR;
    *end = (int32_t)(uint32_t)ssp_ref_end(r + 36 + h.l_name, h.n_cigar, h.pos);
    return SSP_R_PASS;
}

/* Could a record start at bytes[off]?  Every field is tested only while it
 * lies inside bytes[0 .. len), so an offset with fewer than 4 bytes left
 * passes.  n_ref <= 0: the contig fields are not tested. */
SSP_HD int ssp_plausible(const uint8_t *bytes, uint64_t len, uint64_t off, int32_t n_ref)
{
    if (off > len || len - off < 4u) return 1;
    const uint64_t room = len - off;
    const uint8_t *r = bytes + off;
    const int32_t block = (int32_t)ssp_le32(r);
    if (block < 32) return 0;
    if (room >= 8u && n_ref > 0) {
        const int32_t t = (int32_t)ssp_le32(r + 4);
        if (t < -1 || t >= n_ref) return 0;
    }
    if (room >= 12u && (int32_t)ssp_le32(r + 8) < -1) return 0;
    if (room < 13u) return 1;
    const uint32_t l_name = r[12];
    if (l_name < 1u) return 0;
    if (room >= 28u && n_ref > 0) {
        const int32_t t = (int32_t)ssp_le32(r + 24);
        if (t < -1 || t >= n_ref) return 0;
    }
    if (room >= 32u && (int32_t)ssp_le32(r + 28) < -1) return 0;
    if (room < 24u) return 1;
    const uint32_t n_cigar = (uint32_t)r[16] | (uint32_t)r[17] << 8;
    const int32_t l_seq = (int32_t)ssp_le32(r + 20);
    if (l_seq < 0) return 0;
    if (32u + (uint64_t)l_name + 4u * (uint64_t)n_cigar + (((uint64_t)l_seq + 1u) >> 1) + (uint64_t)l_seq >
        (uint64_t)block)
        return 0;
    if (room >= 36u + (uint64_t)l_name && r[35u + l_name] != 0u) return 0;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint64_t at = 36u + (uint64_t)l_name + 4u * (uint64_t)k;
        if (at >= room) break;
        if ((r[at] & 0xfu) > 8u) return 0;
    }
    return 1;
}

/* The guess rule at one offset (off <= len): plausible, and its successor too.
 * A successor the bytes do not hold passes. */
SSP_HD int ssp_guess_ok(const uint8_t *bytes, uint64_t len, uint64_t off, int32_t n_ref)
{
    if (!ssp_plausible(bytes, len, off, n_ref)) return 0;
    if (len - off < 4u) return 1;
    const uint64_t block = (uint64_t)ssp_le32(bytes + off);       /* >= 32: it passed */
    if (block >= len - off - 4u) return 1;
    return ssp_plausible(bytes, len, off + 4u + block, n_ref);
}

/* The first offset of [start, end) the guess rule accepts, or SSP_NO_GUESS. */
SSP_HD uint64_t ssp_guess(const uint8_t *bytes, uint64_t len, uint64_t start, uint64_t end, int32_t n_ref)
{
    for (uint64_t o = start; o < end; ++o)
        if (ssp_guess_ok(bytes, len, o, n_ref)) return o;
    return SSP_NO_GUESS;
}

/* Walks the chain from `at` (<= len) until it reaches `end` (<= len) or breaks,
 * exactly as the loop of ss_pileup_plan steps.  w[x - w_base] is byte x of the
 * span for at <= x < end + 3 (the bytes themselves, or a staged window).  The
 * offsets of the first rel_cap records, relative to `start`, go to rel (may be
 * NULL). */
SSP_HD uint32_t ssp_walk(const uint8_t *w, uint64_t w_base, uint64_t len, uint64_t start, uint64_t at, uint64_t end,
                         uint32_t *rel, uint32_t rel_cap, uint64_t *exit_at, uint32_t *count)
{
    uint32_t n = 0, st = SSP_WALK_EXIT;
    while (at < end) {
        if (len - at < 4u) { st = SSP_WALK_END; break; }
        const int32_t block = (int32_t)ssp_le32(w + (at - w_base));
        if (block < 32) { st = SSP_WALK_BAD; break; }
        if (len - at - 4u < (uint64_t)block) { st = SSP_WALK_END; break; }
        if (rel && n < rel_cap) rel[n] = (uint32_t)(at - start);
        ++n;
        at += 4u + (uint64_t)block;
    }
    *exit_at = at;
    *count = n;
    return st;
}

/* The walk state as a scan element: the contig of the span's last passing
 * record, the maximum of beg over the span's trailing records of that contig
 * (the walk's clamp to 0 at a contig change is applied by ssp_seg_apply, so
 * that a negative in-state W is carried as the host carries it), whether those
 * are all of the span's passing records, and whether the span holds none.
 * ssp_seg_join is associative; joined left to right from the in-state it
 * steps exactly as ss_pileup_plan does ("another contig replaces, the same
 * contig takes the maximum"). */
typedef struct ssp_seg {
    int32_t  tid, w;
    uint32_t single, ident;
} ssp_seg_t;

SSP_HD ssp_seg_t ssp_seg_join(ssp_seg_t a, ssp_seg_t b)
{
    if (a.ident) return b;
    if (b.ident) return a;
    ssp_seg_t r = b;
    if (b.single && a.tid == b.tid) {
        r.w = a.w > b.w ? a.w : b.w;
        r.single = a.single;
    } else {
        r.single = 0u;
    }
    return r;
}

/* The walk state (T, W) after the in-state (t0, w0) and then the span p. */
SSP_HD void ssp_seg_apply(int32_t t0, int64_t w0, ssp_seg_t p, int32_t *t, int64_t *w)
{
    *t = t0;
    *w = w0;
    if (p.ident) return;
    if (p.single && p.tid == t0) {
        if ((int64_t)p.w > w0) *w = p.w;
    } else {
        *t = p.tid;
        *w = p.w > 0 ? p.w : 0;
    }
}

SSP_HD ssp_seg_t ssp_seg_none(void)
{
    ssp_seg_t p;
    p.tid = 0;
    p.w = 0;
    p.single = 1u;
    p.ident = 1u;
    return p;
}

/* The scan elements of one record: fl from ssp_plan_record. */
SSP_HD ssp_seg_t ssp_seg_of(uint32_t fl, int32_t tid, int32_t beg)
{
    ssp_seg_t g;
    g.tid = tid;
    g.w = beg;
    g.single = 1u;
    g.ident = (fl & SSP_R_PASS) ? 0u : 1u;
    return g;
}
SSP_HD int32_t ssp_maxt_of(uint32_t fl, int32_t tid) { return (fl & SSP_R_PASS) ? tid : INT32_MIN; }

/* The load rules for one record.  prev / prev_max: the joined elements and the
 * highest passing contig of all records before it (ssp_seg_none() / INT32_MIN
 * for the first); (t0, w0, max0): the in-state.  Returns 1 if the walk fails
 * at this record, else 0 with *keep (end > W) and *from. */
SSP_HD int ssp_plan_rules(uint32_t fl, int32_t tid, int32_t beg, int32_t end, ssp_seg_t prev, int32_t prev_max,
                          int32_t t0, int64_t w0, int32_t max0, uint32_t *keep, int32_t *from)
{
    *keep = 0u;
    *from = 0;
    if (!(fl & SSP_R_PASS)) return 0;
    const int32_t mx = prev_max > max0 ? prev_max : max0;
    if ((fl & SSP_R_ERR) || tid < mx) return 1;
    int32_t T;
    int64_t W;
    ssp_seg_apply(t0, w0, prev, &T, &W);
    const int64_t b = beg, e = end;
    *keep = e > W ? 1u : 0u;
    *from = (int32_t)((tid != T) ? b : (b > W ? b : W));
    return 0;
}

#define SSP_NO_RECORD 0xffffffffu

/* What one plan leaves besides the arrays. */
typedef struct ssp_plan_res {
    uint64_t consumed;
    int64_t  w;
    uint32_t n;
    int32_t  code, tid, max_tid;       /* code: 0, or -1 (SS_E_INVAL) */
    uint32_t first_err, cut;           /* in: the first failing record and the cap-th kept record, or SSP_NO_RECORD */
} ssp_plan_res_t;

/* Closes a plan over n_rec records: the walk covered the records [0, x), x
 * being the first failing record, the one after the cap-th kept record, or
 * n_rec.  off: the records' offsets; rank[i]: kept records before record i
 * (n_rec + 1 entries); seg / maxt: the inclusive scans; chain_end /
 * chain_bad: where the record chain ended, and whether at a block_size < 32. */
SSP_HD void ssp_plan_finish(const uint8_t *bytes, uint32_t n_rec, int32_t t0, int64_t w0, int32_t max0,
                            uint64_t chain_end, int chain_bad, const uint64_t *off, const uint32_t *rank,
                            const ssp_seg_t *seg, const int32_t *maxt, ssp_plan_res_t *res)
{
    const uint32_t err = res->first_err, cut = res->cut;
    uint32_t x = n_rec;
    if (cut != SSP_NO_RECORD && cut + 1u < x) x = cut + 1u;
    const int failed = err < x;                 /* a failing record after the cap-th kept one is never reached */
    if (failed) x = err;
    res->n = rank[x];
    if (failed) {
        res->consumed = off[err];
        res->code = -1;
    } else if (cut != SSP_NO_RECORD) {
        res->consumed = off[cut] + 4u + (uint64_t)ssp_le32(bytes + off[cut]);
        res->code = 0;
    } else {
        res->consumed = chain_end;
        res->code = chain_bad ? -1 : 0;
    }
    ssp_seg_t p = ssp_seg_none();
    int32_t mx = max0;
    if (x) {
        p = seg[x - 1u];
        if (maxt[x - 1u] > mx) mx = maxt[x - 1u];
    }
    ssp_seg_apply(t0, w0, p, &res->tid, &res->w);
    res->max_tid = mx;
}

#endif /* SS_PLAN_CORE_H */
