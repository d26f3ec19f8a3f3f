/*
 * ss_pileup_core.h -- pileup columns from BAM alignment records, shared
 * verbatim by the host (ss_pileup_region_cpu, tests/native/pileup_driver.c) and
 * the device (ss_pileup.hip), so both build the same columns.  Integer code
 * only, no library calls.
 *
 * A record is read as it lies in the file (SAM spec 4.2):
 *   +0  block_size   +4  refID      +8  pos        +12 l_read_name  +13 mapq
 *   +14 bin          +16 n_cigar    +18 flag       +20 l_seq        +24 next_refID
 *   +28 next_pos     +32 tlen       +36 read_name | cigar (u32) | seq (4 bit) | qual
 * Record offsets have no alignment, so every multi-byte field is assembled
 * from single bytes (ssp_le32).
 *
 * ssp_index() validates a record and writes its descriptor; everything else
 * reads the record only through a valid descriptor.  A descriptor that failed
 * validation has no SSP_VALID bit, an empty span and contributes nothing.
 *
 * The rules are those of cli/column_pileup.h: M positions are entries with a
 * base, D positions deleted entries (raw depth only), N positions nothing; I
 * and S advance the query offset; H, P, = and X move neither coordinate;
 * nothing exists before the record's `from`.
 *
 * Columns are built position by position: the candidates of a tile of
 * positions are a contiguous range of records in load order (ssp_candidates),
 * and a column walks them in that order (ssp_column), so its entries keep the
 * load order whichever thread builds it.
 */
#ifndef SS_PILEUP_CORE_H
#define SS_PILEUP_CORE_H

#include <stdint.h>

#ifdef __HIPCC__
#define SSP_HD __host__ __device__ static inline __attribute__((always_inline))
#else
#define SSP_HD static inline
#endif

#define SSP_TILE 256                    /* positions per tile (one workgroup) */

#define SSP_NONE 0
#define SSP_DEL  1
#define SSP_BASE 2

#define SSP_SINGLE (1u << 16)           /* one M operation covering [beg, end) */
#define SSP_VALID  (1u << 17)

/* One record, validated.  Offsets are byte offsets into the sample's bytes. */
typedef struct ssp_desc {
    int32_t  beg, end;                  /* reference span (M, D and N consume the reference) */
    int32_t  from;                      /* first position the record contributes to, >= beg */
    uint32_t pk;                        /* mapq | strand << 20 */
    uint32_t cig, seq, qual;            /* offsets of the CIGAR words, the 4-bit bases, the qualities */
    uint32_t nc;                        /* n_cigar | SSP_SINGLE | SSP_VALID */
} ssp_desc_t;                           /* 32 bytes */

SSP_HD uint32_t ssp_le32(const uint8_t *p)
{
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

/* Reference end of a record whose CIGAR lies inside the bytes (bam_rec_end of
 * cli/bam_reader.c): pos + the lengths of the M, D and N operations. */
SSP_HD int64_t ssp_ref_end(const uint8_t *cigar, uint32_t n_cigar, int32_t pos)
{
    int64_t end = pos;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t c = ssp_le32(cigar + 4 * (uint64_t)k), op = c & 0xfu;
        if (op == 0u || op == 2u || op == 3u) end += c >> 4;
    }
    return end;
}

/* Validates the record at bytes[off] and writes its descriptor.  Returns 1 if
 * the record is valid.  Nothing past the fixed part is read before the block
 * is known to lie inside the bytes, and nothing past the block ever. */
SSP_HD int ssp_index(const uint8_t *bytes, uint64_t n_bytes, uint64_t off, int32_t from, ssp_desc_t *d)
{
    d->beg = d->end = 0;
    d->from = from;
    d->pk = d->cig = d->seq = d->qual = d->nc = 0;
    if (n_bytes > 0xffffffffull || off > n_bytes || n_bytes - off < 36u) return 0;
    const uint8_t *r = bytes + off;
    const int32_t block = (int32_t)ssp_le32(r);
    if (block < 32 || (uint64_t)block > n_bytes - off - 4u) return 0;
    const int32_t pos = (int32_t)ssp_le32(r + 8);
    const uint32_t l_name = r[12], mapq = r[13];
    const uint32_t n_cigar = (uint32_t)r[16] | (uint32_t)r[17] << 8;
    const uint32_t flag = (uint32_t)r[18] | (uint32_t)r[19] << 8;
    const int32_t l_seq = (int32_t)ssp_le32(r + 20);
    if (l_seq < 0 || pos < 0 || from < pos) return 0;
    const uint64_t need = 32u + (uint64_t)l_name + 4u * (uint64_t)n_cigar + (((uint64_t)l_seq + 1u) >> 1) + (uint64_t)l_seq;
    if (need > (uint64_t)block) return 0;
    const uint8_t *cigar = r + 36 + l_name;
    uint64_t qlen = 0, rlen = 0;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t c = ssp_le32(cigar + 4 * k), op = c & 0xfu, l = c >> 4;
        if (op == 0u || op == 1u || op == 4u) qlen += l;
        if (op == 0u || op == 2u || op == 3u) rlen += l;
    }
    if (qlen > (uint64_t)l_seq || (uint64_t)pos + rlen > 0x7fffffffull) return 0;
    d->beg = pos;
    d->end = (int32_t)((uint64_t)pos + rlen);
    d->pk = mapq | ((flag & 16u) ? 1u << 20 : 0u);
    d->cig = (uint32_t)(off + 36u + l_name);
    d->seq = d->cig + 4u * n_cigar;
    d->qual = d->seq + (((uint32_t)l_seq + 1u) >> 1);
    d->nc = n_cigar | SSP_VALID | ((n_cigar == 1u && (ssp_le32(cigar) & 0xfu) == 0u) ? SSP_SINGLE : 0u);
    return 1;
}

/* The entry of record d at position p: SSP_NONE, SSP_DEL (a deleted entry:
 * raw depth only) or SSP_BASE with the query offset in *q. */
SSP_HD int ssp_lookup(const uint8_t *bytes, const ssp_desc_t *d, int32_t p, uint32_t *q)
{
    if (!(d->nc & SSP_VALID) || p < d->from || p >= d->end) return SSP_NONE;
    if (d->nc & SSP_SINGLE) {
        *q = (uint32_t)(p - d->beg);
        return SSP_BASE;
    }
    const uint32_t n_cigar = d->nc & 0xffffu;
    int64_t x = d->beg;
    uint32_t y = 0;
    for (uint32_t k = 0; k < n_cigar && x <= p; ++k) {
        const uint32_t c = ssp_le32(bytes + d->cig + 4u * k), op = c & 0xfu, l = c >> 4;
        if (op == 0u) {
            if (p < x + l) {
                *q = y + (uint32_t)(p - x);
                return SSP_BASE;
            }
            x += l;
            y += l;
        } else if (op == 2u) {
            if (p < x + l) return SSP_DEL;
            x += l;
        } else if (op == 3u) {
            x += l;
        } else if (op == 1u || op == 4u) {
            y += l;
        }
    }
    return SSP_NONE;
}

/* SS_READ_PACK(mapq, qual[q], nt16(q), strand); q comes from ssp_lookup, so it
 * is below the query length the validation checked against l_seq. */
SSP_HD uint32_t ssp_pack(const uint8_t *bytes, const ssp_desc_t *d, uint32_t q)
{
    const uint32_t b = (bytes[d->seq + (q >> 1)] >> ((~q & 1u) << 2)) & 0xfu;
    return d->pk | (uint32_t)bytes[d->qual + q] << 8 | b << 16;
}

/* The records that can have an entry in [tile_lo, tile_hi): `from` does not
 * decrease, so those with from < tile_hi are a prefix [0, ub); max_end is the
 * running maximum of `end`, so every record before the first one with
 * max_end > tile_lo ends at or before tile_lo. */
SSP_HD void ssp_candidates(const ssp_desc_t *desc, const int32_t *max_end, uint32_t n, int32_t tile_lo,
                           int32_t tile_hi, uint32_t *lb, uint32_t *ub)
{
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if (desc[m].from < tile_hi) a = m + 1; else b = m;
    }
    *ub = a;
    b = a;
    a = 0;
    while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if (max_end[m] > tile_lo) b = m; else a = m + 1;
    }
    *lb = a;
}

/* The column at position p over the candidates [lb, ub), in load order: the
 * raw depth goes to *raw; packed entries are counted and, while fewer than
 * `room` have been met, stored to out (out may be NULL when room is 0).
 * Returns the packed depth. */
SSP_HD uint32_t ssp_column(const uint8_t *bytes, const ssp_desc_t *desc, uint32_t lb, uint32_t ub, int32_t p,
                           uint32_t *raw, uint32_t *out, uint32_t room)
{
    uint32_t r = 0, np = 0;
    for (uint32_t i = lb; i < ub; ++i) {
        const ssp_desc_t d = desc[i];
        uint32_t q = 0;
        const int kind = ssp_lookup(bytes, &d, p, &q);
        if (kind == SSP_NONE) continue;
        ++r;
        if (kind == SSP_BASE) {
            if (np < room) out[np] = ssp_pack(bytes, &d, q);
            ++np;
        }
    }
    *raw = r;
    return np;
}

#endif /* SS_PILEUP_CORE_H */
