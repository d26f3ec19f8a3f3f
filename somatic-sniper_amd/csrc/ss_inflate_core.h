/*
 * ss_inflate_core.h -- DEFLATE (RFC 1951) decoder for BGZF members, shared
 * verbatim by the host (ss_inflate_members_cpu, tests/native/inflate_driver.c)
 * and the device (ss_inflate.hip), so both decode the same items and report the
 * same statuses.  Integer code only, no library calls, no recursion, and no
 * constant tables: the length / distance base and extra-bit tables of RFC 1951
 * section 3.2.5 are regular enough to be computed (ssi_len_base, ssi_dist_base).
 *
 * The decoder is a pull parser.  ssi_next() returns one item at a time:
 *   SSI_LIT     one literal byte                         (*val = the byte)
 *   SSI_MATCH   a back-reference                         (*val = length 3..258, *dist = 1..32768)
 *   SSI_STORED  the payload of a stored block            (*val = byte count, *dist = its offset in the input)
 *   SSI_END     the final block has ended
 *   SSI_ERR     invalid or truncated data
 * and never writes output: the caller owns every store and checks it against
 * the member's output span (ssi_inflate_member below for the host; the kernel
 * in ss_inflate.hip checks a run of 64 items at a time).
 *
 * Bounds: every input read goes through ssi_refill / the stored-block check,
 * both bounded by ssi_bits_t.end (the member's DEFLATE bytes, trailer
 * excluded); bits past the end read as zero and consuming them is an error.
 * Decode tables are indexed by values masked to the table size or by symbols
 * smaller than the counts that built them.
 *
 * Which code-length sets are legal follows zlib's inflate_table():
 *   - an over-subscribed set is an error;
 *   - an incomplete set is an error, except a literal/length or distance set
 *     whose only code has length 1 (zlib: "left > 0 && (type == CODES ||
 *     max != 1)"); the unused 1-bit code is an error when it is met;
 *   - a distance set without any code is legal as long as no match is coded;
 *   - the code-length code itself must be complete;
 *   - the literal/length set must give symbol 256 a length, HLIT <= 286 and
 *     HDIST <= 30 (zlib's inflate()).
 */
#ifndef SS_INFLATE_CORE_H
#define SS_INFLATE_CORE_H

#include <stdint.h>

#ifdef __HIPCC__
#define SSI_HD __host__ __device__ static inline __attribute__((always_inline))
#else
#define SSI_HD static inline
#endif

/* per-member statuses (SS_INF_* in sniper_amd.h) */
#define SSI_OK        0u
#define SSI_E_STREAM  1u
#define SSI_E_SIZE    2u
#define SSI_E_CRC     3u

#define SSI_MEMBER_MAX 65536u           /* BGZF: at most 64 KiB of data per member */
#define SSI_COMP_MAX   (65536u + 8u)    /* DEFLATE bytes + the 8-byte trailer */

#define SSI_LIT    0
#define SSI_MATCH  1
#define SSI_STORED 2
#define SSI_END    3
#define SSI_ERR    4

#define SSI_FAST_LIT  9                 /* first-level table bits */
#define SSI_FAST_DIST 6

/* Decode tables of one member (one wave): 2.3 KiB.  Codes of at most FAST bits
 * resolve in one lookup (entry = symbol << 4 | length, 0 = longer code); longer
 * ones walk the canonical count / symbol arrays. */
typedef struct ssi_tables {
    uint16_t lit_fast[1 << SSI_FAST_LIT];
    uint16_t dist_fast[1 << SSI_FAST_DIST];
    uint16_t lit_count[16], dist_count[16];
    uint16_t lit_sym[288], dist_sym[32];
    uint16_t offs[16], next[16];        /* table-building scratch */
    uint8_t  lens[320];                 /* code lengths of the block being set up */
} ssi_tables_t;

typedef struct ssi_bits {
    const uint8_t *in;
    uint32_t pos, end;                  /* next byte to load, end of the DEFLATE data */
    uint64_t buf;                       /* LSB-first; bits above cnt are zero */
    uint32_t cnt;
} ssi_bits_t;

typedef struct ssi_dec {
    ssi_bits_t b;
    int state;                          /* 0: block header next, 1: in a Huffman block, 2: stored payload pending */
    int final;
    uint32_t stored_len;
} ssi_dec_t;

SSI_HD uint32_t ssi_le32(const uint8_t *p)
{
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

/* ---- bit reader ------------------------------------------------------------ */
/* After a refill the buffer holds at least 33 bits, or everything that is left. */
SSI_HD void ssi_refill(ssi_bits_t *b)
{
    if (b->cnt > 32) return;
    if (b->end - b->pos >= 4) {
        b->buf |= (uint64_t)ssi_le32(b->in + b->pos) << b->cnt;
        b->pos += 4;
        b->cnt += 32;
        return;
    }
    while (b->pos < b->end) {
        b->buf |= (uint64_t)b->in[b->pos++] << b->cnt;
        b->cnt += 8;
    }
}

SSI_HD uint32_t ssi_peek(const ssi_bits_t *b, uint32_t n) { return (uint32_t)b->buf & ((1u << n) - 1u); }

/* consume n bits; 0 when the input does not have them */
SSI_HD int ssi_drop(ssi_bits_t *b, uint32_t n)
{
    if (n > b->cnt) return 0;
    b->buf >>= n;
    b->cnt -= n;
    return 1;
}

/* n <= 16 bits, or -1 at the end of the input */
SSI_HD int32_t ssi_bits(ssi_bits_t *b, uint32_t n)
{
    ssi_refill(b);
    const uint32_t v = ssi_peek(b, n);
    return ssi_drop(b, n) ? (int32_t)v : -1;
}

/* ---- canonical Huffman tables ---------------------------------------------- */
#define SSI_KIND_CODES 0
#define SSI_KIND_LENS  1
#define SSI_KIND_DISTS 2

SSI_HD uint32_t ssi_rev(uint32_t code, uint32_t len)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < len; ++i) {
        r = r << 1 | (code & 1u);
        code >>= 1;
    }
    return r;
}

/* Builds count[16] / sym[n] (and fast[1 << fast_bits] unless fast is NULL) from
 * lens[0..n), n <= 288.  Returns 0, or -1 for a set zlib rejects (see the top). */
SSI_HD int ssi_build(ssi_tables_t *t, const uint8_t *lens, uint32_t n, uint16_t *count, uint16_t *sym,
                     uint16_t *fast, uint32_t fast_bits, int kind)
{
    for (uint32_t l = 0; l < 16; ++l) count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) count[lens[s] & 15u]++;
    if (fast)
        for (uint32_t i = 0; i < (1u << fast_bits); ++i) fast[i] = 0;
    if (count[0] == n) {                       /* no code at all */
        count[0] = 0;
        return kind == SSI_KIND_DISTS ? 0 : -1;
    }
    int32_t left = 1;
    uint32_t max = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        left = (left << 1) - (int32_t)count[l];
        if (left < 0) return -1;               /* over-subscribed */
        if (count[l]) max = l;
    }
    if (left > 0 && (kind == SSI_KIND_CODES || max != 1)) return -1;   /* incomplete */
    count[0] = 0;
    uint32_t off = 0, code = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        t->offs[l] = (uint16_t)off;
        t->next[l] = (uint16_t)code;
        off += count[l];
        code = (code + count[l]) << 1;
    }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = lens[s] & 15u;
        if (!l) continue;
        sym[t->offs[l]++] = (uint16_t)s;       /* offs[l] < count sum <= n */
        const uint32_t c = t->next[l]++;
        if (fast && l <= fast_bits) {
            const uint16_t e = (uint16_t)(s << 4 | l);
            for (uint32_t k = ssi_rev(c, l); k < (1u << fast_bits); k += 1u << l) fast[k] = e;
        }
    }
    return 0;
}

/* One symbol, or -1 (a code the set does not have, or the input ended). */
SSI_HD int32_t ssi_decode(ssi_bits_t *b, const uint16_t *fast, uint32_t fast_bits, const uint16_t *count,
                          const uint16_t *sym)
{
    const uint32_t v = ssi_peek(b, 15);
    if (fast) {
        const uint32_t e = fast[v & ((1u << fast_bits) - 1u)];
        if (e) return ssi_drop(b, e & 15u) ? (int32_t)(e >> 4) : -1;
    }
    int32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        code |= (int32_t)(v >> (l - 1) & 1u);
        const int32_t c = count[l];
        if (code - c < first) return ssi_drop(b, l) ? (int32_t)sym[index + (code - first)] : -1;
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

/* RFC 1951 3.2.5, computed: length symbols 257..285 and distance symbols 0..29 */
SSI_HD uint32_t ssi_len_extra(uint32_t s) { return s < 265u || s == 285u ? 0u : (s - 261u) >> 2; }
SSI_HD uint32_t ssi_len_base(uint32_t s)
{
    if (s < 265u) return s - 254u;
    if (s == 285u) return 258u;
    return 3u + ((4u + ((s - 261u) & 3u)) << ((s - 261u) >> 2));
}
SSI_HD uint32_t ssi_dist_extra(uint32_t s) { return s < 4u ? 0u : (s >> 1) - 1u; }
SSI_HD uint32_t ssi_dist_base(uint32_t s) { return s < 4u ? s + 1u : 1u + ((2u + (s & 1u)) << ((s >> 1) - 1u)); }

/* HCLEN order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each */
SSI_HD uint32_t ssi_clen_order(uint32_t i)
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                        6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12u ? lo >> (5u * i) : hi >> (5u * (i - 12u))) & 31u);
}

SSI_HD int ssi_setup_tables(ssi_tables_t *t, uint32_t nlen, uint32_t ndist)
{
    if (t->lens[256] == 0) return -1;          /* missing end-of-block code */
    if (ssi_build(t, t->lens, nlen, t->lit_count, t->lit_sym, t->lit_fast, SSI_FAST_LIT, SSI_KIND_LENS)) return -1;
    return ssi_build(t, t->lens + nlen, ndist, t->dist_count, t->dist_sym, t->dist_fast, SSI_FAST_DIST,
                     SSI_KIND_DISTS);
}

SSI_HD int ssi_fixed_header(ssi_tables_t *t)
{
    for (uint32_t s = 0; s < 288u; ++s) t->lens[s] = (uint8_t)(s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : 8);
    for (uint32_t s = 0; s < 32u; ++s) t->lens[288u + s] = 5;
    return ssi_setup_tables(t, 288u, 32u);
}

SSI_HD int ssi_dynamic_header(ssi_bits_t *b, ssi_tables_t *t)
{
    const int32_t hdr = ssi_bits(b, 14);
    if (hdr < 0) return -1;
    const uint32_t nlen = ((uint32_t)hdr & 31u) + 257u, ndist = ((uint32_t)hdr >> 5 & 31u) + 1u;
    const uint32_t ncode = ((uint32_t)hdr >> 10) + 4u;
    if (nlen > 286u || ndist > 30u) return -1;
    for (uint32_t i = 0; i < 19u; ++i) t->lens[i] = 0;
    for (uint32_t i = 0; i < ncode; ++i) {
        const int32_t v = ssi_bits(b, 3);
        if (v < 0) return -1;
        t->lens[ssi_clen_order(i)] = (uint8_t)v;
    }
    /* the code-length code lives in the distance arrays until the real sets are built */
    if (ssi_build(t, t->lens, 19u, t->dist_count, t->dist_sym, (uint16_t *)0, 0u, SSI_KIND_CODES)) return -1;
    /* one run of lengths for both sets: a repeat may cross from the
     * literal/length lengths into the distance lengths */
    uint32_t have = 0;
    while (have < nlen + ndist) {
        ssi_refill(b);
        const int32_t s = ssi_decode(b, (const uint16_t *)0, 0u, t->dist_count, t->dist_sym);
        if (s < 0) return -1;
        if (s < 16) {
            t->lens[have++] = (uint8_t)s;
            continue;
        }
        uint32_t rep, val = 0;
        if (s == 16) {
            if (have == 0) return -1;          /* nothing to repeat */
            val = t->lens[have - 1];
            const int32_t e = ssi_bits(b, 2);
            if (e < 0) return -1;
            rep = 3u + (uint32_t)e;
        } else {
            const int32_t e = ssi_bits(b, s == 17 ? 3u : 7u);
            if (e < 0) return -1;
            rep = (s == 17 ? 3u : 11u) + (uint32_t)e;
        }
        if (have + rep > nlen + ndist) return -1;
        while (rep--) t->lens[have++] = (uint8_t)val;
    }
    return ssi_setup_tables(t, nlen, ndist);
}

SSI_HD void ssi_init(ssi_dec_t *d, const uint8_t *in, uint32_t deflate_len)
{
    d->b.in = in;
    d->b.pos = 0;
    d->b.end = deflate_len;
    d->b.buf = 0;
    d->b.cnt = 0;
    d->state = 0;
    d->final = 0;
    d->stored_len = 0;
}

/* The next item (see the top).  Every call consumes input or ends the member,
 * so a member of clen bytes yields fewer than 8 * clen items. */
SSI_HD int ssi_next(ssi_dec_t *d, ssi_tables_t *t, uint32_t *val, uint32_t *dist)
{
    ssi_bits_t *b = &d->b;
    for (;;) {
        if (d->state == 0) {
            if (d->final) return SSI_END;
            const int32_t h = ssi_bits(b, 3);
            if (h < 0) return SSI_ERR;
            d->final = h & 1;
            const int32_t type = h >> 1;
            if (type == 0) {
                if (!ssi_drop(b, b->cnt & 7u)) return SSI_ERR;
                ssi_refill(b);                 /* whole bytes: 40 bits or the rest */
                if (b->cnt < 32u) return SSI_ERR;
                const uint32_t w = (uint32_t)b->buf;
                ssi_drop(b, 32u);
                if ((w & 0xffffu) != (~w >> 16)) return SSI_ERR;     /* LEN != ~NLEN */
                b->pos -= b->cnt >> 3;         /* hand the buffered whole bytes back */
                b->buf = 0;
                b->cnt = 0;
                if ((w & 0xffffu) > b->end - b->pos) return SSI_ERR;
                d->stored_len = w & 0xffffu;
                d->state = 2;
            } else if (type == 1) {
                if (ssi_fixed_header(t)) return SSI_ERR;
                d->state = 1;
            } else if (type == 2) {
                if (ssi_dynamic_header(b, t)) return SSI_ERR;
                d->state = 1;
            } else {
                return SSI_ERR;
            }
            continue;
        }
        if (d->state == 2) {
            d->state = 0;
            if (d->stored_len == 0) continue;
            *val = d->stored_len;
            *dist = b->pos;
            b->pos += d->stored_len;
            return SSI_STORED;
        }
        ssi_refill(b);
        const int32_t s = ssi_decode(b, t->lit_fast, SSI_FAST_LIT, t->lit_count, t->lit_sym);
        if (s < 0) return SSI_ERR;
        if (s < 256) {
            *val = (uint32_t)s;
            return SSI_LIT;
        }
        if (s == 256) {
            d->state = 0;
            continue;
        }
        if (s > 285) return SSI_ERR;           /* 286, 287: in the fixed code, never valid */
        const uint32_t le = ssi_len_extra((uint32_t)s);
        const uint32_t len = ssi_len_base((uint32_t)s) + ssi_peek(b, le);
        if (!ssi_drop(b, le)) return SSI_ERR;
        ssi_refill(b);
        const int32_t ds = ssi_decode(b, t->dist_fast, SSI_FAST_DIST, t->dist_count, t->dist_sym);
        if (ds < 0 || ds > 29) return SSI_ERR; /* 30, 31: never valid */
        const uint32_t de = ssi_dist_extra((uint32_t)ds);
        *dist = ssi_dist_base((uint32_t)ds) + ssi_peek(b, de);
        if (!ssi_drop(b, de)) return SSI_ERR;
        *val = len;
        return SSI_MATCH;
    }
}

/* ---- CRC-32 (gzip: reflected polynomial 0xEDB88320) -------------------------- */
SSI_HD uint32_t ssi_crc_entry(uint32_t i)
{
    for (int k = 0; k < 8; ++k) i = i & 1u ? i >> 1 ^ 0xEDB88320u : i >> 1;
    return i;
}

/* the raw register (start from 0xffffffff, invert at the end) */
SSI_HD uint32_t ssi_crc_bytes(const uint32_t *tab, uint32_t c, const uint8_t *p, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 255u] ^ c >> 8;
    return c;
}

/* a(x) * b(x) mod P, reflected (zlib's multmodp) */
SSI_HD uint32_t ssi_mulmodp(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = b & 1u ? b >> 1 ^ 0xEDB88320u : b >> 1;
    }
    return p;
}

/* x^(8 n) mod P */
SSI_HD uint32_t ssi_xpow8(uint32_t n)
{
    uint32_t p = 1u << 31, sq = 1u << 23;      /* x^0, x^8 */
    for (; n; n >>= 1) {
        if (n & 1u) p = ssi_mulmodp(sq, p);
        sq = ssi_mulmodp(sq, sq);
    }
    return p;
}

/* CRC of A||B from the finished CRCs of A and B (zlib's crc32_combine) */
SSI_HD uint32_t ssi_crc_combine(uint32_t crc_a, uint32_t crc_b, uint32_t len_b)
{
    return ssi_mulmodp(ssi_xpow8(len_b), crc_a) ^ crc_b;
}

/* ---- one member on the calling thread ------------------------------------------
 * in[0..clen): DEFLATE data + the 8-byte trailer.  Writes out[0..olen) only; a
 * member that fails has its whole span zeroed, so a failed member's bytes do
 * not depend on where the decoder stopped. */
SSI_HD uint32_t ssi_decode_member(const uint8_t *in, uint32_t clen, uint8_t *out, uint32_t olen, ssi_tables_t *t,
                                  const uint32_t *crc_tab)
{
    if (clen < 8u) return SSI_E_STREAM;
    const uint32_t crc = ssi_le32(in + clen - 8u), isize = ssi_le32(in + clen - 4u);
    if (isize != olen) return SSI_E_SIZE;
    ssi_dec_t d;
    ssi_init(&d, in, clen - 8u);
    uint32_t op = 0;
    for (;;) {
        uint32_t val = 0, dist = 0;
        const int k = ssi_next(&d, t, &val, &dist);
        if (k == SSI_END) break;
        if (k == SSI_ERR) return SSI_E_STREAM;
        if (k == SSI_LIT) {
            if (op >= olen) return SSI_E_STREAM;
            out[op++] = (uint8_t)val;
        } else if (k == SSI_MATCH) {
            if (dist > op || val > olen - op) return SSI_E_STREAM;
            for (uint32_t i = 0; i < val; ++i) out[op + i] = out[op - dist + i];
            op += val;
        } else {
            if (val > olen - op) return SSI_E_STREAM;
            for (uint32_t i = 0; i < val; ++i) out[op + i] = in[dist + i];
            op += val;
        }
    }
    if (op != isize) return SSI_E_SIZE;
    if ((ssi_crc_bytes(crc_tab, 0xffffffffu, out, op) ^ 0xffffffffu) != crc) return SSI_E_CRC;
    return SSI_OK;
}

SSI_HD uint32_t ssi_inflate_member(const uint8_t *in, uint32_t clen, uint8_t *out, uint32_t olen, ssi_tables_t *t,
                                   const uint32_t *crc_tab)
{
    const uint32_t st = ssi_decode_member(in, clen, out, olen, t, crc_tab);
    if (st != SSI_OK)
        for (uint32_t i = 0; i < olen; ++i) out[i] = 0;
    return st;
}

#endif /* SS_INFLATE_CORE_H */
