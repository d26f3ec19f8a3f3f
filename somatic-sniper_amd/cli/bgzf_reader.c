/* bgzf_reader.c -- see bgzf_reader.h.
 *
 * A BGZF file is a series of gzip members of at most 64 KiB each, whose gzip
 * header carries the member size in the "BC" extra subfield.  Members are
 * independent, so they are inflated in parallel: one I/O thread cuts the file
 * into members and queues them in a ring of slots, workers inflate slots, and
 * the consumer drains slots strictly in file order.
 *
 * Batched mode (bgzf_open_batched): the same ring and consumer, but one batch
 * thread hands whole groups of loaded members to a callback (the GPU inflater
 * in the CLI) instead of workers inflating one member each. */
#include "bgzf_reader.h"

#include <dlfcn.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#define BLK_MAX  65536
#define N_SLOTS  64

enum { SLOT_FREE, SLOT_LOADED, SLOT_BUSY, SLOT_DONE, SLOT_EOF, SLOT_ERR };

typedef struct {
    int state;
    uint32_t clen, ulen, pos;
    uint8_t cbuf[BLK_MAX];
    uint8_t ubuf[BLK_MAX];
} slot_t;

/* batched mode: slot i's compressed bytes are bc + i * BLK_MAX; its output is
 * wherever its batch's packed output put it (u, inside the arena) */
typedef struct {
    int state;
    uint32_t clen, ulen, pos;
    uint8_t *u;
} bslot_t;

struct bgzf_reader {
    FILE *fp;
    int own_fp;
    int n_threads;
    /* synchronous mode */
    slot_t *one;
    void *dec;
    int eof;
    int64_t coff_cur, coff_next;   /* file offsets of the current member and the next one */
    /* threaded mode */
    slot_t *slots;
    slot_t *cur;          /* the slot the consumer is draining (it owns it: no lock) */
    uint64_t next_load, next_read, next_work;
    int stop, io_done;
    pthread_mutex_t mu;
    pthread_cond_t cv_load, cv_work, cv_read;
    pthread_t io;
    pthread_t *workers;
    char err[160];
    /* batched mode (next_load / next_read / next_work, the lock and the conditions as above) */
    bslot_t *bs;
    int batch, n_slots;
    uint8_t *bc;                  /* [n_slots][BLK_MAX] compressed members as read */
    uint8_t *arena;               /* [n_slots][BLK_MAX] output; a batch packs its members from its first slot's place */
    uint8_t *stage;               /* [batch][BLK_MAX] one batch's compressed members, packed */
    uint64_t *coff, *ooff;
    uint32_t *status;
    bgzf_batch_ops_t ops;
    pthread_t bt;
    uint64_t st_members, st_batches, st_fallback;
    void *bcur;                   /* the bslot_t the consumer is draining */
};

/* Reads one member into s (compressed payload + trailer sizes).  Returns 1,
 * 0 at clean end of file, -1 on error. */
static int read_member_into(FILE *fp, uint8_t *cbuf, uint32_t *clen_out, char *err);

static int read_member(FILE *fp, slot_t *s, char *err) { return read_member_into(fp, s->cbuf, &s->clen, err); }

static int read_member_into(FILE *fp, uint8_t *cbuf, uint32_t *clen_out, char *err)
{
    uint8_t h[18];
    size_t got = fread(h, 1, 12, fp);
    if (got == 0) return 0;
    if (got != 12 || h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) {
        snprintf(err, 160, "not a BGZF file (bad gzip member header)");
        return -1;
    }
    const uint32_t xlen = (uint32_t)h[10] | (uint32_t)h[11] << 8;
    uint8_t extra[256];
    if (xlen > sizeof extra || fread(extra, 1, xlen, fp) != xlen) {
        snprintf(err, 160, "truncated BGZF header");
        return -1;
    }
    int bsize = -1;
    for (uint32_t p = 0; p + 4 <= xlen;) {
        const uint32_t sl = (uint32_t)extra[p + 2] | (uint32_t)extra[p + 3] << 8;
        if (extra[p] == 'B' && extra[p + 1] == 'C' && sl == 2 && p + 6 <= xlen)
            bsize = (int)((uint32_t)extra[p + 4] | (uint32_t)extra[p + 5] << 8);
        p += 4 + sl;
    }
    if (bsize < 0) {
        snprintf(err, 160, "gzip member without a BGZF block size");
        return -1;
    }
    const long clen = (long)bsize + 1 - 12 - (long)xlen;      /* deflate data + 8-byte trailer */
    if (clen < 8 || clen > BLK_MAX || fread(cbuf, 1, (size_t)clen, fp) != (size_t)clen) {
        snprintf(err, 160, "truncated BGZF block");
        return -1;
    }
    *clen_out = (uint32_t)clen;
    return 1;
}

/* libdeflate (whole-buffer DEFLATE, 2-3x zlib's inflate rate) is used when
 * the system has it; zlib otherwise.  Only its stable C ABI (libdeflate.h,
 * v1.x) is bound, at run time, so the build does not need its header. */
typedef struct {
    void *(*alloc)(void);
    void (*release)(void *);
    int (*decompress)(void *, const void *, size_t, void *, size_t, size_t *);
    uint32_t (*crc)(uint32_t, const void *, size_t);
} deflate_lib_t;

static deflate_lib_t LD;
static pthread_once_t ld_once = PTHREAD_ONCE_INIT;

static void ld_load(void)
{
    const char *off = getenv("SS_NO_LIBDEFLATE");
    if (off && *off && *off != '0') return;
    void *h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
    deflate_lib_t l;
    *(void **)&l.alloc = dlsym(h, "libdeflate_alloc_decompressor");
    *(void **)&l.release = dlsym(h, "libdeflate_free_decompressor");
    *(void **)&l.decompress = dlsym(h, "libdeflate_deflate_decompress");
    *(void **)&l.crc = dlsym(h, "libdeflate_crc32");
    if (l.alloc && l.release && l.decompress && l.crc) LD = l;
}

/* per-thread decompressor: NULL selects zlib */
static void *dec_new(void)
{
    pthread_once(&ld_once, ld_load);
    return LD.alloc ? LD.alloc() : NULL;
}

static void dec_free(void *d)
{
    if (d) LD.release(d);
}

/* cbuf[0..clen): DEFLATE data + trailer; at most `avail` bytes are written to ubuf */
static int inflate_raw(uint8_t *cbuf, uint32_t clen, uint8_t *ubuf, uint32_t avail, uint32_t *ulen, void *dec)
{
    const uint8_t *t = cbuf + clen - 8;
    const uint32_t isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
    if (isize > BLK_MAX) return -1;
    const uint32_t crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
    if (dec) {
        size_t got = 0;
        if (LD.decompress(dec, cbuf, clen - 8, ubuf, avail, &got) != 0 || got != isize) return -1;
        if (LD.crc(0, ubuf, isize) != crc) return -1;
        *ulen = isize;
        return 0;
    }
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return -1;
    z.next_in = cbuf;
    z.avail_in = clen - 8;
    z.next_out = ubuf;
    z.avail_out = avail;
    const int rc = inflate(&z, Z_FINISH);
    inflateEnd(&z);
    if (rc != Z_STREAM_END || z.total_out != isize) return -1;
    if ((uint32_t)crc32(0L, ubuf, isize) != crc) return -1;
    *ulen = isize;
    return 0;
}

static int inflate_member(slot_t *s, void *dec)
{
    if (inflate_raw(s->cbuf, s->clen, s->ubuf, BLK_MAX, &s->ulen, dec)) return -1;
    s->pos = 0;
    return 0;
}

static void *io_main(void *arg)
{
    bgzf_reader_t *r = (bgzf_reader_t *)arg;
    for (;;) {
        pthread_mutex_lock(&r->mu);
        slot_t *s = &r->slots[r->next_load % N_SLOTS];
        while (!r->stop && s->state != SLOT_FREE) pthread_cond_wait(&r->cv_load, &r->mu);
        if (r->stop) { pthread_mutex_unlock(&r->mu); return NULL; }
        pthread_mutex_unlock(&r->mu);
        char err[160] = {0};
        const int rc = read_member(r->fp, s, err);
        pthread_mutex_lock(&r->mu);
        if (rc == 1) s->state = SLOT_LOADED;
        else {
            s->state = rc == 0 ? SLOT_EOF : SLOT_ERR;
            if (rc < 0) memcpy(r->err, err, sizeof err);
            r->io_done = 1;
        }
        ++r->next_load;
        pthread_cond_broadcast(&r->cv_work);
        pthread_cond_broadcast(&r->cv_read);
        const int done = rc != 1;
        pthread_mutex_unlock(&r->mu);
        if (done) return NULL;
    }
}

static void *worker_main(void *arg)
{
    bgzf_reader_t *r = (bgzf_reader_t *)arg;
    void *dec = dec_new();
    pthread_mutex_lock(&r->mu);
    for (;;) {
        while (!r->stop && r->next_work >= r->next_load && !r->io_done)
            pthread_cond_wait(&r->cv_work, &r->mu);
        if (r->stop || r->next_work >= r->next_load) break;
        slot_t *s = &r->slots[r->next_work % N_SLOTS];
        if (s->state != SLOT_LOADED) break;            /* end-of-file or error marker */
        ++r->next_work;
        s->state = SLOT_BUSY;
        pthread_mutex_unlock(&r->mu);
        const int rc = inflate_member(s, dec);
        pthread_mutex_lock(&r->mu);
        s->state = rc == 0 ? SLOT_DONE : SLOT_ERR;
        if (rc) snprintf(r->err, sizeof r->err, "corrupt BGZF block (inflate / CRC)");
        pthread_cond_broadcast(&r->cv_read);
    }
    pthread_cond_broadcast(&r->cv_work);
    pthread_mutex_unlock(&r->mu);
    dec_free(dec);
    return NULL;
}

/* ---- batched mode ------------------------------------------------------------ */
static void *bio_main(void *arg)
{
    bgzf_reader_t *r = (bgzf_reader_t *)arg;
    for (;;) {
        pthread_mutex_lock(&r->mu);
        const size_t i = (size_t)(r->next_load % (uint64_t)r->n_slots);
        bslot_t *s = &r->bs[i];
        while (!r->stop && s->state != SLOT_FREE) pthread_cond_wait(&r->cv_load, &r->mu);
        if (r->stop) { pthread_mutex_unlock(&r->mu); return NULL; }
        pthread_mutex_unlock(&r->mu);
        char err[160] = {0};
        const int rc = read_member_into(r->fp, r->bc + i * BLK_MAX, &s->clen, err);
        pthread_mutex_lock(&r->mu);
        if (rc == 1) s->state = SLOT_LOADED;
        else {
            s->state = rc == 0 ? SLOT_EOF : SLOT_ERR;
            if (rc < 0) memcpy(r->err, err, sizeof err);
            r->io_done = 1;
        }
        ++r->next_load;
        pthread_cond_broadcast(&r->cv_work);
        pthread_cond_broadcast(&r->cv_read);
        const int done = rc != 1;
        pthread_mutex_unlock(&r->mu);
        if (done) return NULL;
    }
}

static void *batch_main(void *arg)
{
    bgzf_reader_t *r = (bgzf_reader_t *)arg;
    void *dec = dec_new();                                 /* for members the callback turns down */
    const uint64_t B = (uint64_t)r->batch;
    pthread_mutex_lock(&r->mu);
    for (;;) {
        /* a whole group of `batch` slots (groups do not wrap the ring), or what the file still had */
        const uint64_t g_end = (r->next_work / B + 1) * B;
        while (!r->stop && r->next_load < g_end && !r->io_done) pthread_cond_wait(&r->cv_work, &r->mu);
        if (r->stop) break;
        const uint64_t first = r->next_work, lim = r->next_load < g_end ? r->next_load : g_end;
        uint32_t k = 0;
        while (first + k < lim && r->bs[(first + k) % (uint64_t)r->n_slots].state == SLOT_LOADED) ++k;
        if (k == 0) break;                                 /* the end-of-file or error marker */
        bslot_t *s0 = &r->bs[first % (uint64_t)r->n_slots];
        const uint8_t *c0 = r->bc + (size_t)(first % (uint64_t)r->n_slots) * BLK_MAX;
        uint8_t *base = r->arena + (size_t)(first % (uint64_t)r->n_slots) * BLK_MAX;
        for (uint32_t i = 0; i < k; ++i) s0[i].state = SLOT_BUSY;
        r->next_work += k;
        pthread_mutex_unlock(&r->mu);
        r->coff[0] = r->ooff[0] = 0;
        for (uint32_t i = 0; i < k; ++i) {
            const uint8_t *c = c0 + (size_t)i * BLK_MAX;
            memcpy(r->stage + r->coff[i], c, s0[i].clen);
            r->coff[i + 1] = r->coff[i] + s0[i].clen;
            const uint8_t *t = c + s0[i].clen - 4;
            const uint32_t isize = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
            r->ooff[i + 1] = r->ooff[i] + (isize <= BLK_MAX ? isize : 0);   /* oversized: fails below */
            r->status[i] = 1;
        }
        const int rc = r->ops.inflate(r->ops.user, r->stage, r->coff, k, base, r->ooff, r->status);
        uint32_t fell = 0;
        int bad = rc != 0;
        for (uint32_t i = 0; i < k && !bad; ++i) {
            s0[i].u = base + r->ooff[i];
            s0[i].ulen = (uint32_t)(r->ooff[i + 1] - r->ooff[i]);
            s0[i].pos = 0;
            if (r->status[i] == 0) continue;
            ++fell;                                            /* the host decides, with today's error */
            uint32_t got = 0;
            if (inflate_raw(r->stage + r->coff[i], s0[i].clen, s0[i].u, s0[i].ulen, &got, dec) == 0 && got == s0[i].ulen)
                r->status[i] = 0;
        }
        pthread_mutex_lock(&r->mu);
        for (uint32_t i = 0; i < k; ++i) {
            if (bad) {
                s0[i].state = SLOT_ERR;
                snprintf(r->err, sizeof r->err, "BGZF batch inflation failed (code %d)", rc);
            } else if (r->status[i]) {
                s0[i].state = SLOT_ERR;
                snprintf(r->err, sizeof r->err, "corrupt BGZF block (inflate / CRC)");
            } else {
                s0[i].state = SLOT_DONE;
            }
        }
        r->st_members += k;
        r->st_batches += 1;
        r->st_fallback += fell;
        pthread_cond_broadcast(&r->cv_read);
    }
    pthread_cond_broadcast(&r->cv_work);
    pthread_mutex_unlock(&r->mu);
    dec_free(dec);
    return NULL;
}

bgzf_reader_t *bgzf_open_batched(const char *path, uint64_t voff, int batch, const bgzf_batch_ops_t *ops)
{
    if (!ops || !ops->inflate || batch < 1 || batch > 4096 || (voff && strcmp(path, "-") == 0)) return NULL;
    bgzf_reader_t *r = (bgzf_reader_t *)calloc(1, sizeof *r);
    if (!r) return NULL;
    if (strcmp(path, "-") == 0) r->fp = stdin;
    else { r->fp = fopen(path, "rb"); r->own_fp = 1; }
    if (!r->fp) { free(r); return NULL; }
    const int64_t coff = (int64_t)(voff >> 16);
    if (coff > 0 && fseeko(r->fp, (off_t)coff, SEEK_SET) != 0) { fclose(r->fp); free(r); return NULL; }
    r->ops = *ops;
    r->batch = batch;
    r->n_slots = batch * (batch >= 32 ? 2 : (64 + batch - 1) / batch);     /* >= 2 groups and >= 64 slots */
    const size_t ns = (size_t)r->n_slots;
    r->bs = (bslot_t *)calloc(ns, sizeof(bslot_t));
    r->bc = (uint8_t *)malloc(ns * BLK_MAX);
    r->coff = (uint64_t *)calloc((size_t)batch + 1, sizeof(uint64_t));
    r->ooff = (uint64_t *)calloc((size_t)batch + 1, sizeof(uint64_t));
    r->status = (uint32_t *)calloc((size_t)batch, sizeof(uint32_t));
    r->arena = (uint8_t *)(ops->alloc ? ops->alloc(ns * BLK_MAX) : malloc(ns * BLK_MAX));
    r->stage = (uint8_t *)(ops->alloc ? ops->alloc((size_t)batch * BLK_MAX) : malloc((size_t)batch * BLK_MAX));
    if (!r->bs || !r->bc || !r->coff || !r->ooff || !r->status || !r->arena || !r->stage) {
        r->n_slots = 0;                                        /* no thread was started */
        bgzf_close(r);
        return NULL;
    }
    pthread_mutex_init(&r->mu, NULL);
    pthread_cond_init(&r->cv_load, NULL);
    pthread_cond_init(&r->cv_work, NULL);
    pthread_cond_init(&r->cv_read, NULL);
    pthread_create(&r->io, NULL, bio_main, r);
    pthread_create(&r->bt, NULL, batch_main, r);
    uint8_t skip[65536];
    const size_t k = (size_t)(voff & 0xffffu);
    if (k && bgzf_read(r, skip, k) != (long)k) { bgzf_close(r); return NULL; }
    return r;
}

int bgzf_batch_stats(const bgzf_reader_t *r, uint64_t *members, uint64_t *batches, uint64_t *fallback, void **user)
{
    if (!r || !r->bs) return 0;
    pthread_mutex_lock((pthread_mutex_t *)&r->mu);
    if (members) *members = r->st_members;
    if (batches) *batches = r->st_batches;
    if (fallback) *fallback = r->st_fallback;
    pthread_mutex_unlock((pthread_mutex_t *)&r->mu);
    if (user) *user = r->ops.user;
    return 1;
}

static bgzf_reader_t *open_common(const char *path, int n_threads, int64_t coff)
{
    bgzf_reader_t *r = (bgzf_reader_t *)calloc(1, sizeof *r);
    if (!r) return NULL;
    if (strcmp(path, "-") == 0) r->fp = stdin;
    else { r->fp = fopen(path, "rb"); r->own_fp = 1; }
    if (!r->fp) { free(r); return NULL; }
    if (coff > 0 && fseeko(r->fp, (off_t)coff, SEEK_SET) != 0) { fclose(r->fp); free(r); return NULL; }
    r->coff_cur = r->coff_next = coff;
    r->n_threads = n_threads;
    if (n_threads <= 0) {
        r->one = (slot_t *)calloc(1, sizeof(slot_t));
        if (!r->one) { bgzf_close(r); return NULL; }
        r->one->state = SLOT_FREE;
        r->dec = dec_new();
        return r;
    }
    r->slots = (slot_t *)calloc(N_SLOTS, sizeof(slot_t));
    r->workers = (pthread_t *)calloc((size_t)n_threads, sizeof(pthread_t));
    if (!r->slots || !r->workers) { bgzf_close(r); return NULL; }
    pthread_mutex_init(&r->mu, NULL);
    pthread_cond_init(&r->cv_load, NULL);
    pthread_cond_init(&r->cv_work, NULL);
    pthread_cond_init(&r->cv_read, NULL);
    pthread_create(&r->io, NULL, io_main, r);
    for (int i = 0; i < n_threads; ++i) pthread_create(&r->workers[i], NULL, worker_main, r);
    return r;
}

bgzf_reader_t *bgzf_open(const char *path, int n_threads) { return open_common(path, n_threads, 0); }

bgzf_reader_t *bgzf_open_at(const char *path, int n_threads, uint64_t voff)
{
    if (strcmp(path, "-") == 0) return NULL;
    bgzf_reader_t *r = open_common(path, n_threads, (int64_t)(voff >> 16));
    if (!r) return NULL;
    uint8_t skip[65536];
    const size_t k = (size_t)(voff & 0xffffu);
    if (k && bgzf_read(r, skip, k) != (long)k) { bgzf_close(r); return NULL; }
    return r;
}

int64_t bgzf_tell(const bgzf_reader_t *r)
{
    if (r->slots || r->bs) return -1;
    const slot_t *s = r->one;
    if (s->state != SLOT_DONE || s->pos == s->ulen) return r->coff_next << 16;
    return r->coff_cur << 16 | (int64_t)s->pos;
}

long bgzf_read(bgzf_reader_t *r, void *dst, size_t n)
{
    uint8_t *out = (uint8_t *)dst;
    size_t done = 0;
    if (r->bs) {                                       /* batched: the threaded drain below, on the batch ring */
        while (done < n) {
            bslot_t *s = (bslot_t *)r->bcur;
            if (!s) {
                pthread_mutex_lock(&r->mu);
                s = &r->bs[r->next_read % (uint64_t)r->n_slots];
                while (r->next_read >= r->next_load || (s->state != SLOT_DONE && s->state != SLOT_EOF &&
                                                         s->state != SLOT_ERR))
                    pthread_cond_wait(&r->cv_read, &r->mu);
                const int st = s->state;
                pthread_mutex_unlock(&r->mu);
                if (st == SLOT_EOF) break;
                if (st == SLOT_ERR) return -1;
                r->bcur = s;
            }
            size_t k = s->ulen - s->pos;
            if (k > n - done) k = n - done;
            memcpy(out + done, s->u + s->pos, k);
            s->pos += (uint32_t)k;
            done += k;
            if (s->pos == s->ulen) {
                r->bcur = NULL;
                pthread_mutex_lock(&r->mu);
                s->state = SLOT_FREE;
                ++r->next_read;
                pthread_cond_broadcast(&r->cv_load);
                pthread_mutex_unlock(&r->mu);
            }
        }
        return (long)done;
    }
    if (!r->slots) {                                   /* synchronous */
        slot_t *s = r->one;
        while (done < n) {
            if (s->state != SLOT_DONE || s->pos == s->ulen) {
                if (r->eof) break;
                const int64_t at = r->coff_next;
                const int rc = read_member(r->fp, s, r->err);
                if (rc == 0) { r->eof = 1; break; }
                if (rc < 0 || inflate_member(s, r->dec)) {
                    if (!r->err[0]) snprintf(r->err, sizeof r->err, "corrupt BGZF block (inflate / CRC)");
                    return -1;
                }
                s->state = SLOT_DONE;
                r->coff_cur = at;
                r->coff_next = (int64_t)ftello(r->fp);
                continue;
            }
            size_t k = s->ulen - s->pos;
            if (k > n - done) k = n - done;
            memcpy(out + done, s->ubuf + s->pos, k);
            s->pos += (uint32_t)k;
            done += k;
        }
        return (long)done;
    }
    while (done < n) {
        slot_t *s = r->cur;
        if (!s) {                                      /* wait for the next member in file order */
            pthread_mutex_lock(&r->mu);
            s = &r->slots[r->next_read % N_SLOTS];
            while (r->next_read >= r->next_load || (s->state != SLOT_DONE && s->state != SLOT_EOF &&
                                                     s->state != SLOT_ERR))
                pthread_cond_wait(&r->cv_read, &r->mu);
            const int st = s->state;
            pthread_mutex_unlock(&r->mu);
            if (st == SLOT_EOF) break;
            if (st == SLOT_ERR) return -1;
            r->cur = s;
        }
        size_t k = s->ulen - s->pos;
        if (k > n - done) k = n - done;
        memcpy(out + done, s->ubuf + s->pos, k);
        s->pos += (uint32_t)k;
        done += k;
        if (s->pos == s->ulen) {                       /* drained: hand the slot back to the loader */
            r->cur = NULL;
            pthread_mutex_lock(&r->mu);
            s->state = SLOT_FREE;
            ++r->next_read;
            pthread_cond_broadcast(&r->cv_load);
            pthread_mutex_unlock(&r->mu);
        }
    }
    return (long)done;
}

const char *bgzf_error(const bgzf_reader_t *r) { return r->err[0] ? r->err : "ok"; }

void bgzf_close(bgzf_reader_t *r)
{
    if (!r) return;
    if (r->slots) {
        pthread_mutex_lock(&r->mu);
        r->stop = 1;
        pthread_cond_broadcast(&r->cv_load);
        pthread_cond_broadcast(&r->cv_work);
        pthread_mutex_unlock(&r->mu);
        pthread_join(r->io, NULL);
        for (int i = 0; i < r->n_threads; ++i) pthread_join(r->workers[i], NULL);
        pthread_mutex_destroy(&r->mu);
        pthread_cond_destroy(&r->cv_load);
        pthread_cond_destroy(&r->cv_work);
        pthread_cond_destroy(&r->cv_read);
    }
    if (r->bs && r->n_slots) {
        pthread_mutex_lock(&r->mu);
        r->stop = 1;
        pthread_cond_broadcast(&r->cv_load);
        pthread_cond_broadcast(&r->cv_work);
        pthread_mutex_unlock(&r->mu);
        pthread_join(r->io, NULL);
        pthread_join(r->bt, NULL);
        pthread_mutex_destroy(&r->mu);
        pthread_cond_destroy(&r->cv_load);
        pthread_cond_destroy(&r->cv_work);
        pthread_cond_destroy(&r->cv_read);
    }
    if (r->ops.release) {
        if (r->arena) r->ops.release(r->arena);
        if (r->stage) r->ops.release(r->stage);
    } else {
        free(r->arena);
        free(r->stage);
    }
    free(r->bs);
    free(r->bc);
    free(r->coff);
    free(r->ooff);
    free(r->status);
    free(r->slots);
    free(r->workers);
    free(r->one);
    dec_free(r->dec);
    if (r->own_fp && r->fp) fclose(r->fp);
    free(r);
}
