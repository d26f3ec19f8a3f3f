/* pileup_driver.c -- stand-alone driver of the shared pileup core
 * (somatic-sniper_amd/csrc/ss_pileup_core.h), the CPU twin and the planner
 * (csrc/ss_pileup_plan.c) for the sanitizer build
 * (make -C somatic-sniper_amd sanitize -> build/san/pileup-asan).
 *
 *   pileup-asan corpus.bin
 *
 * corpus.bin (tests/pileup_model.py write_corpus): u32 count, then per case
 * i32 lo, hi, expected return code (99: any, mutated records), ref_len (-1:
 * no reference) + the reference bytes, and per sample u32 n, u64 n_bytes, the
 * bytes, n u64 record offsets, n i32 `from`.  Every input gets a heap block of
 * exactly its length and every output one of exactly the size the first call
 * reports, so a read or write outside them is an ASan report; UBSan watches
 * the loads, shifts and arithmetic.  The planner then walks each sample's
 * bytes.  Prints "ok=1 cases=N" and exits 0 when every return code matched. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sniper_amd.h"

static int rd(FILE *f, void *p, size_t n) { return n && fread(p, 1, n, f) != n ? -1 : 0; }

static void *exact(size_t n)
{
    void *p = malloc(n ? n : 1);
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    return p;
}

typedef struct {
    uint8_t *bytes;
    uint64_t *off;
    int32_t *from;
    ss_pileup_sample_t s;
} sample_t;

static int read_sample(FILE *f, sample_t *x)
{
    uint32_t n;
    uint64_t nb;
    if (rd(f, &n, 4) || rd(f, &nb, 8) || nb > (1u << 28) || n > (1u << 24)) return -1;
    x->bytes = (uint8_t *)exact((size_t)nb);
    x->off = (uint64_t *)exact(sizeof(uint64_t) * n);
    x->from = (int32_t *)exact(sizeof(int32_t) * n);
    if (rd(f, x->bytes, (size_t)nb) || rd(f, x->off, sizeof(uint64_t) * n) || rd(f, x->from, sizeof(int32_t) * n))
        return -1;
    x->s.bytes = x->bytes;
    x->s.n_bytes = nb;
    x->s.rec_off = x->off;
    x->s.from = x->from;
    x->s.n = n;
    x->s.pad = 0;
    return 0;
}

static void free_sample(sample_t *x)
{
    free(x->bytes);
    free(x->off);
    free(x->from);
}

static void plan(const sample_t *x)
{
    const uint32_t cap = (uint32_t)(x->s.n_bytes / 36 + 1);
    uint64_t *off = (uint64_t *)exact(sizeof(uint64_t) * cap);
    int32_t *from = (int32_t *)exact(sizeof(int32_t) * cap), *tid = (int32_t *)exact(sizeof(int32_t) * cap);
    ss_pileup_state_t st;
    memset(&st, 0, sizeof st);
    uint32_t n = 0;
    size_t used = 0;
    (void)ss_pileup_plan(x->bytes, (size_t)x->s.n_bytes, -1, 0, &st, off, from, tid, cap, &n, &used);
    if (n > cap || used > x->s.n_bytes) { fprintf(stderr, "planner passed its bounds\n"); exit(1); }
    free(off);
    free(from);
    free(tid);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s corpus.bin\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    uint32_t n_cases = 0;
    if (!f || rd(f, &n_cases, 4)) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    int bad = 0;
    for (uint32_t i = 0; i < n_cases; ++i) {
        int32_t hd[4];
        if (rd(f, hd, sizeof hd) || hd[3] > (1 << 24)) { fprintf(stderr, "case %u: bad header\n", i); return 2; }
        const int32_t lo = hd[0], hi = hd[1], want = hd[2], ref_len = hd[3];
        uint8_t *ref = ref_len >= 0 ? (uint8_t *)exact((size_t)ref_len) : NULL;
        sample_t t, n;
        if ((ref_len > 0 && rd(f, ref, (size_t)ref_len)) || read_sample(f, &t) || read_sample(f, &n)) {
            fprintf(stderr, "case %u: short read\n", i);
            return 2;
        }
        ss_pileup_out_t o;
        memset(&o, 0, sizeof o);
        uint32_t off0[2] = {0, 0}, none[1] = {0};       /* capacities 0: only off_*[0] may be stored */
        o.pos = (int32_t *)none;
        o.ref = (uint8_t *)none;
        o.raw_t = o.raw_n = o.reads_t = o.reads_n = none;
        o.off_t = &off0[0];
        o.off_n = &off0[1];
        int rc = ss_pileup_region_cpu(&t.s, &n.s, ref, ref_len < 0 ? 0 : ref_len, lo, hi, &o);
        if (rc == SS_E_CAPACITY || rc == SS_OK) {
            /* outputs of exactly the sizes reported, then the call again */
            const size_t ns = (size_t)o.n_sites, nt = (size_t)o.n_reads_t, nn = (size_t)o.n_reads_n;
            o.cap_sites = ns;
            o.cap_reads_t = nt;
            o.cap_reads_n = nn;
            o.pos = (int32_t *)exact(4 * ns);
            o.ref = (uint8_t *)exact(ns);
            o.raw_t = (uint32_t *)exact(4 * ns);
            o.raw_n = (uint32_t *)exact(4 * ns);
            o.off_t = (uint32_t *)exact(4 * (ns + 1));
            o.off_n = (uint32_t *)exact(4 * (ns + 1));
            o.reads_t = (uint32_t *)exact(4 * nt);
            o.reads_n = (uint32_t *)exact(4 * nn);
            rc = ss_pileup_region_cpu(&t.s, &n.s, ref, ref_len < 0 ? 0 : ref_len, lo, hi, &o);
            if (rc == SS_E_CAPACITY || o.n_sites != ns || o.n_reads_t != nt || o.n_reads_n != nn) {
                fprintf(stderr, "case %u: the second call disagrees with the first\n", i);
                bad = 1;
            } else if (o.off_t[ns] != nt || o.off_n[ns] != nn) {
                fprintf(stderr, "case %u: offsets do not end at the totals\n", i);
                bad = 1;
            }
            free(o.pos);
            free(o.ref);
            free(o.raw_t);
            free(o.raw_n);
            free(o.off_t);
            free(o.off_n);
            free(o.reads_t);
            free(o.reads_n);
        }
        if (want != 99 && rc != want) {
            fprintf(stderr, "case %u: return code %d (want %d)\n", i, rc, want);
            bad = 1;
        }
        plan(&t);
        plan(&n);
        free_sample(&t);
        free_sample(&n);
        free(ref);
    }
    fclose(f);
    printf("ok=%d cases=%u\n", !bad, n_cases);
    return bad;
}
