/*
 * ss_pileup.hip -- pileup columns from BAM records on the GPU
 * (include/sniper_amd.h, "pileup columns from BAM records"): the kernels, the
 * ss_pileup_t handle and the device / host entry points.  DESIGN.md section 13.
 * The planner on the device (ss_pileup_plan_device) is
 * the last part of this file, with its own notes.
 *
 * One call builds one region [lo, hi) of one contig for both samples:
 *   ss_pileup_index   one lane per record: validates it (ss_pileup_core.h) and
 *                     writes its descriptor; a hipCUB scan then gives the
 *                     running maximum of the records' ends;
 *   ss_pileup_count   one workgroup per tile of 256 positions, one thread per
 *                     position: two binary searches bound the tile's candidate
 *                     records, every thread walks them in load order and counts
 *                     its column's raw and packed entries for both samples;
 *                     the tile's site and entry sums are reduced in the block;
 *   ss_pileup_tiles   one workgroup: exclusive scan of the tile sums (u64), the
 *                     region's totals;
 *   ss_pileup_fill    the walk of the count kernel again: a block scan places
 *                     every site of the tile, each present position writes its
 *                     header and its packed entries in load order.
 * No atomics touch the output and no order depends on scheduling, so the
 * arrays are the same from run to run.
 *
 * Bounds.  A record is read only through a descriptor ssp_index validated
 * against the sample's byte span; descriptors, counts and tile arrays are
 * indexed by values below the sizes the host allocated them with; every store
 * to the caller's arrays is checked against the capacities in the kernel.
 */
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sniper_amd.h"
#include "ss_pileup_core.h"
#include "ss_plan_core.h"

extern "C" int ssp_sample_args_ok(const ss_pileup_sample_t *s);     /* ss_pileup_plan.c */
typedef int (*ssp_rewalk_fn)(void *ctx, uint32_t k, uint64_t entry, ssp_chunk_t *c);
extern "C" int ssp_plan_stitch(ssp_chunk_t *c, uint32_t n_chunks, uint64_t chunk, uint64_t len, ssp_rewalk_fn rewalk,
                               void *ctx, uint64_t *n_rec, uint64_t *end_at, uint32_t *end_status,
                               uint32_t *n_repaired);                /* ss_pileup_plan.c */

struct ssp_max_op {
    __host__ __device__ int32_t operator()(int32_t a, int32_t b) const { return a > b ? a : b; }
};

/* one sample as the count / fill kernels see it */
struct ssp_dsample {
    const uint8_t *bytes;
    const ssp_desc_t *desc;
    const int32_t *max_end;
    uint32_t n;
};

struct ssp_fill_args {
    const uint8_t *ref;          /* ref[p - ref_pos0] for ref_pos0 <= p < ref_len, or NULL */
    int64_t ref_pos0, ref_len;
    uint64_t cap_sites, cap_t, cap_n;
    int32_t *pos;
    uint8_t *refo;
    uint32_t *raw_t, *raw_n, *off_t, *off_n, *reads_t, *reads_n;
};

__global__ __launch_bounds__(256) void ss_pileup_index(const uint8_t *__restrict__ bytes, uint64_t n_bytes,
                                                       const uint64_t *__restrict__ rec_off, uint64_t off_base,
                                                       const int32_t *__restrict__ from, uint32_t n,
                                                       ssp_desc_t *__restrict__ desc, int32_t *__restrict__ end,
                                                       uint32_t *__restrict__ n_invalid)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int32_t f = from[i];
    const uint64_t off = rec_off[i];
    ssp_desc_t d;
    int ok = off >= off_base && ssp_index(bytes, n_bytes, off - off_base, f, &d);
    if (ok && i && f < from[i - 1]) ok = 0;                /* `from` must not decrease */
    if (!ok) {
        d.beg = d.end = 0;
        d.from = f;
        d.pk = d.cig = d.seq = d.qual = d.nc = 0;
        atomicAdd(n_invalid, 1u);
    }
    desc[i] = d;
    end[i] = d.end;
}

/* the tile's candidate ranges of both samples, found by thread 0 and made
 * wave-uniform for the walk */
static __device__ __forceinline__ void ssp_tile_candidates(const ssp_dsample &t, const ssp_dsample &n, int32_t tile_lo,
                                                           int32_t tile_hi, uint32_t *s_b, uint32_t b[4])
{
    if (threadIdx.x == 0) {
        ssp_candidates(t.desc, t.max_end, t.n, tile_lo, tile_hi, &s_b[0], &s_b[1]);
        ssp_candidates(n.desc, n.max_end, n.n, tile_lo, tile_hi, &s_b[2], &s_b[3]);
    }
    __syncthreads();
    for (int k = 0; k < 4; ++k) b[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_b[k]);
}

static __device__ __forceinline__ uint32_t ssp_wave_incl(uint32_t v, uint32_t lane)
{
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, s, 64);
        if (lane >= (uint32_t)s) v += u;
    }
    return v;
}

/* Exclusive scan of v over the 256 threads of the block; *total is the
 * block's sum.  s_w: 4 words of LDS. */
static __device__ __forceinline__ uint32_t ssp_block_excl(uint32_t v, uint32_t *s_w, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t incl = ssp_wave_incl(v, lane);
    __syncthreads();                                       /* s_w may still be read from the previous scan */
    if (lane == 63u) s_w[wave] = incl;
    __syncthreads();
    uint32_t base = 0, sum = 0;
    for (uint32_t w = 0; w < 4u; ++w) {
        const uint32_t x = s_w[w];
        if (w < wave) base += x;
        sum += x;
    }
    *total = sum;
    return base + incl - v;
}

__global__ __launch_bounds__(256) void ss_pileup_count(ssp_dsample t, ssp_dsample n, int32_t lo, int32_t hi,
                                                       uint4 *__restrict__ cnt, uint32_t *__restrict__ tile_sum)
{
    __shared__ uint32_t s_b[4], s_w[4];
    const int64_t tl = (int64_t)lo + (int64_t)blockIdx.x * SSP_TILE;
    const int32_t tile_lo = (int32_t)tl, tile_hi = (int32_t)(tl + SSP_TILE < hi ? tl + SSP_TILE : hi);
    uint32_t b[4];
    ssp_tile_candidates(t, n, tile_lo, tile_hi, s_b, b);
    /* the last tile may end at INT32_MAX: the guard is on the thread index, and p is formed only under it */
    const bool active = threadIdx.x < (uint32_t)(tile_hi - tile_lo);
    const int32_t p = active ? tile_lo + (int32_t)threadIdx.x : tile_lo;
    uint32_t rt = 0, rn = 0, pt = 0, pn = 0;
    if (active) {
        pt = ssp_column(t.bytes, t.desc, b[0], b[1], p, &rt, nullptr, 0);
        pn = ssp_column(n.bytes, n.desc, b[2], b[3], p, &rn, nullptr, 0);
        cnt[(uint32_t)(p - lo)] = make_uint4(rt, rn, pt, pn);
    }
    const bool present = rt > 0 && rn > 0;
    uint32_t sites, nt, nn;
    (void)ssp_block_excl(present ? 1u : 0u, s_w, &sites);
    (void)ssp_block_excl(present ? pt : 0u, s_w, &nt);
    (void)ssp_block_excl(present ? pn : 0u, s_w, &nn);
    if (threadIdx.x == 0) {
        tile_sum[3u * blockIdx.x] = sites;
        tile_sum[3u * blockIdx.x + 1u] = nt;
        tile_sum[3u * blockIdx.x + 2u] = nn;
    }
}

/* tile_base[3 i ..] = sums of the tiles before tile i; totals[0..2] = all tiles */
__global__ __launch_bounds__(256) void ss_pileup_tiles(const uint32_t *__restrict__ tile_sum, uint32_t n_tiles,
                                                       uint64_t *__restrict__ tile_base, uint64_t *__restrict__ totals)
{
    __shared__ uint64_t s[3][256];
    const uint32_t per = (n_tiles + 255u) / 256u;
    const uint32_t a = threadIdx.x * per < n_tiles ? threadIdx.x * per : n_tiles;
    const uint32_t e = a + per < n_tiles ? a + per : n_tiles;
    uint64_t x[3] = {0, 0, 0};
    for (uint32_t i = a; i < e; ++i)
        for (int k = 0; k < 3; ++k) x[k] += tile_sum[3u * i + k];
    for (int k = 0; k < 3; ++k) s[k][threadIdx.x] = x[k];
    __syncthreads();
    if (threadIdx.x < 3u) {
        uint64_t run = 0;
        for (int i = 0; i < 256; ++i) {
            const uint64_t v = s[threadIdx.x][i];
            s[threadIdx.x][i] = run;
            run += v;
        }
        totals[threadIdx.x] = run;
    }
    __syncthreads();
    for (int k = 0; k < 3; ++k) x[k] = s[k][threadIdx.x];
    for (uint32_t i = a; i < e; ++i)
        for (int k = 0; k < 3; ++k) {
            tile_base[3u * i + k] = x[k];
            x[k] += tile_sum[3u * i + k];
        }
}

__global__ __launch_bounds__(256) void ss_pileup_fill(ssp_dsample t, ssp_dsample n, int32_t lo, int32_t hi,
                                                      const uint4 *__restrict__ cnt,
                                                      const uint64_t *__restrict__ tile_base,
                                                      const uint64_t *__restrict__ totals, ssp_fill_args o)
{
    __shared__ uint32_t s_b[4], s_w[4];
    const int64_t tl = (int64_t)lo + (int64_t)blockIdx.x * SSP_TILE;
    const int32_t tile_lo = (int32_t)tl, tile_hi = (int32_t)(tl + SSP_TILE < hi ? tl + SSP_TILE : hi);
    uint32_t b[4];
    ssp_tile_candidates(t, n, tile_lo, tile_hi, s_b, b);
    const bool active = threadIdx.x < (uint32_t)(tile_hi - tile_lo);      /* as in ss_pileup_count */
    const int32_t p = active ? tile_lo + (int32_t)threadIdx.x : tile_lo;
    uint4 c = make_uint4(0, 0, 0, 0);
    if (active) c = cnt[(uint32_t)(p - lo)];
    const bool present = c.x > 0 && c.y > 0;
    uint32_t tot;
    const uint64_t site = tile_base[3u * blockIdx.x] + ssp_block_excl(present ? 1u : 0u, s_w, &tot);
    const uint64_t ot = tile_base[3u * blockIdx.x + 1u] + ssp_block_excl(present ? c.z : 0u, s_w, &tot);
    const uint64_t on = tile_base[3u * blockIdx.x + 2u] + ssp_block_excl(present ? c.w : 0u, s_w, &tot);
    if (blockIdx.x == 0 && threadIdx.x == 0 && totals[0] <= o.cap_sites) {
        o.off_t[totals[0]] = (uint32_t)totals[1];
        o.off_n[totals[0]] = (uint32_t)totals[2];
    }
    /* nothing is stored past a capacity */
    if (!present || site >= o.cap_sites || ot + c.z > o.cap_t || on + c.w > o.cap_n) return;
    o.pos[site] = p;
    o.refo[site] = (o.ref && p >= o.ref_pos0 && p < o.ref_len) ? o.ref[p - o.ref_pos0] : (uint8_t)'N';
    o.raw_t[site] = c.x;
    o.raw_n[site] = c.y;
    o.off_t[site] = (uint32_t)ot;
    o.off_n[site] = (uint32_t)on;
    uint32_t raw;
    if (c.z) (void)ssp_column(t.bytes, t.desc, b[0], b[1], p, &raw, o.reads_t + ot, c.z);
    if (c.w) (void)ssp_column(n.bytes, n.desc, b[2], b[3], p, &raw, o.reads_n + on, c.w);
}

/* ---------------------------------------------------------------- handle ---- */
#ifdef SS_DEBUG_CANARY
#define SSP_GUARD ((size_t)4096)
#else
#define SSP_GUARD ((size_t)0)
#endif

struct ssp_buf {
    void *base;      /* hipMalloc'd; the usable part starts SSP_GUARD bytes in */
    size_t bytes;
};

enum {
    B_DESC_T, B_DESC_N, B_END_T, B_END_N, B_MAX_T, B_MAX_N, B_CNT, B_TSUM, B_TBASE, B_TOTALS, B_SCAN,
    /* staging of ss_pileup_region_host */
    B_BYTES_T, B_BYTES_N, B_OFF_T, B_OFF_N, B_FROM_T, B_FROM_N, B_REF,
    B_OPOS, B_OREF, B_ORAW_T, B_ORAW_N, B_OOFF_T, B_OOFF_N, B_OREADS_T, B_OREADS_N,
    /* ss_pileup_plan_device: the chunk table, the kept chunks, one entry per record, the result, the runs */
    B_PCHUNK, B_PEMIT, B_POFF, B_PTID, B_PBEG, B_PEND, B_PFLAG, B_PSEG, B_PMAXT, B_PRANK, B_PFROM, B_PRUNV, B_PRES,
    B_PRUNK, B_PRUNA, B_PNRUN,
    B_COUNT
};

struct ss_pileup {
    int device;
    hipStream_t stream;          /* the host path's stream */
    hipStream_t last;            /* the stream of the latest launch */
    ssp_buf buf[B_COUNT];
    uint64_t sticky_invalid;     /* invalid records of device calls since the last check */
    int corrupt;                 /* a guard band of a buffer that has since been replaced was damaged */
    /* the latest count */
    int counted;
    ssp_dsample ds[2];
    const uint8_t *ref;
    int64_t ref_pos0, ref_len;
    int32_t lo, hi;
    uint64_t tot[3];
    double plan_ms[3];           /* the latest ss_pileup_plan_device: guess + walk, stitch, emit + plan (host clock) */
};

#define HIPCHK(x)                                   \
    do {                                            \
        if ((x) != hipSuccess) return SS_E_HIP;     \
    } while (0)

static inline void *buf_user(const ssp_buf &b) { return b.base ? (char *)b.base + SSP_GUARD : nullptr; }

static int buf_guards_ok(ss_pileup_t *h, const ssp_buf &b)
{
#ifdef SS_DEBUG_CANARY
    if (!b.base) return SS_OK;
    std::vector<unsigned char> g(2 * SSP_GUARD);
    if (hipMemcpyAsync(g.data(), b.base, SSP_GUARD, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipMemcpyAsync(g.data() + SSP_GUARD, (char *)b.base + SSP_GUARD + b.bytes, SSP_GUARD, hipMemcpyDeviceToHost,
                       h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
        return SS_E_HIP;
    for (size_t i = 0; i < g.size(); ++i)
        if (g[i] != 0xA5) {
            fprintf(stderr, "[sniper_amd] guard band of pileup buffer %p (%zu bytes) overwritten at %s%zu\n",
                    buf_user(b), b.bytes, i < SSP_GUARD ? "-" : "+", i < SSP_GUARD ? SSP_GUARD - i : i - SSP_GUARD);
            return SS_E_CORRUPT;
        }
#else
    (void)h; (void)b;
#endif
    return SS_OK;
}

/* the handle's work has ended */
static void buf_free(ss_pileup_t *h, ssp_buf &b)
{
    if (!b.base) return;
    if (buf_guards_ok(h, b) == SS_E_CORRUPT) h->corrupt = 1;
    (void)hipFree(b.base);
    b.base = nullptr;
    b.bytes = 0;
}

static int wait_all(ss_pileup_t *h)
{
    HIPCHK(hipStreamSynchronize(h->last));
    if (h->last != h->stream) HIPCHK(hipStreamSynchronize(h->stream));
    return SS_OK;
}

/* at least `bytes` usable bytes; contents are not kept.  Waits for the
 * handle's work before a buffer is replaced. */
static int buf_ensure(ss_pileup_t *h, int which, size_t bytes, void **user)
{
    ssp_buf &b = h->buf[which];
    if (!(b.base && b.bytes >= bytes)) {
        if (int rc = wait_all(h)) return rc;
        buf_free(h, b);
        size_t sz = bytes < 4096 ? 4096 : bytes + bytes / 4;
        sz = (sz + 255) & ~(size_t)255;
        if (hipMalloc(&b.base, sz + 2 * SSP_GUARD) != hipSuccess) {
            (void)hipGetLastError();
            b.base = nullptr;
            return SS_E_NOMEM;
        }
        b.bytes = sz;
#ifdef SS_DEBUG_CANARY
        HIPCHK(hipMemsetAsync(b.base, 0xA5, SSP_GUARD, h->stream));
        HIPCHK(hipMemsetAsync((char *)b.base + SSP_GUARD + sz, 0xA5, SSP_GUARD, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
#endif
    }
    *user = buf_user(b);
    return SS_OK;
}

extern "C" int ss_pileup_create(int device, ss_pileup_t **out)
{
    if (!out) return SS_E_INVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        return SS_E_NODEV;
    }
    HIPCHK(hipSetDevice(device));
    ss_pileup_t *h = (ss_pileup_t *)calloc(1, sizeof *h);
    if (!h) return SS_E_NOMEM;
    h->device = device;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        free(h);
        return SS_E_HIP;
    }
    h->last = h->stream;
    *out = h;
    return SS_OK;
}

extern "C" int ss_pileup_check(ss_pileup_t *h)
{
    if (!h) return SS_E_INVAL;
    HIPCHK(hipSetDevice(h->device));
    if (int rc = wait_all(h)) return rc;
    if (h->corrupt) return SS_E_CORRUPT;
    for (const ssp_buf &b : h->buf)
        if (int rc = buf_guards_ok(h, b)) return rc;
    if (h->sticky_invalid) {
        h->sticky_invalid = 0;
        return SS_E_INVAL;
    }
    return SS_OK;
}

extern "C" void ss_pileup_destroy(ss_pileup_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)wait_all(h);
    for (ssp_buf &b : h->buf) buf_free(h, b);
    if (h->corrupt) fprintf(stderr, "[sniper_amd] ss_pileup_destroy: device memory corrupted (see above)\n");
    (void)hipStreamDestroy(h->stream);
    free(h);
}

static int launched() { return hipGetLastError() == hipSuccess ? SS_OK : SS_E_HIP; }

/* Pass 1 over device inputs on stream s; off_base[k] is subtracted from sample
 * k's record offsets.  Synchronous.  *n_invalid: records that failed. */
static int count_impl(ss_pileup_t *h, const ss_pileup_sample_t *const smp[2], const uint64_t off_base[2],
                      const uint8_t *ref, int64_t ref_pos0, int64_t ref_len, int32_t lo, int32_t hi, hipStream_t s,
                      uint64_t *n_invalid)
{
    h->counted = 0;
    const uint32_t span = (uint32_t)(hi - lo), n_tiles = (span + SSP_TILE - 1u) / SSP_TILE;
    void *p;
    int rc;
    uint4 *cnt;
    uint32_t *tsum;
    uint64_t *tbase, *totals;
    if ((rc = buf_ensure(h, B_CNT, (size_t)span * sizeof(uint4), &p))) return rc;
    cnt = (uint4 *)p;
    if ((rc = buf_ensure(h, B_TSUM, (size_t)n_tiles * 3 * sizeof(uint32_t), &p))) return rc;
    tsum = (uint32_t *)p;
    if ((rc = buf_ensure(h, B_TBASE, (size_t)n_tiles * 3 * sizeof(uint64_t), &p))) return rc;
    tbase = (uint64_t *)p;
    if ((rc = buf_ensure(h, B_TOTALS, 4 * sizeof(uint64_t), &p))) return rc;
    totals = (uint64_t *)p;                               /* sites, entries t, entries n, invalid records (u32) */
    uint32_t *d_invalid = (uint32_t *)(totals + 3);
    if (h->last != s) HIPCHK(hipStreamSynchronize(h->last));   /* the scratch buffers are shared between calls */
    h->last = s;
    HIPCHK(hipMemsetAsync(totals, 0, 4 * sizeof(uint64_t), s));
    for (int k = 0; k < 2; ++k) {
        const uint32_t n = smp[k]->n;
        ssp_desc_t *desc;
        int32_t *end, *mx;
        if ((rc = buf_ensure(h, B_DESC_T + k, ((size_t)n + 1) * sizeof(ssp_desc_t), &p))) return rc;
        desc = (ssp_desc_t *)p;
        if ((rc = buf_ensure(h, B_END_T + k, ((size_t)n + 1) * sizeof(int32_t), &p))) return rc;
        end = (int32_t *)p;
        if ((rc = buf_ensure(h, B_MAX_T + k, ((size_t)n + 1) * sizeof(int32_t), &p))) return rc;
        mx = (int32_t *)p;
        h->ds[k].bytes = smp[k]->bytes;
        h->ds[k].desc = desc;
        h->ds[k].max_end = mx;
        h->ds[k].n = n;
        if (!n) continue;
        hipLaunchKernelGGL(ss_pileup_index, dim3((n + 255u) / 256u), dim3(256), 0, s, smp[k]->bytes, smp[k]->n_bytes,
                           smp[k]->rec_off, off_base[k], smp[k]->from, n, desc, end, d_invalid);
        if ((rc = launched())) return rc;
        size_t tmp = 0;
        HIPCHK(hipcub::DeviceScan::InclusiveScan(nullptr, tmp, end, mx, ssp_max_op(), (int)n, s));
        if ((rc = buf_ensure(h, B_SCAN, tmp ? tmp : 1, &p))) return rc;
        tmp = h->buf[B_SCAN].bytes;
        HIPCHK(hipcub::DeviceScan::InclusiveScan(p, tmp, end, mx, ssp_max_op(), (int)n, s));
    }
    hipLaunchKernelGGL(ss_pileup_count, dim3(n_tiles), dim3(256), 0, s, h->ds[0], h->ds[1], lo, hi, cnt, tsum);
    if ((rc = launched())) return rc;
    hipLaunchKernelGGL(ss_pileup_tiles, dim3(1), dim3(256), 0, s, (const uint32_t *)tsum, n_tiles, tbase, totals);
    if ((rc = launched())) return rc;
    uint64_t host[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(host, totals, sizeof host, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    h->tot[0] = host[0];
    h->tot[1] = host[1];
    h->tot[2] = host[2];
    *n_invalid = host[3] & 0xffffffffull;
    h->ref = ref;
    h->ref_pos0 = ref_pos0;
    h->ref_len = ref_len;
    h->lo = lo;
    h->hi = hi;
    if (host[1] > SS_PILEUP_MAX_READS || host[2] > SS_PILEUP_MAX_READS) return SS_E_CAPACITY;
    h->counted = 1;
    return SS_OK;
}

static int fill_impl(ss_pileup_t *h, const ss_pileup_out_t *out, hipStream_t s)
{
    if (!h->counted) return SS_E_INVAL;
    if (h->tot[0] > out->cap_sites || h->tot[1] > out->cap_reads_t || h->tot[2] > out->cap_reads_n)
        return SS_E_CAPACITY;
    if (!out->pos || !out->ref || !out->raw_t || !out->raw_n || !out->off_t || !out->off_n ||
        (h->tot[1] && !out->reads_t) || (h->tot[2] && !out->reads_n))
        return SS_E_INVAL;
    ssp_fill_args o;
    o.ref = h->ref;
    o.ref_pos0 = h->ref_pos0;
    o.ref_len = h->ref_len;
    o.cap_sites = out->cap_sites;
    o.cap_t = out->cap_reads_t;
    o.cap_n = out->cap_reads_n;
    o.pos = out->pos;
    o.refo = out->ref;
    o.raw_t = out->raw_t;
    o.raw_n = out->raw_n;
    o.off_t = out->off_t;
    o.off_n = out->off_n;
    o.reads_t = out->reads_t;
    o.reads_n = out->reads_n;
    const uint32_t span = (uint32_t)(h->hi - h->lo), n_tiles = (span + SSP_TILE - 1u) / SSP_TILE;
    if (h->last != s) HIPCHK(hipStreamSynchronize(h->last));
    h->last = s;
    hipLaunchKernelGGL(ss_pileup_fill, dim3(n_tiles), dim3(256), 0, s, h->ds[0], h->ds[1], h->lo, h->hi,
                       (const uint4 *)buf_user(h->buf[B_CNT]), (const uint64_t *)buf_user(h->buf[B_TBASE]),
                       (const uint64_t *)buf_user(h->buf[B_TOTALS]), o);
    return launched();
}

static int region_args_ok(const ss_pileup_sample_t *t, const ss_pileup_sample_t *n, int32_t lo, int32_t hi)
{
    if (!t || !n || lo < 0 || hi <= lo || (uint32_t)(hi - lo) > SS_PILEUP_MAX_SPAN) return 0;
    if (t->n > SS_PILEUP_MAX_RECORDS || n->n > SS_PILEUP_MAX_RECORDS) return 0;
    if (t->n_bytes > 0xffffffffull || n->n_bytes > 0xffffffffull) return 0;
    return 1;
}

extern "C" int ss_pileup_count_device(ss_pileup_t *h, const ss_pileup_sample_t *tumor,
                                      const ss_pileup_sample_t *normal, const uint8_t *ref, int64_t ref_len,
                                      int32_t lo, int32_t hi, uint64_t *n_sites, uint64_t *n_reads_t,
                                      uint64_t *n_reads_n, void *stream)
{
    if (!h || !n_sites || !n_reads_t || !n_reads_n || !region_args_ok(tumor, normal, lo, hi)) return SS_E_INVAL;
    for (const ss_pileup_sample_t *s : {tumor, normal})
        if (s->n && (!s->bytes || !s->rec_off || !s->from)) return SS_E_INVAL;
    HIPCHK(hipSetDevice(h->device));
    const ss_pileup_sample_t *smp[2] = {tumor, normal};
    const uint64_t base[2] = {0, 0};
    uint64_t bad = 0;
    const int rc = count_impl(h, smp, base, ref, 0, ref_len, lo, hi, (hipStream_t)stream, &bad);
    h->sticky_invalid += bad;
    if (rc != SS_OK && rc != SS_E_CAPACITY) return rc;
    *n_sites = h->tot[0];
    *n_reads_t = h->tot[1];
    *n_reads_n = h->tot[2];
    return rc;
}

extern "C" int ss_pileup_fill_device(ss_pileup_t *h, const ss_pileup_out_t *out, void *stream)
{
    if (!h || !out) return SS_E_INVAL;
    HIPCHK(hipSetDevice(h->device));
    return fill_impl(h, out, (hipStream_t)stream);
}

extern "C" int ss_pileup_region_host(ss_pileup_t *h, const ss_pileup_sample_t *tumor,
                                     const ss_pileup_sample_t *normal, const uint8_t *ref, int64_t ref_len, int32_t lo,
                                     int32_t hi, ss_pileup_out_t *out)
{
    if (!h || !out || !region_args_ok(tumor, normal, lo, hi)) return SS_E_INVAL;
    if (!ssp_sample_args_ok(tumor) || !ssp_sample_args_ok(normal)) return SS_E_INVAL;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const ss_pileup_sample_t *src[2] = {tumor, normal};
    ss_pileup_sample_t dev[2];
    uint64_t base[2] = {0, 0};
    void *p;
    int rc;
    for (int k = 0; k < 2; ++k) {
        /* the byte span the records lie in: from the lowest offset to the
         * highest block end (as far as the block sizes can be trusted) */
        const ss_pileup_sample_t *m = src[k];
        uint64_t a = m->n_bytes, b = 0;
        for (uint32_t i = 0; i < m->n; ++i) {
            const uint64_t off = m->rec_off[i];
            uint64_t e = m->n_bytes;
            if (m->n_bytes - off >= 4) {
                const int32_t block = (int32_t)ssp_le32(m->bytes + off);
                if (block >= 0 && (uint64_t)block <= m->n_bytes - off - 4) e = off + 4 + (uint64_t)block;
            }
            if (off < a) a = off;
            if (e > b) b = e;
        }
        if (!m->n) a = b = 0;
        base[k] = a;
        dev[k].n = m->n;
        dev[k].n_bytes = b - a;
        dev[k].pad = 0;
        if ((rc = buf_ensure(h, B_BYTES_T + k, (size_t)(b - a) + 1, &p))) return rc;
        dev[k].bytes = (const uint8_t *)p;
        if ((rc = buf_ensure(h, B_OFF_T + k, ((size_t)m->n + 1) * sizeof(uint64_t), &p))) return rc;
        dev[k].rec_off = (const uint64_t *)p;
        if ((rc = buf_ensure(h, B_FROM_T + k, ((size_t)m->n + 1) * sizeof(int32_t), &p))) return rc;
        dev[k].from = (const int32_t *)p;
        if (b > a) HIPCHK(hipMemcpyAsync((void *)dev[k].bytes, m->bytes + a, (size_t)(b - a), hipMemcpyHostToDevice, s));
        if (m->n) {
            HIPCHK(hipMemcpyAsync((void *)dev[k].rec_off, m->rec_off, (size_t)m->n * sizeof(uint64_t),
                                  hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync((void *)dev[k].from, m->from, (size_t)m->n * sizeof(int32_t), hipMemcpyHostToDevice,
                                  s));
        }
    }
    /* the reference bases of the region */
    const uint8_t *d_ref = nullptr;
    const int64_t ref_hi = ref ? (ref_len < hi ? ref_len : hi) : 0;
    if (ref && ref_hi > lo) {
        if ((rc = buf_ensure(h, B_REF, (size_t)(ref_hi - lo), &p))) return rc;
        HIPCHK(hipMemcpyAsync(p, ref + lo, (size_t)(ref_hi - lo), hipMemcpyHostToDevice, s));
        d_ref = (const uint8_t *)p;
    }
    const ss_pileup_sample_t *smp[2] = {&dev[0], &dev[1]};
    uint64_t bad = 0;
    rc = count_impl(h, smp, base, d_ref, lo, ref_hi, lo, hi, s, &bad);
    if (rc != SS_OK && rc != SS_E_CAPACITY) return rc;
    const uint64_t ns = h->tot[0], nt = h->tot[1], nn = h->tot[2];
    out->n_sites = ns;
    out->n_reads_t = nt;
    out->n_reads_n = nn;
    out->n_invalid = bad;
    if (rc == SS_E_CAPACITY || ns > out->cap_sites || nt > out->cap_reads_t || nn > out->cap_reads_n)
        return SS_E_CAPACITY;
    if (!out->pos || !out->ref || !out->raw_t || !out->raw_n || !out->off_t || !out->off_n ||
        (nt && !out->reads_t) || (nn && !out->reads_n))
        return SS_E_INVAL;
    ss_pileup_out_t d = *out;
    d.cap_sites = ns;
    d.cap_reads_t = nt;
    d.cap_reads_n = nn;
    if ((rc = buf_ensure(h, B_OPOS, (size_t)(ns + 1) * 4, &p))) return rc;
    d.pos = (int32_t *)p;
    if ((rc = buf_ensure(h, B_OREF, (size_t)(ns + 1), &p))) return rc;
    d.ref = (uint8_t *)p;
    if ((rc = buf_ensure(h, B_ORAW_T, (size_t)(ns + 1) * 4, &p))) return rc;
    d.raw_t = (uint32_t *)p;
    if ((rc = buf_ensure(h, B_ORAW_N, (size_t)(ns + 1) * 4, &p))) return rc;
    d.raw_n = (uint32_t *)p;
    if ((rc = buf_ensure(h, B_OOFF_T, (size_t)(ns + 1) * 4, &p))) return rc;
    d.off_t = (uint32_t *)p;
    if ((rc = buf_ensure(h, B_OOFF_N, (size_t)(ns + 1) * 4, &p))) return rc;
    d.off_n = (uint32_t *)p;
    if ((rc = buf_ensure(h, B_OREADS_T, (size_t)(nt + 1) * 4, &p))) return rc;
    d.reads_t = (uint32_t *)p;
    if ((rc = buf_ensure(h, B_OREADS_N, (size_t)(nn + 1) * 4, &p))) return rc;
    d.reads_n = (uint32_t *)p;
    if ((rc = fill_impl(h, &d, s))) return rc;
    if (ns) {
        HIPCHK(hipMemcpyAsync(out->pos, d.pos, (size_t)ns * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->ref, d.ref, (size_t)ns, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->raw_t, d.raw_t, (size_t)ns * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->raw_n, d.raw_n, (size_t)ns * 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(out->off_t, d.off_t, (size_t)(ns + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out->off_n, d.off_n, (size_t)(ns + 1) * 4, hipMemcpyDeviceToHost, s));
    if (nt) HIPCHK(hipMemcpyAsync(out->reads_t, d.reads_t, (size_t)nt * 4, hipMemcpyDeviceToHost, s));
    if (nn) HIPCHK(hipMemcpyAsync(out->reads_n, d.reads_n, (size_t)nn * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    h->counted = 0;              /* the staged inputs may be replaced by the next call */
    return bad ? SS_E_INVAL : SS_OK;
}

/* ------------------------------------------------------- the planner ---- */
/*
 * ss_pileup_plan_device:
 *   ss_plan_walk   one workgroup per chunk of SS_PLAN_CHUNK bytes: stages the
 *                  chunk into LDS with coalesced loads, guesses its entry (256
 *                  offsets tested at a time, the lowest accepted one wins: the
 *                  serial ssp_guess), then one lane chases the chain through
 *                  LDS and writes the chunk's ssp_chunk_t;
 *   the stitch     on the host over the chunk table (24 bytes a chunk), the
 *                  function the CPU twin runs; a wrong guess launches
 *                  ss_plan_walk again for that one chunk from its true entry;
 *   ss_plan_emit   one workgroup per kept chunk: the walk again, now noting the
 *                  offsets in LDS, then one thread per record decodes the head
 *                  and the CIGAR end (ssp_plan_record) and writes the record's
 *                  scan elements;
 *   two hipCUB scans (the walk state, the running maximum contig), ss_plan_keep
 *   (load rules per record, first error by atomicMin on a scratch word),
 *   a hipCUB sum (ranks), ss_plan_out (compaction in order), ss_plan_final
 *   (one thread: n, consumed, code, out-state) and a hipCUB reduce-by-key for
 *   the runs.
 * No atomic touches an output array; the one on the scratch word is a minimum,
 * so every result is the same from run to run.
 *
 * Bounds.  The window is staged with every global load inside bytes[0 .. len);
 * ssp_walk reads a block_size only where 4 bytes are left; a record is decoded
 * only after the walk found it whole; record-indexed stores are below n_rec,
 * stores to the caller's arrays below cap.
 */
#define SSP_PLAN_WIN (SS_PLAN_CHUNK + 48u)      /* the chunk, 4 bytes past it, alignment slack */
#define SSP_PLAN_REL (SS_PLAN_CHUNK / 36u + 2u) /* no record is shorter than 36 bytes */

struct ssp_emit_t {
    uint64_t entry;
    uint32_t chunk, base;        /* the chunk's number; the index of its first record */
};

struct ssp_runv_t {
    int32_t lo, hi;
    uint32_t n;
};

typedef ssp_plan_res_t ssp_plan_res;     /* ss_plan_core.h; first_err and cut are set to SSP_NO_RECORD before the kernels run */

struct ssp_seg_op {
    __host__ __device__ ssp_seg_t operator()(const ssp_seg_t &a, const ssp_seg_t &b) const { return ssp_seg_join(a, b); }
};
struct ssp_runv_op {
    __host__ __device__ ssp_runv_t operator()(const ssp_runv_t &a, const ssp_runv_t &b) const
    {
        ssp_runv_t r;
        r.lo = a.lo < b.lo ? a.lo : b.lo;
        r.hi = a.hi > b.hi ? a.hi : b.hi;
        r.n = a.n + b.n;
        return r;
    }
};

/* Stages bytes[start .. start + want) into s; byte x then lies at
 * s[a + x - start], a (returned) being the misalignment of byte `start`.
 * 16-byte granules that lie whole inside the span go as one vector load, the
 * two ragged ones byte by byte. */
static __device__ __forceinline__ uint32_t ssp_stage(const uint8_t *__restrict__ bytes, uint64_t start, uint32_t want,
                                                     uint8_t *s)
{
    const uint8_t *g0 = bytes + start;
    const uint32_t a = (uint32_t)((uintptr_t)g0 & 15u);
    const uint32_t n_gran = (a + want + 15u) / 16u;
    for (uint32_t g = threadIdx.x; g < n_gran; g += 256u) {
        const int32_t lo = (int32_t)(16u * g) - (int32_t)a;             /* relative to start */
        if (lo >= 0 && (uint32_t)lo + 16u <= want) {
            *(uint4 *)(s + 16u * g) = *(const uint4 *)(g0 + lo);
        } else {
            for (int32_t j = 0; j < 16; ++j)
                if (lo + j >= 0 && (uint32_t)(lo + j) < want) s[16u * g + (uint32_t)j] = g0[lo + j];
        }
    }
    __syncthreads();
    return a;
}

static __device__ __forceinline__ uint32_t ssp_plan_want(uint64_t len, uint64_t start)
{
    return len - start < (uint64_t)SS_PLAN_CHUNK + 4u ? (uint32_t)(len - start) : SS_PLAN_CHUNK + 4u;
}

/* Chunk first + blockIdx.x.  forced == SSP_NO_GUESS: the chunk guesses its
 * entry (chunk 0 enters at 0); else it enters at `forced` (a repair). */
__global__ __launch_bounds__(256) void ss_plan_walk(const uint8_t *__restrict__ bytes, uint64_t len, int32_t n_ref,
                                                    uint32_t first, uint64_t forced, ssp_chunk_t *__restrict__ table)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_win[SSP_PLAN_WIN];
    __shared__ uint32_t s_first[4];
    const uint32_t k = first + blockIdx.x;
    const uint64_t start = (uint64_t)k * SS_PLAN_CHUNK;
    if (start >= len) return;
    const uint64_t end = len - start < SS_PLAN_CHUNK ? len : start + SS_PLAN_CHUNK;
    const uint32_t a = ssp_stage(bytes, start, ssp_plan_want(len, start), s_win);
    uint64_t entry = forced;
    if (forced == SSP_NO_GUESS && k == 0u) entry = 0;
    if (forced == SSP_NO_GUESS && k != 0u) {
        const uint32_t span = (uint32_t)(end - start), lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        for (uint32_t base = 0; base < span; base += 256u) {
            const uint32_t o = base + threadIdx.x;
            const bool ok = o < span && ssp_guess_ok(bytes, len, start + o, n_ref);
            const unsigned long long hit = __ballot(ok);
            if (lane == 0u) s_first[wave] = hit ? base + 64u * wave + (uint32_t)__ffsll((long long)hit) - 1u : 0xffffffffu;
            __syncthreads();
            uint32_t m = 0xffffffffu;
            for (int w = 0; w < 4; ++w) m = s_first[w] < m ? s_first[w] : m;
            __syncthreads();
            if (m != 0xffffffffu) {
                entry = start + m;
                break;
            }
        }
    }
    if (threadIdx.x == 0) {
        ssp_chunk_t c;
        c.entry = entry;
        c.exit = entry;
        c.count = 0;
        c.status = SSP_WALK_EXIT;
        if (entry != SSP_NO_GUESS && entry >= start && entry <= len)
            c.status = ssp_walk(s_win + a, start, len, start, entry, end, nullptr, 0, &c.exit, &c.count);
        table[k] = c;
    }
}

__global__ __launch_bounds__(256) void ss_plan_emit(const uint8_t *__restrict__ bytes, uint64_t len,
                                                    const ssp_emit_t *__restrict__ list, uint32_t flag_mask,
                                                    int mapq_thresh, uint32_t n_rec, uint64_t *__restrict__ off,
                                                    int32_t *__restrict__ tid, int32_t *__restrict__ beg,
                                                    int32_t *__restrict__ rend, uint32_t *__restrict__ flag,
                                                    ssp_seg_t *__restrict__ seg, int32_t *__restrict__ maxt)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_win[SSP_PLAN_WIN];
    __shared__ uint32_t s_rel[SSP_PLAN_REL];
    __shared__ uint32_t s_count;
    const ssp_emit_t e = list[blockIdx.x];
    const uint64_t start = (uint64_t)e.chunk * SS_PLAN_CHUNK;
    if (start >= len || e.entry < start || e.entry > len) return;
    const uint64_t end = len - start < SS_PLAN_CHUNK ? len : start + SS_PLAN_CHUNK;
    const uint32_t a = ssp_stage(bytes, start, ssp_plan_want(len, start), s_win);
    if (threadIdx.x == 0) {
        uint64_t exit_at;
        uint32_t count;
        (void)ssp_walk(s_win + a, start, len, start, e.entry, end, s_rel, SSP_PLAN_REL, &exit_at, &count);
        s_count = count < SSP_PLAN_REL ? count : SSP_PLAN_REL;
    }
    __syncthreads();
    const uint32_t count = s_count;
    for (uint32_t i = threadIdx.x; i < count; i += 256u) {
        const uint64_t idx = (uint64_t)e.base + i;
        if (idx >= n_rec) continue;
        const uint64_t at = start + s_rel[i];                  /* a whole record: the walk checked it against len */
        int32_t t, b, en;
        const uint32_t fl = ssp_plan_record(bytes + at, flag_mask, mapq_thresh, &t, &b, &en);
        off[idx] = at;
        tid[idx] = t;
        beg[idx] = b;
        rend[idx] = en;
        flag[idx] = fl;
        seg[idx] = ssp_seg_of(fl, t, b);
        maxt[idx] = ssp_maxt_of(fl, t);
    }
}

/* seg and maxt hold the inclusive scans.  One thread per record, plus one that
 * writes the closing 0 of the flags the rank sum runs over. */
__global__ __launch_bounds__(256) void ss_plan_keep(uint32_t n_rec, int32_t t0, int64_t w0, int32_t max0,
                                                    const int32_t *__restrict__ tid, const int32_t *__restrict__ beg,
                                                    const int32_t *__restrict__ rend,
                                                    const uint32_t *__restrict__ flag,
                                                    const ssp_seg_t *__restrict__ seg,
                                                    const int32_t *__restrict__ maxt, uint32_t *__restrict__ keep,
                                                    int32_t *__restrict__ from, ssp_plan_res *__restrict__ res)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i64 > n_rec) return;
    const uint32_t i = (uint32_t)i64;
    if (i == n_rec) {
        keep[i] = 0u;
        return;
    }
    uint32_t k;
    int32_t f;
    if (ssp_plan_rules(flag[i], tid[i], beg[i], rend[i], i ? seg[i - 1u] : ssp_seg_none(),
                       i ? maxt[i - 1u] : INT32_MIN, t0, w0, max0, &k, &f))
        atomicMin(&res->first_err, i);
    keep[i] = k;
    from[i] = f;
}

/* rank[i]: kept records before record i (rank[n_rec]: all). */
__global__ __launch_bounds__(256) void ss_plan_out(uint32_t n_rec, uint32_t cap, const uint64_t *__restrict__ off,
                                                   const int32_t *__restrict__ tid, const int32_t *__restrict__ rend,
                                                   const uint32_t *__restrict__ rank,
                                                   const int32_t *__restrict__ from, uint64_t *__restrict__ o_off,
                                                   int32_t *__restrict__ o_from, int32_t *__restrict__ o_tid,
                                                   ssp_runv_t *__restrict__ runv, ssp_plan_res *__restrict__ res)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i64 >= n_rec) return;
    const uint32_t i = (uint32_t)i64, r = rank[i];
    if (rank[i + 1u] == r || i >= res->first_err || r >= cap) return;
    o_off[r] = off[i];
    o_from[r] = from[i];
    o_tid[r] = tid[i];
    ssp_runv_t v;
    v.lo = from[i];
    v.hi = rend[i];
    v.n = 1u;
    runv[r] = v;
    if (r == cap - 1u) res->cut = i;                     /* the cap-th kept record: one writer */
}

__global__ void ss_plan_final(const uint8_t *__restrict__ bytes, uint32_t n_rec, int32_t t0, int64_t w0, int32_t max0,
                              uint64_t chain_end, uint32_t chain_bad, const uint64_t *__restrict__ off,
                              const uint32_t *__restrict__ rank, const ssp_seg_t *__restrict__ seg,
                              const int32_t *__restrict__ maxt, ssp_plan_res *__restrict__ res)
{
    if (blockIdx.x || threadIdx.x) return;
    ssp_plan_finish(bytes, n_rec, t0, w0, max0, chain_end, (int)chain_bad, off, rank, seg, maxt, res);
}

struct ssp_repair_ctx {
    const uint8_t *bytes;
    uint64_t len;
    int32_t n_ref;
    ssp_chunk_t *table;
    hipStream_t s;
};

static int plan_rewalk(void *ctx, uint32_t k, uint64_t entry, ssp_chunk_t *c)
{
    const ssp_repair_ctx *r = (const ssp_repair_ctx *)ctx;
    hipLaunchKernelGGL(ss_plan_walk, dim3(1), dim3(256), 0, r->s, r->bytes, r->len, r->n_ref, k, entry, r->table);
    if (int rc = launched()) return rc;
    HIPCHK(hipMemcpyAsync(c, r->table + k, sizeof *c, hipMemcpyDeviceToHost, r->s));
    HIPCHK(hipStreamSynchronize(r->s));
    return SS_OK;
}

extern "C" int ss_pileup_plan_device(ss_pileup_t *h, const uint8_t *bytes, uint64_t len, int32_t n_ref, int mask,
                                     int thresh, ss_pileup_state_t *state, uint64_t *rec_off, int32_t *from,
                                     int32_t *tid, uint32_t cap, uint32_t *n, uint64_t *consumed,
                                     ss_pileup_run_t *runs, uint32_t cap_runs, uint32_t *n_runs,
                                     uint32_t *n_repaired, void *stream)
{
    if (!h || (!bytes && len) || !state || !n || !n_runs || (cap && (!rec_off || !from || !tid)) ||
        (cap_runs && !runs))
        return SS_E_INVAL;
    const uint64_t nc64 = (len + SS_PLAN_CHUNK - 1u) / SS_PLAN_CHUNK;
    if (nc64 > 0x7fffffffull) return SS_E_INVAL;
    HIPCHK(hipSetDevice(h->device));
    const uint32_t flag_mask = mask < 0 ? (4u | 256u | 512u | 1024u) : (4u | (uint32_t)mask);   /* as ss_pileup_plan */
    const int mapq_thresh = thresh < 0 ? 0 : thresh;
    const int32_t t0 = state->has_prev ? state->tid : 0, max0 = state->has_prev ? state->max_tid : -1;
    const int64_t w0 = state->has_prev ? state->w : 0;
    hipStream_t s = (hipStream_t)stream;
    *n = 0;
    *n_runs = 0;
    if (n_repaired) *n_repaired = 0;
    ssp_plan_res res;
    memset(&res, 0, sizeof res);
    res.code = SS_OK;
    res.tid = t0;
    res.w = w0;
    res.max_tid = max0;
    uint64_t n_rec = 0, chain_end = 0;
    uint32_t chain_st = SSP_WALK_END;
    void *p;
    int rc;
    typedef std::chrono::steady_clock clk;
    const clk::time_point c0 = clk::now();
    clk::time_point c1 = c0, c2 = c0;
    if (cap && len >= 4u) {                               /* else ss_pileup_plan's loop does not run either */
        const uint32_t n_chunks = (uint32_t)nc64;
        if ((rc = buf_ensure(h, B_PCHUNK, (size_t)n_chunks * sizeof(ssp_chunk_t), &p))) return rc;
        ssp_chunk_t *table = (ssp_chunk_t *)p;
        if (h->last != s) HIPCHK(hipStreamSynchronize(h->last));   /* the scratch buffers are shared between calls */
        h->last = s;
        hipLaunchKernelGGL(ss_plan_walk, dim3(n_chunks), dim3(256), 0, s, bytes, len, n_ref, 0u, SSP_NO_GUESS, table);
        if ((rc = launched())) return rc;
        std::vector<ssp_chunk_t> tab(n_chunks);
        HIPCHK(hipMemcpyAsync(tab.data(), table, (size_t)n_chunks * sizeof(ssp_chunk_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        c1 = clk::now();
        ssp_repair_ctx rx = {bytes, len, n_ref, table, s};
        uint32_t rep = 0;
        if ((rc = ssp_plan_stitch(tab.data(), n_chunks, SS_PLAN_CHUNK, len, plan_rewalk, &rx, &n_rec, &chain_end,
                                  &chain_st, &rep)))
            return rc;
        c2 = clk::now();
        if (n_repaired) *n_repaired = rep;
        if (n_rec > 0x7fffffffull) return SS_E_INVAL;
        res.consumed = chain_end;
        res.code = chain_st == SSP_WALK_BAD ? SS_E_INVAL : SS_OK;
        if (n_rec) {
            const uint32_t R = (uint32_t)n_rec;
            std::vector<ssp_emit_t> list;
            uint32_t base = 0;
            for (uint32_t k = 0; k < n_chunks; ++k) {
                if (tab[k].status == SSP_WALK_SKIP || !tab[k].count) continue;
                list.push_back(ssp_emit_t{tab[k].entry, k, base});
                base += tab[k].count;
            }
            const size_t n1 = (size_t)R + 1;
            const uint32_t n_out = R < cap ? R : cap;
            if ((rc = buf_ensure(h, B_PEMIT, list.size() * sizeof(ssp_emit_t), &p))) return rc;
            ssp_emit_t *d_list = (ssp_emit_t *)p;
            if ((rc = buf_ensure(h, B_POFF, n1 * sizeof(uint64_t), &p))) return rc;
            uint64_t *d_off = (uint64_t *)p;
            if ((rc = buf_ensure(h, B_PTID, n1 * sizeof(int32_t), &p))) return rc;
            int32_t *d_tid = (int32_t *)p;
            if ((rc = buf_ensure(h, B_PBEG, n1 * sizeof(int32_t), &p))) return rc;
            int32_t *d_beg = (int32_t *)p;
            if ((rc = buf_ensure(h, B_PEND, n1 * sizeof(int32_t), &p))) return rc;
            int32_t *d_end = (int32_t *)p;
            if ((rc = buf_ensure(h, B_PFLAG, n1 * sizeof(uint32_t), &p))) return rc;
            uint32_t *d_flag = (uint32_t *)p;
            if ((rc = buf_ensure(h, B_PSEG, n1 * sizeof(ssp_seg_t), &p))) return rc;
            ssp_seg_t *d_seg = (ssp_seg_t *)p;
            if ((rc = buf_ensure(h, B_PMAXT, n1 * sizeof(int32_t), &p))) return rc;
            int32_t *d_maxt = (int32_t *)p;
            if ((rc = buf_ensure(h, B_PRANK, n1 * sizeof(uint32_t), &p))) return rc;
            uint32_t *d_rank = (uint32_t *)p;
            if ((rc = buf_ensure(h, B_PFROM, n1 * sizeof(int32_t), &p))) return rc;
            int32_t *d_from = (int32_t *)p;
            if ((rc = buf_ensure(h, B_PRUNV, ((size_t)n_out + 1) * sizeof(ssp_runv_t), &p))) return rc;
            ssp_runv_t *d_runv = (ssp_runv_t *)p;
            if ((rc = buf_ensure(h, B_PRUNK, ((size_t)n_out + 1) * sizeof(int32_t), &p))) return rc;
            int32_t *d_runk = (int32_t *)p;
            if ((rc = buf_ensure(h, B_PRUNA, ((size_t)n_out + 1) * sizeof(ssp_runv_t), &p))) return rc;
            ssp_runv_t *d_runa = (ssp_runv_t *)p;
            if ((rc = buf_ensure(h, B_PNRUN, sizeof(uint32_t), &p))) return rc;
            uint32_t *d_nrun = (uint32_t *)p;
            if ((rc = buf_ensure(h, B_PRES, sizeof(ssp_plan_res), &p))) return rc;
            ssp_plan_res *d_res = (ssp_plan_res *)p;
            size_t t1 = 0, t2 = 0, t3 = 0, t4 = 0;
            HIPCHK(hipcub::DeviceScan::InclusiveScan(nullptr, t1, d_seg, d_seg, ssp_seg_op(), (int)R, s));
            HIPCHK(hipcub::DeviceScan::InclusiveScan(nullptr, t2, d_maxt, d_maxt, ssp_max_op(), (int)R, s));
            HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, t3, d_rank, d_rank, (int)n1, s));
            HIPCHK(hipcub::DeviceReduce::ReduceByKey(nullptr, t4, tid, d_runk, d_runv, d_runa, d_nrun, ssp_runv_op(),
                                                     (int)n_out, s));
            size_t tmp = t1 > t2 ? t1 : t2;
            tmp = tmp > t3 ? tmp : t3;
            tmp = tmp > t4 ? tmp : t4;
            if ((rc = buf_ensure(h, B_SCAN, tmp ? tmp : 1, &p))) return rc;
            void *d_tmp = p;
            tmp = h->buf[B_SCAN].bytes;
            HIPCHK(hipMemcpyAsync(d_list, list.data(), list.size() * sizeof(ssp_emit_t), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemsetAsync(d_res, 0xff, sizeof(ssp_plan_res), s));
            hipLaunchKernelGGL(ss_plan_emit, dim3((uint32_t)list.size()), dim3(256), 0, s, bytes, len,
                               (const ssp_emit_t *)d_list, flag_mask, mapq_thresh, R, d_off, d_tid, d_beg, d_end,
                               d_flag, d_seg, d_maxt);
            if ((rc = launched())) return rc;
            size_t tb = tmp;
            HIPCHK(hipcub::DeviceScan::InclusiveScan(d_tmp, tb, d_seg, d_seg, ssp_seg_op(), (int)R, s));
            tb = tmp;
            HIPCHK(hipcub::DeviceScan::InclusiveScan(d_tmp, tb, d_maxt, d_maxt, ssp_max_op(), (int)R, s));
            const uint32_t blocks = (uint32_t)((n1 + 255u) / 256u);
            hipLaunchKernelGGL(ss_plan_keep, dim3(blocks), dim3(256), 0, s, R, t0, w0, max0, (const int32_t *)d_tid,
                               (const int32_t *)d_beg, (const int32_t *)d_end, (const uint32_t *)d_flag,
                               (const ssp_seg_t *)d_seg, (const int32_t *)d_maxt, d_rank, d_from, d_res);
            if ((rc = launched())) return rc;
            tb = tmp;
            HIPCHK(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, d_rank, d_rank, (int)n1, s));
            hipLaunchKernelGGL(ss_plan_out, dim3(blocks), dim3(256), 0, s, R, cap, (const uint64_t *)d_off,
                               (const int32_t *)d_tid, (const int32_t *)d_end, (const uint32_t *)d_rank,
                               (const int32_t *)d_from, rec_off, from, tid, d_runv, d_res);
            if ((rc = launched())) return rc;
            hipLaunchKernelGGL(ss_plan_final, dim3(1), dim3(64), 0, s, bytes, R, t0, w0, max0, chain_end,
                               chain_st == SSP_WALK_BAD ? 1u : 0u, (const uint64_t *)d_off, (const uint32_t *)d_rank,
                               (const ssp_seg_t *)d_seg, (const int32_t *)d_maxt, d_res);
            if ((rc = launched())) return rc;
            HIPCHK(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (res.n > n_out) return SS_E_HIP;           /* cannot happen: the ranks are below cap and n_rec */
            if (res.n) {
                uint32_t nrun = 0;
                tb = tmp;
                HIPCHK(hipcub::DeviceReduce::ReduceByKey(d_tmp, tb, tid, d_runk, d_runv, d_runa, d_nrun, ssp_runv_op(),
                                                         (int)res.n, s));
                HIPCHK(hipMemcpyAsync(&nrun, d_nrun, sizeof nrun, hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                *n_runs = nrun;
                if (nrun <= cap_runs) {
                    std::vector<int32_t> rk(nrun);
                    std::vector<ssp_runv_t> ra(nrun);
                    HIPCHK(hipMemcpyAsync(rk.data(), d_runk, (size_t)nrun * sizeof(int32_t), hipMemcpyDeviceToHost, s));
                    HIPCHK(hipMemcpyAsync(ra.data(), d_runa, (size_t)nrun * sizeof(ssp_runv_t), hipMemcpyDeviceToHost,
                                          s));
                    HIPCHK(hipStreamSynchronize(s));
                    uint32_t first = 0;
                    for (uint32_t i = 0; i < nrun; ++i) {
                        runs[i].tid = rk[i];
                        runs[i].first = first;
                        runs[i].n = ra[i].n;
                        runs[i].lo = ra[i].lo;
                        runs[i].hi = ra[i].hi;
                        first += ra[i].n;
                    }
                }
            }
        }
    }
    h->plan_ms[0] = std::chrono::duration<double, std::milli>(c1 - c0).count();
    h->plan_ms[1] = std::chrono::duration<double, std::milli>(c2 - c1).count();
    h->plan_ms[2] = std::chrono::duration<double, std::milli>(clk::now() - c2).count();
    state->has_prev = 1;
    state->tid = res.tid;
    state->w = res.w;
    state->max_tid = res.max_tid;
    *n = res.n;
    if (consumed) *consumed = res.consumed;
    if (*n_runs > cap_runs) return SS_E_CAPACITY;
    return res.code;
}

/* measurement hook (tools/plan_bench.py), not in the public header: the phases
 * of the latest ss_pileup_plan_device.  Each phase ends at a point where the
 * call waits for the stream anyway, so the host clock brackets it. */
extern "C" void ss__plan_phase_ms(ss_pileup_t *h, double ms[3])
{
    for (int k = 0; k < 3; ++k) ms[k] = h ? h->plan_ms[k] : 0.0;
}
