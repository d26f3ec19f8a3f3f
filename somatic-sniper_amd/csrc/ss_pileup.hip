/*
 * ss_pileup.hip -- pileup columns from BAM records on the GPU
 * (include/sniper_amd.h, "pileup columns from BAM records"): the kernels, the
 * ss_pileup_t handle and the device / host entry points.  DESIGN.md section 13.
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

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sniper_amd.h"
#include "ss_pileup_core.h"

extern "C" int ssp_sample_args_ok(const ss_pileup_sample_t *s);     /* ss_pileup_plan.c */

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
