/*
 * ss_inflate.hip -- BGZF member inflation on the GPU (include/sniper_amd.h,
 * "BGZF inflation"): the ss_inflate_members kernel, its handle and the host /
 * device / CPU entry points, and the BGZF member scanner.
 *
 * Kernel shape.  One wave64 per member; the Huffman
 * walk is serial in the bitstream, so the rate comes from thousands of members
 * in flight.  Every lane of the wave runs the shared decoder (ss_inflate_core.h)
 * on the same state -- the walk is wave-uniform, nothing is exchanged between
 * lanes while decoding -- and lane k keeps the k-th item of a run of up to 64.
 * The run is then emitted by all lanes: a wave prefix sum of the item lengths
 * gives every item its output position, the whole run is checked against the
 * member's output span before any store, literals are stored in parallel, and
 * matches and stored-block payloads are copied one after the other with the
 * lanes spread over the bytes (source start + (i mod distance) when the
 * distance is shorter than the length).
 *
 * Output goes straight to global memory, so a back-reference may read bytes
 * another lane of the wave stored a moment ago.  The wave tracks the lowest
 * output position stored since its last fence; a match whose source reaches
 * that position first executes a workgroup-scope acquire-release fence (all
 * the wave's stores have completed, no load is moved above it).  Lanes of one
 * wave share the CU's vector L1, so completed stores are visible to the loads
 * that follow.
 *
 * LDS: 2.3 KiB of decode tables per wave + one 1 KiB CRC table per block.
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sniper_amd.h"
#include "ss_inflate_core.h"

#define SSI_WAVES 4                      /* waves (members) per workgroup */

static __device__ __forceinline__ void ssi_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

static __device__ __forceinline__ uint32_t ssi_scan_incl(uint32_t v, uint32_t lane)
{
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, s, 64);
        if (lane >= (uint32_t)s) v += u;
    }
    return v;
}

__global__ __launch_bounds__(SSI_WAVES * 64) void ss_inflate_members(
    const uint8_t *__restrict__ comp, const uint64_t *__restrict__ comp_off, uint64_t comp_base, uint32_t n,
    uint8_t *out, const uint64_t *__restrict__ out_off, uint64_t out_base, uint32_t *__restrict__ status)
{
    __shared__ ssi_tables_t s_tab[SSI_WAVES];
    __shared__ uint32_t s_crc[256];
    s_crc[threadIdx.x] = ssi_crc_entry(threadIdx.x);
    __syncthreads();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t m = blockIdx.x * SSI_WAVES + wave;
    if (m >= n) return;
    ssi_tables_t *t = &s_tab[wave];

    const uint64_t c0 = comp_off[m], c1 = comp_off[m + 1], o0 = out_off[m], o1 = out_off[m + 1];
    /* offsets that decrease, or spans no BGZF member has: nothing is read or written */
    if (c1 < c0 || o1 < o0 || c0 < comp_base || o0 < out_base || c1 - c0 > SSI_COMP_MAX || o1 - o0 > SSI_MEMBER_MAX) {
        if (lane == 0) status[m] = SSI_E_STREAM;
        return;
    }
    const uint8_t *in = comp + (c0 - comp_base);
    uint8_t *outp = out + (o0 - out_base);
    const uint32_t clen = (uint32_t)(c1 - c0), olen = (uint32_t)(o1 - o0);

    uint32_t st = SSI_OK, crc_want = 0;
    if (clen < 8u) st = SSI_E_STREAM;
    else {
        crc_want = ssi_le32(in + clen - 8u);
        if (ssi_le32(in + clen - 4u) != olen) st = SSI_E_SIZE;
    }
    uint32_t op = 0;
    if (st == SSI_OK) {
        ssi_dec_t d;
        ssi_init(&d, in, clen - 8u);
        uint32_t dirty_lo = 0xffffffffu;     /* lowest position stored since the last fence */
        int done = 0;
        while (!done && st == SSI_OK) {
            /* decode a run: lane k keeps item k */
            int my_kind = SSI_END;
            uint32_t my_val = 0, my_dist = 0, cnt = 0;
            while (cnt < 64u) {
                uint32_t val = 0, dist = 0;
                const int k = ssi_next(&d, t, &val, &dist);
                if (k == SSI_END) { done = 1; break; }
                if (k == SSI_ERR) { st = SSI_E_STREAM; break; }
                if (lane == cnt) { my_kind = k; my_val = val; my_dist = dist; }
                ++cnt;
            }
            /* positions; every item is checked against the span before any store of the run */
            const uint32_t my_len = my_kind == SSI_END ? 0u : my_kind == SSI_LIT ? 1u : my_val;
            const uint32_t incl = ssi_scan_incl(my_len, lane);      /* <= 64 * 65535 */
            const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
            const uint32_t my_pos = op + (incl - my_len);
            const bool bad = my_kind != SSI_END &&
                             (my_pos > olen || my_len > olen - my_pos || (my_kind == SSI_MATCH && my_dist > my_pos));
            if (__ballot(bad)) { st = SSI_E_STREAM; break; }
            if (st != SSI_OK) break;
            if (my_kind == SSI_LIT) outp[my_pos] = (uint8_t)my_val;
            if (__ballot(my_kind == SSI_LIT) && op < dirty_lo) dirty_lo = op;
            uint64_t copies = __ballot(my_kind == SSI_MATCH || my_kind == SSI_STORED);
            while (copies) {
                const int l = __builtin_ctzll(copies);
                copies &= copies - 1;
                const uint32_t p = (uint32_t)__shfl((int)my_pos, l, 64);
                const uint32_t len = (uint32_t)__shfl((int)my_val, l, 64);
                const uint32_t ds = (uint32_t)__shfl((int)my_dist, l, 64);
                const int kd = __shfl(my_kind, l, 64);
                if (kd == SSI_STORED) {
                    /* ds + len <= clen - 8: checked by ssi_next */
                    for (uint32_t i = lane; i < len; i += 64u) outp[p + i] = in[ds + i];
                } else {
                    const uint32_t src = p - ds;                     /* ds <= p: checked above */
                    if (src + (len < ds ? len : ds) > dirty_lo) {
                        ssi_fence();
                        dirty_lo = 0xffffffffu;
                    }
                    if (ds >= len) {
                        for (uint32_t i = lane; i < len; i += 64u) outp[p + i] = outp[src + i];
                    } else {
                        for (uint32_t i = lane; i < len; i += 64u) outp[p + i] = outp[src + i % ds];
                    }
                }
                if (p < dirty_lo) dirty_lo = p;
            }
            op += total;
        }
        if (st == SSI_OK && op != olen) st = SSI_E_SIZE;
    }
    if (st == SSI_OK) {
        /* CRC-32: each lane over 1/64 of the output, combined pairwise with x^(8 len) mod P */
        ssi_fence();
        const uint32_t per = (olen + 63u) >> 6;
        const uint32_t beg = lane * per < olen ? lane * per : olen;
        const uint32_t end = beg + per < olen ? beg + per : olen;
        uint32_t c = ssi_crc_bytes(s_crc, 0xffffffffu, outp + beg, end - beg) ^ 0xffffffffu;
        uint32_t clen_l = end - beg;
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t rc = (uint32_t)__shfl_down((int)c, s, 64);
            const uint32_t rl = (uint32_t)__shfl_down((int)clen_l, s, 64);
            if ((lane & (uint32_t)(2 * s - 1)) == 0u) {
                c = ssi_crc_combine(c, rc, rl);
                clen_l += rl;
            }
        }
        c = (uint32_t)__shfl((int)c, 0, 64);
        if (c != crc_want) st = SSI_E_CRC;
    }
    if (st != SSI_OK) {
        /* a failed member's span is zeroed, as on the host; the fence keeps
         * these stores behind the run stores other lanes made to the same bytes */
        ssi_fence();
        for (uint32_t i = lane; i < olen; i += 64u) outp[i] = 0;
    }
    if (lane == 0) status[m] = st;
}

/* ---------------------------------------------------------------- handle ---- */
#ifdef SS_DEBUG_CANARY
#define SSI_GUARD ((size_t)4096)
#else
#define SSI_GUARD ((size_t)0)
#endif

struct ssi_buf {
    void *base;      /* hipMalloc'd; the usable part starts SSI_GUARD bytes in */
    size_t bytes;
};

struct ss_inflate {
    int device;
    uint32_t max_members;
    hipStream_t stream;
    ssi_buf comp, out, coff, ooff, status;
    int corrupt;     /* a guard band of a buffer that has since been replaced was damaged */
};

#define HIPCHK(x)                                   \
    do {                                            \
        if ((x) != hipSuccess) return SS_E_HIP;     \
    } while (0)

static inline void *buf_user(const ssi_buf &b) { return b.base ? (char *)b.base + SSI_GUARD : nullptr; }

static int buf_guards_ok(ss_inflate_t *h, const ssi_buf &b)
{
#ifdef SS_DEBUG_CANARY
    if (!b.base) return SS_OK;
    std::vector<unsigned char> g(2 * SSI_GUARD);
    if (hipMemcpyAsync(g.data(), b.base, SSI_GUARD, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipMemcpyAsync(g.data() + SSI_GUARD, (char *)b.base + SSI_GUARD + b.bytes, SSI_GUARD, hipMemcpyDeviceToHost,
                       h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
        return SS_E_HIP;
    for (size_t i = 0; i < g.size(); ++i)
        if (g[i] != 0xA5) {
            fprintf(stderr, "[sniper_amd] guard band of inflate buffer %p (%zu bytes) overwritten at %s%zu\n",
                    buf_user(b), b.bytes, i < SSI_GUARD ? "-" : "+", i < SSI_GUARD ? SSI_GUARD - i : i - SSI_GUARD);
            return SS_E_CORRUPT;
        }
#else
    (void)h; (void)b;
#endif
    return SS_OK;
}

/* the handle's stream is idle */
static void buf_free(ss_inflate_t *h, ssi_buf &b)
{
    if (!b.base) return;
    if (buf_guards_ok(h, b) == SS_E_CORRUPT) h->corrupt = 1;
    (void)hipFree(b.base);
    b.base = nullptr;
    b.bytes = 0;
}

/* at least `bytes` usable bytes; contents are not kept.  Waits for the
 * handle's stream before a buffer is replaced. */
static int buf_ensure(ss_inflate_t *h, ssi_buf &b, size_t bytes)
{
    if (b.base && b.bytes >= bytes) return SS_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    buf_free(h, b);
    size_t sz = bytes < 4096 ? 4096 : bytes + bytes / 4;
    sz = (sz + 255) & ~(size_t)255;
    if (hipMalloc(&b.base, sz + 2 * SSI_GUARD) != hipSuccess) {
        (void)hipGetLastError();
        b.base = nullptr;
        return SS_E_NOMEM;
    }
    b.bytes = sz;
#ifdef SS_DEBUG_CANARY
    HIPCHK(hipMemsetAsync(b.base, 0xA5, SSI_GUARD, h->stream));
    HIPCHK(hipMemsetAsync((char *)b.base + SSI_GUARD + sz, 0xA5, SSI_GUARD, h->stream));
#endif
    return SS_OK;
}

extern "C" int ss_inflate_create(int device, uint32_t max_members, ss_inflate_t **out)
{
    if (!out || max_members == 0 || max_members > (1u << 24)) return SS_E_INVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        return SS_E_NODEV;
    }
    HIPCHK(hipSetDevice(device));
    ss_inflate_t *h = (ss_inflate_t *)calloc(1, sizeof *h);
    if (!h) return SS_E_NOMEM;
    h->device = device;
    h->max_members = max_members;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        free(h);
        return SS_E_HIP;
    }
    const size_t offb = ((size_t)max_members + 1) * sizeof(uint64_t);
    int rc = buf_ensure(h, h->coff, offb);
    if (rc == SS_OK) rc = buf_ensure(h, h->ooff, offb);
    if (rc == SS_OK) rc = buf_ensure(h, h->status, (size_t)max_members * sizeof(uint32_t));
    if (rc != SS_OK) {
        ss_inflate_destroy(h);
        return rc;
    }
    *out = h;
    return SS_OK;
}

extern "C" int ss_inflate_check(ss_inflate_t *h)
{
    if (!h) return SS_E_INVAL;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->corrupt) return SS_E_CORRUPT;
    for (const ssi_buf *b : {&h->comp, &h->out, &h->coff, &h->ooff, &h->status})
        if (int rc = buf_guards_ok(h, *b)) return rc;
    return SS_OK;
}

extern "C" void ss_inflate_destroy(ss_inflate_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    for (ssi_buf *b : {&h->comp, &h->out, &h->coff, &h->ooff, &h->status}) buf_free(h, *b);
    if (h->corrupt) fprintf(stderr, "[sniper_amd] ss_inflate_destroy: device memory corrupted (see above)\n");
    (void)hipStreamDestroy(h->stream);
    free(h);
}

static int launch(const uint8_t *comp, const uint64_t *comp_off, uint64_t comp_base, uint32_t n, uint8_t *out,
                  const uint64_t *out_off, uint64_t out_base, uint32_t *status, hipStream_t s)
{
    const uint32_t blocks = (n + SSI_WAVES - 1) / SSI_WAVES;
    hipLaunchKernelGGL(ss_inflate_members, dim3(blocks), dim3(SSI_WAVES * 64), 0, s, comp, comp_off, comp_base, n, out,
                       out_off, out_base, status);
    return hipGetLastError() == hipSuccess ? SS_OK : SS_E_HIP;
}

extern "C" int ss_inflate_members_device(ss_inflate_t *h, const uint8_t *comp, const uint64_t *comp_off, uint32_t n,
                                         uint8_t *out, const uint64_t *out_off, uint32_t *status, void *stream)
{
    if (!h || n > h->max_members) return SS_E_INVAL;
    if (n == 0) return SS_OK;
    if (!comp || !comp_off || !out_off || !status) return SS_E_INVAL;   /* out may be NULL when every span is empty */
    HIPCHK(hipSetDevice(h->device));
    return launch(comp, comp_off, 0, n, out, out_off, 0, status, (hipStream_t)stream);
}

/* offsets must not decrease, a member has at most 64 KiB + 8 input bytes and
 * 64 KiB of output */
static int offsets_ok(const uint64_t *comp_off, const uint64_t *out_off, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i) {
        if (comp_off[i + 1] < comp_off[i] || out_off[i + 1] < out_off[i]) return 0;
        if (comp_off[i + 1] - comp_off[i] > SSI_COMP_MAX || out_off[i + 1] - out_off[i] > SSI_MEMBER_MAX) return 0;
    }
    return 1;
}

extern "C" int ss_inflate_members_host(ss_inflate_t *h, const uint8_t *comp, const uint64_t *comp_off, uint32_t n,
                                       uint8_t *out, const uint64_t *out_off, uint32_t *status)
{
    if (!h || n > h->max_members) return SS_E_INVAL;
    if (n == 0) return SS_OK;
    if (!comp || !comp_off || !out_off || !status || !offsets_ok(comp_off, out_off, n)) return SS_E_INVAL;
    if (!out && out_off[n] != out_off[0]) return SS_E_INVAL;
    HIPCHK(hipSetDevice(h->device));
    const uint64_t cb = comp_off[0], ob = out_off[0];
    const size_t cbytes = (size_t)(comp_off[n] - cb), obytes = (size_t)(out_off[n] - ob);
    int rc;
    if ((rc = buf_ensure(h, h->comp, cbytes + 1)) != SS_OK || (rc = buf_ensure(h, h->out, obytes + 1)) != SS_OK)
        return rc;
    uint8_t *d_comp = (uint8_t *)buf_user(h->comp), *d_out = (uint8_t *)buf_user(h->out);
    uint64_t *d_coff = (uint64_t *)buf_user(h->coff), *d_ooff = (uint64_t *)buf_user(h->ooff);
    uint32_t *d_status = (uint32_t *)buf_user(h->status);
    hipStream_t s = h->stream;
    /* page-locked arrays (ss_host_alloc) go to the device by DMA straight from
     * where they are; the runtime stages pageable ones itself */
    if (cbytes) HIPCHK(hipMemcpyAsync(d_comp, comp + cb, cbytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_coff, comp_off, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_ooff, out_off, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    if ((rc = launch(d_comp, d_coff, cb, n, d_out, d_ooff, ob, d_status, s)) != SS_OK) return rc;
    if (obytes) HIPCHK(hipMemcpyAsync(out + ob, d_out, obytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status, d_status, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return SS_OK;
}

extern "C" int ss_inflate_members_cpu(const uint8_t *comp, const uint64_t *comp_off, uint32_t n, uint8_t *out,
                                      const uint64_t *out_off, uint32_t *status)
{
    if (n == 0) return SS_OK;
    if (!comp || !comp_off || !out_off || !status || !offsets_ok(comp_off, out_off, n)) return SS_E_INVAL;
    if (!out && out_off[n] != out_off[0]) return SS_E_INVAL;
    ssi_tables_t *t = (ssi_tables_t *)malloc(sizeof *t);
    if (!t) return SS_E_NOMEM;
    uint32_t crc_tab[256];
    for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = ssi_crc_entry(i);
    for (uint32_t i = 0; i < n; ++i)
        status[i] = ssi_inflate_member(comp + comp_off[i], (uint32_t)(comp_off[i + 1] - comp_off[i]), out + out_off[i],
                                       (uint32_t)(out_off[i + 1] - out_off[i]), t, crc_tab);
    free(t);
    return SS_OK;
}

/* ------------------------------------------------------------ BGZF scan ---- */
extern "C" int ss_bgzf_scan(const uint8_t *file, size_t len, uint64_t *comp_span, uint64_t *out_off, uint32_t cap,
                            uint32_t *n_members, size_t *consumed)
{
    if ((!file && len) || !comp_span || !out_off || !n_members) return SS_E_INVAL;
    size_t at = 0;
    uint32_t n = 0;
    uint64_t oo = 0;
    while (n < cap && len - at >= 12) {
        const uint8_t *h = file + at;
        if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return SS_E_INVAL;
        const size_t xlen = (size_t)h[10] | (size_t)h[11] << 8;
        if (len - at - 12 < xlen) break;                       /* incomplete */
        long bsize = -1;
        for (size_t p = 0; p + 4 <= xlen;) {
            const uint8_t *x = h + 12 + p;
            const size_t sl = (size_t)x[2] | (size_t)x[3] << 8;
            if (x[0] == 'B' && x[1] == 'C' && sl == 2 && p + 6 <= xlen) bsize = (long)x[4] | (long)x[5] << 8;
            p += 4 + sl;
        }
        if (bsize < 0) return SS_E_INVAL;
        const long clen = bsize + 1 - 12 - (long)xlen;         /* DEFLATE data + trailer */
        if (clen < 8) return SS_E_INVAL;
        if (len - at < (size_t)bsize + 1) break;               /* incomplete */
        const size_t pay = at + 12 + xlen;
        const uint32_t isize = ssi_le32(file + pay + (size_t)clen - 4);
        if (isize > SSI_MEMBER_MAX) return SS_E_INVAL;
        /* the next member's gzip header lies between two payloads, so every
         * member gets its own (start, end) pair */
        comp_span[2 * (size_t)n] = pay;
        comp_span[2 * (size_t)n + 1] = pay + (size_t)clen;
        out_off[n] = oo;
        oo += isize;
        at += (size_t)bsize + 1;
        ++n;
    }
    out_off[n] = oo;
    *n_members = n;
    if (consumed) *consumed = at;
    return SS_OK;
}
