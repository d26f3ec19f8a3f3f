/* bgzf_reader.h -- sequential reader of BGZF files (the BAM container,
 * SAM spec section 4.1) with block-parallel inflation on a thread pool. */
#ifndef SS_BGZF_READER_H
#define SS_BGZF_READER_H

#include <stddef.h>
#include <stdint.h>

typedef struct bgzf_reader bgzf_reader_t;

/* path "-" reads stdin.  n_threads <= 0 inflates on the calling thread. */
bgzf_reader_t *bgzf_open(const char *path, int n_threads);
/* The same, reading from virtual offset voff (compressed member offset << 16
 * | offset inside the member, as a BAM index stores it); not for stdin. */
bgzf_reader_t *bgzf_open_at(const char *path, int n_threads, uint64_t voff);
/* Virtual offset of the next byte bgzf_read returns (synchronous readers,
 * n_threads <= 0, only; -1 otherwise). */
int64_t bgzf_tell(const bgzf_reader_t *r);
/* Reads up to n bytes; returns the count (< n only at end of data) or -1 on a
 * malformed / truncated file. */
long bgzf_read(bgzf_reader_t *r, void *dst, size_t n);
/* Batched inflation behind a callback (the reader itself stays free of the GPU
 * library: ss-index links it alone).  The I/O thread fills a ring of
 * 2 * batch slots (at least), one batch thread packs each group of `batch`
 * loaded members -- fewer at the end of the file -- one after the other and
 * hands them to ops->inflate, and bgzf_read drains the slots in file order as
 * in the threaded mode.  Member i of a call is comp[comp_off[i] ..
 * comp_off[i+1]) (DEFLATE data + the 8-byte gzip trailer), its output span
 * out[out_off[i] .. out_off[i+1]) is ISIZE bytes long; the callback returns 0
 * and one status per member (0 = inflated and verified).  A member with
 * another status is inflated again on the host (libdeflate / zlib), so a
 * corrupt file reads and fails exactly as without the callback; a call that
 * fails as a whole is a read error.  alloc / release (NULL: malloc / free)
 * provide the buffers the callback sees, so they can be page-locked. */
typedef int (*bgzf_batch_fn)(void *user, const uint8_t *comp, const uint64_t *comp_off, uint32_t n, uint8_t *out,
                             const uint64_t *out_off, uint32_t *status);
typedef struct bgzf_batch_ops {
    bgzf_batch_fn inflate;
    void *user;
    void *(*alloc)(size_t bytes);
    void (*release)(void *p);
} bgzf_batch_ops_t;
/* voff as bgzf_open_at (0: the start of the file; "-" only with voff 0); batch in [1, 4096] */
bgzf_reader_t *bgzf_open_batched(const char *path, uint64_t voff, int batch, const bgzf_batch_ops_t *ops);
/* 1 and the counts so far for a batched reader (members handed to the
 * callback, calls, members inflated again on the host), 0 otherwise */
int bgzf_batch_stats(const bgzf_reader_t *r, uint64_t *members, uint64_t *batches, uint64_t *fallback, void **user);
void bgzf_close(bgzf_reader_t *r);
const char *bgzf_error(const bgzf_reader_t *r);

#endif
