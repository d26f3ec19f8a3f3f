/* inflate_driver.c -- stand-alone driver of the shared DEFLATE decoder
 * (somatic-sniper_amd/csrc/ss_inflate_core.h) for the sanitizer builds
 * (make -C somatic-sniper_amd sanitize -> build/san/inflate-asan).
 *
 *   inflate-asan corpus.bin
 *
 * corpus.bin (tests/inflate_corpus.py write_file): u32 count, then per member
 * u32 clen, u32 olen, u32 expected status, u32 CRC-32 of the expected output
 * (zeros for a member that must fail) and the clen input bytes; status
 * 0xffffffff accepts any outcome (mutated members).  Every member
 * gets heap blocks of exactly its input and output sizes, so a read or write
 * outside its spans is an ASan report; UBSan watches the shifts and the
 * arithmetic.  Prints "ok=1 members=N" and exits 0 when every status and
 * every output matched. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ss_inflate_core.h"

static int rd32(FILE *f, uint32_t *v)
{
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) return -1;
    *v = ssi_le32(b);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s corpus.bin\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    uint32_t n = 0;
    if (!f || rd32(f, &n)) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    uint32_t crc_tab[256];
    for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = ssi_crc_entry(i);
    ssi_tables_t *t = (ssi_tables_t *)malloc(sizeof *t);
    int bad = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t clen, olen, want_status, want_crc;
        if (rd32(f, &clen) || rd32(f, &olen) || rd32(f, &want_status) || rd32(f, &want_crc) || clen > SSI_COMP_MAX ||
            olen > SSI_MEMBER_MAX + 1u) {
            fprintf(stderr, "member %u: bad record\n", i);
            return 2;
        }
        uint8_t *in = (uint8_t *)malloc(clen ? clen : 1), *out = (uint8_t *)malloc(olen ? olen : 1);
        if (!in || !out || !t || fread(in, 1, clen, f) != clen) {
            fprintf(stderr, "member %u: short read\n", i);
            return 2;
        }
        memset(out, 0xA5, olen ? olen : 1);
        const uint32_t st = ssi_inflate_member(in, clen, out, olen, t, crc_tab);
        const uint32_t crc = ssi_crc_bytes(crc_tab, 0xffffffffu, out, olen) ^ 0xffffffffu;
        if (want_status == 0xffffffffu) {               /* mutated member: any status, checked for safety only */
            if (st > SSI_E_CRC) bad = 1;
        } else if (st != want_status || crc != want_crc) {
            fprintf(stderr, "member %u: status %u (want %u), output crc %08x (want %08x)\n", i, st, want_status, crc,
                    want_crc);
            bad = 1;
        }
        /* the lane-parallel CRC of the kernel: 64 pieces combined pairwise */
        if (st == SSI_OK) {
            const uint32_t per = (olen + 63u) >> 6;
            uint32_t c[64], l[64];
            for (uint32_t k = 0; k < 64; ++k) {
                const uint32_t beg = k * per < olen ? k * per : olen, end = beg + per < olen ? beg + per : olen;
                c[k] = ssi_crc_bytes(crc_tab, 0xffffffffu, out + beg, end - beg) ^ 0xffffffffu;
                l[k] = end - beg;
            }
            for (uint32_t s = 1; s < 64; s <<= 1)
                for (uint32_t k = 0; k < 64; k += 2 * s) {
                    c[k] = ssi_crc_combine(c[k], c[k + s], l[k + s]);
                    l[k] += l[k + s];
                }
            if (c[0] != crc) {
                fprintf(stderr, "member %u: combined crc %08x != %08x\n", i, c[0], crc);
                bad = 1;
            }
        }
        free(in);
        free(out);
    }
    free(t);
    fclose(f);
    printf("ok=%d members=%u\n", !bad, n);
    return bad;
}
