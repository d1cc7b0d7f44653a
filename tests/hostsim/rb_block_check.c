/*
 * rb_block_check.c -- TEST: rb_block (a vrank's final block by the halving rule) against
 * rb_windows' rindex / rcount of the last step, for every vrank of p = 2 .. 32 and counts from
 * below p (empty blocks) to past 2^31.  Stand-alone, built with the sanitizers.
 */
#include <stdio.h>

#include "ftar_raben.h"

int main(void)
{
    const size_t counts[] = {1, 3, 17, 1031, 4099, ((size_t)1 << 31) + 5};
    int bad = 0, n = 0;
    for (int steps = 1; steps <= 5; steps++)
        for (size_t k = 0; k < sizeof(counts) / sizeof(counts[0]); k++) {
            rb_ctx x = {.count = counts[k], .steps = steps};
            for (int u = 0; u < 1 << steps; u++, n++) {
                int64_t ri[MAXSTEPS], si[MAXSTEPS], rc[MAXSTEPS], sc[MAXSTEPS], off, len;
                rb_windows(u, x.count, steps, ri, si, rc, sc);
                rb_block(&x, u, &off, &len);
                if (off != ri[steps - 1] || len != rc[steps - 1]) {
                    printf("p=%d count=%zu vrank=%d: rb_block (%lld, %lld), rb_windows (%lld, %lld)\n", 1 << steps,
                           x.count, u, (long long)off, (long long)len, (long long)ri[steps - 1],
                           (long long)rc[steps - 1]);
                    bad++;
                }
            }
        }
    printf("%d blocks checked, %d differ\n", n, bad);
    return bad != 0;
}
