/* Single-core CPU baseline for tools/lz77_bench.py: LPF with sources and the greedy LZ77 parse from a text and its suffix array
 * (layout of sa_amd_saca_u8: n + 1 entries, SA[0] = n), by the definition of include/suffix_array_amd.h.
 * A stack pass over SA[1 .. n] gives the nearest smaller neighbours P and N in text order; the matches are then compared in
 * text order, starting from the previous position's match minus one (lp(p) >= lp(p - 1) - 1, likewise ln), so the compares are
 * amortised over the text.  gcc -O2 -shared -fPIC -o lz77_cpu.so lz77_cpu.c */
#include <stdint.h>
#include <stdlib.h>

static int64_t extend(const uint8_t *t, int64_t n, int64_t p, int64_t q, int64_t h)
{
    if (q >= n) return 0;
    if (h < 0) h = 0;
    const int64_t lim = n - (p > q ? p : q);
    if (h > lim) h = lim;
    while (h < lim && t[p + h] == t[q + h]) ++h;
    return h;
}

/* phrases: 2 * capacity entries; returns the number of phrases, or -1 when memory runs out */
int64_t lz77_cpu(const uint8_t *t, int64_t n, const uint32_t *sa, uint32_t *lpf, uint32_t *src, uint32_t *phrases, int64_t capacity)
{
    if (n == 0) return 0;
    uint32_t *P = malloc((size_t)n * 4), *N = malloc((size_t)n * 4), *st = malloc((size_t)n * 4);
    if (!P || !N || !st) { free(P); free(N); free(st); return -1; }
    const uint32_t *a = sa + 1;
    int64_t top = 0;
    for (int64_t i = 0; i < n; ++i) {
        while (top && a[st[top - 1]] > a[i]) N[a[st[--top]]] = a[i];
        P[a[i]] = top ? a[st[top - 1]] : (uint32_t)n;
        st[top++] = (uint32_t)i;
    }
    while (top) N[a[st[--top]]] = (uint32_t)n;
    int64_t lp = 0, ln = 0;
    for (int64_t p = 0; p < n; ++p) {
        lp = extend(t, n, p, P[p], lp - 1);
        ln = extend(t, n, p, N[p], ln - 1);
        lpf[p] = (uint32_t)(lp >= ln ? lp : ln);
        src[p] = (lp | ln) == 0 ? 0xffffffffu : (lp >= ln ? P[p] : N[p]);
    }
    free(P); free(N); free(st);
    int64_t z = 0;
    for (int64_t p = 0; p < n; ++z) {
        const uint32_t l = lpf[p] ? lpf[p] : 1u;
        if (z < capacity) { phrases[2 * z] = src[p]; phrases[2 * z + 1] = l; }
        p += l;
    }
    return z;
}
