/*
 * selftest.c -- the oracle and the corpus generators under AddressSanitizer + UndefinedBehaviorSanitizer
 * (`make -C oracle sanitize`, run by tests/test_oracle.py::test_sanitized_selftest).  GPU sanitizers are not
 * available on this pool, so the CPU side of the test infrastructure is what gets sanitized.
 * Checks: known answers of SURVEY.md section 8a (the last one is the reference's doc-test vector,
 * src/lib.rs:28-29), naive sort == SA-IS == both integrity checks on random and adversarial inputs,
 * the multi-threaded verifier, LCP statistics, every generator at ragged sizes; oracle_lz77 and oracle_match_stats against
 * brute force written from the definitions of include/suffix_array_amd.h on adversarial families at n <= 300.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int32_t oracle_naive_sa(const uint8_t *s, uint32_t *sa, int64_t n);
int32_t oracle_sais(const uint8_t *s, uint32_t *sa, int64_t n);
int32_t oracle_check_integrity(const uint8_t *s, int64_t n, const uint32_t *sa, int64_t sa_len);
int32_t oracle_verify_sa(const uint8_t *s, int64_t n, const uint32_t *sa, int64_t sa_len);
int32_t oracle_verify_sa_mt(const uint8_t *s, int64_t n, const uint32_t *sa, int64_t sa_len, int32_t threads);
int32_t oracle_lcp_stats(const uint8_t *s, int64_t n, const uint32_t *sa, uint64_t *out);
void oracle_bucket_table(const uint8_t *s, int64_t n, uint32_t *bkt);
int64_t oracle_lz77(const uint8_t *t, int64_t n, const uint32_t *sa, uint32_t *lpf, uint32_t *src, uint32_t *phrases, int64_t capacity);
int32_t oracle_match_stats(const uint8_t *t, int64_t n, const uint32_t *sa, const uint8_t *q, int64_t m, int64_t cap, uint32_t *ml,
                           uint32_t *pos);
void sa_gen_uniform(uint8_t *out, int64_t n, uint64_t seed);
void sa_gen_sigma(uint8_t *out, int64_t n, uint64_t seed, int32_t sigma, int32_t base);
void sa_gen_dna(uint8_t *out, int64_t n, uint64_t seed);
void sa_gen_dna_repeats(uint8_t *out, int64_t n, uint64_t seed, double repeat_fraction);
int32_t sa_gen_english(uint8_t *out, int64_t n, uint64_t seed, int32_t vocab);
int32_t sa_gen_english_corpus(uint8_t *out, int64_t n, uint64_t seed, int32_t vocab, double dup_fraction);

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "selftest: %s failed at line %d\n", #c, __LINE__); ++failures; } } while (0)

static void check_text(const uint8_t *t, int64_t n)
{
    uint32_t *a = malloc(((size_t)n + 1) * 4), *b = malloc(((size_t)n + 1) * 4);
    CHECK(oracle_sais(t, a, n) == 0);
    if (n <= 20000) { CHECK(oracle_naive_sa(t, b, n) == 0); CHECK(memcmp(a, b, ((size_t)n + 1) * 4) == 0); }
    CHECK(oracle_verify_sa(t, n, a, n + 1) == 1);
    CHECK(oracle_verify_sa_mt(t, n, a, n + 1, 3) == 1);
    if (n <= 5000) CHECK(oracle_check_integrity(t, n, a, n + 1) == 1);
    if (n >= 3) {
        uint32_t x = a[1]; a[1] = a[2]; a[2] = x;
        CHECK(oracle_verify_sa(t, n, a, n + 1) == 0);
        CHECK(oracle_verify_sa_mt(t, n, a, n + 1, 2) == 0);
        x = a[1]; a[1] = a[2]; a[2] = x;
    }
    uint64_t st[32];
    CHECK(oracle_lcp_stats(t, n, a, st) == 0);
    free(a); free(b);
}

/* ---- brute force from the definitions of include/suffix_array_amd.h ---- */
#define BN 300                                  /* the families below have at most this many bytes */
#define NONE32 0xffffffffu

static int64_t brute_lcp(const uint8_t *x, int64_t lx, const uint8_t *y, int64_t ly)
{
    int64_t h = 0;
    while (h < lx && h < ly && x[h] == y[h]) ++h;
    return h;
}

/* slice order: lexicographic, a proper prefix is smaller */
static int brute_less(const uint8_t *x, int64_t lx, const uint8_t *y, int64_t ly)
{
    const int64_t h = brute_lcp(x, lx, y, ly);
    if (h < lx && h < ly) return x[h] < y[h];
    return lx < ly;
}

static void check_lz77(const uint8_t *t, int64_t n, const uint32_t *a)
{
    uint32_t lpf[BN + 1], src[BN + 1], ph[2 * BN + 2], elpf[BN + 1], esrc[BN + 1], eph[2 * BN + 2];
    for (int64_t i = 1; i <= n; ++i) {          /* P, N: the nearest slot on either side that holds a smaller position */
        const int64_t p = a[i];
        int64_t P = n, N = n;
        for (int64_t j = i - 1; j >= 1; --j) if ((int64_t)a[j] < p) { P = a[j]; break; }
        for (int64_t k = i + 1; k <= n; ++k) if ((int64_t)a[k] < p) { N = a[k]; break; }
        const int64_t lp = P == n ? 0 : brute_lcp(t + p, n - p, t + P, n - P), ln = N == n ? 0 : brute_lcp(t + p, n - p, t + N, n - N);
        elpf[p] = (uint32_t)(lp > ln ? lp : ln);
        esrc[p] = elpf[p] == 0 ? NONE32 : (lp >= ln ? (uint32_t)P : (uint32_t)N);
        int64_t best = 0;                       /* LPF[p] is also the longest prefix of T[p..] that starts at some q < p */
        for (int64_t q = 0; q < p; ++q) { const int64_t h = brute_lcp(t + p, n - p, t + q, n - q); if (h > best) best = h; }
        CHECK((int64_t)elpf[p] == best);
    }
    int64_t ez = 0;
    for (int64_t p = 0; p < n; ++ez) {
        const uint32_t len = elpf[p] ? elpf[p] : 1u;
        eph[2 * ez] = esrc[p]; eph[2 * ez + 1] = len;
        p += len;
    }
    memset(ph, 0xEE, sizeof ph);
    CHECK(oracle_lz77(t, n, a, lpf, src, ph, n) == ez);
    CHECK(memcmp(lpf, elpf, (size_t)n * 4) == 0 && memcmp(src, esrc, (size_t)n * 4) == 0 && memcmp(ph, eph, (size_t)ez * 8) == 0);
    for (int64_t k = 2 * ez; k < 2 * BN + 2; ++k) CHECK(ph[k] == 0xEEEEEEEEu);
    memset(ph, 0xEE, sizeof ph);                /* a cut capacity: the true count, the true prefix, nothing behind it */
    const int64_t cut = ez / 2;
    CHECK(oracle_lz77(t, n, a, lpf, src, ph, cut) == ez);
    CHECK(memcmp(ph, eph, (size_t)cut * 8) == 0);
    for (int64_t k = 2 * cut; k < 2 * BN + 2; ++k) CHECK(ph[k] == 0xEEEEEEEEu);
    CHECK(oracle_lz77(t, n, a, lpf, src, NULL, 0) == ez);
}

static void check_match(const uint8_t *t, int64_t n, const uint32_t *a, const uint8_t *q, int64_t m)
{
    const int64_t caps[] = { 1, 2, 3, 7, 64, 65, m > 1 ? m - 1 : 1, m > 0 ? m : 1, m + 5 };
    for (size_t ci = 0; ci < sizeof caps / sizeof caps[0]; ++ci) {
        const int64_t C = caps[ci];
        uint32_t ml[BN + 2], pos[BN + 2];
        memset(ml, 0xEE, sizeof ml); memset(pos, 0xEE, sizeof pos);
        CHECK(oracle_match_stats(t, n, a, q, m, C, ml + 1, pos + 1) == 0);
        CHECK(ml[0] == 0xEEEEEEEEu && pos[0] == 0xEEEEEEEEu && ml[m + 1] == 0xEEEEEEEEu && pos[m + 1] == 0xEEEEEEEEu);
        for (int64_t j = 0; j < m; ++j) {
            const uint8_t *w = q + j;
            const int64_t c = C < m - j ? C : m - j;
            int64_t i = 0;                      /* slots whose suffix is smaller than w (no order of the slots is assumed) */
            for (int64_t k = 0; k <= n; ++k) i += brute_less(t + a[k], n - a[k], w, c);
            CHECK(i >= 1 && i <= n + 1);
            const int64_t x = brute_lcp(w, c, t + a[i - 1], n - a[i - 1]), y = i <= n ? brute_lcp(w, c, t + a[i], n - a[i]) : -1;
            const int64_t best = x > y ? x : y;
            CHECK((int64_t)ml[j + 1] == best);
            CHECK(pos[j + 1] == (best == 0 ? NONE32 : (x > y ? a[i - 1] : a[i])));
            int64_t longest = 0;                /* ML[j] is also the longest prefix of w that occurs anywhere in T */
            for (int64_t p = 0; p < n; ++p) { const int64_t h = brute_lcp(w, c, t + p, n - p); if (h > longest) longest = h; }
            CHECK(best == longest);
        }
    }
}

static void check_extensions(const uint8_t *t, int64_t n, uint64_t seed)
{
    uint32_t a[BN + 1];
    uint8_t q[BN + 8];
    CHECK(n <= BN);
    CHECK(oracle_naive_sa(t, a, n) == 0);
    check_lz77(t, n, a);
    check_match(t, n, a, t, n);                                         /* the text itself */
    if (n > 1) check_match(t, n, a, t + 1, n - 1);
    check_match(t, n, a, t, 0);                                         /* the empty query */
    for (int64_t i = 0; i < n; ++i) q[i] = (uint8_t)(t[i] ^ (i % 37 == 0));      /* one byte in 37 changed */
    check_match(t, n, a, q, n);
    sa_gen_sigma(q, BN / 2, seed, 3, n ? t[0] : 'a');                   /* bytes around the text's first one */
    check_match(t, n, a, q, BN / 2);
    memset(q, 0x7e, 40);                                                /* a byte none of the families holds */
    check_match(t, n, a, q, 40);
}

static void check_extension_families(void)
{
    uint8_t t[BN + 1];
    static const int sizes[] = { 0, 1, 2, 3, 7, 64, 65, 129, 255, 256, 257, BN };
    for (size_t k = 0; k < sizeof sizes / sizeof sizes[0]; ++k) {
        const int64_t n = sizes[k];
        memset(t, 0, (size_t)n); check_extensions(t, n, k);                                              /* one byte value */
        memset(t, 0xff, (size_t)n); check_extensions(t, n, k);
        for (int64_t i = 0; i < n; ++i) t[i] = (uint8_t)("ab"[i & 1]);
        check_extensions(t, n, k);
        for (int64_t i = 0; i < n; ++i) t[i] = (uint8_t)("abc"[i % 3]);
        check_extensions(t, n, k);
        for (int64_t i = 0; i < n; ++i) t[i] = (uint8_t)(i < n / 2 ? 0x00 : 0xff);                      /* zeros, then ffs */
        check_extensions(t, n, k);
        for (int64_t i = 0; i < n; ++i) t[i] = (uint8_t)(i == n / 2 ? 'a' : 'b');                       /* b^k a b^k */
        check_extensions(t, n, k);
        for (int64_t i = 0; i < n; ++i) t[i] = (uint8_t)__builtin_parityll((unsigned long long)i);      /* Thue-Morse */
        check_extensions(t, n, k);
        {   /* Fibonacci word */
            static uint8_t f[2 * BN + 2], g[2 * BN + 2];
            int64_t lf = 1, lg = 2;
            f[0] = 'a'; g[0] = 'a'; g[1] = 'b';
            while (lg < n) {
                uint8_t tmp[2 * BN + 2];
                memcpy(tmp, g, (size_t)lg); memcpy(tmp + lg, f, (size_t)lf);
                memcpy(f, g, (size_t)lg);
                const int64_t nl = lg + lf; lf = lg; lg = nl;
                memcpy(g, tmp, (size_t)lg);
            }
            memcpy(t, g, (size_t)n); check_extensions(t, n, k);
        }
        for (int64_t i = 0; i < n; ++i) t[i] = (uint8_t)(i & 0xff);                                      /* ramp, repeated */
        check_extensions(t, n, k);
        for (int64_t i = 0; i < n / 2; ++i) t[i] = (uint8_t)((i * 7 + 3) & 0xff);                       /* a text twice */
        for (int64_t i = n / 2; i < n; ++i) t[i] = t[i - n / 2];
        check_extensions(t, n, k);
        sa_gen_sigma(t, n, 11 + k, 2, 'a'); check_extensions(t, n, k);
        sa_gen_sigma(t, n, 12 + k, 4, 0); check_extensions(t, n, k);
        sa_gen_dna_repeats(t, n, 13 + k, 0.3); check_extensions(t, n, k);
        sa_gen_uniform(t, n, 14 + k); check_extensions(t, n, k);
    }
}

int main(void)
{
    static const struct { const char *s; int n; uint32_t sa[18]; } known[] = {
        { "", 0, { 0 } }, { "a", 1, { 1, 0 } }, { "aa", 2, { 2, 1, 0 } }, { "banana", 6, { 6, 5, 3, 1, 0, 4, 2 } },
        { "mississippi", 11, { 11, 10, 7, 4, 1, 0, 9, 8, 6, 3, 5, 2 } },
        { "splendid splendor", 17, { 17, 8, 7, 5, 14, 3, 12, 6, 2, 11, 4, 13, 15, 1, 10, 16, 0, 9 } },
    };
    for (size_t k = 0; k < sizeof known / sizeof known[0]; ++k) {
        uint32_t out[18];
        CHECK(oracle_sais((const uint8_t *)known[k].s, out, known[k].n) == 0);
        CHECK(memcmp(out, known[k].sa, ((size_t)known[k].n + 1) * 4) == 0);
        CHECK(oracle_naive_sa((const uint8_t *)known[k].s, out, known[k].n) == 0);
        CHECK(memcmp(out, known[k].sa, ((size_t)known[k].n + 1) * 4) == 0);
    }
    static const int sizes[] = { 0, 1, 2, 3, 63, 64, 65, 255, 257, 1000, 4095, 4097, 30011 };
    for (size_t k = 0; k < sizeof sizes / sizeof sizes[0]; ++k) {
        const int64_t n = sizes[k];
        uint8_t *t = malloc((size_t)n + 1);
        sa_gen_uniform(t, n, 1 + k); check_text(t, n);
        sa_gen_sigma(t, n, 2 + k, 3, 250); check_text(t, n);
        sa_gen_dna(t, n, 3 + k); check_text(t, n);
        sa_gen_dna_repeats(t, n, 4 + k, 0.3); check_text(t, n);
        CHECK(sa_gen_english(t, n, 5 + k, 500) == 0); check_text(t, n);
        CHECK(sa_gen_english_corpus(t, n, 6 + k, 500, 0.2) == 0); check_text(t, n);
        memset(t, 0xff, (size_t)n); check_text(t, n);
        for (int64_t i = 0; i < n; ++i) t[i] = (uint8_t)("ab"[i & 1]);
        check_text(t, n);
        free(t);
    }
    {   /* a corpus large enough for every generator layer (copies, second printings) */
        const int64_t n = (3 << 20) + 17;
        uint8_t *t = malloc((size_t)n);
        CHECK(sa_gen_english_corpus(t, n, 3, 50000, 0.08) == 0);
        check_text(t, n);
        uint32_t *bkt = malloc((256 * 257 + 1) * 4);
        oracle_bucket_table(t, n, bkt);
        CHECK(bkt[256 * 257] == (uint32_t)n + 1);
        free(bkt); free(t);
    }
    check_extension_families();
    if (failures) { fprintf(stderr, "selftest: %d failures\n", failures); return 1; }
    puts("selftest ok");
    return 0;
}
