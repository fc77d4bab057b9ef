/* The plain inverse Burrows-Wheeler walk on one CPU core, as a yardstick for tools/bwt_bench.py: psi and the first column by a
 * counting sort, then n dependent loads.  Reads B (n bytes) from the file argv[1], primary from argv[2]; prints the milliseconds of
 * the counting sort and of the walk and a checksum of the text. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

static double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec / 1e6;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    const long primary = atol(argv[2]);
    uint8_t *B = malloc((size_t)n + 1), *T = malloc((size_t)n + 1);
    uint32_t *psi = malloc(((size_t)n + 1) * 4);
    if (!B || !T || !psi || fread(B, 1, (size_t)n, f) != (size_t)n) return 2;
    fclose(f);
    const double t0 = now_ms();
    long start[257] = { 0 };
    for (long b = 0; b < n; ++b) start[B[b] + 1]++;
    for (int c = 0; c < 256; ++c) start[c + 1] += start[c];
    long first[257];
    for (int c = 0; c <= 256; ++c) first[c] = start[c] + 1;
    psi[0] = (uint32_t)primary;
    for (long b = 0; b < n; ++b) psi[1 + start[B[b]]++] = (uint32_t)(b < primary ? b : b + 1);
    const double t1 = now_ms();
    uint32_t row = (uint32_t)primary;
    int c = 0;
    for (long j = 0; j < n; ++j) {
        while (c < 255 && first[c + 1] <= (long)row) ++c;
        while (first[c] > (long)row) --c;
        T[j] = (uint8_t)c;
        row = psi[row];
    }
    const double t2 = now_ms();
    uint64_t sum = 0;
    for (long j = 0; j < n; ++j) sum = sum * 31 + T[j];
    printf("n=%ld sort_ms=%.1f walk_ms=%.1f closed=%d checksum=%llu\n", n, t1 - t0, t2 - t1, row == 0, (unsigned long long)sum);
    return 0;
}
