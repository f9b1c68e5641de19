// detect_check.cpp -- sdrreceiver_amd/csrc/sdrx_detect.h as a stand-alone program (no GPU, no library): the argument check and the
// per-sample arithmetic of the detector leaves -- envelope, carrier sum, carrier, AM and FM pre-quantisation values, ANG -- on
// records read from standard input as white-space separated words (floats as 8 hex digits of their bits).
//
//   detect_check --geometry     prints  geometry <block> <threads>
//   detect_check                reads records, one answer line each:
//       cfg KIND R0 R1 R2            (integers)                            answer:  ok   or  refused <why>
//       ang Y X                      (two floats)                          answer:  ang <bits>
//       am GAIN N RE IM ...          (N samples, 1 <= N < 2^24)            answer:  am <S decimal> <carrier bits> <N pre bits>
//       fm GAIN PRE PIM N RE IM ...  ((PRE, PIM) = z[-1])                  answer:  fm <N pre bits>
// The exit status is 0 when every record was well-formed, whatever the answers.  tests/test_host_detect.py holds it to
// sdrreceiver_amd/detect.py, under AddressSanitizer and UndefinedBehaviorSanitizer.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../sdrreceiver_amd/csrc/sdrx_detect.h"

using namespace sdrx;

static uint32_t bits_of(float x)
{
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    return u;
}
static float float_of(uint32_t u)
{
    float x;
    memcpy(&x, &u, sizeof x);
    return x;
}
static bool read_float(float *out)
{
    unsigned u = 0;
    if (scanf("%x", &u) != 1)
        return false;
    *out = float_of((uint32_t)u);
    return true;
}
static bool read_samples(long long n, std::vector<float> &z)
{
    z.resize(2 * (size_t)n);
    for (float &v : z)
        if (!read_float(&v))
            return false;
    return true;
}
static void put_bits(std::string &out, float v)
{
    char word[16];
    snprintf(word, sizeof word, " %08" PRIx32, bits_of(v));
    out += word;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--geometry")) {
        printf("geometry %d %d\n", kDetBlock, kDetThreads);
        return 0;
    }
    char word[16];
    std::vector<float> z;
    while (scanf("%15s", word) == 1) {
        if (!strcmp(word, "cfg")) {
            long long v[4];
            if (scanf("%lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3]) != 4) {
                fprintf(stderr, "detect_check: malformed cfg record\n");
                return 2;
            }
            const DetectCfg d = {(int32_t)v[0], {(int32_t)v[1], (int32_t)v[2], (int32_t)v[3]}};
            if (const char *why = detect_args(d))
                printf("refused %s\n", why);
            else
                printf("ok\n");
        } else if (!strcmp(word, "ang")) {
            float y, x;
            if (!read_float(&y) || !read_float(&x)) {
                fprintf(stderr, "detect_check: malformed ang record\n");
                return 2;
            }
            printf("ang %08" PRIx32 "\n", bits_of(detect_ang(y, x)));
        } else if (!strcmp(word, "am")) {
            float gain;
            long long n = 0;
            if (!read_float(&gain) || scanf("%lld", &n) != 1 || n < 1 || n >= (1 << 24) || !read_samples(n, z)) {
                fprintf(stderr, "detect_check: malformed am record\n");
                return 2;
            }
            uint64_t S = 0;
            for (long long i = 0; i < n; ++i)
                S += detect_env_q(detect_env(z[2 * (size_t)i], z[2 * (size_t)i + 1]));
            const float c = detect_carrier(S, (int)n);
            std::string out = "am " + std::to_string((unsigned long long)S);
            put_bits(out, c);
            for (long long i = 0; i < n; ++i)
                put_bits(out, detect_am_pre(detect_env(z[2 * (size_t)i], z[2 * (size_t)i + 1]), c, gain));
            printf("%s\n", out.c_str());
        } else if (!strcmp(word, "fm")) {
            float gain, p, q;
            long long n = 0;
            if (!read_float(&gain) || !read_float(&p) || !read_float(&q) || scanf("%lld", &n) != 1 || n < 1 || n >= (1 << 24) || !read_samples(n, z)) {
                fprintf(stderr, "detect_check: malformed fm record\n");
                return 2;
            }
            std::string out = "fm";
            for (long long i = 0; i < n; ++i) {
                const float a = z[2 * (size_t)i], b = z[2 * (size_t)i + 1];
                put_bits(out, detect_fm_pre(a, b, p, q, gain));
                p = a, q = b;
            }
            printf("%s\n", out.c_str());
        } else {
            fprintf(stderr, "detect_check: unknown record '%s'\n", word);
            return 2;
        }
    }
    return 0;
}
