// postdet_check.cpp -- sdrreceiver_amd/csrc/sdrx_postdet.h as a stand-alone program (no GPU, no library): the argument check, the
// Kaiser design and the per-output arithmetic of the post-detection filter on records read from standard input as white-space
// separated words (floats as 8 hex digits of their bits, doubles as decimal or hexadecimal literals).
//
//   postdet_check --limits      prints  limits <max taps> <max decim>
//   postdet_check               reads records, one answer line each:
//       cfg DECIM NTAPS R0 R1                  (integers)                 answer:  ok   or  refused <why>
//       design FS CUTOFF NTAPS ATTEN           (doubles, NTAPS integer)   answer:  design <rc> <pass_hz> <stop_hz> <NTAPS tap bits>
//                                                                                  (doubles as %a; rc != 0: no taps)
//       fir T R H[T] HIST[T-1] N PRE[N]        (N % R == 0)               answer:  fir <N / R output bits> | <T - 1 new history bits>
// The history of the answer is the last T - 1 values of [HIST | PRE]: what the next frame's record is given.  The exit status is
// 0 when every record was well-formed, whatever the answers.  tests/test_host_postdet.py holds it to sdrreceiver_amd/postdet.py,
// under AddressSanitizer and UndefinedBehaviorSanitizer.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../sdrreceiver_amd/csrc/sdrx_postdet.h"

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
static bool read_floats(size_t n, std::vector<float> &v, size_t at)
{
    for (size_t i = 0; i < n; ++i)
        if (!read_float(&v[at + i]))
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
    if (argc > 1 && !strcmp(argv[1], "--limits")) {
        printf("limits %d %d\n", kPdMaxTaps, kPdMaxDecim);
        return 0;
    }
    char word[16];
    std::vector<float> h, ext;
    while (scanf("%15s", word) == 1) {
        if (!strcmp(word, "cfg")) {
            long long v[4];
            if (scanf("%lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3]) != 4) {
                fprintf(stderr, "postdet_check: malformed cfg record\n");
                return 2;
            }
            const PostCfg p = {(int32_t)v[0], (int32_t)v[1], {(int32_t)v[2], (int32_t)v[3]}};
            if (const char *why = postdet_args(p))
                printf("refused %s\n", why);
            else
                printf("ok\n");
        } else if (!strcmp(word, "design")) {
            double fs, cutoff, atten;
            long long N;
            if (scanf("%lf %lf %lld %lf", &fs, &cutoff, &N, &atten) != 4 || N < -1000 || N > 1000) {
                fprintf(stderr, "postdet_check: malformed design record\n");
                return 2;
            }
            float taps[kPdMaxTaps];
            double pass = 0, stop = 0;
            const int rc = postdet_design(fs, cutoff, (int)N, atten, taps, &pass, &stop);
            char head[128];
            snprintf(head, sizeof head, "design %d %a %a", rc, pass, stop);
            std::string out = head;
            for (long long k = 0; rc == 0 && k < N; ++k)
                put_bits(out, taps[k]);
            printf("%s\n", out.c_str());
        } else if (!strcmp(word, "fir")) {
            long long T = 0, R = 0, n = 0;
            if (scanf("%lld %lld", &T, &R) != 2 || T < 1 || T > kPdMaxTaps || R < 1 || R > kPdMaxDecim) {
                fprintf(stderr, "postdet_check: malformed fir record\n");
                return 2;
            }
            h.assign((size_t)T, 0.0f);
            ext.assign((size_t)T - 1, 0.0f);
            if (!read_floats((size_t)T, h, 0) || !read_floats((size_t)T - 1, ext, 0) || scanf("%lld", &n) != 1 || n < 1 || n >= (1 << 24) || n % R) {
                fprintf(stderr, "postdet_check: malformed fir record\n");
                return 2;
            }
            ext.resize((size_t)(T - 1 + n), 0.0f); // ext[T - 1 + i] = pre[i]
            if (!read_floats((size_t)n, ext, (size_t)T - 1)) {
                fprintf(stderr, "postdet_check: malformed fir record\n");
                return 2;
            }
            std::string out = "fir";
            for (long long m = 0; m < n / R; ++m)
                put_bits(out, postdet_fir(h.data(), (int)T, ext.data() + (T - 1) + m * R));
            out += " |";
            for (long long j = 0; j < T - 1; ++j)
                put_bits(out, ext[(size_t)(n + j)]);
            printf("%s\n", out.c_str());
        } else {
            fprintf(stderr, "postdet_check: unknown record '%s'\n", word);
            return 2;
        }
    }
    return 0;
}
