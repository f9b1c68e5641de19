// resample_check.cpp -- sdrreceiver_amd/csrc/sdrx_resample.h at real rates, as a stand-alone program (no GPU, no library): the
// ratios and frame lengths of the front ends DESIGN.md 4s names, the refusal of a frame that is no multiple of 16 and the pair
// resample_nearest_frames offers instead, positions past 2^31, and every chunk's window inside [-(T-1), n_in).  Built with
// -fsanitize=address,undefined by tests/test_host_resample.py; prints "resample_check ok" or the first thing wrong.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sdrreceiver_amd/csrc/sdrx_resample.h"

using namespace sdrx;

static int g_bad = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            printf("FAILED %s: ", #cond);    \
            printf(__VA_ARGS__);             \
            printf("\n");                    \
            ++g_bad;                         \
        }                                    \
    } while (0)

struct Case {
    int fs_in, fs_out, T, L, M, n_in, n_out; // at 0.25 s
};

int main()
{
    const Case cases[] = {
        {6000000, 6144000, 32, 128, 125, 1500000, 1536000},
        {10000000, 6144000, 32, 384, 625, 2500000, 1536000},
        {3000000, 1536000, 32, 64, 125, 750000, 384000},
        {2400000, 1536000, 24, 16, 25, 600000, 384000},
        {2048000, 1536000, 16, 3, 4, 512000, 384000},
    };
    for (const Case &c : cases) {
        ResamplePlan P;
        const char *why = resample_ratio(c.fs_in, c.fs_out, c.T, P);
        CHECK(!why, "%d -> %d: %s", c.fs_in, c.fs_out, why ? why : "");
        CHECK(P.L == c.L && P.M == c.M, "%d -> %d: L %d M %d", c.fs_in, c.fs_out, P.L, P.M);
        why = resample_frames(P, c.fs_out / 4);
        CHECK(!why, "%d -> %d frames: %s", c.fs_in, c.fs_out, why ? why : "");
        CHECK(P.n_in == c.n_in && P.n_out == c.n_out, "%d -> %d: frames %d -> %d", c.fs_in, c.fs_out, P.n_in, P.n_out);
        int a = 0, b = 0;
        CHECK(resample_nearest_frames(P, 0.25, 16, a, b) && a == c.n_in && b == c.n_out, "%d -> %d: nearest %d -> %d", c.fs_in, c.fs_out, a, b);
        // every chunk's window inside [-(T-1), n_in), windows in ascending order, the longest what resample_max_window says;
        // and output by output: the reads i - (T-1) .. i lie inside the window of the output's chunk
        long long longest = 0, prev_lo = -(1LL << 62);
        for (int ch = 0; (long long)ch * kRsChunk < P.n_out; ++ch) {
            long long lo, hi;
            resample_window(ch, P.n_out, P.M, P.L, P.T, lo, hi);
            CHECK(lo >= -(P.T - 1) && hi < P.n_in && lo <= hi && lo >= prev_lo, "%d -> %d chunk %d: window [%lld, %lld]", c.fs_in, c.fs_out, ch, lo, hi);
            prev_lo = lo;
            longest = hi - lo + 1 > longest ? hi - lo + 1 : longest;
            const long long m0 = (long long)ch * kRsChunk, m1 = m0 + kRsChunk < P.n_out ? m0 + kRsChunk : P.n_out;
            for (long long m = m0; m < m1; ++m) {
                long long i;
                int ph;
                resample_pos(m, P.M, P.L, i, ph);
                if (!(i - (P.T - 1) >= lo && i <= hi && ph >= 0 && ph < P.L && i * P.L + ph == m * P.M)) {
                    CHECK(false, "%d -> %d output %lld: i %lld ph %d outside [%lld, %lld]", c.fs_in, c.fs_out, m, i, ph, lo, hi);
                    break;
                }
            }
        }
        CHECK(longest == resample_max_window(P) && longest <= 4LL * (kRsChunk - 1) + 1 + P.T, "%d -> %d: longest window %lld", c.fs_in, c.fs_out, longest);
        // the design: finite taps that sum to L per phase set (a DC gain of L over the prototype), symmetric
        std::vector<float> h((size_t)P.L * P.T);
        double pass = 0;
        CHECK(resample_design(P, 80.0, h.data(), &pass) == 0 && pass > 0, "%d -> %d: design", c.fs_in, c.fs_out);
        double sum = 0;
        bool sym = true;
        for (size_t k = 0; k < h.size(); ++k) {
            sum += h[k];
            sym = sym && h[k] == h[h.size() - 1 - k];
        }
        CHECK(sym && sum > 0.999 * P.L && sum < 1.001 * P.L, "%d -> %d: taps sum %g", c.fs_in, c.fs_out, sum);
    }
    { // 2.5 -> 1.536 MS/s: 384 000 outputs need 625 000 inputs, no multiple of 16; the nearest valid pair with whole tiles
        ResamplePlan P;
        CHECK(!resample_ratio(2500000, 1536000, 32, P) && P.L == 384 && P.M == 625, "2.5 -> 1.536: L %d M %d", P.L, P.M);
        const char *why = resample_frames(P, 384000);
        CHECK(why && strstr(why, "multiple of 16"), "2.5 -> 1.536 with 384000: %s", why ? why : "accepted");
        int a = 0, b = 0;
        CHECK(resample_nearest_frames(P, 0.25, 1024, a, b) && a == 620000 && b == 380928, "2.5 -> 1.536: nearest %d -> %d", a, b);
        CHECK(!resample_frames(P, b) && P.n_in == a, "2.5 -> 1.536: the offered pair is refused");
    }
    { // positions are 64-bit: 6 143 999 * 625 = 3 839 999 375 > 2^32 - 1... > 2^31
        long long i;
        int ph;
        resample_pos(6143999, 625, 384, i, ph);
        CHECK(i == 9999998 && ph == 143, "m = 6143999: i %lld ph %d", i, ph);
        CHECK(i * 384 + ph == 3839999375LL, "m = 6143999: p %lld", i * 384 + ph);
    }
    { // the rules
        ResamplePlan P;
        CHECK(resample_ratio(625000, 96000, 32, P) != nullptr, "96/625 accepted");  // M / L = 6.5
        CHECK(resample_ratio(1000, 2001, 32, P) != nullptr, "L = 2001 accepted");
        CHECK(resample_ratio(3000, 4000, 12, P) == nullptr && resample_ratio(3000, 4000, 10, P) != nullptr, "T rule");
        CHECK(resample_ratio(1023000, 1024000, 64, P) != nullptr, "L T = 65536 accepted");
        CHECK(!resample_ratio(3000, 5000, 8, P) && resample_design(P, 80.0, nullptr, nullptr) == 2, "5/3 with T = 8 designed");
        CHECK(!resample_ratio(4000, 3000, 16, P) && resample_design(P, 50.0, nullptr, nullptr) == 1 && resample_design(P, 120.5, nullptr, nullptr) == 1,
              "atten_db rule");
    }
    if (g_bad)
        return 1;
    printf("resample_check ok\n");
    return 0;
}
