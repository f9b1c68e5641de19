// front_check.cpp -- sdrreceiver_amd/csrc/sdrx_front.h at real sizes, as a stand-alone program (no GPU, no library): the frame
// lengths per stage, every tile's window inside [-(N-1), n_in_stage), every output's reads inside its tile's window and the LDS
// slots the kernel computes for them inside the two halves it stages, for 5 000 000 real samples through 1, 2 and 3 stages,
// 2 500 000 complex samples, and frames with a short last tile; the rules of sdrx_set_front and the built-in design.  Built with
// -fsanitize=address,undefined by tests/test_host_front.py; prints "front_check ok" or the first thing wrong.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sdrreceiver_amd/csrc/sdrx_front.h"

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
    int real, stages, K, in_frame, n0;
};

// one stage of n_out outputs: windows and reads, tile by tile; the staged halves as vectors, so that a slot outside them is the
// sanitizer's to find
static void check_stage(const Case &c, int s, long long n_out)
{
    const int N = front_taps(c.K), C = front_centre(c.K);
    const long long n_in = 2 * n_out;
    long long prev_hi = -1, longest = 0;
    for (int t = 0; (long long)t * kFrTile < n_out; ++t) {
        long long lo, hi;
        front_window(t, n_out, N, lo, hi);
        CHECK(lo >= -(N - 1) && hi < n_in && lo <= hi && hi > prev_hi, "K %d stage %d tile %d: window [%lld, %lld] of %lld", c.K, s, t, lo, hi, n_in);
        prev_hi = hi;
        const long long W = hi - lo + 1;
        longest = W > longest ? W : longest;
        CHECK(W <= kFrMaxWindow, "K %d stage %d tile %d: window of %lld", c.K, s, t, W);
        if (W > kFrMaxWindow)
            return;
        std::vector<long long> even((size_t)((W + 1) / 2)), odd((size_t)(W / 2)); // the absolute index each slot holds
        for (long long w = 0; w < W; ++w)
            ((w & 1) ? odd : even)[(size_t)(w >> 1)] = lo + w;
        CHECK((long long)even.size() <= kFrWinHalf && (long long)odd.size() <= kFrWinHalf, "K %d: halves of %zu and %zu", c.K, even.size(), odd.size());
        const long long m0 = (long long)t * kFrTile, count = n_out - m0 < kFrTile ? n_out - m0 : kFrTile;
        CHECK(count % 16 == 0 || n_out % 16 != 0, "K %d stage %d tile %d: %lld outputs", c.K, s, t, count);
        for (long long j = 0; j < count; ++j) {
            const long long m = m0 + j;
            bool ok = 2 * m - (N - 1) >= lo && 2 * m <= hi;
            for (int i = 0; ok && i <= 2 * c.K + 1; ++i) // the even taps k = 2 i
                ok = even.at((size_t)front_even_slot((int)j, i, c.K)) == 2 * m - 2 * i;
            ok = ok && odd.at((size_t)front_odd_slot((int)j, c.K)) == 2 * m - C;
            if (!ok) {
                CHECK(false, "K %d stage %d output %lld: reads outside [%lld, %lld] or a wrong slot", c.K, s, m, lo, hi);
                return;
            }
        }
        // a real stage relies on lo = 2 (mod 4): the sign pattern of (-j)^n by the slot's parity
        CHECK(((lo % 4) + 4) % 4 == 2, "K %d tile %d: lo %lld", c.K, t, lo);
    }
    CHECK(longest == (n_out >= kFrTile ? 2LL * kFrTile + N - 2 : 2 * n_out + N - 2), "K %d stage %d: longest window %lld", c.K, s, longest);
}

int main()
{
    const Case cases[] = {
        {1, 1, 15, 5000000, 2500000}, {1, 2, 15, 5000000, 1250000}, {1, 3, 15, 5000000, 625000}, {0, 1, 15, 2500000, 1250000},
        {1, 1, 31, 5000000, 2500000}, {0, 3, 2, 2560000, 320000},
        // the shapes of the device tests: a short last tile of 272, the longest history, in front of the resampler
        {1, 1, 2, 2592, 1296}, {1, 1, 31, 4096, 2048}, {0, 1, 7, 2560, 1280}, {0, 2, 3, 8192, 2048}, {1, 3, 7, 16384, 2048}, {1, 1, 7, 6400, 3200},
        {0, 1, 31, 2 * 1040, 1040}, {1, 2, 31, 4 * 272, 272},
    };
    for (const Case &c : cases) {
        FrontPlan P;
        CHECK(!front_args(c.real, c.stages, c.K), "%d %d %d refused", c.real, c.stages, c.K);
        P.real = c.real, P.stages = c.stages, P.K = c.K;
        const char *why = front_frames(P, c.n0);
        if (c.n0 % 16) { // 5 000 000 samples through three stages leave 625 000: no frame the library takes (the kernels behind mask
                         // whole lanes of 16 samples), but the windows and reads are checked at this size all the same
            CHECK(why && strstr(why, "multiple of 16"), "n0 %d: %s", c.n0, why ? why : "accepted");
            P.n0 = c.n0, P.in_frame = c.in_frame;
        } else {
            CHECK(!why, "n0 %d: %s", c.n0, why ? why : "");
        }
        CHECK(P.in_frame == c.in_frame && P.in_frame % 4 == 0, "n0 %d stages %d: in_frame %d", c.n0, c.stages, P.in_frame);
        CHECK(front_stage_in(P, 1) == c.in_frame && front_stage_out(P, c.stages) == c.n0, "n0 %d: stage lengths", c.n0);
        for (int s = 1; s <= c.stages; ++s) {
            CHECK(front_stage_in(P, s) == 2 * front_stage_out(P, s) && (s == 1 || front_stage_in(P, s) == front_stage_out(P, s - 1)), "stage %d", s);
            check_stage(c, s, front_stage_out(P, s));
        }
    }
    { // the rules
        CHECK(front_args(2, 1, 7) && front_args(-1, 1, 7) && front_args(0, 0, 7) && front_args(0, 4, 7) && front_args(0, 1, 1) && front_args(0, 1, 32),
              "a bad argument accepted");
        FrontPlan P;
        P.stages = 3, P.K = 7;
        CHECK(front_frames(P, 1000) != nullptr && front_frames(P, 0) != nullptr, "a frame that is no multiple of 16 accepted");
        CHECK(front_frames(P, 268435456) != nullptr, "2^31 samples accepted");
        P.K = 31;
        CHECK(front_frames(P, 48) != nullptr && front_frames(P, 64) == nullptr, "history rule");
    }
    { // the design: unit DC gain, symmetric, the zeros exact, the centre 0.5; the refusals
        for (int K = 3; K <= 31; ++K) {
            std::vector<float> h((size_t)front_taps(K));
            double tw = 0;
            CHECK(front_design(K, 80.0, h.data(), &tw) == 0 && tw > 0 && tw < 0.5, "K %d: design", K);
            double sum = 0;
            bool sym = true;
            for (size_t k = 0; k < h.size(); ++k) {
                sum += h[k];
                sym = sym && h[k] == h[h.size() - 1 - k];
            }
            CHECK(sym && sum > 0.999 && sum < 1.001 && h[(size_t)front_centre(K)] == 0.5f && front_bad_tap(h.data(), K) == -1, "K %d: taps sum %g", K, sum);
            h[1] = -0.0f;
            CHECK(front_bad_tap(h.data(), K) == 1, "K %d: a negative zero accepted", K);
        }
        CHECK(front_design(2, 80.0, nullptr, nullptr) == 2 && front_design(2, 60.0, nullptr, nullptr) == 0, "K = 2");
        CHECK(front_design(7, 50.0, nullptr, nullptr) == 1 && front_design(7, 120.5, nullptr, nullptr) == 1 && front_design(7, 120.0, nullptr, nullptr) == 0,
              "atten_db rule");
    }
    if (g_bad)
        return 1;
    printf("front_check ok\n");
    return 0;
}
