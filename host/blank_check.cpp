// blank_check.cpp -- sdrreceiver_amd/csrc/sdrx_blank.h as a stand-alone program (no GPU, no library): the argument check, the
// rank rule and the threshold of the impulse blanker on a histogram and settings read from standard input.
//
//   blank_check --geometry      prints  geometry <lane> <tile> <workgroup> <halo> <bins> <max_bin> <max_guard>
//   blank_check                 reads records from standard input, one answer line each:
//       cfg RATIO FLOOR RANK_Q16 GUARD     (floats as strtof reads them: 4, 1e-3, inf, nan)
//       n SAMPLES
//       bin B COUNT                        (any number of them; bins not named hold 0)
//       carry TAIL_GAP                     (optional: the carry the frame starts with)
//       end
//   answer:  ok <next_ref_bin> <thr_bits of a frame that uses it, 8 hex digits> <edge bits> <carry_in>
//        or  refused <why>                 (the settings are not offered, a bin or a count out of range, counts that do not sum to n)
// The exit status is 0 when every record was well-formed, whatever the answers.  tests/test_host_blank.py holds it to
// sdrreceiver_amd/blank.py, under AddressSanitizer and UndefinedBehaviorSanitizer.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../sdrreceiver_amd/csrc/sdrx_blank.h"

using namespace sdrx;

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--geometry")) {
        printf("geometry %d %d %d %d %d %d %d\n", kBlankThread, 64 * kBlankThread, kBlankWg, kBlankHalo, kBlankBins, kBlankMaxBin, kBlankMaxGuard);
        return 0;
    }
    std::vector<uint32_t> hist((size_t)kBlankBins, 0u);
    float ratio = 0, floor = 0;
    long long rank = 0, guard = 0, n = -1, tail_gap = kBlankNoHit;
    bool have_cfg = false;
    std::string bad;
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        char word[16] = "";
        if (sscanf(line, "%15s", word) != 1)
            continue;
        if (!strcmp(word, "cfg")) {
            char a[64], b[64];
            if (sscanf(line, "%*s %63s %63s %lld %lld", a, b, &rank, &guard) != 4) {
                fprintf(stderr, "blank_check: malformed cfg line\n");
                return 2;
            }
            ratio = strtof(a, nullptr), floor = strtof(b, nullptr);
            have_cfg = true;
        } else if (!strcmp(word, "n")) {
            if (sscanf(line, "%*s %lld", &n) != 1) {
                fprintf(stderr, "blank_check: malformed n line\n");
                return 2;
            }
        } else if (!strcmp(word, "carry")) {
            if (sscanf(line, "%*s %lld", &tail_gap) != 1) {
                fprintf(stderr, "blank_check: malformed carry line\n");
                return 2;
            }
        } else if (!strcmp(word, "bin")) {
            long long b = -1, count = -1;
            if (sscanf(line, "%*s %lld %lld", &b, &count) != 2) {
                fprintf(stderr, "blank_check: malformed bin line\n");
                return 2;
            }
            if (b < 0 || b >= kBlankBins || count < 0 || count > 0x7fffffffLL)
                bad = "a bin outside 0 .. 2047 or a count outside 0 .. 2^31 - 1";
            else
                hist[(size_t)b] = (uint32_t)count;
        } else if (!strcmp(word, "end")) {
            const char *why = nullptr;
            if (!have_cfg || n < 1 || n > 0x7fffffffLL)
                why = "no settings, or n outside 1 .. 2^31 - 1";
            else if (!bad.empty())
                why = bad.c_str();
            else if (rank < -0x7fffffffLL || rank > 0x7fffffffLL || guard < -0x7fffffffLL || guard > 0x7fffffffLL)
                why = "rank_q16 or guard is no 32-bit integer";
            else if (tail_gap < 0)
                why = "a negative carry";
            else
                why = blank_args(ratio, floor, (int)rank, (int)guard);
            if (!why) {
                uint64_t sum = 0;
                for (uint32_t c : hist)
                    sum += c;
                if (sum != (uint64_t)n)
                    why = "the counts do not sum to n";
            }
            if (why) {
                printf("refused %s\n", why);
            } else {
                const int next = blank_rank_bin(hist.data(), (uint32_t)n, (uint32_t)rank);
                const int gap = tail_gap < kBlankNoHit ? (int)tail_gap : kBlankNoHit;
                printf("ok %d %08" PRIx32 " %08" PRIx32 " %d\n", next, blank_float_bits(blank_threshold(next, ratio, floor)), blank_float_bits(blank_edge(next)),
                       blank_carry_in((int)n, (int)guard, gap));
            }
            std::fill(hist.begin(), hist.end(), 0u);
            have_cfg = false, n = -1, tail_gap = kBlankNoHit;
            bad.clear();
        } else {
            fprintf(stderr, "blank_check: unknown line '%s'\n", word);
            return 2;
        }
    }
    return 0;
}
