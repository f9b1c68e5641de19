// iq_check.cpp -- sdrreceiver_amd/csrc/sdrx_iqbal.h as a stand-alone program (no GPU, no library): the argument check, the
// quantiser and the step of the IQ balance correction on sums and settings read from standard input.
//
//   iq_check --geometry         prints  geometry <lane> <tile> <workgroup> <clamp>
//   iq_check                    reads records from standard input, one answer line each:
//       cfg MU MINPOWER C0 D0 FLAGS        (floats as strtof reads them: 0.25, 1e-3, inf, nan; FLAGS an unsigned integer)
//       pair C_BITS D_BITS                 (optional: the pair the frame used, 8 hex digits each; without it c0, d0)
//       n SAMPLES
//       sums S_I S_Q S_IQ S_II S_QQ        (decimal integers: the first three signed, the last two unsigned 64-bit)
//       end
//   answer:  ok <measured> <adapted> <rejected> <next_c bits, 8 hex digits> <next_d bits>
//        or  refused <why>                 (the settings are not offered, n outside 1 .. 2^31 - 1, sums no frame of n can have)
//       q X ...                            (any number of floats, or bits as 0xXXXXXXXX)  answer:  q <q(X)> ...
// The exit status is 0 when every record was well-formed, whatever the answers.  tests/test_host_iq.py holds it to
// sdrreceiver_amd/iqbal.py, under AddressSanitizer and UndefinedBehaviorSanitizer.
#include <cerrno>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../sdrreceiver_amd/csrc/sdrx_iqbal.h"

using namespace sdrx;

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--geometry")) {
        printf("geometry %d %d %d %d\n", kIqThread, 64 * kIqThread, kIqWg, kIqClamp);
        return 0;
    }
    float mu = 0, min_power = 0, c0 = 0, d0 = 0, c = 0, d = 0;
    unsigned long long flags = 0;
    long long n = -1;
    IqSums S{};
    bool have_cfg = false, have_pair = false, have_sums = false;
    static char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        char word[16] = "";
        if (sscanf(line, "%15s", word) != 1)
            continue;
        if (!strcmp(word, "cfg")) {
            char a[64], b[64], e[64], f[64];
            if (sscanf(line, "%*s %63s %63s %63s %63s %llu", a, b, e, f, &flags) != 5) {
                fprintf(stderr, "iq_check: malformed cfg line\n");
                return 2;
            }
            mu = strtof(a, nullptr), min_power = strtof(b, nullptr), c0 = strtof(e, nullptr), d0 = strtof(f, nullptr);
            have_cfg = true;
        } else if (!strcmp(word, "pair")) {
            unsigned cb = 0, db = 0;
            if (sscanf(line, "%*s %x %x", &cb, &db) != 2) {
                fprintf(stderr, "iq_check: malformed pair line\n");
                return 2;
            }
            c = iq_bits_float(cb), d = iq_bits_float(db);
            have_pair = true;
        } else if (!strcmp(word, "n")) {
            if (sscanf(line, "%*s %lld", &n) != 1) {
                fprintf(stderr, "iq_check: malformed n line\n");
                return 2;
            }
        } else if (!strcmp(word, "sums")) {
            long long a = 0, b = 0, e = 0;
            unsigned long long f = 0, g = 0;
            if (sscanf(line, "%*s %lld %lld %lld %llu %llu", &a, &b, &e, &f, &g) != 5) {
                fprintf(stderr, "iq_check: malformed sums line\n");
                return 2;
            }
            S.s_i = a, S.s_q = b, S.s_iq = e, S.s_ii = f, S.s_qq = g;
            have_sums = true;
        } else if (!strcmp(word, "q")) {
            std::string out = "q";
            char *p = line + 1, *end = nullptr;
            for (;;) {
                while (*p == ' ' || *p == '\t')
                    ++p;
                if (*p == '\n' || *p == '\0')
                    break;
                float x;
                if (p[0] == '0' && p[1] == 'x') {
                    x = iq_bits_float((uint32_t)strtoul(p, &end, 16));
                } else {
                    x = strtof(p, &end);
                }
                if (end == p) {
                    fprintf(stderr, "iq_check: malformed q line\n");
                    return 2;
                }
                p = end;
                out += " " + std::to_string(iq_q(x));
            }
            printf("%s\n", out.c_str());
        } else if (!strcmp(word, "end")) {
            const char *why = nullptr;
            const uint64_t lim = n > 0 ? (uint64_t)n * (uint64_t)kIqClamp : 0u, lim2 = lim * (uint64_t)kIqClamp;
            auto mag = [](int64_t v) { return v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v; };
            if (!have_cfg || !have_sums || n < 1 || n > 0x7fffffffLL)
                why = "no settings, no sums, or n outside 1 .. 2^31 - 1";
            else if (flags > 0xffffffffull)
                why = "flags is no 32-bit word";
            else if ((why = iq_args(mu, min_power, c0, d0, (uint32_t)flags, nullptr)))
                ;
            else if (have_pair && !iq_pair_ok(c, d))
                why = "the pair is none the stage can hold";
            else if (mag(S.s_i) > lim || mag(S.s_q) > lim || mag(S.s_iq) > lim2 || S.s_ii > lim2 || S.s_qq > lim2)
                why = "sums no frame of n samples can have";
            if (why) {
                printf("refused %s\n", why);
            } else {
                const IqStep r = iq_step(S, (uint32_t)n, mu, min_power, have_pair ? c : c0, have_pair ? d : d0);
                printf("ok %u %u %u %08" PRIx32 " %08" PRIx32 "\n", r.measured, r.adapted, r.rejected, iq_float_bits(r.c_next), iq_float_bits(r.d_next));
            }
            have_cfg = have_pair = have_sums = false, n = -1;
            S = IqSums{};
        } else {
            fprintf(stderr, "iq_check: unknown line '%s'\n", word);
            return 2;
        }
    }
    return 0;
}
