// shift_check.cpp -- sdrreceiver_amd/csrc/sdrx_shift.h as a stand-alone program (no GPU, no library): the tables, the Hz <->
// increment conversion, the argument check, the per-sample index split, the rotation and the frame advance of the frequency
// shift, on records read from standard input.
//
//   shift_check --geometry      prints  geometry <lane> <tile> <workgroup> <table entries>
//   shift_check --tables        prints  tables <3 * 256 * 2 floats as 8 hex digits each: A | B | C, (re, im) interleaved>
//   shift_check                 reads records from standard input, one answer line each:
//       inc FS HZ                    (doubles as strtod reads them)       answer:  inc <8 hex digits>   or  refused
//       hz FS INC                    (INC: 8 hex digits)                  answer:  hz <the double, %.17g>
//       cfg FLAGS R0 R1 R2 R3 R4     (unsigned integers)                  answer:  ok   or  refused <why>
//       frame PHASE INC N J ...      (PHASE, INC hex; N decimal, 1 .. 2^31 - 1; any number of sample indices J < N)
//                                    answer:  frame <next phase, hex> then for every J:  <p hex> <h> <m> <l> <rot re bits> <rot im bits>
//       mix RE IM P                  (a sample's bits and a phase, hex)   answer:  mix <y re bits> <y im bits>
// The exit status is 0 when every record was well-formed, whatever the answers.  tests/test_host_shift.py holds it to
// sdrreceiver_amd/shift.py, under AddressSanitizer and UndefinedBehaviorSanitizer.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../sdrreceiver_amd/csrc/sdrx_shift.h"

using namespace sdrx;

int main(int argc, char **argv)
{
    std::vector<float> tab(3 * kShTab * 2);
    shift_tables(tab.data());
    if (argc > 1 && !strcmp(argv[1], "--geometry")) {
        printf("geometry %d %d %d %d\n", kShThread, 64 * kShThread, kShWg, kShTab);
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "--tables")) {
        std::string out = "tables";
        char word[16];
        for (float v : tab) {
            snprintf(word, sizeof word, " %08" PRIx32, shift_float_bits(v));
            out += word;
        }
        printf("%s\n", out.c_str());
        return 0;
    }
    std::vector<ShiftC> entries(3 * kShTab);
    for (int k = 0; k < 3 * kShTab; ++k)
        entries[(size_t)k] = ShiftC{tab[2 * (size_t)k], tab[2 * (size_t)k + 1]};
    const ShiftC *A = entries.data(), *B = A + kShTab, *C = A + 2 * kShTab;
    static char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        char word[16] = "";
        if (sscanf(line, "%15s", word) != 1)
            continue;
        if (!strcmp(word, "inc")) {
            char a[64], b[64];
            if (sscanf(line, "%*s %63s %63s", a, b) != 2) {
                fprintf(stderr, "shift_check: malformed inc line\n");
                return 2;
            }
            uint32_t inc = 0;
            if (shift_inc(strtod(a, nullptr), strtod(b, nullptr), &inc))
                printf("inc %08" PRIx32 "\n", inc);
            else
                printf("refused\n");
        } else if (!strcmp(word, "hz")) {
            char a[64];
            unsigned inc = 0;
            if (sscanf(line, "%*s %63s %x", a, &inc) != 2) {
                fprintf(stderr, "shift_check: malformed hz line\n");
                return 2;
            }
            printf("hz %.17g\n", shift_hz(strtod(a, nullptr), (uint32_t)inc));
        } else if (!strcmp(word, "cfg")) {
            unsigned long long v[6];
            if (sscanf(line, "%*s %llu %llu %llu %llu %llu %llu", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) != 6) {
                fprintf(stderr, "shift_check: malformed cfg line\n");
                return 2;
            }
            const uint32_t reserved[5] = {(uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5]};
            const char *why = v[0] > 0xffffffffull ? "flags is no 32-bit word" : shift_args((uint32_t)v[0], reserved);
            if (why)
                printf("refused %s\n", why);
            else
                printf("ok\n");
        } else if (!strcmp(word, "frame")) {
            unsigned phase = 0, inc = 0;
            long long n = 0;
            int used = 0;
            if (sscanf(line, "%*s %x %x %lld%n", &phase, &inc, &n, &used) != 3 || n < 1 || n > 0x7fffffffLL) {
                fprintf(stderr, "shift_check: malformed frame line\n");
                return 2;
            }
            std::string out;
            char buf[96];
            snprintf(buf, sizeof buf, "frame %08" PRIx32, shift_advance((uint32_t)phase, (uint32_t)n, (uint32_t)inc));
            out = buf;
            char *p = line + used, *end = nullptr;
            for (;;) {
                while (*p == ' ' || *p == '\t')
                    ++p;
                if (*p == '\n' || *p == '\0')
                    break;
                const long long j = strtoll(p, &end, 10);
                if (end == p || j < 0 || j >= n) {
                    fprintf(stderr, "shift_check: malformed sample index\n");
                    return 2;
                }
                p = end;
                const uint32_t ph = shift_advance((uint32_t)phase, (uint32_t)j, (uint32_t)inc);
                int h, m, l;
                shift_split(ph, h, m, l);
                const ShiftC r = shift_rot(A, B, C, ph);
                snprintf(buf, sizeof buf, " %08" PRIx32 " %d %d %d %08" PRIx32 " %08" PRIx32, ph, h, m, l, shift_float_bits(r.re), shift_float_bits(r.im));
                out += buf;
            }
            printf("%s\n", out.c_str());
        } else if (!strcmp(word, "mix")) {
            unsigned re = 0, im = 0, ph = 0;
            if (sscanf(line, "%*s %x %x %x", &re, &im, &ph) != 3) {
                fprintf(stderr, "shift_check: malformed mix line\n");
                return 2;
            }
            const ShiftC y = shift_apply(ShiftC{shift_bits_float(re), shift_bits_float(im)}, shift_rot(A, B, C, (uint32_t)ph));
            printf("mix %08" PRIx32 " %08" PRIx32 "\n", shift_float_bits(y.re), shift_float_bits(y.im));
        } else {
            fprintf(stderr, "shift_check: unknown line '%s'\n", word);
            return 2;
        }
    }
    return 0;
}
