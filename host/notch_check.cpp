// notch_check.cpp -- sdrreceiver_amd/csrc/sdrx_notch.h as a stand-alone program (no GPU, no library): the geometry, the argument
// check with the spacing rule, the restart rule of a live change, the order of the block correlation's sums and the step rule of a
// tone over a frame's blocks, on records read from standard input.  Floats travel as 8 hex digits, doubles as 16.
//
//   notch_check --geometry      prints  geometry <lane> <tile> <block> <slots> <spacing> <rad-to-inc, %.17g>
//   notch_check                 reads records from standard input, one answer line each:
//       cfg N FLAGS PULL R0 MU AFC COH R1 INC0 x 8 R x 8      (MU, AFC, COH: float bits, hex; the rest unsigned decimal)
//                                    answer:  ok   or  refused <why>
//       restart NB FLAGSB INC0 x 8 NA FLAGSA INC0 x 8          (the settings before and after a live change)
//                                    answer:  restart <mask, decimal>
//       lanes V x 256                (one component's lane sums of a block)            answer:  lanes <the block's sum>
//       corr P0 INC LEN RE IM ...    (P0, INC hex; LEN samples, 1 .. 4096)             answer:  corr <c re> <c im>
//       step N MU AFC COH PULL PHASE INC INC0 ARE AIM  CRE CIM ...   (N decimal, PULL decimal, PHASE INC INC0 hex; one c per block)
//                                    answer:  step <phase> <inc> <a re> <a im> <phase_used> <inc_used> | <inc> <inc_next> <a re> <a im>
//                                             <coherent> <adapted> <clamped> <rejected> <S_re> <S_im> <P> <E> | <used re> <used im> ...
//       sub YRE YIM URE UIM P        (a sample, an amplitude, a phase: hex)            answer:  sub <y re> <y im>
// The exit status is 0 when every record was well-formed, whatever the answers.  tests/test_host_notch.py holds it to
// sdrreceiver_amd/notch.py, under AddressSanitizer and UndefinedBehaviorSanitizer.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../sdrreceiver_amd/csrc/sdrx_notch.h"

using namespace sdrx;

static uint64_t double_bits(double x)
{
    uint64_t u;
    memcpy(&u, &x, sizeof u);
    return u;
}

static bool hex32(std::istringstream &in, uint32_t &v)
{
    std::string w;
    if (!(in >> w) || w.empty() || w.size() > 8 || w.find_first_not_of("0123456789abcdefABCDEF") != std::string::npos)
        return false;
    v = (uint32_t)strtoul(w.c_str(), nullptr, 16);
    return true;
}

static bool dec32(std::istringstream &in, uint32_t &v)
{
    unsigned long long w = 0;
    if (!(in >> w) || w > 0xffffffffull)
        return false;
    v = (uint32_t)w;
    return true;
}

static int malformed(const char *what)
{
    fprintf(stderr, "notch_check: malformed %s line\n", what);
    return 2;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--geometry")) {
        printf("geometry %d %d %d %d %" PRIu32 " %.17g\n", kNtLane, 64 * kNtLane, kNtBlock, kNtMax, kNtSpacing, kNtRadToInc);
        return 0;
    }
    std::vector<float> tab(3 * kShTab * 2);
    shift_tables(tab.data());
    std::vector<ShiftC> entries(3 * kShTab);
    for (int k = 0; k < 3 * kShTab; ++k)
        entries[(size_t)k] = ShiftC{tab[2 * (size_t)k], tab[2 * (size_t)k + 1]};
    const ShiftC *A = entries.data(), *B = A + kShTab, *C = A + 2 * kShTab;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string word;
        if (!(in >> word))
            continue;
        if (word == "cfg") {
            NotchCfg c;
            uint32_t mu = 0, afc = 0, coh = 0;
            bool ok = dec32(in, c.n_tones) && dec32(in, c.flags) && dec32(in, c.max_pull) && dec32(in, c.reserved0) && hex32(in, mu) && hex32(in, afc) &&
                      hex32(in, coh) && dec32(in, c.reserved1);
            for (int k = 0; ok && k < kNtMax; ++k)
                ok = dec32(in, c.inc0[k]);
            for (int k = 0; ok && k < 8; ++k)
                ok = dec32(in, c.reserved[k]);
            if (!ok)
                return malformed("cfg");
            c.mu = shift_bits_float(mu), c.afc_gain = shift_bits_float(afc), c.min_coherence = shift_bits_float(coh);
            const char *why = notch_args(c);
            if (why)
                printf("refused %s\n", why);
            else
                printf("ok\n");
        } else if (word == "restart") {
            NotchCfg c[2];
            memset(c, 0, sizeof c);
            bool ok = true;
            for (int s = 0; ok && s < 2; ++s) {
                ok = dec32(in, c[s].n_tones) && dec32(in, c[s].flags) && c[s].n_tones <= (uint32_t)kNtMax;
                for (int k = 0; ok && k < kNtMax; ++k)
                    ok = dec32(in, c[s].inc0[k]);
            }
            if (!ok)
                return malformed("restart");
            printf("restart %" PRIu32 "\n", notch_restart_mask(c[0], c[1]));
        } else if (word == "lanes") {
            float v[4][64];
            for (int w = 0; w < 4; ++w)
                for (int l = 0; l < 64; ++l) {
                    uint32_t u = 0;
                    if (!hex32(in, u))
                        return malformed("lanes");
                    v[w][l] = shift_bits_float(u);
                }
            const float s = notch_wg_sum(notch_wave_sum(v[0]), notch_wave_sum(v[1]), notch_wave_sum(v[2]), notch_wave_sum(v[3]));
            printf("lanes %08" PRIx32 "\n", shift_float_bits(s));
        } else if (word == "corr") {
            uint32_t p0 = 0, inc = 0, len = 0;
            if (!hex32(in, p0) || !hex32(in, inc) || !dec32(in, len) || len < 1 || len > (uint32_t)kNtBlock)
                return malformed("corr");
            std::vector<ShiftC> x(len);
            for (ShiftC &s : x) {
                uint32_t re = 0, im = 0;
                if (!hex32(in, re) || !hex32(in, im))
                    return malformed("corr");
                s = ShiftC{shift_bits_float(re), shift_bits_float(im)};
            }
            const ShiftC c = notch_block_corr(x.data(), (int)len, A, B, C, p0, inc);
            printf("corr %08" PRIx32 " %08" PRIx32 "\n", shift_float_bits(c.re), shift_float_bits(c.im));
        } else if (word == "step") {
            uint32_t n = 0, mu = 0, afc = 0, coh = 0, pull = 0, are = 0, aim = 0;
            NotchTone T;
            memset(&T, 0, sizeof T);
            if (!dec32(in, n) || !hex32(in, mu) || !hex32(in, afc) || !hex32(in, coh) || !dec32(in, pull) || !hex32(in, T.phase) || !hex32(in, T.inc) ||
                !hex32(in, T.inc0) || !hex32(in, are) || !hex32(in, aim) || n < 1 || n > 0x7fffffffu)
                return malformed("step");
            T.a_re = shift_bits_float(are), T.a_im = shift_bits_float(aim);
            const int nb = notch_blocks((int)n);
            std::vector<ShiftC> c((size_t)nb * kNtMax, ShiftC{0.0f, 0.0f}), used((size_t)nb * kNtMax, ShiftC{0.0f, 0.0f});
            for (int b = 0; b < nb; ++b) {
                uint32_t re = 0, im = 0;
                if (!hex32(in, re) || !hex32(in, im))
                    return malformed("step");
                c[(size_t)b * kNtMax] = ShiftC{shift_bits_float(re), shift_bits_float(im)};
            }
            NotchToneRecord R;
            notch_step_tone(c.data(), used.data(), (int)n, T, shift_bits_float(mu), shift_bits_float(afc), shift_bits_float(coh), pull, R);
            printf("step %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " |", T.phase, T.inc, shift_float_bits(T.a_re),
                   shift_float_bits(T.a_im), T.phase_used, T.inc_used);
            printf(" %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64
                   " %016" PRIx64 " |",
                   R.inc, R.inc_next, R.a_re_bits, R.a_im_bits, R.coherent, R.adapted, R.clamped, R.rejected, double_bits(R.s_re), double_bits(R.s_im),
                   double_bits(R.p), double_bits(R.e));
            for (int b = 0; b < nb; ++b)
                printf(" %08" PRIx32 " %08" PRIx32, shift_float_bits(used[(size_t)b * kNtMax].re), shift_float_bits(used[(size_t)b * kNtMax].im));
            printf("\n");
        } else if (word == "sub") {
            uint32_t v[5];
            for (uint32_t &u : v)
                if (!hex32(in, u))
                    return malformed("sub");
            const ShiftC y = notch_canonical(notch_subtract(ShiftC{shift_bits_float(v[0]), shift_bits_float(v[1])}, ShiftC{shift_bits_float(v[2]), shift_bits_float(v[3])},
                                                            shift_rot(A, B, C, v[4])));
            printf("sub %08" PRIx32 " %08" PRIx32 "\n", shift_float_bits(y.re), shift_float_bits(y.im));
        } else {
            fprintf(stderr, "notch_check: unknown line '%s'\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
