// host/adc_levels_check.cpp -- sdrx_host::adc_levels on a record read from standard input, for tests/test_adc_model.py: no GPU
// and no library needed (the function is arithmetic on the record alone).
//   in:  n_complex fmt  sum_i sum_sq_i min_i max_i at_lo_i at_hi_i run_i  (the same seven of q)  sum_iq  bits[0..16]
//   out: dc_i dc_q rms peak headroom_db clip_share longest_rail_run bits_used gain_imbalance phase_error, one line, %.17g
#include <cinttypes>
#include <cstdio>

#include "sdrx_host.hpp"

static bool read_arm(sdrx_adc_arm &a)
{
    return std::scanf("%" SCNd64 " %" SCNu64 " %" SCNd32 " %" SCNd32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &a.sum, &a.sum_sq, &a.min, &a.max, &a.at_lo, &a.at_hi,
                      &a.longest_rail_run) == 7;
}

int main()
{
    sdrx_adc_meter r;
    std::memset(&r, 0, sizeof r);
    r.measured = 1;
    bool ok = std::scanf("%" SCNu32 " %" SCNd32, &r.n_complex, &r.fmt) == 2 && read_arm(r.i) && read_arm(r.q) && std::scanf("%" SCNd64, &r.sum_iq) == 1;
    for (int k = 0; ok && k < 17; ++k)
        ok = std::scanf("%" SCNu32, &r.bits[k]) == 1;
    if (!ok) {
        std::fprintf(stderr, "adc_levels_check: malformed record\n");
        return 2;
    }
    const sdrx_host::adc_levels_t L = sdrx_host::adc_levels(r);
    std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %u %d %.17g %.17g\n", L.dc_i, L.dc_q, L.rms, L.peak, L.headroom_db, L.clip_share, L.longest_rail_run,
                L.bits_used, L.gain_imbalance, L.phase_error);
    return 0;
}
