// compress.hip -- vfo::compress (vfo.cpp:389-424) as k_compress: the int8 payload of a VFO's stream.
// Relies on dev_helpers.hip (ldc, gld2) and meter.hip (to_schar, meter_iq, meter_block_store).

// ------------------------------------------------------------------------------------ k_compress
// vfo::compress (vfo.cpp:389-424): cstyle 1 packs the high nibbles of (re/scalecomp)*128 and
// (im/scalecomp)*128 into one byte; otherwise two int8 per sample.
template <bool METER = false, bool PARK = false>
__global__ __launch_bounds__(256) void k_compress(const K3Vfo *__restrict__ vfos, const BlockWork *__restrict__ work,
                                                  unsigned long long frame_no, ParkArg<PARK> P)
{
    const BlockWork bw = work[blockIdx.x];
    if constexpr (PARK)
        if (ldc(P.act + bw.vfo) == 0)
            return;
    const K3Vfo *Dp = vfos + bw.vfo;
    const int blk = bw.blk;
    const int par = (int)(frame_no & 1ull);
    struct {
        signed char *pay;
        int n, cstyle, scalecomp;
    } D = {Dp->pay[par], Dp->n, Dp->cstyle, Dp->scalecomp};
    const float2 *z = Dp->s[par];
    MeterAcc macc = meter_zero();
    for (int i = blk * 4096 + threadIdx.x; i < min(D.n, (blk + 1) * 4096); i += 256) {
        const float2 v = gld2(z + i);
        if (D.cstyle == 1) {
            const float sc = (float)D.scalecomp;
            const float pre_re = (v.x / sc) * 128.0f, pre_im = (v.y / sc) * 128.0f;
            const int re = to_schar(pre_re);
            const int im = to_schar(pre_im);
            D.pay[i] = (signed char)((re & 0xF0) | ((im & 0xF0) >> 4));
            if constexpr (METER)
                meter_iq(macc, pre_re, pre_im, re, im);
        } else {
            const float pre_re = v.x * 128.0f, pre_im = v.y * 128.0f;
            const int re = to_schar(pre_re), im = to_schar(pre_im);
            D.pay[2 * i] = (signed char)re;
            D.pay[2 * i + 1] = (signed char)im;
            if constexpr (METER)
                meter_iq(macc, pre_re, pre_im, re, im);
        }
    }
    if constexpr (METER) {
        __shared__ MeterAcc red[4];
        meter_block_store(macc, reinterpret_cast<unsigned char *>(D.pay) + Dp->meter_rel + 16 * blk, (int)threadIdx.x, red);
    }
}
